// lane_group.h -- cross-lane primitives of a GROUP of G lanes (a DPP row of 16, or the whole wave of 64), device only:
// the wavefront barrier, group-uniform values, group ballots / shuffles / arg-min and the DPP prefix sums.  Free of
// device variables, so any unit may include it (agent_group.h -- the neighbour walk and the ClearPath search on top of
// these -- defines one and belongs to agent_kernels.hip alone).
#pragma once

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// A value that is the same in every lane of a wave-wide group BY CONSTRUCTION (read from LDS at a uniform
// address, the result of a reduction): tell the compiler, so that it lives in a scalar register and the loops
// it controls stay uniform -- otherwise one such value in a `break` makes the whole loop divergent, and every
// counter inside it a per-lane VGPR under exec masks (measured: 40 % of the search's instructions were SALU
// bookkeeping for branches that no lane ever takes differently).  Rows of 16 lanes: identity.
template <int G> __device__ __forceinline__ int   uni(int v)   { return G == 64 ? __builtin_amdgcn_readfirstlane(v) : v; }
template <int G> __device__ __forceinline__ float uni(float v) { return G == 64 ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))) : v; }

template <int G> struct grp {
    static __device__ __forceinline__ int lane() { return (int)(threadIdx.x & (G - 1)); }
    static __device__ __forceinline__ int base() { return (int)(threadIdx.x & 63 & ~(G - 1)); }
    static __device__ __forceinline__ unsigned long long ballot(bool p)
    {
        const unsigned long long m = __ballot(p);
        if(G == 64) return m;
        return (m >> base()) & ((1ull << (G & 63)) - 1ull);
    }
    static __device__ __forceinline__ bool any(bool p) { return ballot(p) != 0ull; }
    static __device__ __forceinline__ int shfl(int v, int src) { return __shfl(v, base() + src); }
    static __device__ __forceinline__ float shfl(float v, int src) { return __shfl(v, base() + src); }
    // lexicographic (key, idx) arg-min over the group; key = +inf means "no candidate"
    static __device__ __forceinline__ void argmin(float &key, int &idx)
    {
#pragma unroll
        for(int d = G / 2; d >= 1; d >>= 1) {
            const float ok = __shfl_xor(key, d);
            const int   oi = __shfl_xor(idx, d);
            const bool take = (ok < key) || (ok == key && oi < idx);
            if(take) { key = ok; idx = oi; }
        }
    }
};

// inclusive prefix sum inside every row of 16 lanes (DPP row_shr, zero fill)
__device__ __forceinline__ int row_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);    // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);    // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);    // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);    // row_shr:8
    return v;
}

// inclusive prefix sum over the 64 lanes: four row_shr steps inside each row of 16, then the two
// row broadcasts (DPP; zero fill outside the row)
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);    // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);    // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);    // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);    // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 -> rows 2, 3
    return v;
}
