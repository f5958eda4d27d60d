// circle_window.h -- a circle's tile sets as a 64x64 bit window held by one wave (lane = window row, u64 = window columns), device
// only: the cap of the reference's scratch arrays replayed in row-major order and M_Tile_Contour (tile.c:759) as one dilation.
// Shared by blocker_kernels.hip (the tiles a blocker covers, caps of 1 024) and seek_seed_kernels.hip (the tiles an enemy or a
// surround target seeds, caps of 512).  Free of device variables, so any unit may include it.
#pragma once
#include "wave_bits.h"

// keep the first `cap` set bits of the tile (row-major: lane ascending, then bit ascending)
__device__ __forceinline__ uint64_t cap_rowmajor(uint64_t m, int cap, int lane)
{
    int cnt = __popcll(m), incl = cnt;
#pragma unroll
    for(int d = 1; d < 64; d <<= 1) {
        int o = __shfl_up(incl, d);
        if(lane >= d) incl += o;
    }
    const int before = incl - cnt;
    if(before >= cap) return 0;
    int keep = cap - before;
    if(keep >= cnt) return m;
    // lowest `keep` set bits
    uint64_t out = 0;
    for(int k = 0; k < keep; k++) { uint64_t b = m & (~m + 1); out |= b; m ^= b; }
    return out;
}

// M_Tile_Contour (tile.c:759) of a set inside the window: unmarked in-map cells with a marked
// 8-neighbour
__device__ __forceinline__ uint64_t contour_of(uint64_t m, uint64_t inmap)
{
    const u64x s = mk(m);
    const u64x up = from_n(s), dn = from_s(s);
    const u64x h  = s  | from_w(s)  | from_e(s);
    const u64x hu = up | from_w(up) | from_e(up);
    const u64x hd = dn | from_w(dn) | from_e(dn);
    return to64(andn(h | hu | hd, s)) & inmap;
}
