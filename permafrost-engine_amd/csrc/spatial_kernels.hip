// spatial_kernels.hip -- the BUILD side of the device spatial hash (bitmap_grid.h) for gfx950, hand-written HIP.
//
//   k_sp_bbox     bounding box of a stepped slab (optional filter of what is hashed)
//   k_sp_count .. k_sp_place   fixed-point cell binning, the two-pass scan, and the POOL -- one 16-byte record {pos,
//                 radius, flag bits | uid} + one velocity per inserted entity, in the cell order and per-cell order
//                 bg_ent_cleanup produces after inserting uids 0..n-1, so that a query's candidates are contiguous
//                 runs and a hit needs no second gather.
//   k_sp_build_small   the same for a small world in one workgroup.
// The query side (sp_query_wave, the row walk of agent_group.h) lives with its callers in agent_kernels.hip.
#include "navhip_internal.h"
#include "agent_internal.h"
#include "agent_thread.h"
#include "lane_group.h"

// ---------------------------------------------------------------------------------------------
// spatial hash (bitmap_grid.h): build
// ---------------------------------------------------------------------------------------------
#define SP_MAX_QUERY_R 30   /* largest query radius of the movement tick (separation, movement.c:1695) */
// Optional slab filter: when a rank steps only the entities [work_begin, work_end), nothing farther
// than the largest query radius of the tick (r = 30) from the bounding box of THOSE entities can be
// returned by any of its queries, and leaving such entities out changes neither the order nor the
// caps of what is returned.  box = {max(-ix), max(ix), max(-iy), max(iy)} over the slab in the
// x256 fixed point the queries compare in; INT_MIN-initialised.
// (Four-wave workgroups: a 1024-thread block waits for sixteen free wave slots on one CU -- 26 us beside the
// field builds, in front of the whole spatial hash.  Two boxes alternate between builds: the build that
// consumes box[p] (k_sp_count) re-initialises box[p ^ 1] for its successor, so there is no memset.)
__global__ __launch_bounds__(256) void k_sp_bbox(const float *pos_xz, int begin, int end, int32_t *box)
{
    __shared__ int32_t part[4][4];
    int32_t v[4] = {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
    for(int i = begin + blockIdx.x * 256 + threadIdx.x; i < end; i += gridDim.x * 256) {
        const int32_t ix = bg_scale(pos_xz[2 * i]), iy = bg_scale(pos_xz[2 * i + 1]);
        v[0] = max(v[0], -ix); v[1] = max(v[1], ix); v[2] = max(v[2], -iy); v[3] = max(v[3], iy);
    }
#pragma unroll
    for(int q = 0; q < 4; q++) {
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1) v[q] = max(v[q], __shfl_xor(v[q], d));
        if((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = v[q];
    }
    __syncthreads();
    if(threadIdx.x < 4) {
        int32_t m = INT32_MIN;
        for(int w = 0; w < 4; w++) m = max(m, part[w][threadIdx.x]);
        if(m != INT32_MIN) atomicMax(&box[threadIdx.x], m);
    }
}

__device__ __forceinline__ bool sp_in_box(const int32_t *box, int32_t ix, int32_t iy)
{
    if(!box) return true;
    const int32_t m = SP_MAX_QUERY_R * 256 + 256;     // BG_SCALE_F(largest radius) + 1 wu of slack
    // (int64: the INT_MIN box of an empty slab must reject everything without overflowing)
    return (int64_t)ix >= -(int64_t)box[0] - m && (int64_t)ix <= (int64_t)box[1] + m
        && (int64_t)iy >= -(int64_t)box[2] - m && (int64_t)iy <= (int64_t)box[3] + m;
}
// Pass 1: cell of every entity + its arrival rank in the cell (the counters are zero on entry:
// cleared at allocation, then by k_sp_scan_add of the previous build).
__global__ __launch_bounds__(256) void k_sp_count(nh_grid G, const float *pos_xz, int n,
                                                  int32_t *ent_cell, int32_t *ent_rank,
                                                  int32_t *cell_count, const int32_t *box, int32_t *box_next,
                                                  int32_t *n_active)
{
    int i = blockIdx.x * 256 + threadIdx.x;
    if(box_next && i < 4) box_next[i] = INT32_MIN;           // (the box of the NEXT build)
    if(n_active && i == 0) *n_active = 0;                    // (the list k_sp_place fills: its reader, the last walk, is through)
    if(i >= n) return;
    const int32_t ix = bg_scale(pos_xz[2 * i]), iy = bg_scale(pos_xz[2 * i + 1]);
    if(!sp_in_box(box, ix, iy)) { ent_cell[i] = -1; return; }
    const int c = sp_cell_of(G, ix, iy);
    ent_cell[i] = c;
    ent_rank[i] = atomicAdd(&cell_count[c], 1);
}

// A rank that steps a slab only fills the cells its box (+ the query reach) covers; every other cell is
// empty and is never looked at by a query of the slab either.  The scans skip the blocks of cells that lie
// entirely in grid rows outside the box: their block sum is 0 and their cell_start entries stay unwritten.
// (rows [r0, r1] of the box in cells; a block is a run of NH_SCAN_T consecutive cells, row-major)
__device__ __forceinline__ bool sp_block_outside_box(const nh_grid &G, const int32_t *box, int first_cell, int ncells)
{
    if(!box) return false;
    const int32_t m = SP_MAX_QUERY_R * 256 + 256;
    const int64_t y0 = -(int64_t)box[2] - m, y1 = (int64_t)box[3] + m;          // fixed-point rows of the box
    if(y1 < y0) return true;                                                     // empty slab: nothing is inserted
    // cell rows (clamped like sp_cell_of clamps an element into the grid)
    const int64_t r0 = min(max((y0 - G.origin_y) >> 12, (int64_t)0), (int64_t)G.grid_h - 1);
    const int64_t r1 = min(max((y1 - G.origin_y) >> 12, (int64_t)0), (int64_t)G.grid_h - 1);
    const int last_cell = min(first_cell + NH_SCAN_T, ncells) - 1;
    // (one row more at the end: a query reads cell_start one past its last cell -- the first cell of the
    // row after r1)
    return last_cell < r0 * G.grid_w || first_cell >= (r1 + 2) * G.grid_w;
}

// exclusive scan of cell_count[0..ncells) -> cell_start[0..ncells], two passes over NH_SCAN_T-cell
// blocks: (1) block-local exclusive scan + block totals, (2) add the sum of the preceding totals.
// (Blocks of four waves: a 1024-thread block needs sixteen free wave slots on ONE compute unit at the
// same moment, and beside the cohesion kernel's stream of one-wave blocks it waited for them for
// 50 us -- on the critical path of the tick.)
__global__ __launch_bounds__(NH_SCAN_T) void k_sp_scan_local(const int32_t *cell_count, int32_t *cell_start,
                                                             int32_t *block_sum, int ncells,
                                                             nh_grid G, const int32_t *box)
{
    __shared__ int32_t wsum[NH_SCAN_T / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if(sp_block_outside_box(G, box, blockIdx.x * NH_SCAN_T, ncells)) {
        if(t == 0) block_sum[blockIdx.x] = 0;
        return;
    }
    const int i = blockIdx.x * NH_SCAN_T + t;
    int32_t v = (i < ncells) ? cell_count[i] : 0;
    int32_t incl = v;
#pragma unroll
    for(int d = 1; d < 64; d <<= 1) {
        int32_t o = __shfl_up(incl, d);
        if(lane >= d) incl += o;
    }
    if(lane == 63) wsum[w] = incl;
    __syncthreads();
    int32_t woff = 0, tot = 0;
#pragma unroll
    for(int k = 0; k < NH_SCAN_T / 64; k++) {
        int32_t x = wsum[k];
        if(k < w) woff += x;
        tot += x;
    }
    if(i < ncells) cell_start[i] = woff + incl - v;
    if(t == 0) block_sum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(NH_SCAN_T) void k_sp_scan_add(int32_t *cell_start, const int32_t *block_sum,
                                                           int ncells, int nblocks, int32_t *zero_counts,
                                                           nh_grid G, const int32_t *box)
{
    __shared__ int32_t wsum[NH_SCAN_T / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // (the last block always runs: it writes the grand total, cell_start[ncells])
    if((int)blockIdx.x != nblocks - 1 && sp_block_outside_box(G, box, blockIdx.x * NH_SCAN_T, ncells)) return;
    // sum of the totals of the blocks before this one (and, in the last block, of all blocks)
    int32_t part = 0, all = 0;
    for(int k = t; k < nblocks; k += NH_SCAN_T) {
        int32_t x = block_sum[k];
        all += x;
        if(k < (int)blockIdx.x) part += x;
    }
    const bool last = (int)blockIdx.x == nblocks - 1;
    int32_t red = last ? all : part;          // the last block needs both: two reductions
#pragma unroll
    for(int d = 32; d >= 1; d >>= 1) { red += __shfl_xor(red, d); part += __shfl_xor(part, d); }
    if(lane == 0) wsum[w] = red;
    __syncthreads();
    int32_t tot = 0;
#pragma unroll
    for(int k = 0; k < NH_SCAN_T / 64; k++) tot += wsum[k];
    __syncthreads();
    if(lane == 0) wsum[w] = part;
    __syncthreads();
    int32_t off = 0;
#pragma unroll
    for(int k = 0; k < NH_SCAN_T / 64; k++) off += wsum[k];
    const int i = blockIdx.x * NH_SCAN_T + t;
    if(i < ncells) cell_start[i] += off;
    if(zero_counts && i < ncells) zero_counts[i] = 0;     // consumed by k_sp_scan_local: clean for the next build
    if(last && t == 0) cell_start[ncells] = tot;
}
// Pass 3: entities into their cell's range in arrival order (no atomics: the rank is known)
__global__ __launch_bounds__(256) void k_sp_scatter(const int32_t *ent_cell, const int32_t *ent_rank, int n,
                                                    const int32_t *cell_start, int32_t *tmp_id)
{
    int i = blockIdx.x * 256 + threadIdx.x;
    if(i >= n) return;
    const int c = ent_cell[i];
    if(c < 0) return;                            // outside the slab filter
    tmp_id[cell_start[c] + ent_rank[i]] = i;
}

// Pass 4: per-cell order + the pool records.  bg_ent_insert pushes at the head of the cell's
// overflow chain and bg_ent_cleanup copies the chain head-first (bitmap_grid.h:1102-1121,
// 1515-1521), so after inserting uids 0..n-1 each cell holds its elements in DESCENDING uid order:
// the final slot of an element is its cell's start + the number of cell mates with a larger uid
// (one thread per element counts them: cells hold a handful of elements).
#define SP_BLOCK 64
__global__ __launch_bounds__(SP_BLOCK) void k_sp_place(nh_grid G, const float *pos_xz, nh_pack_src src,
                                                  const int32_t *ent_cell, const int32_t *tmp_id,
                                                  int n, int work_begin, int work_end,
                                                  float4 *recA, float2 *recV, int32_t *pool_of,
                                                  int32_t *active, int32_t *n_active)
{
    // one thread per ENTITY (not per pool slot): its inputs are coalesced loads that do not wait for the
    // slot search, the only gathers are the cell's bounds and its handful of ids, and the record goes out
    // as a scattered store.  (Per slot the kernel was a chain of five dependent gathers -- id, cell, bounds,
    // cell mates, the entity's six attribute arrays -- and took 60 us beside the cohesion kernel.)
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    const int c = i < n ? ent_cell[i] : -1;      // (-1: outside the slab filter)
    int slot = -1;
    bool walks = false;
    if(c >= 0) {
        float4 a;
        float2 v;
        pool_record(i, pos_xz, src, work_begin, work_end, a, v);
        const int b = G.cell_start[c], e = G.cell_start[c + 1];
        int larger = 0;
        for(int q = b; q < e; q++) larger += tmp_id[q] > i;
        slot = b + larger;
        recA[slot] = a;
        recV[slot] = v;
        pool_of[i] = slot;
        walks = !(__float_as_uint(a.w) & NH_PB_IDLE);
    }
    // A rank that steps a slab: the pool slots whose entity has a work item, as a LIST (any order), so that the neighbour
    // walk runs one row per listed slot instead of striding rows over a pool of which seven eighths are idle -- a row
    // then walked up to six entities one after the other and the launch took as long for an eighth of the entities as
    // for all of them (38 against 47 us).  One atomic per wave (the slab is a contiguous uid range: few waves have any).
    if(active) {
        const unsigned long long m = __ballot(walks);
        if(m) {
            const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
            int base = 0;
            if(lane == leader) base = atomicAdd(n_active, __popcll(m));
            base = __shfl(base, leader);
            if(walks) active[base + __popcll(m & ((1ull << lane) - 1ull))] = slot;
        }
    }
}

// The whole build for a SMALL world in one workgroup: counts, scan, arrival order and placement out of LDS between
// barriers instead of five dependent launches.  The front of the step is a chain of launches of ~5 us each whatever
// they do; for a thousand entities that chain IS the front (31 us of a 97-us tick at configs[0]), and with the step's
// hand-overs at 2-3 us and the cohesion term enqueued first nothing else is in front of k_agent_mid any more.  (Round 6
// built this once before the hand-overs changed and removed it: the tick was bound by its events and the host then,
// profiles/r06_ab_small_world_hash_rejected.txt.)  Same results: the order inside a cell is fixed by the uids, not by
// who arrives first.  Leaves the global counters untouched (they stay zero for the next large build).
#define SP_SMALL_N     1024       /* entities */
#define SP_SMALL_CELLS 8192       /* cells */
#define SP_SMALL_T     256
__global__ __launch_bounds__(SP_SMALL_T) void k_sp_build_small(nh_grid G, const float *pos_xz, nh_pack_src src, int n, int ncells,
                                                            int work_begin, int work_end, int32_t *cell_start, float4 *recA, float2 *recV, int32_t *pool_of)
{
    __shared__ int32_t  start[SP_SMALL_CELLS + 1];          // counts, then the exclusive scan
    __shared__ uint16_t ecell[SP_SMALL_N], erank[SP_SMALL_N], order[SP_SMALL_N];
    __shared__ int32_t  wsum[SP_SMALL_T / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for(int c = t; c <= ncells; c += SP_SMALL_T) start[c] = 0;
    __syncthreads();
    for(int i = t; i < n; i += SP_SMALL_T) {
        const int c = sp_cell_of(G, bg_scale(pos_xz[2 * i]), bg_scale(pos_xz[2 * i + 1]));
        ecell[i] = (uint16_t)c;
        erank[i] = (uint16_t)atomicAdd(&start[c], 1);
    }
    __syncthreads();
    // exclusive scan, SP_SMALL_T cells at a time with a running carry
    int32_t carry = 0;
    for(int base = 0; base < ncells; base += SP_SMALL_T) {
        const int c = base + t;
        const int32_t v = c < ncells ? start[c] : 0;
        const int32_t incl = wave_incl_scan(v);
        if(lane == 63) wsum[w] = incl;
        __syncthreads();
        int32_t woff = 0, tot = 0;
#pragma unroll
        for(int k = 0; k < SP_SMALL_T / 64; k++) { const int32_t x = wsum[k]; if(k < w) woff += x; tot += x; }
        if(c < ncells) { start[c] = carry + woff + incl - v; cell_start[c] = carry + woff + incl - v; }
        carry += tot;
        __syncthreads();
    }
    if(t == 0) { start[ncells] = carry; cell_start[ncells] = carry; }
    __syncthreads();
    for(int i = t; i < n; i += SP_SMALL_T) order[start[ecell[i]] + erank[i]] = (uint16_t)i;
    __syncthreads();
    // descending uid inside a cell (k_sp_place)
    for(int i = t; i < n; i += SP_SMALL_T) {
        float4 a;
        float2 v;
        pool_record(i, pos_xz, src, work_begin, work_end, a, v);
        const int c = ecell[i], b = start[c], e = start[c + 1];
        int larger = 0;
        for(int q = b; q < e; q++) larger += order[q] > i;
        recA[b + larger] = a;
        recV[b + larger] = v;
        pool_of[i] = b + larger;
    }
}

// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
// The two-pass exclusive scan on its own: count[0..n) -> start[0..n].  box (or null): the slab filter over G's rows of
// cells; zero_counts (or null): cleared once consumed.  (The cohesion regrouping scans its bins with it.)
void nh_launch_scan(const int32_t *count, int32_t *start, int32_t *block_sum, int n, int32_t *zero_counts,
                    const nh_grid &G, const int32_t *box, hipStream_t s)
{
    const int nblocks = (n + NH_SCAN_T - 1) / NH_SCAN_T;
    hipLaunchKernelGGL(k_sp_scan_local, dim3(nblocks), dim3(NH_SCAN_T), 0, s, count, start, block_sum, n, G, box);
    hipLaunchKernelGGL(k_sp_scan_add, dim3(nblocks), dim3(NH_SCAN_T), 0, s, start, block_sum, n, nblocks, zero_counts, G, box);
}

// Four dependent launches, no memset (cell_count is zeroed by k_sp_scan_add once it has been
// consumed; the box of the slab filter is the exception).
void nh_launch_spatial_build(nh_grid &G, const float *d_pos_xz, nh_spatial_scratch &S,
                             int slab_begin, int slab_end, hipStream_t s)
{
    const int n = G.n, ncells = G.grid_w * G.grid_h;
    // a strict sub-range of the entities is stepped: hash only what its queries can reach
    const int32_t *box = nullptr;
    int32_t *box_next = nullptr;
    if(S.box && (slab_begin > 0 || slab_end < n)) {
        int32_t *mine = S.box + 4 * (S.box_parity & 1);
        box_next = S.box + 4 * ((S.box_parity & 1) ^ 1);
        if(slab_end > slab_begin)
            hipLaunchKernelGGL(k_sp_bbox, dim3(min(128, (slab_end - slab_begin + 255) / 256)), dim3(256), 0, s,
                               d_pos_xz, slab_begin, slab_end, mine);
        box = mine;
    }
    G.cell_start = S.cell_start; G.recA = S.recA; G.recV = S.recV; G.pool_of = S.pool_of;
    // (a slab: the list of pool slots with a work item lives in ent_rank's buffer, which is free once k_sp_scatter has
    // read it; its length behind the two slab boxes)
    int32_t *active = box ? S.ent_rank : nullptr, *n_active = box ? S.box + 8 : nullptr;
    G.active = active; G.n_active = n_active;
    if(!box && n > 0 && n <= SP_SMALL_N && ncells <= SP_SMALL_CELLS) {
        // a small world, all of it stepped: one workgroup instead of five launches
        hipLaunchKernelGGL(k_sp_build_small, dim3(1), dim3(SP_SMALL_T), 0, s, G, d_pos_xz, S.src, n, ncells, slab_begin, slab_end, S.cell_start, S.recA,
                           S.recV, S.pool_of);
        return;
    }
    if(n > 0)
        hipLaunchKernelGGL(k_sp_count, dim3((n + 255) / 256), dim3(256), 0, s, G, d_pos_xz, n,
                           S.ent_cell, S.ent_rank, S.cell_count, box, box_next, n_active);
    nh_launch_scan(S.cell_count, S.cell_start, S.block_sum, ncells, S.cell_count, G, box, s);
    if(n > 0) {
        hipLaunchKernelGGL(k_sp_scatter, dim3((n + 255) / 256), dim3(256), 0, s, S.ent_cell, S.ent_rank, n,
                           S.cell_start, S.tmp_id);
        hipLaunchKernelGGL(k_sp_place, dim3((n + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, s, G, d_pos_xz, S.src,
                           S.ent_cell, S.tmp_id, n, slab_begin, slab_end, S.recA, S.recV, S.pool_of, active, n_active);
    }
}
