// agent_kernels.hip -- per-agent movement step for gfx950 (MI355X), hand-written HIP.
//
// Reference semantics (permafrost-engine):
//   src/game/movement.c   move_velocity_work :3395, point_seek_vpref :1870, point_seek_total_force
//                         :1745, arrive_force_point :1546, cohesion_force :1653, separation_force
//                         :1690, nullify_impass_components :1831, find_neighbours :2768,
//                         enemy_seek_vpref :1946, vec2_truncate :643, position accept :2336-2358
//   src/game/clearpath.c  G_ClearPath_NewVelocity :694 and everything under it
//   src/phys/collision.c  C_InfiniteLineIntersection :820, C_RayRayIntersection2D :854
//   src/lib/public/bitmap_grid.h  bg_*_inrange_circle :1376 (candidate order + fixed-point test)
//   src/navigation/nav.c  N_DesiredPointSeekVelocity :3468, n_interpolated_flow_dir :3407,
//                         N_PositionPathable/Blocked :4055/:4070;  src/map/tile.c :356,:391,:547
//
// Arithmetic mirrors the reference's C expression by expression (agent_math.h); all
// order-dependent float sums are evaluated in the reference's own order.
//
// Kernels of one tick (step_api.hip wires the streams; the spatial hash is built by spatial_kernels.hip, the
// cohesion term comes from cohesion_kernels.hip):
//   k_agent_nbr   one ROW of 16 lanes per entity, pool order: separation force + ClearPath neighbour
//                 lists in one walk (agent_group.h).  Needs only the snapshot: runs beside the field
//                 builds.
//   k_agent_mid   one THREAD per entity: the scalar chain -- flow sampling, arrive force, priority
//                 ladder -> preferred velocity.  Agents without ClearPath neighbours are truncated +
//                 position-tested here; the rest go to device-side work lists by neighbour count.
//   k_cp_small / k_cp_rows / k_cp_heavy
//                 ClearPath for the listed agents: a ROW of 16 lanes per agent -- 1..4 neighbours on a
//                 lean kernel of its own (one attempt, no queue; eight waves per SIMD), 5..16 on the
//                 general search --, a WORKGROUP per agent with 17..64 (a crowd: its waves share the ray
//                 pairs); lanes spread over cones / ray pairs, branch and bound on the distance to
//                 des_v, a candidate queue, a lexicographic arg-min that reproduces the reference's
//                 first-wins rule; work units numbered heaviest first, drawn by tickets.  Rows on the
//                 caller's stream, the rest beside them on a side stream.
//   k_agent_full  one WAVE per listed agent, the whole step (irregular gathers: garrisoned
//                 neighbours, wide queries).
// Test utilities: k_spatial_query (the wave query on its own), k_region_lookup (sample_region in batches),
// k_clearpath<> / k_clearpath_team (the search on given neighbour lists), navhip_debug_cp_attempts.
//
// The ONE unit of the library that includes agent_group.h (it defines the device variable nh_cp_attempts).
#include "navhip_internal.h"
#include "agent_internal.h"
#include "agent_group.h"

// (this code object's own copy of the table: the library is built without relocatable device code)
static __constant__ double c_exp2_64[64] = { NH_EXP2_64_TABLE };

// ---------------------------------------------------------------------------------------------
// spatial hash: query.  All 64 lanes cooperate on ONE query; returns the number written (wave
// uniform).  Visiting order == bg_*_inrange_circle (bitmap_grid.h:1408-1466): coarse 8x8 blocks
// row-major, inside a block fine rows top to bottom, cells left to right, packed elements in
// order.  Cells of one fine row are contiguous in the cell-sorted pool, so a (block,row) pair is
// one contiguous range that the lanes test 64 elements at a time; ballot + prefix popcount
// appends hits in order and enforces `maxout` exactly where the reference stops.
// The hits are POOL SLOTS (uid = recA[slot].w >> 8).
// (No query of the movement tick reaches farther than r = 30: the slab filter of the build, SP_MAX_QUERY_R in
// spatial_kernels.hip, leaves out what lies beyond that -- a wider query in the tick has to raise that bound.)
// ---------------------------------------------------------------------------------------------
// out_d2 (optional, [maxout]): squared fixed-point distance of every hit (fits int32 for the
// ranges the movement tick uses), so that a narrower query around the same point can be derived
// from this one without touching memory again.
__device__ int sp_query_wave(const nh_grid &G, float x, float z, float range, int maxout,
                             uint32_t *out_ids, int lane, int32_t *out_d2 = nullptr)
{
    if(maxout <= 0 || range < 0.0f) return 0;
    const int32_t icx = bg_scale(x), icy = bg_scale(z), ir = bg_scale(range);
    const int64_t ir2 = (int64_t)ir * (int64_t)ir;
    sp_extent E;
    if(!sp_query_extent(G, icx, icy, ir, E)) return 0;

    int written = 0;
    if(E.wide) {
        // wide-query fast path (bitmap_grid.h:1389-1397): the clean pool is scanned linearly
        const int npool = G.cell_start[G.grid_w * G.grid_h];     // == G.n unless a slab filter is on
        for(int base = 0; base < npool; base += 64) {
            int k = base + lane;
            bool hit = false;
            int64_t d2 = 0;
            if(k < npool) {
                const float4 c = G.recA[k];
                int64_t dx = (int64_t)bg_scale(c.x) - icx, dy = (int64_t)bg_scale(c.y) - icy;
                d2 = dx * dx + dy * dy;
                hit = d2 <= ir2;
            }
            uint64_t m = __ballot(hit);
            int p = written + __popcll(m & ((1ull << lane) - 1ull));
            if(hit && p < maxout) {
                out_ids[p] = (uint32_t)k;
                if(out_d2) out_d2[p] = (int32_t)d2;
            }
            written += __popcll(m);
            if(written >= maxout) return maxout;
        }
        return written;
    }

    // A SEGMENT = the cells of one fine row inside one coarse block, contiguous in the pool.  One
    // pass resolves 64 segments in visiting order -- lane = ((coarse row, block column) << 3) | fine
    // row, with CB (a power of two) block columns and 8 / CB coarse rows per pass, so the r = 30 and
    // r = 10 boxes of the movement tick (at most 2 x 2 coarse blocks) take a single pass: two
    // cell_start loads per lane, a DPP prefix sum, then the candidates 64 at a time, each lane
    // finding its segment by binary search over the prefix.
    const int cxc_lo = E.cx_lo >> 3, cxc_hi = E.cx_hi >> 3, ncx = cxc_hi - cxc_lo + 1;
    const int cyc_lo = E.cy_lo >> 3, cyc_hi = E.cy_hi >> 3;
    const int lgcb = ncx <= 1 ? 0 : ncx <= 2 ? 1 : ncx <= 4 ? 2 : 3;
    const int CB = 1 << lgcb, CR = 8 >> lgcb;
    // squared distances fit 32 bits when the box is small (r = 30: |d| <= 7680 + 4095)
    const bool small = ir <= 16000;
    for(int cyc0 = cyc_lo; cyc0 <= cyc_hi; cyc0 += CR) {
        for(int cbase = 0; cbase < ncx; cbase += CB) {
            const int sg = lane >> 3, fyi = lane & 7;
            const int cyc = cyc0 + (sg >> lgcb), cxi = cbase + (sg & (CB - 1));
            int bb = 0, len = 0;
            if(cyc <= cyc_hi && cxi < ncx) {
                const int fy = cyc * 8 + fyi;
                if(fy >= E.cy_lo && fy <= E.cy_hi) {
                    const int cxc = cxc_lo + cxi;
                    const int fx0 = max(cxc * 8, E.cx_lo), fx1 = min(cxc * 8 + 8, E.cx_hi + 1);
                    bb = G.cell_start[fy * G.grid_w + fx0];
                    len = G.cell_start[fy * G.grid_w + fx1] - bb;
                }
            }
            const int incl = wave_incl_scan(len);
            const int total = __shfl(incl, 63);
            if(total == 0) continue;
            const int bo = bb - (incl - len);                         // pool index of candidate q: bo + q
            for(int base = 0; base < total; base += 64) {
                const int q = base + lane;
                // first lane whose inclusive prefix exceeds q = the segment of candidate q (empty
                // segments are stepped over because the prefix does not move); every lane runs
                // the shuffles
                int lo = 0;
#pragma unroll
                for(int st = 32; st >= 1; st >>= 1) {
                    const int pv = __shfl(incl, lo + st - 1);
                    if(pv <= q) lo += st;
                }
                const int kk = __shfl(bo, lo & 63) + q;
                const int k = (q < total) ? kk : -1;
                bool hit = false;
                int32_t d2s = 0;
                if(k >= 0) {
                    const float4 c = G.recA[k];
                    const int32_t sx = bg_scale(c.x), sy = bg_scale(c.y);
                    if(small) {
                        // (elements clamped into a border cell may be far away: range-check before
                        // squaring in 32 bits)
                        const int32_t dx = sx - icx, dy = sy - icy;
                        const bool near = (uint32_t)(dx + 32767) < 65535u && (uint32_t)(dy + 32767) < 65535u;
                        d2s = near ? dx * dx + dy * dy : 0x7fffffff;
                        hit = d2s <= (int32_t)ir2;
                    }else{
                        const int64_t dx = (int64_t)sx - icx, dy = (int64_t)sy - icy;
                        const int64_t d2 = dx * dx + dy * dy;
                        hit = d2 <= ir2;
                        d2s = (int32_t)d2;
                    }
                }
                uint64_t m = __ballot(hit);
                int p = written + __popcll(m & ((1ull << lane) - 1ull));
                if(hit && p < maxout) {
                    out_ids[p] = (uint32_t)k;
                    if(out_d2) out_d2[p] = d2s;
                }
                written += __popcll(m);
                if(written >= maxout) return maxout;
            }
        }
    }
    return written;
}

// filter_garrisoned, position.c:100-119: walk backwards, overwrite with the current last
__device__ __forceinline__ uint32_t slot_bits(const nh_grid &G, uint32_t slot)
{
    return __float_as_uint(G.recA[slot].w);
}

__device__ int filter_garrisoned_wave(const nh_grid &G, uint32_t *ids, int count, int lane)
{
    bool any = false;
    for(int base = 0; base < count; base += 64) {
        int k = base + lane;
        any |= (k < count) && (slot_bits(G, ids[k]) & NH_PB_GARRISONED);
    }
    if(!__any(any)) return count;
    int ret = count;
    if(lane == 0) {
        for(int i = count - 1; i >= 0; i--) {
            if(slot_bits(G, ids[i]) & NH_PB_GARRISONED) {
                ids[i] = ids[ret - 1];
                ret--;
            }
        }
    }
    wave_sync();
    return __shfl(ret, 0);
}

// ---------------------------------------------------------------------------------------------
// wave-per-agent pieces of k_agent_full
// ---------------------------------------------------------------------------------------------
// waves (= agents) per workgroup of the wave-per-agent kernels; 2 measured best for the round-1
// k_agent_step (1: 0.490, 2: 0.483, 4: 0.494, 8: 0.521 ms/tick in one session)
#define AG_WAVES 2
struct wave_lds {
    uint32_t ids30[128];                       // separation query result (cap 128, :1695)
    union {
        uint32_t ids10[512];                   // ClearPath neighbour query result (cap 512, :2779)
        float    sep[256];                     // earlier: separation terms (x, z)[128]
    } u;
    int32_t  d2_30[128];                       // squared fixed-point distances of the r=30 hits
    uint32_t ids10d[128];                      // r=10 list derived from the r=30 list
};

// separation_force, movement.c:1690.  ids30/n30 already gathered (pool slots); wave-uniform result.
__device__ v2 separation_wave(const nh_grid &G, uint32_t my_slot, v2 me, float my_radius,
                              uint32_t my_bits, const uint32_t *ids30, int n30, float *sep,
                              float scaled_max_force, int lane, const double *exp_tab)
{
    if(n30 == 0) return mkv(0.0f, 0.0f);
    for(int base = 0; base < n30; base += 64) {
        int k = base + lane;
        if(k < n30) {
            uint32_t curr = ids30[k];
            const float4 ra = G.recA[curr];                                 // {pos, radius, bits}
            uint32_t fl = __float_as_uint(ra.w);
            v2 term = mkv(0.0f, 0.0f);
            bool skip = (curr == my_slot) || !(fl & NH_PB_MOVABLE) || ((my_bits ^ fl) & NH_PB_AIR);
            if(!skip) {
                v2 t2;
                if(separation_term(me, my_radius, mkv(ra.x, ra.y), ra.z, exp_tab, t2)) term = t2;
            }
            ((f2*)sep)[k] = f2{term.x, term.z};
        }
    }
    wave_sync();
    // ret += diff, strictly in candidate order (every lane evaluates the same chain; x and z ride
    // in one packed add)
    f2 acc = {0.0f, 0.0f};
    for(int k = 0; k < n30; k++)
        acc = acc + ((const f2*)sep)[k];
    wave_sync();
    const v2 ret = vscale(mkv(acc.x, acc.y), -1.0f);
    return vtrunc(ret, scaled_max_force);
}

// find_neighbours, movement.c:2768: classify the r=10 query result into dynamic / static lists
__device__ void classify_neighbours(const nh_grid &G, uint32_t my_slot, uint32_t my_bits,
                                    const uint32_t *ids10, int n10, float *dyn, int &n_dyn,
                                    float *stat, int &n_stat, int lane)
{
    n_dyn = 0; n_stat = 0;
    for(int base = 0; base < n10; base += 64) {
        int k = base + lane;
        int cls = 0;                              // 0 skip, 1 dynamic, 2 static
        float rec[5] = {0, 0, 0, 0, 0};
        if(k < n10) {
            uint32_t curr = ids10[k];
            const float4 ra = G.recA[curr];
            uint32_t fl = __float_as_uint(ra.w);
            float rad = ra.z;
            bool skip = (curr == my_slot) || !(fl & NH_PB_MOVABLE) || (rad == 0.0f)
                     || ((my_bits ^ fl) & NH_PB_AIR);
            if(!skip) {
                rec[0] = ra.x; rec[1] = ra.y;
                rec[4] = rad;
                if(fl & NH_PB_STATIC) {
                    cls = 2;                       // static: velocity forced to zero (:2820)
                }else{
                    const float2 vel = G.recV[curr];
                    cls = 1;
                    rec[2] = vel.x; rec[3] = vel.y;
                }
            }
        }
        uint64_t md = __ballot(cls == 1), ms = __ballot(cls == 2);
        uint64_t lt = (1ull << lane) - 1ull;
        if(cls == 1) {
            int p = n_dyn + __popcll(md & lt);
            if(p < 32) { for(int q = 0; q < 5; q++) dyn[5 * p + q] = rec[q]; }     // MAX_NEIGHBOURS
        }else if(cls == 2) {
            int p = n_stat + __popcll(ms & lt);
            if(p < 32) { for(int q = 0; q < 5; q++) stat[5 * p + q] = rec[q]; }
        }
        n_dyn = min(32, n_dyn + __popcll(md));
        n_stat = min(32, n_stat + __popcll(ms));
    }
    wave_sync();
}

// The r = 10 neighbour query (find_neighbours, movement.c:2779) as a filter of the r = 30 query of
// the same agent (separation_force, :1695).  Valid when the r = 30 list is COMPLETE (its cap of 128
// did not bind) and both queries scan in the same mode: every entity within 10 is then in the list,
// and two entities keep their relative order in any query that returns both (the visiting key --
// coarse block, fine row, cell, slot -- does not depend on the query).  Returns the derived count,
// or -1 when the r = 10 query has to run on its own.  Must see the list BEFORE filter_garrisoned
// permutes it.
__device__ int derive_r10(const nh_grid &G, v2 me, const uint32_t *ids30, const int32_t *d2_30,
                          int n30raw, uint32_t *out, int lane)
{
    if(n30raw >= 128) return -1;
    // an r=30 box covers at most 5x5 cells: on a grid of more than 33 cells neither query can take
    // the wide path (25 * 4 < 34 * 3) and both scan in block order
    if((int64_t)G.grid_w * G.grid_h <= 33) {
        const int32_t icx = bg_scale(me.x), icy = bg_scale(me.z);
        sp_extent E30, E10;
        const bool ok30 = sp_query_extent(G, icx, icy, bg_scale(30.0f), E30);
        const bool ok10 = sp_query_extent(G, icx, icy, bg_scale(10.0f), E10);
        if(!ok30 || !ok10 || E30.wide != E10.wide) return -1;
    }
    const int32_t ir10 = bg_scale(10.0f);
    const int32_t lim = ir10 * ir10;
    int written = 0;
    for(int base = 0; base < n30raw; base += 64) {
        const int k = base + lane;
        const bool hit = k < n30raw && d2_30[k] <= lim;
        const uint64_t m = __ballot(hit);
        const int p = written + __popcll(m & ((1ull << lane) - 1ull));
        if(hit) out[p] = ids30[k];
        written += __popcll(m);
    }
    wave_sync();
    return written;
}

// ---------------------------------------------------------------------------------------------
// k_agent_nbr: one ROW of 16 lanes per pool slot (NBR_BLOCK / 16 entities per workgroup)
// ---------------------------------------------------------------------------------------------
// STRIDED (a rank that steps a slab of a large job; the name is history): the launch is sized by the slab and takes its
// pool slots from the list k_sp_place made of the entities with a work item.  With the whole snapshot stepped every
// pool slot has its own row.
#define NBR_WAVES 7        /* 72 VGPRs; 8 needs five spilled dwords per lane */
// Threads per workgroup of the front's kernels.  ONE wave: they run beside the cohesion kernel's stream of
// one-wave workgroups and the field builds, which take every wave slot the moment it frees up -- a workgroup
// of four waves waits until four slots of ONE compute unit are free at the same moment.
#define NBR_BLOCK 64
template <bool STRIDED>
__global__ __launch_bounds__(NBR_BLOCK) __attribute__((amdgpu_waves_per_eu(NBR_WAVES, 8)))
void k_agent_nbr(nh_grid G, int npool_max, nh_nbr NB, float scaled_max_force)
{
    __shared__ double exp_tab[64];
    __shared__ __attribute__((aligned(16))) float2 terms[NBR_BLOCK / 16][16];
    if(threadIdx.x < 64) exp_tab[threadIdx.x] = c_exp2_64[threadIdx.x];
    __syncthreads();
    const int grp_i = threadIdx.x >> 4;
    if(!STRIDED) {
        const int k = blockIdx.x * (NBR_BLOCK / 16) + grp_i;
        if(k >= npool_max || k >= G.cell_start[G.grid_w * G.grid_h]) return;
        if(__float_as_uint(G.recA[k].w) & NH_PB_IDLE) return;         // no work item (or outside the slab)
        nbr_walk_row(G, k, scaled_max_force, exp_tab, terms[grp_i], NB);
    }else{
        // a slab: one row per pool slot k_sp_place listed (the entities with a work item)
        const int r = blockIdx.x * (NBR_BLOCK / 16) + grp_i;
        if(r >= *G.n_active) return;
        nbr_walk_row(G, G.active[r], scaled_max_force, exp_tab, terms[grp_i], NB);
    }
}

// wave-aggregated append to a device work list: one atomic per wave and list, on the wave's sub-list
__device__ __forceinline__ void worklist_push(const nh_worklists &WL, int which, bool want, int uid)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(want);
    if(!m) return;
    const int sub = (int)((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (NH_WL_SUB - 1));
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if(lane == leader) base = atomicAdd(&WL.count[which * NH_WL_SUB + sub], __popcll(m));
    base = __shfl(base, leader);
    if(want) WL.ids[((size_t)which * NH_WL_SUB + sub) * WL.cap + base + __popcll(m & ((1ull << lane) - 1ull))] = uid;
}

// ---------------------------------------------------------------------------------------------
// k_agent_mid: the per-agent scalar chain -- desired direction, arrive force, probes, priority
// ladder, vpref -- in uid order (every per-entity input / output is contiguous), ONE thread per entity.
// The work is a chain of dependent loads and IEEE divide / sqrt sequences at 1.5 waves per SIMD; with the loads
// requested ahead of the chain (mid_thread, sample_flow) one lane per entity beats two or four
// (profiles/archive/r03_ab_mid_lanes.txt).  Splitting it -- the sampling half beside the cohesion term, the rest behind the
// join (round 5), or the rest at the head of every ClearPath search (round 6) -- was measured twice and lost twice
// (profiles/r05_ab_split_mid_*.txt, r06_ab_step_without_mid_rejected.txt): the launch is latency, and the chip is
// not idle beside it.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_agent_mid(nh_step_params P, nh_nbr NB, const float *coh_xz,
                                                  nh_mid_rec *mid, nh_worklists WL, nh_step_outs O,
                                                  float scaled_max_force, double force_thresh)
{
    const int uid = P.work_begin + (int)(blockIdx.x * 64 + threadIdx.x);
    const bool live = uid < P.work_end;
    int disp = DISP_DONE;
    if(live) {
        nh_mid_rec R;
        v2 out_vel;
        disp = mid_thread(P, uid, NB, coh_xz, scaled_max_force, force_thresh, R, out_vel);
        if(O.vdes_xz)  { O.vdes_xz[2 * uid] = R.vdes[0]; O.vdes_xz[2 * uid + 1] = R.vdes[1]; }
        if(O.vpref_xz) { O.vpref_xz[2 * uid] = R.vpref[0]; O.vpref_xz[2 * uid + 1] = R.vpref[1]; }
        if(disp == DISP_DONE) {
            post_thread(P, uid, mkv(P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1]), P.state[uid], P.flags[uid],
                        P.radius[uid], out_vel, R.vel_cap, R.status, O);
        }else{
            mid[uid] = R;
        }
    }
#pragma unroll
    for(int w = 0; w <= NH_WL_FULL; w++)
        worklist_push(WL, w, live && disp == DISP_ROW0 + w, uid);
}

// ---------------------------------------------------------------------------------------------
// ClearPath for every listed agent: two launches by problem size (the per-agent cost spans three
// orders of magnitude; one kernel for all needed the registers of the largest and the LDS of each),
// side by side on two streams.
// ---------------------------------------------------------------------------------------------
#define CP_WAVES 4
// waves per workgroup of k_cp_rows (its waves work on their own: the workgroup only shares the unit tables)
#define CPR_WAVES 4
// problems on the workgroup lists from which one wave takes one problem (k_cp_heavy_solo) instead of a team
#define CP_SOLO_MIN 8192

// Running totals of the work units of a kernel's sub-lists, by the first wave of the workgroup: entry k
// holds `cnt[k]` agents = (cnt[k] + per - 1) / per units; unit_end[k] = units of the entries up to and
// including k.  (One thread adding up 128-256 entries in front of every workgroup's first barrier was 770-1 500
// wave instructions per workgroup: a fifth of everything k_cp_small executed.)
template <typename F>
__device__ __forceinline__ void unit_totals(int32_t *unit_end, int ntab, F units_of)
{
    if(threadIdx.x >= 64) return;
    const int lane = threadIdx.x, per_lane = (ntab + 63) >> 6;        // consecutive entries per lane
    int local = 0;
    for(int j = 0; j < per_lane; j++) {
        const int k = lane * per_lane + j;
        if(k < ntab) local += units_of(k);
    }
    int run = wave_incl_scan(local) - local;
    for(int j = 0; j < per_lane; j++) {
        const int k = lane * per_lane + j;
        if(k < ntab) { run += units_of(k); unit_end[k] = run; }
    }
}

// first k with end[k] > u (n - 1 when there is none), for a wave-uniform u, by the whole wave: the running
// totals do not decrease, so it is the number of entries <= u -- one or two ballots instead of a binary search
// of seven dependent LDS reads
__device__ __forceinline__ int first_above(const int32_t *end, int n, int u)
{
    const int lane = threadIdx.x & 63;
    int below = 0;
    for(int base = 0; base < n; base += 64) {
        const int k = base + lane;
        below += __popcll(__ballot(k < n && end[k] <= u));
    }
    return min(below, n - 1);
}

// Drawing work units, every wave on its own (no workgroup barrier: a wave that holds a long unit does
// not keep its neighbours waiting).  The units are numbered heaviest first.  All but the last one to
// two rounds are dealt out statically -- wave w takes units w, w + nw, ... : every wave gets the same
// mix of heavy and light ones, and no atomics --; the rest, the lightest units, are drawn by ticket and
// fill the gaps the uneven ones left.  Ticket unit v belongs to stripe v % NH_CP_STRIPES; a wave draws
// from its stripe's counter (one unit per ticket) and moves on to the next stripe when one is
// exhausted.  (One counter for everything was an atomic on ONE address per unit, ~5 ns each in a row,
// and two memory round trips before every unit -- more than the light units themselves cost; purely
// static dealing left the chip waiting for the unluckiest waves.)  The stripes' counters lie in
// separate 128-byte lines; a counter seen exhausted by a plain load is not drawn from again.
// Returns -1 when nothing is left.
struct unit_draw { int stripe, abandoned, round; };
__device__ __forceinline__ int next_unit(unit_draw &D, int32_t *counters, int total, int gw, int nw, int lane)
{
#define NH_CP_TICKET_ROUNDS 1
    const int static_rounds = max(0, total / nw - NH_CP_TICKET_ROUNDS);
    const int r = D.round++;
    if(r < static_rounds) return gw + r * nw;
    if(r == static_rounds) { D.stripe = gw % NH_CP_STRIPES; D.abandoned = 0; }
    const int first = static_rounds * nw, rest = total - first;       // ticket units: first .. total-1
    while(D.abandoned < NH_CP_STRIPES) {
        const int st = D.stripe;
        const int n_s = st < rest ? (rest - st + NH_CP_STRIPES - 1) / NH_CP_STRIPES : 0;
        int32_t *cnt = counters + 32 * st;
        if(__atomic_load_n(cnt, __ATOMIC_RELAXED) < n_s) {
            int t = 0;
            if(lane == 0) t = atomicAdd(cnt, 1);
            t = __builtin_amdgcn_readfirstlane(t);
            if(t < n_s) return first + t * NH_CP_STRIPES + st;
        }
        D.stripe = (st + 1) % NH_CP_STRIPES;
        D.abandoned++;
    }
    return -1;
}


// ---- k_cp_small: the lists of 1-2 and 3-4 neighbours -- three quarters of the searching agents
// outside a crowd.  One wave per unit of four agents, one attempt each (clearpath_small_row); an agent
// without any admissible candidate goes onto the retry list, which a launch of k_cp_rows works off. ----
#define CPS_WAVES 4          /* waves (units) per workgroup */
__global__ __launch_bounds__(CPS_WAVES * 64) void k_cp_small(nh_step_params P, nh_nbr NB, const nh_mid_rec *mid,
                                                            nh_worklists WL, nh_step_outs O)
{
    __shared__ __attribute__((aligned(16))) float4 cones[CPS_WAVES * 4][8];
    __shared__ int32_t unit_end[2 * NH_WL_SUB];
    __shared__ int32_t sub_cnt[2 * NH_WL_SUB];
    const int wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for(int k = threadIdx.x; k < 2 * NH_WL_SUB; k += CPS_WAVES * 64)
        sub_cnt[k] = WL.count[(NH_WL_ROW1 - k / NH_WL_SUB) * NH_WL_SUB + k % NH_WL_SUB];
    __syncthreads();
    unit_totals(unit_end, 2 * NH_WL_SUB, [&](int k) { return (sub_cnt[k] + 3) >> 2; });
    __syncthreads();
    const int u = blockIdx.x * CPS_WAVES + wib;               // one unit per wave
    bool live = u < unit_end[2 * NH_WL_SUB - 1];
    int uid = 0;
    bool found = true;
    if(live) {
        const int k = first_above(unit_end, 2 * NH_WL_SUB, u), rel = u - (k ? unit_end[k - 1] : 0);
        const int list = NH_WL_ROW1 - k / NH_WL_SUB, sub = k % NH_WL_SUB;
        const int idx = rel * 4 + (lane >> 4);
        live = idx < sub_cnt[k];                                // (else: a row beyond the end of its sub-list)
        if(live) {
            uid = WL.ids[((size_t)list * NH_WL_SUB + sub) * WL.cap + idx];
            const nh_mid_rec R = mid[uid];
            const uint32_t c = NB.cnt[uid];
            const int n_dyn = (int)(c & 0xff), n_stat = (int)((c >> 8) & 0xff);
            cpent ent;
            ent.pos = mkv(P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1]);
            ent.vel = mkv(P.vel_xz[2 * uid], P.vel_xz[2 * uid + 1]);
            ent.radius = P.radius[uid];
            const int gl = lane & 15;
            const bool have = gl < n_dyn + n_stat, isdyn = gl < n_dyn;
            cpent nb; nb.pos = mkv(0, 0); nb.vel = mkv(0, 0); nb.radius = 0;
            if(have) nb = nbr_load(NB, uid, isdyn ? gl : 32 + gl - n_dyn);
            const v2 nv = clearpath_small_row(ent, mkv(R.vpref[0], R.vpref[1]), nb, isdyn, have,
                                              cones[wib * 4 + (lane >> 4)], found);
            if(found && gl == 0)
                post_thread(P, uid, ent.pos, P.state[uid], P.flags[uid], ent.radius, nv, R.vel_cap, R.status, O);
        }
    }
    worklist_push(WL, NH_WL_RETRY, live && !found && (lane & 15) == 0, uid);
}

// ---- k_cp_rows: the four row lists (1-16 neighbours), a row of 16 lanes per agent, four agents per
// unit, the units numbered heaviest list first (9-16, 5-8, 3-4, 1-2 neighbours) ---------------------
// (the lists list0, list0 - 1, ... : nlists of them, at most four; ticket_set: which set of stripe
// counters -- the retry launch runs beside the main one)
#define CP_ROWS_OCC 4           /* (pinned like k_cp_heavy: four waves per SIMD, 128 registers -- see the note on hole inheritance below) */
__attribute__((amdgpu_waves_per_eu(CP_ROWS_OCC, CP_ROWS_OCC)))
__global__ __launch_bounds__(CPR_WAVES * 64) void k_cp_rows(nh_step_params P, nh_nbr NB, const nh_mid_rec *mid,
                                                           nh_worklists WL, nh_step_outs O, int list0, int nlists,
                                                           int ticket_set, nh_signal lists_ready)
{
    // (this launch follows k_agent_mid on its stream: that it runs says the work lists are complete)
    if(lists_ready.flag && blockIdx.x == 0 && threadIdx.x == 0) {
#ifdef NH_HOSTSIM
        *lists_ready.flag = lists_ready.seq;
#else
        __hip_atomic_store(lists_ready.flag, lists_ready.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
    __shared__ cp_lds<16> lds[CPR_WAVES * 4];
    // unit_end[k] = units of the sub-lists up to and including k (k = order * NH_WL_SUB + sub)
    __shared__ int32_t unit_end[4 * NH_WL_SUB];
    __shared__ int32_t sub_cnt[4 * NH_WL_SUB];
    // HOLE INHERITANCE (profiles/HISTORY.md 3.7).  This launch reaches the device a few microseconds before k_cp_heavy (which waits
    // for an event of the other stream) and fills every SIMD; k_cp_heavy's persistent workgroups move into the
    // register and LDS ranges its workgroups leave behind and keep them for the whole launch.  A hole smaller than a
    // k_cp_heavy wave (128 registers) or workgroup is lost to it: 119 instead of 121 registers here (120 instead of
    // 128 allocated), or 37.5 KB of LDS there against 36 here, cost the crowded world a quarter of k_cp_heavy's
    // waves (4.9 -> 6.1 ms per tick, profiles/archive/r04_ab_hole_inheritance.txt).  So: this kernel allocates the same 128
    // registers per lane (v127 named as clobbered), and its workgroup owns at least k_cp_heavy's LDS.
    asm volatile("" ::: "v127");
    static_assert(sizeof(cp_lds<16>) * CPR_WAVES * 4 + 8 * 4 * NH_WL_SUB >= sizeof(cp_lds<64>) * CP_WAVES + 8 * NH_WL_SUB + 4 + sizeof(cp_team),
                  "k_cp_rows' workgroup must own at least k_cp_heavy's LDS (hole inheritance)");
    const int wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ntab = nlists * NH_WL_SUB;
    // (usually nothing to do for the retry launch: one parallel look)
    if(nlists == 1 && !__any(WL.count[list0 * NH_WL_SUB + lane] != 0)) return;
    for(int k = threadIdx.x; k < ntab; k += CPR_WAVES * 64)
        sub_cnt[k] = WL.count[(list0 - k / NH_WL_SUB) * NH_WL_SUB + k % NH_WL_SUB];
    __syncthreads();
    unit_totals(unit_end, ntab, [&](int k) { return (sub_cnt[k] + 3) >> 2; });
    __syncthreads();
    const int total = unit_end[ntab - 1];
    int32_t *counters = WL.count + NH_WL_LISTS * NH_WL_SUB + 32 * (1 + ticket_set * NH_CP_STRIPES);
    const int gw = blockIdx.x * CPR_WAVES + wib, nw = gridDim.x * CPR_WAVES;
    cp_lds<16> &S = lds[wib * 4 + (lane >> 4)];
    unit_draw D; D.round = 0;
    for(;;) {
        const int u = next_unit(D, counters, total, gw, nw, lane);
        if(u < 0) break;
        const int k = first_above(unit_end, ntab, u), rel = u - (k ? unit_end[k - 1] : 0);
        const int list = list0 - k / NH_WL_SUB, sub = k % NH_WL_SUB;
        const int idx = rel * 4 + (lane >> 4);
        if(idx < sub_cnt[k]) {                  // (else: a row beyond the end of its sub-list)
            const int uid = WL.ids[((size_t)list * NH_WL_SUB + sub) * WL.cap + idx];
            const nh_mid_rec R = mid[uid];
            const uint32_t c = NB.cnt[uid];
            const int n_dyn = (int)(c & 0xff), n_stat = (int)((c >> 8) & 0xff);
            cpent ent;
            ent.pos = mkv(P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1]);
            ent.vel = mkv(P.vel_xz[2 * uid], P.vel_xz[2 * uid + 1]);
            ent.radius = P.radius[uid];
            cp_load_lists<16>(P.grid, NB, uid, n_dyn, n_stat, S);
            const v2 nv = clearpath_grp<16>(ent, mkv(R.vpref[0], R.vpref[1]), n_dyn, n_stat, S);
            if((lane & 15) == 0)
                post_thread(P, uid, ent.pos, P.state[uid], P.flags[uid], ent.radius, nv, R.vel_cap, R.status, O);
        }
    }
}

// ---- k_cp_heavy: the heavy list (33-64 neighbours), then the wave list (17-32).  A search of up to 16 000 ray
// pairs on one wave takes hundreds of microseconds -- as long as everything else of the tick --, and even among
// problems of 20-30 neighbours the cost spreads over a factor of ten (how early an admissible candidate turns up
// decides how much is pruned).  So: one problem per WORKGROUP, its waves search it as a team (clearpath_grp<64, true>)
// -- the launch is bound by its LONGEST problems, and a team quarters every problem's latency.  In a jam, from
// CP_SOLO_MIN problems on (92 000 in the crowded world), there are more problems than waves, the load balances over
// problems, and a team would only repeat the cone / rank construction four times: every WAVE takes a problem of its
// own, its first one by wave number, then a ticket per wave and problem.  (A two-pass schedule -- every wave on its
// own, searches that find no bound handed over to teams -- was measured and lost: profiles/archive/r04_ab_cp_bail_100.txt.)
#define CP_HEAVY_OCC 4          /* (pinned: a few registers above 128 would silently cost a wave per SIMD) */
__attribute__((amdgpu_waves_per_eu(CP_HEAVY_OCC, CP_HEAVY_OCC)))
__global__ __launch_bounds__(CP_WAVES * 64) void k_cp_heavy(nh_step_params P, nh_nbr NB, const nh_mid_rec *mid,
                                                            nh_worklists WL, nh_step_outs O, int32_t *zero_next)
{
    __shared__ cp_lds<64> lds[CP_WAVES];
    __shared__ int32_t hv_end[2 * NH_WL_SUB];       // sub-lists of the heavy list, then of the wave list
    __shared__ int32_t h_ticket;
    __shared__ cp_team team;
    const int wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // The last launch of the step on the side stream clears the OTHER set of list counters for the next step.
    // On THIS stream because the library copies every step's counters to pinned host memory behind the step, on
    // this stream too (navhip_step_lists_peek): the clearing of a set is ordered behind the copy of that set by the
    // stream itself.  (Its users -- the previous step -- finished before this step's k_agent_mid started.)
    if(blockIdx.x == 0 && zero_next)
        for(int i = threadIdx.x; i < (int)NH_WL_COUNTERS; i += CP_WAVES * 64) zero_next[i] = 0;
    cp_lds<64> &S = lds[wib];
    // (outside a crowd there is nothing to do: one parallel look at the 128 counters)
    if(!__any((WL.count[NH_WL_HEAVY * NH_WL_SUB + lane] | WL.count[NH_WL_WAVE * NH_WL_SUB + lane]) != 0)) return;
    unit_totals(hv_end, 2 * NH_WL_SUB, [&](int k) {
        return WL.count[(k < NH_WL_SUB ? NH_WL_HEAVY : NH_WL_WAVE) * NH_WL_SUB + k % NH_WL_SUB]; });
    __syncthreads();
    const int n_heavy = hv_end[2 * NH_WL_SUB - 1];
    int32_t *ticket = WL.count + NH_WL_LISTS * NH_WL_SUB;
    if(n_heavy >= CP_SOLO_MIN) {
        // ---- a jam: one problem per wave
        const int nw = (int)gridDim.x * CP_WAVES;
        for(int round = 0; ; round++) {
            int t = (int)blockIdx.x * CP_WAVES + wib;
            if(round > 0) {
                int v = 0x7fffffff;
                if(lane == 0 && nw + __atomic_load_n(ticket, __ATOMIC_RELAXED) < n_heavy) v = nw + atomicAdd(ticket, 1);
                t = __shfl(v, 0);
            }
            if(t >= n_heavy) break;
            const int k = first_above(hv_end, 2 * NH_WL_SUB, t), idx = t - (k ? hv_end[k - 1] : 0);
            const int uid = WL.ids[((size_t)(k < NH_WL_SUB ? NH_WL_HEAVY : NH_WL_WAVE) * NH_WL_SUB + k % NH_WL_SUB) * WL.cap + idx];
            const nh_mid_rec R = mid[uid];
            const uint32_t c = NB.cnt[uid];
            const int n_dyn = (int)(c & 0xff), n_stat = (int)((c >> 8) & 0xff);
            cpent ent;
            ent.pos = mkv(P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1]);
            ent.vel = mkv(P.vel_xz[2 * uid], P.vel_xz[2 * uid + 1]);
            ent.radius = P.radius[uid];
            cp_load_lists<64>(P.grid, NB, uid, n_dyn, n_stat, S);
            const v2 nv = clearpath_grp<64>(ent, mkv(R.vpref[0], R.vpref[1]), n_dyn, n_stat, S);
            if(lane == 0)
                post_thread(P, uid, ent.pos, P.state[uid], P.flags[uid], ent.radius, nv, R.vel_cap, R.status, O);
        }
        return;
    }
    // ---- one problem per workgroup
    for(int round = 0; ; round++) {
        int t = blockIdx.x;
        if(round > 0) {
            __syncthreads();
            if(threadIdx.x == 0) {
                int v = 0x7fffffff;
                if((int)gridDim.x + __atomic_load_n(ticket, __ATOMIC_RELAXED) < n_heavy)
                    v = (int)gridDim.x + atomicAdd(ticket, 1);
                h_ticket = v;
            }
            __syncthreads();
            t = h_ticket;
        }
        if(t >= n_heavy) break;
        const int k = first_above(hv_end, 2 * NH_WL_SUB, t), idx = t - (k ? hv_end[k - 1] : 0);
        const int uid = WL.ids[((size_t)(k < NH_WL_SUB ? NH_WL_HEAVY : NH_WL_WAVE) * NH_WL_SUB + k % NH_WL_SUB) * WL.cap + idx];
        const nh_mid_rec R = mid[uid];
        const uint32_t c = NB.cnt[uid];
        const int n_dyn = (int)(c & 0xff), n_stat = (int)((c >> 8) & 0xff);
        cpent ent;
        ent.pos = mkv(P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1]);
        ent.vel = mkv(P.vel_xz[2 * uid], P.vel_xz[2 * uid + 1]);
        ent.radius = P.radius[uid];
        const v2 vpref = mkv(R.vpref[0], R.vpref[1]);
        cp_load_lists<64>(P.grid, NB, uid, n_dyn, n_stat, S);
        const v2 nv = clearpath_grp<64, true>(ent, vpref, n_dyn, n_stat, S, wib, CP_WAVES, &team);
        if(wib == 0 && lane == 0)
            post_thread(P, uid, ent.pos, P.state[uid], P.flags[uid], ent.radius, nv, R.vel_cap, R.status, O);
    }
}

// ---------------------------------------------------------------------------------------------
// k_agent_full: one WAVE per listed agent, the whole neighbour-dependent part on the wave: r = 30
// query + garrison filter + separation, the priority ladder, r = 10 neighbours, ClearPath.
// (The exact path for what the row walk declines.)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AG_WAVES * 64) void k_agent_full(nh_step_params P, const float *coh_xz,
                                                              const nh_mid_rec *mid, nh_worklists WL,
                                                              nh_step_outs O, float scaled_max_force,
                                                              double force_thresh, int32_t *zero_next)
{
    __shared__ wave_lds lds[AG_WAVES];
    __shared__ cp_lds<64> cps[AG_WAVES];
    __shared__ double exp_tab[64];
    const int wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // (zero_next: the other set of list counters, when this launch is the one that clears it -- k_cp_heavy is)
    if(blockIdx.x == 0 && zero_next)
        for(int i = threadIdx.x; i < (int)NH_WL_COUNTERS; i += AG_WAVES * 64) zero_next[i] = 0;
    // usually there is nothing to do: one parallel look at the 64 sub-list counters
    if(!__any(WL.count[NH_WL_FULL * NH_WL_SUB + lane] != 0)) return;
    if(threadIdx.x < 64) exp_tab[threadIdx.x] = c_exp2_64[threadIdx.x];
    __syncthreads();
    wave_lds &W = lds[wib];
    cp_lds<64> &S = cps[wib];
    const nh_grid &G = P.grid;
    for(int sub = 0; sub < NH_WL_SUB; sub++) {
    const int count = WL.count[NH_WL_FULL * NH_WL_SUB + sub];
    for(int idx = blockIdx.x * AG_WAVES + wib; idx < count; idx += gridDim.x * AG_WAVES) {
        const int uid = WL.ids[((size_t)NH_WL_FULL * NH_WL_SUB + sub) * WL.cap + idx];
        const nh_mid_rec R = mid[uid];
        const uint32_t my_slot = (uint32_t)G.pool_of[uid];
        const uint32_t my_bits = slot_bits(G, my_slot);
        const v2 me = mkv(P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1]);
        const v2 vel = mkv(P.vel_xz[2 * uid], P.vel_xz[2 * uid + 1]);
        const float my_radius = P.radius[uid];
        int n30raw = -1;                 // size of the unfiltered r=30 list (-1: no such query)
        v2 vpref = mkv(0.0f, 0.0f);
        wave_sync();
        if(R.mode != AM_ZERO_VPREF) {
            // separation (movement.c:1690): r = 30 query, cap 128
            int n30 = sp_query_wave(G, me.x, me.z, 30.0f, 128, W.ids30, lane, W.d2_30);
            wave_sync();
            n30raw = n30;
            const int n10d = derive_r10(G, me, W.ids30, W.d2_30, n30raw, W.ids10d, lane);
            n30 = filter_garrisoned_wave(G, W.ids30, n30, lane);
            if(n10d < 0) n30raw = -1; else n30raw = n10d;
            const v2 separation = separation_wave(G, my_slot, me, my_radius, my_bits, W.ids30, n30,
                                                  W.u.sep, scaled_max_force, lane, exp_tab);
            vpref = vpref_from_forces(P, uid, R.mode, me, vel, P.flock[uid], mkv(R.arrive[0], R.arrive[1]),
                                      separation, R.probes, coh_xz, scaled_max_force, force_thresh);
        }
        // find_neighbours :2768: r = 10 query, cap 512 -- taken from the r = 30 list when that list
        // is complete (n30raw now holds the derived count, -1 = not derivable)
        uint32_t *ids10 = W.u.ids10;
        int n10;
        if(n30raw >= 0) {
            ids10 = W.ids10d;
            n10 = n30raw;
        }else{
            n10 = sp_query_wave(G, me.x, me.z, 10.0f, 512, W.u.ids10, lane);
            wave_sync();
        }
        n10 = filter_garrisoned_wave(G, ids10, n10, lane);
        int n_dyn, n_stat;
        classify_neighbours(G, my_slot, my_bits, ids10, n10, S.dyn, n_dyn, S.stat, n_stat, lane);
        cpent ent; ent.pos = me; ent.vel = vel; ent.radius = my_radius;
        const v2 nv = clearpath_grp<64>(ent, vpref, n_dyn, n_stat, S);
        if(lane == 0) {
            if(O.vpref_xz) { O.vpref_xz[2 * uid] = vpref.x; O.vpref_xz[2 * uid + 1] = vpref.z; }
            post_thread(P, uid, me, P.state[uid], P.flags[uid], my_radius, nv, R.vel_cap, R.status, O);
        }
    }
    }
}

// ---------------------------------------------------------------------------------------------
// test / utility kernels
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_spatial_query(nh_grid G, const float *query_xz, int nq,
                                                       float range, int maxout, int32_t *out_counts,
                                                       uint32_t *out_ids)
{
    const int q = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if(q >= nq) return;
    uint32_t *mine = out_ids + (size_t)q * maxout;
    int n = sp_query_wave(G, query_xz[2 * q], query_xz[2 * q + 1], range, maxout, mine, lane);
    wave_sync();
    for(int k = lane; k < n; k += 64) mine[k] = slot_bits(G, mine[k]) >> NH_PB_UID_SHIFT;   // slot -> uid
    if(lane == 0) out_counts[q] = n;
}

// N_DesiredGroupArrivalVelocity (nav.c:3561): direction under each point in the chunk field of its mapping
// row + "the tile is a sink inside the zone's disc" (:3596-3600)
__global__ __launch_bounds__(256) void k_region_lookup(nh_step_params P, int nq, const float *pos, const int32_t *rows,
                                                       const int32_t *centre_abs, const int32_t *radius,
                                                       uint8_t *out_dir, uint8_t *out_at_slot)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if(q >= nq) return;
    uint8_t dir = 0xff, at = 0;
    tiledesc t;
    const int row = rows[q];
    if(row >= 0 && tile_for_point(P, pos[2 * q], pos[2 * q + 1], t)) {
        const int slot = P.region_field_slot[(size_t)row * (P.map.w * P.map.h) + t.chunk_r * P.map.w + t.chunk_c];
        if(slot >= 0) {
            dir = P.field_pool[((size_t)slot << 12) + t.tile_r * 64 + t.tile_c] & 0xf;
            if(dir == NAVHIP_FD_NONE && centre_abs) {
                // M_Tile_Distance(res, &centre_tile, &tile, &dr, &dc), tile.c:414
                const int dr = (t.chunk_r * 64 + t.tile_r) - centre_abs[2 * q];
                const int dc = (t.chunk_c * 64 + t.tile_c) - centre_abs[2 * q + 1];
                at = (dr * dr + dc * dc) <= radius[q] * radius[q];
            }
        }
    }
    out_dir[q] = dir;
    if(out_at_slot) out_at_slot[q] = at;
}

void nh_launch_region_lookup(const nh_step_params &P, int nq, const float *d_pos, const int32_t *d_rows,
                             const int32_t *d_centre_abs, const int32_t *d_radius, uint8_t *d_dir, uint8_t *d_at_slot,
                             hipStream_t s)
{
    if(nq > 0)
        hipLaunchKernelGGL(k_region_lookup, dim3((nq + 255) / 256), dim3(256), 0, s, P, nq, d_pos, d_rows, d_centre_abs,
                           d_radius, d_dir, d_at_slot);
}

// G_ClearPath_NewVelocity for nq independent problems on groups of GW lanes (GW = 64: any problem;
// GW = 16: n_dyn + n_stat <= 16 -- the row path of the agent step)
template <int GW>
__global__ __launch_bounds__(128) void k_clearpath(int nq, const float *ent, const float *des_v,
                                                   const float *dyn, const int32_t *n_dyn,
                                                   const float *stat, const int32_t *n_stat,
                                                   float *out)
{
    __shared__ cp_lds<GW> lds[128 / GW];
    const int gi = threadIdx.x / GW, gl = threadIdx.x & (GW - 1);
    const int q = uni<GW>((int)(blockIdx.x * (128 / GW) + gi));           // (a wave-wide group: the same in every lane)
    if(q >= nq) return;
    cp_lds<GW> &S = lds[gi];
    const int nd = n_dyn[q], ns = n_stat[q];
    for(int i = gl; i < nd * 5; i += GW) S.dyn[i] = dyn[(size_t)q * 160 + i];
    for(int i = gl; i < ns * 5; i += GW) S.stat[i] = stat[(size_t)q * 160 + i];
    wave_sync();
    cpent e; e.pos = mkv(ent[5 * q], ent[5 * q + 1]); e.vel = mkv(ent[5 * q + 2], ent[5 * q + 3]);
    e.radius = ent[5 * q + 4];
    const v2 r = clearpath_grp<GW>(e, mkv(des_v[2 * q], des_v[2 * q + 1]), nd, ns, S);
    if(gl == 0) { out[2 * q] = r.x; out[2 * q + 1] = r.z; }
}

// the same for a team of CP_WAVES waves per problem (what k_cp_heavy runs)
__global__ __launch_bounds__(CP_WAVES * 64) void k_clearpath_team(int nq, const float *ent, const float *des_v,
                                                                  const float *dyn, const int32_t *n_dyn,
                                                                  const float *stat, const int32_t *n_stat,
                                                                  float *out)
{
    __shared__ cp_lds<64> lds[CP_WAVES];
    __shared__ cp_team team;
    const int wib = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x;
    cp_lds<64> &S = lds[wib];
    const int nd = n_dyn[q], ns = n_stat[q];
    for(int i = lane; i < nd * 5; i += 64) S.dyn[i] = dyn[(size_t)q * 160 + i];
    for(int i = lane; i < ns * 5; i += 64) S.stat[i] = stat[(size_t)q * 160 + i];
    wave_sync();
    cpent e; e.pos = mkv(ent[5 * q], ent[5 * q + 1]); e.vel = mkv(ent[5 * q + 2], ent[5 * q + 3]);
    e.radius = ent[5 * q + 4];
    const v2 r = clearpath_grp<64, true>(e, mkv(des_v[2 * q], des_v[2 * q + 1]), nd, ns, S, wib, CP_WAVES, &team);
    if(threadIdx.x == 0) { out[2 * q] = r.x; out[2 * q + 1] = r.z; }
}

// ClearPath retry statistics (developer diagnostics: scripts/, bench.py --cp-stats)
extern "C" int navhip_debug_cp_attempts(unsigned long long out[9], int reset)
{
    if(hipDeviceSynchronize() != hipSuccess) return 1;
    if(hipMemcpyFromSymbol(out, HIP_SYMBOL(nh_cp_attempts), 9 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if(reset) {
        unsigned long long z[9] = {0};
        if(hipMemcpyToSymbol(HIP_SYMBOL(nh_cp_attempts), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}



// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
void nh_launch_agent_nbr(const nh_step_params &P, const nh_nbr &NB, hipStream_t s)
{
    if(P.n_ents > 0 && P.work_end > P.work_begin) {
        const float smf = (float)((double)(0.75f / (float)P.hz) * 20.0);
        const int slab = P.work_end - P.work_begin;
        if(slab == P.n_ents) {
            hipLaunchKernelGGL(k_agent_nbr<false>, dim3((P.n_ents + NBR_BLOCK / 16 - 1) / (NBR_BLOCK / 16)), dim3(NBR_BLOCK), 0, s,
                               P.grid, P.n_ents, NB, smf);
        }else{
            // a row per entity of the slab (the list of k_sp_place holds at most that many)
            const int rows = slab;
            hipLaunchKernelGGL(k_agent_nbr<true>, dim3((rows + NBR_BLOCK / 16 - 1) / (NBR_BLOCK / 16)), dim3(NBR_BLOCK), 0, s,
                               P.grid, P.n_ents, NB, smf);
        }
    }
}

// entries a sub-list can receive: its producers are the k_agent_mid waves with index = sub (mod NH_WL_SUB), each of
// which steps 64 entities
int nh_worklist_cap(int n_work)
{
    const int waves = (n_work + 63) / 64;
    // (+ 16: the retry list is filled by k_cp_small's waves -- four entries each, a few more of them per
    // sub-list than there are k_agent_mid waves' worth)
    return ((waves + NH_WL_SUB - 1) / NH_WL_SUB) * 64 + 16;
}

// k_agent_mid + the consumers of its work lists.  The list counters alternate between two sets:
// a launch sequence uses one and zeroes the other for its successor (no memset on the stream).
// Returns whether anything was launched (the caller flips the parity only then: a step that launches nothing
// does not clear the other set either); *forked: the second chain went onto `side`, so NH_HO_MID says when the work lists
// were complete and NH_HO_END when the step had ended on s.
bool nh_launch_agent_finish(const nh_step_params &P, const nh_nbr &NB, float *d_coh, nh_mid_rec *d_mid,
                            nh_worklists WL, int parity, const nh_step_outs &O, hipStream_t s,
                            hipStream_t side, navhip_ctx *ctx, bool *forked)
{
    const int nwork = P.work_end - P.work_begin;
    if(!(P.n_ents > 0 && nwork > 0)) return false;
    // SCALED_MAX_FORCE and the 1 % force threshold of movement.c:1870-1905 (same for every agent)
    const float smf = (float)((double)(0.75f / (float)P.hz) * 20.0);
    const double thresh = ((double)(0.75f / (float)P.hz) * 20.0) * 0.01;
    int32_t *zero_next = WL.count + (parity ^ 1) * NH_WL_COUNTERS;
    WL.count += parity * NH_WL_COUNTERS;
    hipLaunchKernelGGL(k_agent_mid, dim3((nwork + 63) / 64), dim3(64), 0, s, P, NB, (const float*)d_coh, d_mid, WL, O, smf, thresh);
    // the ClearPath launches.  s: the rows of 5-16 neighbours, the irregular agents.  side: the agents with 1-4
    // neighbours (most of them, outside a crowd), whatever of them needs the retry logic, then the workgroup problems
    // (17-64 neighbours).  Every wave / workgroup keeps drawing units until none are left.  (The workgroup problems on
    // a third stream beside the small ones were measured and lost -- one more fork and join on the agent stream, and in
    // a jam the searches race k_cp_rows for the chip instead of inheriting it: profiles/archive/r04_ab_cp_three_streams.txt.)
    // side: the fork.  Its hand-overs go through device memory (stream_set.hip): k_cp_rows -- it follows k_agent_mid on s --
    // stores "the work lists are complete" when it starts, and a one-lane kernel in front of k_cp_small waits for that.
    const bool fork = side != nullptr && side != s;
    hipStream_t sh = fork ? side : s;
    const nh_signal lists_ready = fork ? nh_handover_by_kernel(ctx, NH_HO_MID, s) : nh_signal{nullptr, 0};
    *forked = fork;
    const int nblk = min(4096 / CP_WAVES, (nwork + 15) / 16 + 1);      // 4096 persistent waves: four per SIMD
    const int nblk_rows = min(4096 / CPR_WAVES, (nwork + 15) / 16 * (CP_WAVES / CPR_WAVES) + 1);
    // (the rows first: behind a host that is not ahead of the device -- the tick after a synchronisation -- every
    // launch in front of it delays its start by one enqueue)
    hipLaunchKernelGGL(k_cp_rows, dim3(nblk_rows), dim3(CPR_WAVES * 64), 0, s, P, NB, (const nh_mid_rec*)d_mid, WL, O,
                       (int)NH_WL_ROW3, 2, 0, lists_ready);
    if(fork) nh_handover_wait(ctx, NH_HO_MID, sh);
    hipLaunchKernelGGL(k_cp_small, dim3((nwork / 4 + 2 * NH_WL_SUB + CPS_WAVES - 1) / CPS_WAVES + 1), dim3(CPS_WAVES * 64), 0, sh, P, NB,
                       (const nh_mid_rec*)d_mid, WL, O);
    hipLaunchKernelGGL(k_cp_rows, dim3(64 * CP_WAVES / CPR_WAVES), dim3(CPR_WAVES * 64), 0, sh, P, NB, (const nh_mid_rec*)d_mid, WL, O,
                       (int)NH_WL_RETRY, 1, 1, nh_signal{nullptr, 0});
    // (the last launch on `side` clears the other set of list counters: see k_cp_heavy)
    hipLaunchKernelGGL(k_cp_heavy, dim3(nblk), dim3(CP_WAVES * 64), 0, sh, P, NB, (const nh_mid_rec*)d_mid, WL, O, zero_next);
    if(fork) nh_handover_signal(ctx, NH_HO_CP, sh);
    hipLaunchKernelGGL(k_agent_full, dim3(min(1024, (nwork + AG_WAVES - 1) / AG_WAVES)), dim3(AG_WAVES * 64), 0, s, P,
                       (const float*)d_coh, (const nh_mid_rec*)d_mid, WL, O, smf, thresh, (int32_t*)nullptr);
    // the join; the waiting kernel also says that the step has ended on s: a prefetch that follows directly starts its
    // side streams behind that (NAVHIP_PREFETCH_FOLLOWS_STEP)
    if(fork) nh_handover_wait(ctx, NH_HO_CP, s, -1, NH_HO_END);
    return true;
}

void nh_launch_spatial_query(const nh_grid &G, const float *d_query, int nq, float range, int maxout,
                             int32_t *d_counts, uint32_t *d_ids, hipStream_t s)
{
    if(nq > 0)
        hipLaunchKernelGGL(k_spatial_query, dim3((nq + 3) / 4), dim3(256), 0, s, G, d_query, nq, range,
                           maxout, d_counts, d_ids);
}

void nh_launch_clearpath(int nq, const float *ent, const float *des_v, const float *dyn,
                         const int32_t *n_dyn, const float *stat, const int32_t *n_stat, float *out,
                         int rows, hipStream_t s)
{
    if(nq <= 0) return;
    if(rows == 2)
        hipLaunchKernelGGL(k_clearpath_team, dim3(nq), dim3(CP_WAVES * 64), 0, s, nq, ent, des_v, dyn,
                           n_dyn, stat, n_stat, out);
    else if(rows)
        hipLaunchKernelGGL(k_clearpath<16>, dim3((nq + 7) / 8), dim3(128), 0, s, nq, ent, des_v, dyn,
                           n_dyn, stat, n_stat, out);
    else
        hipLaunchKernelGGL(k_clearpath<64>, dim3((nq + 1) / 2), dim3(128), 0, s, nq, ent, des_v, dyn,
                           n_dyn, stat, n_stat, out);
}
