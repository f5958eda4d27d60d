// surround_query_kernels.hip -- the two unit queries of STATE_SURROUND_ENTITY (movement.c:2509-2567) on the device, for a
// MOVABLE target (a circle) and for a static one (a building: the tile list of its OBB, registered once):
// M_NavObjAdjacentFrom (map.c:1061 -> N_ObjAdjacentToDynamicWith, nav.c:4965 -> n_objects_adjacent, nav.c:1682) and
// M_NavClosestReachableAdjacentPosFrom (map.c:860 -> N_ClosestReachableAdjacentPosDynamic, nav.c:4637 ->
// n_closest_adjacent_pos, nav.c:1636) from both positions the tick can test; for a static target N_ObjAdjacentToStaticWith
// (nav.c:4932) and N_ClosestReachableAdjacentPosStatic (nav.c:4621), which end in the same two functions over the list
// M_Tile_AllUnderObj (tile.c:594) returned.  The kernels, their launches, the entry points
// (navhip_surround_queries[_ex][_dev]) and the resident table of static tile lists (navhip_static_targets_set) live here;
// nothing else launches them.  They read the probemask rows and the islands plane, as the destination queries do, and
// write the shapes of navhip_state_aux_in.surround_query / .surround_dest_xz.
//
// k_surround_rows   one wave per row.  Decides what needs no flood: no target, NAVHIP_SQ_HOST, touching.  Both circles'
//                   tile sets (M_Tile_AllUnderCircle, tile.c:687) are bit windows centred on the target's tile (lane =
//                   window row, as k_blockers_circles holds them); n_objects_adjacent's pair test is one 8-neighbour
//                   dilation of the target's set and an AND.  A row that goes on leaves its record -- the target's tiles,
//                   both sources and their islands -- and appends one work item per target tile.
// k_surround_flood  one wave per work item (row, target tile), a fixed grid striding over the list: the flood of
//                   n_closest_island_tiles with maxout = 1 (dq_flood_first, nav_flood.h) for source 0's island, and a
//                   second one only when source 1's island differs.  Leaves the answer tile, "none" or "window".
// k_surround_pick   one wave per row: the minimum of n_closest_adjacent_pos over the tile answers in M_Tile_AllUnderCircle
//                   order.  Lengths are non-negative floats, so (bits of the length, tile index) compares as integers and
//                   the lowest pair is the reference's strict-< winner: of equal lengths the earlier target tile.
// Every kernel is built twice: ST = false is the form without a table (navhip_surround_queries[_dev], or no set
// registered) -- a row's work items and answers are indexed by the tile of the 17 x 17 window, SQ_TILES per row.  ST = true
// adds the static rows: their work items and answers are indexed by the LIST INDEX of the row's set (the list is the four
// outline supercovers and then the interior, not row-major: a bit window would lose the order the pick needs), and a row
// takes `stride` = max(SQ_TILES, the longest registered list) slots.  The touching test of a static row holds the unit's
// circle as bit rows centred on the unit's tile, dilates it once and lets the lanes stride over the list.
// Floods are not shared between rows: units that surround one target from one island repeat each other's.
#include <hip/hip_runtime.h>
#include <math.h>
#include "navhip_internal.h"
#include "stage_plan.h"
#include "agent_internal.h"
#include "agent_math.h"         // nav_layer_for
#include "lane_group.h"
#include "wave_bits.h"
#include "nav_flood.h"
#include "circle_tiles.h"
#include <algorithm>
#include <string>
#include <vector>

#define SQ_NT      8                        /* ceil(radius / 4) of unit and target: at most this (radius 32)       */
#define SQ_SIDE    (2 * SQ_NT + 1)          /* the window M_Tile_AllUnderCircle scans: 17 x 17 tiles, row-major    */
#define SQ_TILES   (SQ_SIDE * SQ_SIDE)      /* 289, far below the reference's cap of 2048 (nav.c:4647)             */
#define SQ_FLOOD_BLOCKS 4096                /* the grid of k_surround_flood                                        */
#define SQ_NONE    0xffffffffu              /* a tile answer: the flood visited the whole map without a hit        */
#define SQ_WINDOW  0xfffffffeu              /* ... it has to leave the window                                      */

struct sq_world { int n_ents; const float *pos_xz, *radius; const uint32_t *flags; };
// the resident table of static tile lists (first occurrences only), and the set of every row: all NULL / 0 without one
struct sq_sets { int n_sets; const int32_t *off; const uint32_t *tiles; const int32_t *target_set; };   // tiles: row << 16 | column

struct sq_row {
    uint32_t tiles[SQ_SIDE];                // the target's tiles: bit dc + SQ_NT of word dr + SQ_NT
    float    sx[2], sz[2];                  // the sources: pos + new_vel, pos
    int32_t  tr, tc;                        // the target's tile; a static row: the offset and the length of its list
    uint16_t iid[2];                        // the global island of each source's tile
    uint8_t  layer, done, query;            // done: `query` is the row's answer, nothing else is computed
    uint8_t  stat;                          // a static row: tiles[] is unused
};

// One wave per row.  items: [nq * stride] work items row * stride + tile (a static row: + list index), n_items: their
// count (zeroed before).  ST = false: stride is SQ_TILES and S is not read.
template <bool ST>
__global__ __launch_bounds__(64) void k_surround_rows(dq_map M, sq_world W, sq_sets S, uint32_t stride_in, const float *new_vel,
                                                      const int32_t *units, const int32_t *target, int nq, sq_row *rows,
                                                      uint32_t *items, uint32_t *n_items)
{
    __shared__ uint64_t grown_rows[ST ? 64 : 1];          // a static row: the unit's dilated circle, row by row
    const uint32_t stride = ST ? stride_in : (uint32_t)SQ_TILES;
    const int k = (int)blockIdx.x;
    if(k >= nq) return;
    const int lane = (int)(threadIdx.x & 63);
    const int u = units ? units[k] : k, t = target[k];
    uint8_t query = NAVHIP_SQ_HOST, layer = 0;
    bool done = true, stat = false;
    uint64_t T = 0;
    float sx[2] = {0.0f, 0.0f}, sz[2] = {0.0f, 0.0f};
    int tr = 0, tc = 0;
    int set_off = 0, set_n = 0;
    uint16_t iid[2] = {0, 0};
    do {
        // (a row the host form refuses before the launch; the device form cannot read it there: the row is the host's)
        if(u < 0 || u >= W.n_ents) break;
        const float ux = W.pos_xz[2 * u], uz = W.pos_xz[2 * u + 1], urad = W.radius[u];
        layer = (uint8_t)nav_layer_for(W.flags[u], urad);
        const dq_layer L = M.layers[layer];
        if(!L.probemask || !L.islands) break;
        if(t < 0) { query = 0; break; }                                       // no target: the caller keeps -1 / -2
        if(t >= W.n_ents) break;
        if(!(W.flags[t] & NAVHIP_ENTITY_FLAG_MOVABLE)) {
            // a static target: the row of the table its unit names, or the host's (no table, no set, a set outside it)
            if(!ST || !S.target_set) break;
            const int ts = S.target_set[k];
            if(ts < 0 || ts >= S.n_sets) break;
            stat = true;
            set_off = S.off[ts]; set_n = S.off[ts + 1] - set_off;
        }
        if(ST && stat) {
            if(ux != ux || uz != uz || urad != urad) break;
            const double un = ceil((double)(urad / 4));                       // tile.c:698
            if(!(un <= (double)SQ_NT)) break;
            const int nu = (int)un;
            // M_Tile_AllUnderCircle of the unit (a centre off the map: no tiles) as bit rows of the 64 x 64 window centred on
            // ITS tile: the circle fills 17 x 17 of it at most.  n_objects_adjacent's pair test: dilate the circle once by
            // its 8 neighbours, then a tile of the list touches when its bit is set (a list tile outside the window is
            // more than one tile from every tile of the circle; the dilation may reach off the map, the list never does)
            int ur = 0, uc = 0;
            const bool u_on = dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, ux, uz, &ur, &uc);
            const int abs_r = ur - 32 + lane;
            uint64_t U = 0;
            if(u_on && abs_r >= 0 && abs_r < M.h * 64 && lane - 32 >= -nu && lane - 32 <= nu) {
                for(int dc = -nu; dc <= nu; dc++) {
                    const int c = uc + dc;
                    if(c < 0 || c >= M.w * 64) continue;
                    if(circle_hits_tile(M, ux, uz, urad, abs_r, c)) U |= 1ull << (32 + dc);
                }
            }
            const u64x s = mk(U), up = from_n(s), dn = from_s(s);
            const u64x grown = (s | from_w(s) | from_e(s)) | (up | from_w(up) | from_e(up)) | (dn | from_w(dn) | from_e(dn));
            grown_rows[ST ? lane : 0] = to64(grown);
            wave_sync();
            bool hit = false;
            for(int i = lane; i < set_n; i += 64) {
                const uint32_t tile = S.tiles[set_off + i];
                const int dr = (int)(tile >> 16) - ur + 32, dc = (int)(tile & 0xffffu) - uc + 32;
                if(dr >= 0 && dr < 64 && dc >= 0 && dc < 64) hit = hit || ((grown_rows[ST ? dr : 0] >> dc) & 1ull);
            }
            if(__any(hit)) { query = NAVHIP_SQ_ADJACENT; break; }
            sx[0] = ux + new_vel[2 * u]; sz[0] = uz + new_vel[2 * u + 1];
            sx[1] = ux; sz[1] = uz;
            int s_r[2], s_c[2];
            if(!dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, sx[0], sz[0], &s_r[0], &s_c[0])) break;
            if(!dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, sx[1], sz[1], &s_r[1], &s_c[1])) break;
            iid[0] = dq_island(M, L, s_r[0], s_c[0]);
            iid[1] = dq_island(M, L, s_r[1], s_c[1]);
            query = 0;
            done = false;
            break;
        }
        const float tx = W.pos_xz[2 * t], tz = W.pos_xz[2 * t + 1], trad = W.radius[t];
        if(ux != ux || uz != uz || urad != urad || tx != tx || tz != tz || trad != trad) break;
        const double un = ceil((double)(urad / 4)), tn = ceil((double)(trad / 4));   // tile.c:698
        if(!(un <= (double)SQ_NT) || !(tn <= (double)SQ_NT)) break;
        const int nu = (int)un, nt = (int)tn;
        // M_Tile_AllUnderCircle of both circles (a centre off the map: no tiles, tile.c:691-693) in the 64 x 64 window
        // centred on the target's tile; a tile of the unit outside it is more than one tile from every tile of the target
        int ur = 0, uc = 0;
        const bool t_on = dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, tx, tz, &tr, &tc);
        const bool u_on = dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, ux, uz, &ur, &uc);
        if(!t_on) { tr = 0; tc = 0; }
        const int abs_r = tr - 32 + lane;
        const bool row_ok = abs_r >= 0 && abs_r < M.h * 64;
        uint64_t U = 0;
        if(t_on && row_ok && lane - 32 >= -nt && lane - 32 <= nt) {
            for(int dc = -nt; dc <= nt; dc++) {
                const int c = tc + dc;
                if(c < 0 || c >= M.w * 64) continue;                          // M_Tile_RelativeDesc fails
                if(circle_hits_tile(M, tx, tz, trad, abs_r, c)) T |= 1ull << (32 + dc);
            }
        }
        if(u_on && row_ok && abs_r - ur >= -nu && abs_r - ur <= nu) {
            for(int dc = -nu; dc <= nu; dc++) {
                const int c = uc + dc, b = c - tc + 32;
                if(c < 0 || c >= M.w * 64 || b < 0 || b > 63) continue;
                if(circle_hits_tile(M, ux, uz, urad, abs_r, c)) U |= 1ull << b;
            }
        }
        // n_objects_adjacent (nav.c:1695-1706): a pair of tiles within one row and one column of each other
        const u64x s = mk(T), up = from_n(s), dn = from_s(s);
        const u64x grown = (s | from_w(s) | from_e(s)) | (up | from_w(up) | from_e(up)) | (dn | from_w(dn) | from_e(dn));
        if(__any((to64(grown) & U) != 0ull)) { query = NAVHIP_SQ_ADJACENT; break; }
        // n_closest_adjacent_pos: the sources and their islands (a source off the map: the reference asserts, nav.c:1645)
        sx[0] = ux + new_vel[2 * u]; sz[0] = uz + new_vel[2 * u + 1];
        sx[1] = ux; sz[1] = uz;
        int s_r[2], s_c[2];
        if(!dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, sx[0], sz[0], &s_r[0], &s_c[0])) break;
        if(!dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, sx[1], sz[1], &s_r[1], &s_c[1])) break;
        iid[0] = dq_island(M, L, s_r[0], s_c[0]);
        iid[1] = dq_island(M, L, s_r[1], s_c[1]);
        query = 0;
        done = false;
    } while(0);
    // the record, and the work items of a row that goes on: its tiles in row-major order
    sq_row *R = rows + k;
    const int dr = lane - 32 + SQ_NT;
    const uint32_t mine = (done || dr < 0 || dr >= SQ_SIDE) ? 0u : ((uint32_t)(T >> (32 - SQ_NT)) & ((1u << SQ_SIDE) - 1u));
    if(dr >= 0 && dr < SQ_SIDE) R->tiles[dr] = mine;
    const int cnt = __popc(mine), incl = wave_incl_scan(cnt);
    if(ST && stat) { tr = set_off; tc = done ? 0 : set_n; }               // a static row: one work item per list entry
    const int total = (ST && stat) ? tc : uni<64>(__shfl(incl, 63));
    int base = 0;
    if(lane == 0) {
        R->sx[0] = sx[0]; R->sx[1] = sx[1]; R->sz[0] = sz[0]; R->sz[1] = sz[1];
        R->tr = tr; R->tc = tc; R->iid[0] = iid[0]; R->iid[1] = iid[1];
        R->layer = layer; R->done = done ? 1 : 0; R->query = query; R->stat = stat ? 1 : 0;
        if(total > 0) base = (int)atomicAdd(n_items, (uint32_t)total);
    }
    base = uni<64>(__shfl(base, 0));
    if(ST && stat) {
        for(int i = lane; i < total; i += 64) items[base + i] = (uint32_t)k * stride + (uint32_t)i;
        return;
    }
    uint32_t m = mine;
    int at = base + incl - cnt;
    while(m) {
        const int b = __builtin_ctz(m);
        m &= m - 1;
        items[at++] = (uint32_t)k * stride + (uint32_t)(dr * SQ_SIDE + b);
    }
}

// One wave per work item.  ans: [nq][2][stride] the answer tile (row << 16 | column), SQ_NONE or SQ_WINDOW.
template <bool ST>
__global__ __launch_bounds__(64) void k_surround_flood(dq_map M, sq_sets S, uint32_t stride_in, const sq_row *rows,
                                                       const uint32_t *items, const uint32_t *n_items, uint32_t *ans)
{
    __shared__ uint16_t fr[2][DQ_FRONTIER];
    __shared__ uint32_t ring[DQ_FRONTIER];
    const uint32_t stride = ST ? stride_in : (uint32_t)SQ_TILES;
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t n = *n_items;
    for(uint32_t it = blockIdx.x; it < n; it += gridDim.x) {
        // (ST: the item is the same in every lane; said so, the list lookup and the longer index arithmetic stay scalar)
        const uint32_t item = ST ? (uint32_t)uni<64>((int)items[it]) : items[it], k = item / stride, t = item - k * stride;
        const sq_row *R = rows + k;
        const dq_layer L = M.layers[ST ? uni<64>((int)R->layer) : (int)R->layer];
        int r = R->tr + (int)(t / SQ_SIDE) - SQ_NT, c = R->tc + (int)(t % SQ_SIDE) - SQ_NT;
        if(ST && R->stat) {                           // entry t of the row's list
            const uint32_t tile = S.tiles[R->tr + (int)t];
            r = (int)(tile >> 16); c = (int)(tile & 0xffffu);
        }
        if(ST) { r = uni<64>(r); c = uni<64>(c); }
        uint32_t a[2];
        for(int s = 0; s < 2; s++) {
            if(s == 1 && R->iid[1] == R->iid[0]) { a[1] = a[0]; break; }
            int ar = 0, ac = 0;
            const int rc = dq_flood_first(M, L, r, c, (uint32_t)R->iid[s], fr, ring, &ar, &ac);
            a[s] = rc < 0 ? SQ_WINDOW : (rc == 0 ? SQ_NONE : (((uint32_t)ar << 16) | (uint32_t)ac));
            wave_sync();
        }
        if(lane == 0) {
            ans[((size_t)k * 2 + 0) * stride + t] = a[0];
            ans[((size_t)k * 2 + 1) * stride + t] = a[1];
        }
    }
}

// One wave per row: the rows' answers in the shapes of navhip_state_aux_in.surround_query / .surround_dest_xz.  A static row
// runs over the entries of its list with the key (bits of the length, list index): of equal lengths the earlier ENTRY, whose
// answer need not be the row-major-first of the tied tiles.
template <bool ST>
__global__ __launch_bounds__(64) void k_surround_pick(dq_map M, uint32_t stride_in, const sq_row *rows, const uint32_t *ans, int nq,
                                                      uint8_t *out_query, float *out_dest_xz)
{
    const uint32_t stride = ST ? stride_in : (uint32_t)SQ_TILES;
    const int k = (int)blockIdx.x;
    if(k >= nq) return;
    const int lane = (int)(threadIdx.x & 63);
    const sq_row *R = rows + k;
    uint8_t query = R->query;
    float dest[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if(!R->done) {
        bool window = false;
        for(int s = 0; s < 2; s++) {
            const uint32_t *A = ans + ((size_t)k * 2 + s) * stride;
            const bool stat = ST && R->stat;
            const int n_t = stat ? R->tc : SQ_TILES;
            uint32_t best_len = 0xffffffffu, best_t = 0xffffffffu;
            for(int t = lane; t < n_t; t += 64) {
                if(!stat && !((R->tiles[t / SQ_SIDE] >> (t % SQ_SIDE)) & 1u)) continue;
                const uint32_t a = A[t];
                if(a == SQ_WINDOW) window = true;
                if(a == SQ_WINDOW || a == SQ_NONE) continue;
                // the tile's corner and its distance from the source, nav.c:1662-1669
                const float x = M.map_x - (float)(int)(a & 0xffffu) * 4.0f;
                const float z = M.map_z + (float)(int)(a >> 16) * 4.0f;
                const uint32_t len = __float_as_uint(len2f(R->sx[s] - x, R->sz[s] - z));
                if(len < best_len) { best_len = len; best_t = (uint32_t)t; }
            }
#pragma unroll
            for(int d = 32; d >= 1; d >>= 1) {
                const uint32_t ol = (uint32_t)__shfl_xor((int)best_len, d), ot = (uint32_t)__shfl_xor((int)best_t, d);
                if(ol < best_len || (ol == best_len && ot < best_t)) { best_len = ol; best_t = ot; }
            }
            best_t = (uint32_t)uni<64>((int)best_t);
            if(best_t != 0xffffffffu) {
                const uint32_t a = A[best_t];
                query |= (uint8_t)(NAVHIP_SQ_HAS_DEST_0 << s);
                dest[2 * s]     = M.map_x - (float)(int)(a & 0xffffu) * 4.0f;
                dest[2 * s + 1] = M.map_z + (float)(int)(a >> 16) * 4.0f;
            }
        }
        if(__any(window)) {                       // a flood of the row left the window: the whole row is the host's
            query = NAVHIP_SQ_HOST;
            dest[0] = dest[1] = dest[2] = dest[3] = 0.0f;
        }
    }
    if(lane == 0) {
        out_query[k] = query;
        for(int j = 0; j < 4; j++) out_dest_xz[4 * (size_t)k + j] = dest[j];
    }
}

#define SQ_FAIL(why) nh_fail(ctx, NAVHIP_ERR_ARG, "navhip_surround_queries: ", why)

// Entity_NavLayerWithRadius on the host: nav_layer_for (agent_math.h) is device code in the device build
static int sq_host_layer(uint32_t flags, float radius)
{
    const int base = (flags & NAVHIP_ENTITY_FLAG_WATER) ? 4 : (flags & NAVHIP_ENTITY_FLAG_AIR) ? 8 : 0;
    return base + (radius >= 15.0f ? 3 : radius >= 10.0f ? 2 : radius >= 5.0f ? 1 : 0);
}

#define SQ_SET_MAX 2048                     /* the reference's tds[2048] (nav.c:4631, :4941)                       */

// the launches of both device forms; target_set NULL, or no set registered: the kernels without the static arm
static int sq_launch(navhip_ctx *ctx, const navhip_world *w, const float *new_vel_xz, const int32_t *units, const int32_t *target,
                     const int32_t *target_set, int nq, uint8_t *out_query, float *out_dest_xz, hipStream_t s)
{
    int rc = nh_refresh_derived(ctx, s);          // the row masks of uploads since the last build
    if(rc) return rc;
    const bool st = target_set && ctx->static_sets_n > 0;
    const size_t stride = st && ctx->static_sets_longest > SQ_TILES ? (size_t)ctx->static_sets_longest : (size_t)SQ_TILES;
    if((size_t)nq * stride > 0xffffffffull) return SQ_FAIL("too many rows for one call: " + std::to_string(nq));
    // scratch: the item count, the rows' records, the work items, the tile answers, sized from nq and the longest registered
    // list (grown on demand: nothing is allocated after the first call at a given nq and table)
    const size_t rows_off = 256, items_off = rows_off + nh_up256(sizeof(sq_row) * (size_t)nq);
    const size_t ans_off = items_off + nh_up256(sizeof(uint32_t) * stride * (size_t)nq);
    rc = nh_ensure_buf(ctx, ctx->surround_query_scratch, ans_off + sizeof(uint32_t) * 2 * stride * (size_t)nq);
    if(rc) return rc;
    char *base = (char*)ctx->surround_query_scratch.p;
    uint32_t *d_count = (uint32_t*)base, *d_items = (uint32_t*)(base + items_off), *d_ans = (uint32_t*)(base + ans_off);
    sq_row *d_rows = (sq_row*)(base + rows_off);
    const dq_map M = dq_map_of(ctx, w->map_pos_x, w->map_pos_z);
    const sq_world W = {w->n_ents, w->pos_xz, w->radius, w->flags};
    sq_sets S = {0, nullptr, nullptr, nullptr};
    if(st) {
        const char *tab = (const char*)ctx->static_sets.p;
        S = sq_sets{ctx->static_sets_n, (const int32_t*)tab, (const uint32_t*)(tab + nh_up256(4 * ((size_t)ctx->static_sets_n + 1))), target_set};
    }
    const size_t most = (size_t)nq * stride;
    const dim3 flood_grid((unsigned)(most < SQ_FLOOD_BLOCKS ? most : SQ_FLOOD_BLOCKS));
    HIPCHK(ctx, hipMemsetAsync(d_count, 0, sizeof(uint32_t), s));
    if(st) {
        hipLaunchKernelGGL(k_surround_rows<true>, dim3(nq), dim3(64), 0, s, M, W, S, (uint32_t)stride, new_vel_xz, units, target, nq,
                           d_rows, d_items, d_count);
        hipLaunchKernelGGL(k_surround_flood<true>, flood_grid, dim3(64), 0, s, M, S, (uint32_t)stride, (const sq_row*)d_rows,
                           (const uint32_t*)d_items, (const uint32_t*)d_count, d_ans);
        hipLaunchKernelGGL(k_surround_pick<true>, dim3(nq), dim3(64), 0, s, M, (uint32_t)stride, (const sq_row*)d_rows,
                           (const uint32_t*)d_ans, nq, out_query, out_dest_xz);
    }else{
        hipLaunchKernelGGL(k_surround_rows<false>, dim3(nq), dim3(64), 0, s, M, W, S, (uint32_t)stride, new_vel_xz, units, target, nq,
                           d_rows, d_items, d_count);
        hipLaunchKernelGGL(k_surround_flood<false>, flood_grid, dim3(64), 0, s, M, S, (uint32_t)stride, (const sq_row*)d_rows,
                           (const uint32_t*)d_items, (const uint32_t*)d_count, d_ans);
        hipLaunchKernelGGL(k_surround_pick<false>, dim3(nq), dim3(64), 0, s, M, (uint32_t)stride, (const sq_row*)d_rows,
                           (const uint32_t*)d_ans, nq, out_query, out_dest_xz);
    }
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

extern "C" {

int navhip_static_targets_set(navhip_ctx *ctx, int n_sets, const int32_t *tiles_off, const int16_t *tiles)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    auto fail = [&](const std::string &why) { ctx->last_error = "navhip_static_targets_set: " + why; return NAVHIP_ERR_ARG; };
    if(n_sets < 0) return fail("a negative count");
    if(n_sets > 0 && (!tiles_off || !tiles)) return fail("a missing array");
    // every list, before the table is touched
    std::vector<int32_t> off((size_t)n_sets + 1, 0);
    std::vector<uint32_t> kept;
    int longest = 0;
    const int rows = ctx->h * 64, cols = ctx->w * 64;
    if(n_sets > 0 && tiles_off[0] < 0) return fail("non-monotonic offsets: tiles_off[0] = " + std::to_string(tiles_off[0]));
    for(int j = 0; j < n_sets; j++) {
        const int32_t b = tiles_off[j], e = tiles_off[j + 1];
        const std::string set = "set " + std::to_string(j);
        if(e < b) return fail(set + ": non-monotonic offsets (" + std::to_string(b) + " then " + std::to_string(e) + ")");
        if(e - b > SQ_SET_MAX) return fail(set + ": a list longer than 2048 entries (" + std::to_string(e - b) + ")");
        const size_t first = kept.size();
        for(int32_t i = b; i < e; i++) {
            const int r = tiles[2 * (size_t)i], c = tiles[2 * (size_t)i + 1];
            if(r < 0 || r >= rows || c < 0 || c >= cols)
                return fail(set + ": entry " + std::to_string(i - b) + " (" + std::to_string(r) + ", " + std::to_string(c) + ") is a tile off the map");
            // M_Tile_AllUnderObj returns the corner tiles of the outline once per edge, and outline tiles again when their
            // centre is inside.  The first occurrence of a tile is kept, in order: a later duplicate runs the same flood to
            // the same answer and the same length, which can never win n_closest_adjacent_pos's strict < against the
            // earlier entry, and n_objects_adjacent asks about the set of tiles only.  Dropping it changes no answer and
            // saves its floods.
            const uint32_t word = ((uint32_t)r << 16) | (uint32_t)c;
            bool seen = false;
            for(size_t q = first; q < kept.size() && !seen; q++) seen = kept[q] == word;
            if(!seen) kept.push_back(word);
        }
        off[(size_t)j + 1] = (int32_t)kept.size();
        longest = std::max(longest, (int)(kept.size() - first));
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // a query that still reads the old table: on the context's stream it is waited for here; on a caller's stream the
    // caller orders the two (include/navhip.h)
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->static_sets_n = 0; ctx->static_sets_longest = 0;
    if(n_sets == 0) return NAVHIP_OK;
    const size_t tiles_at = nh_up256(4 * off.size());
    int rc = nh_ensure_buf(ctx, ctx->static_sets, tiles_at + 4 * kept.size() + 4);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpy(ctx->static_sets.p, off.data(), 4 * off.size(), hipMemcpyHostToDevice));
    if(!kept.empty()) HIPCHK(ctx, hipMemcpy((char*)ctx->static_sets.p + tiles_at, kept.data(), 4 * kept.size(), hipMemcpyHostToDevice));
    ctx->static_sets_n = n_sets; ctx->static_sets_longest = longest;
    return NAVHIP_OK;
}

int navhip_surround_queries_ex_dev(navhip_ctx *ctx, const navhip_world *w, const float *new_vel_xz, const int32_t *units,
                                   const int32_t *target, const int32_t *target_set, int nq, uint8_t *out_query,
                                   float *out_dest_xz, void *stream)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    if(nq < 0) return SQ_FAIL("a negative count");
    if(!w || (nq > 0 && (!w->pos_xz || !w->radius || !w->flags || !new_vel_xz || !target || !out_query || !out_dest_xz)))
        return SQ_FAIL("a missing array");
    if(!units && nq != w->n_ents)
        return SQ_FAIL("the dense form has one row per entity: nq " + std::to_string(nq) + ", n_ents " + std::to_string(w->n_ents));
    if(nq == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return sq_launch(ctx, w, new_vel_xz, units, target, target_set, nq, out_query, out_dest_xz, stream ? (hipStream_t)stream : ctx->stream);
}

int navhip_surround_queries_dev(navhip_ctx *ctx, const navhip_world *w, const float *new_vel_xz, const int32_t *units,
                                const int32_t *target, int nq, uint8_t *out_query, float *out_dest_xz, void *stream)
{
    return navhip_surround_queries_ex_dev(ctx, w, new_vel_xz, units, target, nullptr, nq, out_query, out_dest_xz, stream);
}

int navhip_surround_queries_ex(navhip_ctx *ctx, const navhip_world *w, const float *new_vel_xz, const int32_t *units,
                               const int32_t *target, const int32_t *target_set, int nq, uint8_t *out_query, float *out_dest_xz)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    if(nq < 0) return SQ_FAIL("a negative count");
    if(!w || !w->pos_xz || !w->radius || !w->flags || !new_vel_xz || !target || !out_query || !out_dest_xz)
        return SQ_FAIL("a missing array");
    if(!units && nq != w->n_ents)
        return SQ_FAIL("the dense form has one row per entity: nq " + std::to_string(nq) + ", n_ents " + std::to_string(w->n_ents));
    // every row, before anything is launched
    for(int k = 0; k < nq; k++) {
        const int u = units ? units[k] : k;
        const std::string row = "row " + std::to_string(k);
        if(u < 0 || u >= w->n_ents) return SQ_FAIL(row + ": unit " + std::to_string(u) + " is outside the world");
        const navhip_layer &L = ctx->layers[sq_host_layer(w->flags[u], w->radius[u])];
        if(!L.cost || !L.blockers || !L.islands)
            return SQ_FAIL(row + ": its unit's layer has no resident cost / blockers / islands planes");
        const int t = target[k];
        if(target_set && t >= 0 && t < w->n_ents && !(w->flags[t] & NAVHIP_ENTITY_FLAG_MOVABLE)
           && (target_set[k] < 0 || target_set[k] >= ctx->static_sets_n))
            return SQ_FAIL(row + ": set " + std::to_string(target_set[k]) + " of its static target is outside the table of "
                                + std::to_string(ctx->static_sets_n) + " sets");
    }
    if(nq == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    navhip_world d;
    const float *d_vel; const int32_t *d_units = nullptr, *d_target, *d_set = nullptr;
    uint8_t *d_query; float *d_dest;
    const size_t rows = (size_t)nq;
    // the three arrays of the snapshot in the world's own slots (which drops a resident snapshot), the rest in one arena
    int rc = nh_stage_world(ctx, w, &d, s, {offsetof(navhip_world, pos_xz), offsetof(navhip_world, radius), offsetof(navhip_world, flags)});
    if(rc) return rc;
    nh_plan P;
    P.in(new_vel_xz, 8 * (size_t)w->n_ents, 16, (void**)&d_vel);
    if(units) P.in(units, 4 * rows, 0, (void**)&d_units);
    P.in(target, 4 * rows, 0, (void**)&d_target);
    if(target_set) P.in(target_set, 4 * rows, 0, (void**)&d_set);
    P.out(P.scratch(rows, (void**)&d_query), out_query, 1, 0, rows);
    P.out(P.scratch(16 * rows, (void**)&d_dest), out_dest_xz, 16, 0, rows);
    rc = P.reserve(ctx, NH_STAGE_CALL0);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = sq_launch(ctx, &d, d_vel, d_units, d_target, d_set, nq, d_query, d_dest, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

int navhip_surround_queries(navhip_ctx *ctx, const navhip_world *w, const float *new_vel_xz, const int32_t *units,
                            const int32_t *target, int nq, uint8_t *out_query, float *out_dest_xz)
{
    return navhip_surround_queries_ex(ctx, w, new_vel_xz, units, target, nullptr, nq, out_query, out_dest_xz);
}

}   // extern "C"
