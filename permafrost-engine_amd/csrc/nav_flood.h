// nav_flood.h -- the level-by-level replay of the reference's FIFO floods over the nav grid by one wave, device only: the
// map view (dq_map: probemask rows and islands plane per layer), the tile of a point, the candidates of a level, their
// ring positions and the floods themselves.  Shared by dest_query_kernels.hip (dq_flood: N_ClosestPathable and the island
// tile list of N_IsMaximallyClose), surround_query_kernels.hip (dq_flood_first: the first island tile next to a tile
// of the target) and order_query_kernels.hip (dq_flood_first without the blockers test: N_ClosestReachableDest).  How a flood is replayed is described at the top of dest_query_kernels.hip.  Free of device variables,
// so any unit may include it.
#pragma once
#include "navhip_internal.h"
#include "lane_group.h"
#include <cmath>

#define DQ_R         63            /* Chebyshev radius of the window                                            */
#define DQ_FRONTIER  512           /* >= 8 * DQ_R tiles of a Chebyshev ring, >= 4 * 2 * DQ_R of a Manhattan one  */
#define DQ_MAX_TILES 256           /* FIELD_RES_R * 2 + FIELD_RES_C * 2, nav.c:4722                              */
#define DQ_NOKEY     0x7fffffffu
#define DQ_HIT       0x80000000u   /* in a ring word: the tile is a hit of the island flood                     */

struct dq_layer { const uint64_t *probemask; const uint16_t *islands; };
struct dq_map { int w, h; float map_x, map_z; dq_layer layers[NAVHIP_NAV_LAYER_MAX]; };

// the view of a context's resident planes: a layer without cost and blockers planes has no probemask here
static inline dq_map dq_map_of(const navhip_ctx *ctx, float map_pos_x, float map_pos_z)
{
    dq_map M;
    M.w = ctx->w; M.h = ctx->h; M.map_x = map_pos_x; M.map_z = map_pos_z;
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++) {
        const navhip_layer &L = ctx->layers[l];
        M.layers[l] = dq_layer{(L.cost && L.blockers) ? L.probemask : nullptr, L.islands};
    }
    return M;
}

// n_tile_blocked (nav.c:235) of an absolute tile: cost_base == COST_IMPASSABLE or blockers > 0; bit 1 alone: blockers > 0
__device__ __forceinline__ uint32_t dq_probe(const dq_map &M, const dq_layer &L, int r, int c)
{
    const uint64_t *row = L.probemask + (((((size_t)((r >> 6) * M.w + (c >> 6))) << 6) + (size_t)(r & 63)) << 1);
    return (uint32_t)((row[0] >> (c & 63)) & 1ull) | ((uint32_t)((row[1] >> (c & 63)) & 1ull) << 1);
}

__device__ __forceinline__ uint16_t dq_island(const dq_map &M, const dq_layer &L, int r, int c)
{
    return L.islands[((size_t)((r >> 6) * M.w + (c >> 6)) << 12) + (size_t)((r & 63) * 64 + (c & 63))];
}

// M_Tile_DescForPoint2D (tile.c:547) as absolute tile coordinates; false: outside the map (the reference asserts)
#ifdef NH_HOSTSIM
#define DQ_HOST_DEVICE
#else
#define DQ_HOST_DEVICE __host__ __device__
#endif
DQ_HOST_DEVICE inline bool dq_tile_for_point(int w, int h, float map_x, float map_z, float x, float z, int *out_r, int *out_c)
{
    const float width = (float)(w * 256), height = (float)(h * 256);
    if(!(x <= map_x) || !(x >= map_x - width)) return false;
    if(!(z >= map_z) || !(z <= map_z + height)) return false;
    int chunk_r = (int)(fabsf(map_z - z) / 256.0f);        // exact: division by a power of two
    int chunk_c = (int)(fabsf(map_x - x) / 256.0f);
    chunk_r = chunk_r < 0 ? 0 : (chunk_r > h - 1 ? h - 1 : chunk_r);
    chunk_c = chunk_c < 0 ? 0 : (chunk_c > w - 1 ? w - 1 : chunk_c);
    const float base_x = map_x - (float)(chunk_c * 256);
    const float base_z = map_z + (float)(chunk_r * 256);
    int tile_r = (int)(fabsf(base_z - z) / 4.0f);
    int tile_c = (int)(fabsf(base_x - x) / 4.0f);
    tile_r = tile_r < 0 ? 0 : (tile_r > 63 ? 63 : tile_r);
    tile_c = tile_c < 0 ? 0 : (tile_c > 63 ? 63 : tile_c);
    *out_r = chunk_r * 64 + tile_r; *out_c = chunk_c * 64 + tile_c;
    return true;
}

__device__ __forceinline__ uint32_t dq_wave_min(uint32_t v)
{
#pragma unroll
    for(int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
    return (uint32_t)uni<64>((int)v);
}

__device__ __forceinline__ int dq_abs(int v) { return v < 0 ? -v : v; }

// manhattan_dist (nav.c:1213) of two absolute tiles, as the reference computes it: chunk * TILES_PER_CHUNK_HEIGHT + tile
// with the MAP's 32 tiles per chunk under the nav grid's 64 -- every chunk border between the two takes 32 off
__device__ __forceinline__ int dq_manhattan(int ar, int ac, int br, int bc)
{
    return dq_abs((ar - 32 * (ar >> 6)) - (br - 32 * (br >> 6))) + dq_abs((ac - 32 * (ac >> 6)) - (bc - 32 * (bc >> 6)));
}

// The deltas (row, column) of the two floods in the reference's order: (0,0) (0,-1) (0,+1) (-1,0) (+1,0) (-1,-1) (-1,+1)
// (+1,-1) (+1,+1) of n_closest_island_tiles (nav.c:1257-1267); N_ClosestPathable's four (nav.c:4165-4170) are its second
// to fifth
template <bool ISL> __device__ __forceinline__ void dq_delta(int j, int *dr, int *dc)
{
    if(!ISL) j++;
    if(j < 5) {
        *dr = j == 3 ? -1 : (j == 4 ? 1 : 0);
        *dc = j == 1 ? -1 : (j == 2 ? 1 : 0);
    }else{
        *dr = j < 7 ? -1 : 1;
        *dc = (j & 1) ? -1 : 1;
    }
}

// the distance the levels of a flood are rings of, and the position of a tile on its ring [0, 8 R) / [0, 4 R)
template <bool ISL> __device__ __forceinline__ int dq_dist(int dr, int dc)
{
    return ISL ? max(dq_abs(dr), dq_abs(dc)) : dq_abs(dr) + dq_abs(dc);
}
template <bool ISL> __device__ __forceinline__ int dq_ring_pos(int dr, int dc, int R)
{
    if(ISL) {
        if(dr == -R) return dc + R;                       // the top side with both corners: 2 R + 1
        if(dr == R)  return 3 * R + 1 + dc;               // the bottom side with both corners
        if(dc == -R) return 5 * R + 1 + dr;               // the left side without corners: 2 R - 1
        return 7 * R + dr;                                // the right side without corners
    }
    if(dc > 0 && dr >= 0) return dr;
    if(dr > 0 && dc <= 0) return R - dc;
    if(dc < 0 && dr <= 0) return 2 * R - dr;
    return 3 * R + dc;
}

struct dq_cand { int dr, dc; uint32_t key; int state; };        // state: 0 = none, 1 = a tile of ring R inside the window, 2 = ... outside it
// candidate j of frontier entry i (relative tile fr): what the reference's loop body sees behind its visited test
template <bool ISL> __device__ __forceinline__ dq_cand dq_candidate(const dq_map &M, int sr, int sc, uint32_t fr, int i, int j, int R)
{
    dq_cand k;
    int ddr, ddc;
    dq_delta<ISL>(j, &ddr, &ddc);
    k.dr = (int)(fr >> 8) - 128 + ddr; k.dc = (int)(fr & 255u) - 128 + ddc;
    k.key = (uint32_t)(i * (ISL ? 9 : 4) + j);
    k.state = 0;
    const int r = sr + k.dr, c = sc + k.dc;
    if(dq_dist<ISL>(k.dr, k.dc) != R || r < 0 || c < 0 || r >= M.h * 64 || c >= M.w * 64) return k;     // visited, or M_Tile_RelativeDesc fails
    k.state = (dq_abs(k.dr) > DQ_R || dq_abs(k.dc) > DQ_R) ? 2 : 1;
    return k;
}

// One flood from the tile (sr, sc).
//   ISL = false  N_ClosestPathable behind its early return: the start tile is blocked.  Returns 1 with the first tile in
//                queue order that is not blocked in *ans_r / *ans_c, 0 when the flood visited the whole map without one.
//   ISL = true   n_closest_island_tiles: the hits in the reference's order in tiles[] ((row, column) pairs of int16 as one
//                word), their number in *n_hits; returns 1.
// Either returns -1 when the flood leaves the window (NAVHIP_DQ_HOST).
// (internal linkage, like dq_flood_first below: two units instantiate it, and on the host emulator each copy must use the
// cross-lane primitives of its own unit)
template <bool ISL> static __device__ int dq_flood(const dq_map &M, const dq_layer &L, int sr, int sc, uint32_t giid,
                                            uint16_t (*fr)[DQ_FRONTIER], uint32_t *ring,
                                            int *ans_r, int *ans_c, uint32_t *tiles, int *n_hits)
{
    const int lane = (int)(threadIdx.x & 63);
    const int ND = ISL ? 9 : 4;
    int cur = 0, nf = 1, nh = 0, first_mh = -1;
    if(lane == 0) fr[0][0] = (uint16_t)((128 << 8) | 128);
    wave_sync();
    for(int R = 1; nf > 0; R++) {
        // ---- the lowest key of every tile of ring R
        const int ring_n = min(ISL ? 8 * R : 4 * R, DQ_FRONTIER);
        for(int p = lane; p < ring_n; p += 64) ring[p] = DQ_NOKEY;
        wave_sync();
        uint32_t out_key = DQ_NOKEY;                  // the lowest key of a tile of ring R outside the window
        uint32_t free_key = DQ_NOKEY;                 // ISL = false: ... of a tile that is not blocked
        for(int base = 0; base < nf; base += 64) {
            const int i = base + lane;
            if(i >= nf) continue;
            const uint32_t f = fr[cur][i];
            for(int j = 0; j < ND; j++) {
                const dq_cand k = dq_candidate<ISL>(M, sr, sc, f, i, j, R);
                if(k.state == 0) continue;
                if(!ISL && dq_probe(M, L, sr + k.dr, sc + k.dc) == 1u) free_key = min(free_key, k.key);
                if(k.state == 2) out_key = min(out_key, k.key);
                else atomicMin(&ring[dq_ring_pos<ISL>(k.dr, k.dc, R)], k.key);
            }
        }
        out_key = dq_wave_min(out_key);
        wave_sync();
        uint32_t stop_key = DQ_NOKEY;                 // ISL: the candidate at which `goto done` fires for the distance
        if(!ISL) {
            // the answer is the first tile of the level in queue order that is not blocked, inside the window or not (the
            // reference pops the whole level in front of it: only a NEXT level needs the window)
            free_key = dq_wave_min(free_key);
            if(free_key != DQ_NOKEY) {
                const dq_cand k = dq_candidate<ISL>(M, sr, sc, fr[cur][free_key / ND], (int)(free_key / ND), (int)(free_key % ND), R);
                *ans_r = sr + k.dr; *ans_c = sc + k.dc;
                return 1;
            }
            if(out_key != DQ_NOKEY) return -1;
        }else{
            // ---- the hits among the survivors (marked in their ring word); the first one fixes first_mh_dist
            uint32_t hit_key = DQ_NOKEY;
            for(int base = 0; base < nf; base += 64) {
                const int i = base + lane;
                if(i >= nf) continue;
                const uint32_t f = fr[cur][i];
                for(int j = 1; j < ND; j++) {
                    const dq_cand k = dq_candidate<ISL>(M, sr, sc, f, i, j, R);
                    if(k.state != 1) continue;
                    const int p = dq_ring_pos<ISL>(k.dr, k.dc, R);
                    if(ring[p] != k.key) continue;
                    const int r = sr + k.dr, c = sc + k.dc;
                    if((uint32_t)dq_island(M, L, r, c) == giid && !(dq_probe(M, L, r, c) & 2u)) {
                        ring[p] = k.key | DQ_HIT;
                        hit_key = min(hit_key, k.key);
                    }
                }
            }
            wave_sync();
            uint32_t after_key = 0;                   // the distance test holds from this key on
            if(first_mh < 0) {
                hit_key = dq_wave_min(hit_key);
                if(hit_key != DQ_NOKEY) {
                    const dq_cand k = dq_candidate<ISL>(M, sr, sc, fr[cur][hit_key / ND], (int)(hit_key / ND), (int)(hit_key % ND), R);
                    first_mh = dq_manhattan(sr, sc, sr + k.dr, sc + k.dc);         // (0 across a chunk border: no distance stop then, nav.c:1288)
                    after_key = hit_key + 1;
                }
            }
            if(first_mh > 0) {
                // the first candidate behind the visited test (a survivor: a later duplicate of a tile is visited by then)
                // whose Manhattan distance exceeds first_mh_dist
                for(int base = 0; base < nf; base += 64) {
                    const int i = base + lane;
                    if(i >= nf) continue;
                    const uint32_t f = fr[cur][i];
                    for(int j = 1; j < ND; j++) {
                        const dq_cand k = dq_candidate<ISL>(M, sr, sc, f, i, j, R);
                        if(k.state != 1 || k.key < after_key || dq_manhattan(sr, sc, sr + k.dr, sc + k.dc) <= first_mh) continue;
                        if((ring[dq_ring_pos<ISL>(k.dr, k.dc, R)] & ~DQ_HIT) == k.key) stop_key = min(stop_key, k.key);
                    }
                }
                stop_key = dq_wave_min(stop_key);
            }
        }
        // ---- survivors in key order: the next frontier; ISL: the hits in front of the stop, appended to the list
        const uint32_t end_key = min(stop_key, out_key);
        const int nxt = cur ^ 1;
        int nn = 0;
        for(int base = 0; base < nf; base += 64) {
            const int i = base + lane;
            uint32_t alive = 0, hits = 0;
            uint32_t f = 0;
            if(i < nf) {
                f = fr[cur][i];
                for(int j = 0; j < ND; j++) {
                    const dq_cand k = dq_candidate<ISL>(M, sr, sc, f, i, j, R);
                    if(k.state != 1) continue;
                    const uint32_t word = ring[dq_ring_pos<ISL>(k.dr, k.dc, R)];
                    if((word & ~DQ_HIT) != k.key) continue;
                    alive |= 1u << j;
                    if(ISL && (word & DQ_HIT) && k.key < end_key) hits |= 1u << j;
                }
            }
            const int na = __popc(alive), nhit = __popc(hits);
            const int ia = wave_incl_scan(na), ih = ISL ? wave_incl_scan(nhit) : 0;
            int at = nn + ia - na, ht = nh + ih - nhit;
            for(int j = 0; j < ND; j++) {
                if(!((alive >> j) & 1u)) continue;
                int ddr, ddc;
                dq_delta<ISL>(j, &ddr, &ddc);
                const int dr = (int)(f >> 8) - 128 + ddr, dc = (int)(f & 255u) - 128 + ddc;
                if(at < DQ_FRONTIER) fr[nxt][at] = (uint16_t)(((dr + 128) << 8) | (dc + 128));
                at++;
                if(ISL && ((hits >> j) & 1u)) {
                    if(ht < DQ_MAX_TILES) tiles[ht] = (uint32_t)(uint16_t)(int16_t)(sr + dr) | ((uint32_t)(uint16_t)(int16_t)(sc + dc) << 16);
                    ht++;
                }
            }
            nn += uni<64>(__shfl(ia, 63));
            if(ISL) nh += uni<64>(__shfl(ih, 63));
        }
        wave_sync();
        if(ISL) {
            if(nh >= DQ_MAX_TILES) { *n_hits = DQ_MAX_TILES; return 1; }      // ret == maxout, nav.c:1298
            if(out_key < stop_key) return -1;                                  // a tile outside the window in front of the stop
            if(stop_key != DQ_NOKEY) { *n_hits = nh; return 1; }              // nav.c:1288
        }
        cur = nxt; nf = min(nn, DQ_FRONTIER);
    }
    if(ISL) *n_hits = nh;
    return ISL ? 1 : 0;
}

// A third mode: n_closest_island_tiles (nav.c:1226) with maxout = 1 and the island GIVEN (n_closest_adjacent_pos,
// nav.c:1658: the island of the source, not of the start tile).  `ret == maxout` fires at the first hit, so first_mh_dist
// plays no part: the answer is the first tile in queue order with islands == giid && blockers == 0 -- the lowest key among
// the candidates of ring R that pass (a later duplicate of a tile holds a higher key than its first visit, so the minimum
// over all candidates is the minimum over first visits).  The start tile is visited before the loop and never tested.  As
// in the ISL = false arm, candidates outside the window are tested as well: the reference pops the whole level in front of
// the hit, and only a NEXT level needs the window.  Returns 1 with the tile in *ans_r / *ans_c, 0 when the flood visited
// the whole map without a hit, -1 when it has to leave the window (NAVHIP_SQ_HOST).
// BLK = false is the same flood with ignore_blockers = true (N_ClosestReachableDest, nav.c:4115): the island alone decides,
// and the probemask rows are not read (order_query_kernels.hip).
template <bool BLK = true>
static __device__ inline int dq_flood_first(const dq_map &M, const dq_layer &L, int sr, int sc, uint32_t giid,
                                     uint16_t (*fr)[DQ_FRONTIER], uint32_t *ring, int *ans_r, int *ans_c)
{
    const int lane = (int)(threadIdx.x & 63);
    const int ND = 9;
    int cur = 0, nf = 1;
    if(lane == 0) fr[0][0] = (uint16_t)((128 << 8) | 128);
    wave_sync();
    for(int R = 1; nf > 0; R++) {
        // ---- the lowest key of every tile of ring R, and of a tile that passes the predicate
        const int ring_n = min(8 * R, DQ_FRONTIER);
        for(int p = lane; p < ring_n; p += 64) ring[p] = DQ_NOKEY;
        wave_sync();
        uint32_t out_key = DQ_NOKEY, hit_key = DQ_NOKEY;
        for(int base = 0; base < nf; base += 64) {
            const int i = base + lane;
            if(i >= nf) continue;
            const uint32_t f = fr[cur][i];
            for(int j = 1; j < ND; j++) {
                const dq_cand k = dq_candidate<true>(M, sr, sc, f, i, j, R);
                if(k.state == 0) continue;
                const int r = sr + k.dr, c = sc + k.dc;
                if((uint32_t)dq_island(M, L, r, c) == giid && (!BLK || !(dq_probe(M, L, r, c) & 2u))) hit_key = min(hit_key, k.key);
                if(k.state == 2) out_key = min(out_key, k.key);
                else atomicMin(&ring[dq_ring_pos<true>(k.dr, k.dc, R)], k.key);
            }
        }
        out_key = dq_wave_min(out_key);
        hit_key = dq_wave_min(hit_key);
        wave_sync();
        if(hit_key != DQ_NOKEY) {
            const dq_cand k = dq_candidate<true>(M, sr, sc, fr[cur][hit_key / ND], (int)(hit_key / ND), (int)(hit_key % ND), R);
            *ans_r = sr + k.dr; *ans_c = sc + k.dc;
            return 1;
        }
        if(out_key != DQ_NOKEY) return -1;
        // ---- survivors in key order: the next frontier
        const int nxt = cur ^ 1;
        int nn = 0;
        for(int base = 0; base < nf; base += 64) {
            const int i = base + lane;
            uint32_t alive = 0, f = 0;
            if(i < nf) {
                f = fr[cur][i];
                for(int j = 1; j < ND; j++) {
                    const dq_cand k = dq_candidate<true>(M, sr, sc, f, i, j, R);
                    if(k.state == 1 && ring[dq_ring_pos<true>(k.dr, k.dc, R)] == k.key) alive |= 1u << j;
                }
            }
            const int na = __popc(alive);
            const int ia = wave_incl_scan(na);
            int at = nn + ia - na;
            for(int j = 1; j < ND; j++) {
                if(!((alive >> j) & 1u)) continue;
                int ddr, ddc;
                dq_delta<true>(j, &ddr, &ddc);
                const int dr = (int)(f >> 8) - 128 + ddr, dc = (int)(f & 255u) - 128 + ddc;
                if(at < DQ_FRONTIER) fr[nxt][at] = (uint16_t)(((dr + 128) << 8) | (dc + 128));
                at++;
            }
            nn += uni<64>(__shfl(ia, 63));
        }
        wave_sync();
        cur = nxt; nf = min(nn, DQ_FRONTIER);
    }
    return 0;
}
