// dest_query_kernels.hip -- the two nav queries of the arrival test that depend on the destination only, on the device:
// N_ClosestPathable (nav.c:4126) and the tile list N_IsMaximallyClose walks (nav.c:4707: n_closest_island_tiles(dest tile,
// its global island, ignore_blockers = false), nav.c:1226).  The kernels, their launches and the two entry points
// (navhip_dest_queries[_dev]) live here; nothing else launches them.  They read the probemask rows and the islands plane.
//
// Both reference searches are FIFO floods that expand through EVERY tile (the predicate never gates expansion), so the
// queue order depends on the start tile and the map bounds only, and -- the map being a rectangle -- the tiles of BFS
// level R are exactly the on-map tiles at distance R from the start: Manhattan for the 4-connected flood, Chebyshev for
// the 8-connected one.  One wave replays a flood level by level:
//   - the frontier of level R - 1 sits in LDS in queue order; lane i takes entry i and emits its neighbours in the
//     reference's delta order with key i * ndeltas + j;
//   - a candidate was "not visited in an earlier level" iff its distance is R (the visited set of the reference is every
//     on-map tile closer than that), and it is the one the reference pushes iff it holds the lowest key of its tile in
//     this level: an LDS atomicMin over one word per tile of the ring (8 R or 4 R tiles: a closed-form ring position
//     instead of a per-tile array over the window);
//   - survivors, compacted in key order (per-lane counts, the DPP prefix of lane_group.h), are the next frontier: the
//     tiles on which the reference evaluates its predicate, in the order it does.
// The window is the 127 x 127 tiles centred on the start (Chebyshev radius DQ_R): a flood that has to push an on-map tile
// outside it in front of its answer ends with NAVHIP_DQ_HOST, never with a wrong answer.
#include "navhip_internal.h"
#include "lane_group.h"
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#define DQ_R         63            /* Chebyshev radius of the window                                            */
#define DQ_FRONTIER  512           /* >= 8 * DQ_R tiles of a Chebyshev ring, >= 4 * 2 * DQ_R of a Manhattan one  */
#define DQ_MAX_TILES 256           /* FIELD_RES_R * 2 + FIELD_RES_C * 2, nav.c:4722                              */
#define DQ_NOKEY     0x7fffffffu
#define DQ_HIT       0x80000000u   /* in a ring word: the tile is a hit of the island flood                     */

static_assert(sizeof(navhip_dest_query) == 16, "navhip_dest_query must stay 16 bytes");

struct dq_layer { const uint64_t *probemask; const uint16_t *islands; };
struct dq_map { int w, h; float map_x, map_z; dq_layer layers[NAVHIP_NAV_LAYER_MAX]; };

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
template <bool ISL> __device__ int dq_flood(const dq_map &M, const dq_layer &L, int sr, int sc, uint32_t giid,
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

// One wave per query.  tiles: [n][DQ_MAX_TILES] words of scratch, count: [n].
__global__ __launch_bounds__(64) void k_dest_query(dq_map M, const navhip_dest_query *q, int n, float *out_nearest_xz,
                                                   uint8_t *out_status, int32_t *count, uint32_t *tiles)
{
    __shared__ uint16_t fr[2][DQ_FRONTIER];
    __shared__ uint32_t ring[DQ_FRONTIER];
    const int qi = (int)blockIdx.x;
    if(qi >= n) return;
    const int lane = (int)(threadIdx.x & 63);
    const navhip_dest_query Q = q[qi];
    const float nan = __int_as_float(0x7fc00000);
    float nx = nan, nz = 0.0f;
    int nt = 0, sr = 0, sc = 0;
    // (a record the host form refuses before the launch; the device form cannot read it there: the row is the host's)
    bool host = Q.layer < 0 || Q.layer >= NAVHIP_NAV_LAYER_MAX || !(Q.flags & (NAVHIP_DQ_NEAREST | NAVHIP_DQ_TILES))
             || (Q.flags & ~(uint32_t)(NAVHIP_DQ_NEAREST | NAVHIP_DQ_TILES));
    const dq_layer L = M.layers[host ? 0 : Q.layer];
    host = host || !L.probemask || ((Q.flags & NAVHIP_DQ_TILES) && !L.islands)
        || !dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, Q.x, Q.z, &sr, &sc);
    if(!host && (Q.flags & NAVHIP_DQ_NEAREST)) {
        if(dq_probe(M, L, sr, sc) == 1u) {
            nx = Q.x; nz = Q.z;                                               // nav.c:4141-4144
        }else{
            int ar = 0, ac = 0;
            const int rc = dq_flood<false>(M, L, sr, sc, 0, fr, ring, &ar, &ac, nullptr, nullptr);
            if(rc < 0) host = true;
            if(rc > 0) {
                // M_Tile_Bounds (tile.c:356) .x / .z, expression by expression
                nx = (M.map_x - (float)((ac >> 6) * 256)) - (float)((ac & 63) * 4);
                nz = (M.map_z + (float)((ar >> 6) * 256)) + (float)((ar & 63) * 4);
            }
        }
    }
    if(!host && (Q.flags & NAVHIP_DQ_TILES)) {
        wave_sync();
        const int rc = dq_flood<true>(M, L, sr, sc, (uint32_t)dq_island(M, L, sr, sc), fr, ring, nullptr, nullptr,
                                      tiles + (size_t)qi * DQ_MAX_TILES, &nt);
        if(rc < 0) host = true;
    }
    if(lane == 0) {
        out_nearest_xz[2 * qi] = host ? nan : nx; out_nearest_xz[2 * qi + 1] = host ? 0.0f : nz;
        out_status[qi] = host ? NAVHIP_DQ_HOST : 0;
        count[qi] = host ? 0 : nt;
    }
}

// count[0..n) -> off[0..n]: one workgroup, DQ_SCAN_T counts at a time with a running carry
#define DQ_SCAN_T 256
__global__ __launch_bounds__(DQ_SCAN_T) void k_dest_query_offsets(const int32_t *count, int32_t *off, int n)
{
    __shared__ int32_t wsum[DQ_SCAN_T / 64];
    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
    int32_t carry = 0;
    for(int base = 0; base < n; base += DQ_SCAN_T) {
        const int i = base + t;
        const int32_t v = i < n ? count[i] : 0;
        const int32_t incl = wave_incl_scan(v);
        if(lane == 63) wsum[w] = incl;
        __syncthreads();
        int32_t woff = 0, tot = 0;
#pragma unroll
        for(int k = 0; k < DQ_SCAN_T / 64; k++) { const int32_t x = wsum[k]; if(k < w) woff += x; tot += x; }
        if(i < n) off[i] = carry + woff + incl - v;
        carry += tot;
        __syncthreads();
    }
    if(t == 0) off[n] = carry;
}

// the lists, packed: one wave per query; nothing is written beyond the caller's cap
__global__ __launch_bounds__(64) void k_dest_query_pack(const int32_t *count, const int32_t *off, const uint32_t *tiles, int n,
                                                        uint32_t *out_tiles, int tiles_cap)
{
    const int qi = (int)blockIdx.x;
    if(qi >= n) return;
    const int c = count[qi], o = off[qi];
    for(int k = (int)(threadIdx.x & 63); k < c; k += 64)
        if(o + k < tiles_cap) out_tiles[o + k] = tiles[(size_t)qi * DQ_MAX_TILES + k];
}

static int dq_fail(navhip_ctx *ctx, const std::string &why)
{
    ctx->last_error = "navhip_dest_queries: " + why;
    return NAVHIP_ERR_ARG;
}

extern "C" {

int navhip_dest_queries_dev(navhip_ctx *ctx, const navhip_dest_query *q, int n, float map_pos_x, float map_pos_z,
                            float *out_nearest_xz, int32_t *out_tiles_off, int16_t *out_tiles, int tiles_cap,
                            uint8_t *out_status, void *stream)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    if(n < 0 || tiles_cap < 0) return dq_fail(ctx, "a negative count");
    if(!out_tiles_off || (n > 0 && (!q || !out_nearest_xz || !out_status)) || (tiles_cap > 0 && !out_tiles))
        return dq_fail(ctx, "a missing array");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    int rc = nh_refresh_derived(ctx, s);          // the row masks of uploads since the last build
    if(rc) return rc;
    // scratch: the counts, then the unpacked lists (grown on demand: nothing is allocated after the first call at a given n)
    const size_t counts_bytes = nh_up256(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    rc = nh_ensure_buf(ctx, ctx->dest_query_scratch, counts_bytes + sizeof(uint32_t) * DQ_MAX_TILES * (size_t)n);
    if(rc) return rc;
    int32_t *d_count = (int32_t*)ctx->dest_query_scratch.p;
    uint32_t *d_tiles = (uint32_t*)((char*)ctx->dest_query_scratch.p + counts_bytes);
    dq_map M;
    M.w = ctx->w; M.h = ctx->h; M.map_x = map_pos_x; M.map_z = map_pos_z;
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++) {
        const navhip_layer &L = ctx->layers[l];
        M.layers[l] = dq_layer{(L.cost && L.blockers) ? L.probemask : nullptr, L.islands};
    }
    if(n > 0) hipLaunchKernelGGL(k_dest_query, dim3(n), dim3(64), 0, s, M, q, n, out_nearest_xz, out_status, d_count, d_tiles);
    hipLaunchKernelGGL(k_dest_query_offsets, dim3(1), dim3(DQ_SCAN_T), 0, s, (const int32_t*)d_count, out_tiles_off, n);
    if(n > 0) hipLaunchKernelGGL(k_dest_query_pack, dim3(n), dim3(64), 0, s, (const int32_t*)d_count, (const int32_t*)out_tiles_off,
                                 (const uint32_t*)d_tiles, n, (uint32_t*)out_tiles, tiles_cap);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_dest_queries(navhip_ctx *ctx, const navhip_dest_query *q, int n, float map_pos_x, float map_pos_z,
                        float *out_nearest_xz, int32_t *out_tiles_off, int16_t *out_tiles, int tiles_cap, uint8_t *out_status)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    if(n < 0 || tiles_cap < 0) return dq_fail(ctx, "a negative count");
    if(!out_tiles_off || (n > 0 && (!q || !out_nearest_xz || !out_status)) || (tiles_cap > 0 && !out_tiles))
        return dq_fail(ctx, "a missing array");
    // every record, before anything is launched
    for(int i = 0; i < n; i++) {
        const std::string row = "query " + std::to_string(i);
        const uint32_t known = NAVHIP_DQ_NEAREST | NAVHIP_DQ_TILES;
        if(!(q[i].flags & known) || (q[i].flags & ~known)) return dq_fail(ctx, row + ": flags name no query or an unknown one");
        if(q[i].layer < 0 || q[i].layer >= NAVHIP_NAV_LAYER_MAX) return dq_fail(ctx, row + ": no such layer");
        const navhip_layer &L = ctx->layers[q[i].layer];
        if(!L.cost || !L.blockers) return dq_fail(ctx, row + ": its layer has no resident cost / blockers planes");
        if((q[i].flags & NAVHIP_DQ_TILES) && !L.islands) return dq_fail(ctx, row + ": its layer has no resident islands plane");
        int r, c;
        if(!dq_tile_for_point(ctx->w, ctx->h, map_pos_x, map_pos_z, q[i].x, q[i].z, &r, &c))
            return dq_fail(ctx, row + ": the position is outside the map");
    }
    if(n == 0) { out_tiles_off[0] = 0; return NAVHIP_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the lists come back through a device array of the full size: the caller's cap is tested against the real total
    const navhip_dest_query *d_q;
    float *d_nearest; int32_t *d_off; int16_t *d_tiles; uint8_t *d_status;
    const size_t full = (size_t)DQ_MAX_TILES * (size_t)n;
    int rc = nh_stage_in(ctx, NH_STAGE_CALL0, q, sizeof(navhip_dest_query) * (size_t)n, (const void**)&d_q, s);
    if(!rc) rc = nh_stage_reserve(ctx, NH_STAGE_CALL1, 8 * (size_t)n, (void**)&d_nearest);
    if(!rc) rc = nh_stage_reserve(ctx, NH_STAGE_CALL2, 4 * ((size_t)n + 1), (void**)&d_off);
    if(!rc) rc = nh_stage_reserve(ctx, NH_STAGE_CALL3, 4 * full, (void**)&d_tiles);
    if(!rc) rc = nh_stage_reserve(ctx, NH_STAGE_CALL4, (size_t)n, (void**)&d_status);
    if(!rc) rc = navhip_dest_queries_dev(ctx, d_q, n, map_pos_x, map_pos_z, d_nearest, d_off, d_tiles, (int)full, d_status, s);
    if(rc) return rc;
    std::vector<int32_t> off((size_t)n + 1);
    HIPCHK(ctx, hipMemcpyAsync(off.data(), d_off, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if(off[n] > tiles_cap)
        return dq_fail(ctx, "tiles_cap " + std::to_string(tiles_cap) + " is below the " + std::to_string(off[n]) + " tiles of the answer");
    HIPCHK(ctx, hipMemcpyAsync(out_nearest_xz, d_nearest, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    if(off[n] > 0) HIPCHK(ctx, hipMemcpyAsync(out_tiles, d_tiles, 4 * (size_t)off[n], hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(out_status, d_status, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    memcpy(out_tiles_off, off.data(), 4 * ((size_t)n + 1));
    return NAVHIP_OK;
}

}   // extern "C"
