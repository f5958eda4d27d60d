// order_query_kernels.hip -- the nav queries of an ORDER on the device: what move_process_cmds (movement.c:3246) asks when a
// SET_DEST or SET_ENTER_RANGE command is carried out, and make_flock (:804) once per flock:
//   N_ClosestReachableInRange (nav.c:5067)  the tile under the circle around the target that lies on the source's island and
//                                           is closest to the source (do_set_enter_range, movement.c:3069)
//   N_ClosestReachableDest    (nav.c:4085)  the destination itself, or the first tile of the source's island in the queue
//                                           order of n_closest_island_tiles(dest tile, src island, ignore_blockers = true,
//                                           maxout = 1) (do_set_dest, movement.c:2951)
//   N_LocationsReachable      (nav.c:4593)  source and destination on one island (combat.c:486)
//   N_DestIDForPos[Attacking] (nav.c:3367, :3376 -> n_dest_id :839)
// The kernel, its launch and the two entry points (navhip_order_queries[_dev]) live here; nothing else launches it.  It reads
// the islands plane and nothing else: no blockers, no probemask rows.
//
// k_order_query  one wave per row, in the shape of k_dest_query.
//   in range   M_Tile_AllUnderCircle (tile.c:687): the lanes stride the (2 nt + 1)^2 box around the target's tile in
//              row-major order, 64 tiles a batch; off-map tiles are skipped and do not count; a tile exists while fewer than
//              2048 tiles passed the circle test in front of it (the reference's tds[2048]: a running count over the batches,
//              ballot and popcount).  The pick of nav.c:5099-5120 is the minimum of (bits of the length, box index): lengths
//              are non-negative floats, so the pair compares as integers, and the strict < of the reference keeps the earlier
//              of equal lengths.  A box of at most 2048 tiles (nt <= 22) cannot reach the cap: there the island test goes
//              first and only tiles of the source's island take the circle test.
//   reachable  equal islands: the input, bit for bit.  Otherwise dq_flood_first<false> (nav_flood.h): the level-by-level
//              replay of the FIFO flood described at the top of dest_query_kernels.hip, the blockers test switched off.  An
//              answer outside the window of 127 x 127 tiles around the start is NAVHIP_OQ_HOST: the row holds to the window
//              as include/navhip.h states it for every flood (a search that has to visit a tile outside it).
//   dest id    n_dest_id of the tile of the answer.
#include "navhip_internal.h"
#include "stage_plan.h"
#include "lane_group.h"
#include "nav_flood.h"        // dq_map, dq_tile_for_point, dq_island, dq_flood_first
#include "circle_tiles.h"     // circle_hits_tile, len2f
#include <cmath>
#include <cstring>
#include <string>

static_assert(sizeof(navhip_order_query) == 32, "navhip_order_query must stay 32 bytes");

#define OQ_CAP     2048                     /* the reference's tds[2048], nav.c:5090                                */
#define OQ_NT_MAX  32                       /* ceil(range / 4) at most: a box of 65 x 65 tiles                      */
#define OQ_KNOWN   (NAVHIP_OQ_IN_RANGE | NAVHIP_OQ_REACHABLE)
#define OQ_FACTION_NONE 15                  /* FACTION_ID_NONE: N_DestIDForPos                                     */

// Why a row is not answered: the host form refuses the call with these words, the resident form returns the row as
// NAVHIP_OQ_HOST.  island_layers: bit l = layer l has a resident islands plane.
enum { OQ_ROW_OK = 0, OQ_ROW_FLAGS, OQ_ROW_LAYER, OQ_ROW_ISLANDS, OQ_ROW_FACTION, OQ_ROW_NAN, OQ_ROW_SRC, OQ_ROW_DST, OQ_ROW_RANGE };
DQ_HOST_DEVICE inline int oq_row_refusal(int w, int h, float map_x, float map_z, uint32_t island_layers, const navhip_order_query &Q)
{
    if(Q.flags & ~(uint32_t)OQ_KNOWN) return OQ_ROW_FLAGS;
    if(Q.layer < 0 || Q.layer >= NAVHIP_NAV_LAYER_MAX) return OQ_ROW_LAYER;
    if(!((island_layers >> Q.layer) & 1u)) return OQ_ROW_ISLANDS;
    if(Q.faction < 0 || Q.faction > OQ_FACTION_NONE) return OQ_ROW_FACTION;
    if(Q.src_x != Q.src_x || Q.src_z != Q.src_z || Q.dst_x != Q.dst_x || Q.dst_z != Q.dst_z || Q.range != Q.range) return OQ_ROW_NAN;
    int r, c;
    if(!dq_tile_for_point(w, h, map_x, map_z, Q.src_x, Q.src_z, &r, &c)) return OQ_ROW_SRC;
    if(!dq_tile_for_point(w, h, map_x, map_z, Q.dst_x, Q.dst_z, &r, &c)) return OQ_ROW_DST;
    if(!(ceil((double)(Q.range / 4)) <= (double)OQ_NT_MAX)) return OQ_ROW_RANGE;      // tile.c:698
    return OQ_ROW_OK;
}

// One wave per row.
__global__ __launch_bounds__(64) void k_order_query(dq_map M, uint32_t island_layers, const navhip_order_query *q, int n,
                                                    float *out_dest_xz, uint32_t *out_dest_id, uint8_t *out_status)
{
    __shared__ uint16_t fr[2][DQ_FRONTIER];
    __shared__ uint32_t ring[DQ_FRONTIER];
    const int qi = (int)blockIdx.x;
    if(qi >= n) return;
    const int lane = (int)(threadIdx.x & 63);
    const navhip_order_query Q = q[qi];
    // (a row the host form refuses before the launch; the device form cannot read it there: the row is the host's)
    bool host = oq_row_refusal(M.w, M.h, M.map_x, M.map_z, island_layers, Q) != OQ_ROW_OK;
    const dq_layer L = M.layers[host ? 0 : Q.layer];
    uint8_t status = 0;
    float dx = Q.dst_x, dz = Q.dst_z;
    uint32_t id = 0;
    if(!host) {
        int sr = 0, sc = 0, tr = 0, tc = 0;
        dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, Q.src_x, Q.src_z, &sr, &sc);
        dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, Q.dst_x, Q.dst_z, &tr, &tc);
        const uint16_t src_iid = dq_island(M, L, sr, sc);
        if(src_iid == dq_island(M, L, tr, tc)) status |= NAVHIP_OQ_SAME_ISLAND;                  // nav.c:4615
        if(Q.flags & NAVHIP_OQ_IN_RANGE) {
            // ---- M_Tile_AllUnderCircle and the pick of nav.c:5099-5120
            const double tn = ceil((double)(Q.range / 4));                                       // tile.c:698
            const int nt = tn < 0.0 ? -1 : (int)tn;                                              // below 0: `dr <= ntiles` never holds
            const int side = 2 * nt + 1, box = nt < 0 ? 0 : side * side;
            const bool cap_binds = box > OQ_CAP;
            uint32_t best_len = 0x7f800000u, best_i = 0xffffffffu;                               // min_dist = INFINITY
            int seen = 0;
            for(int base = 0; base < box && seen < OQ_CAP; base += 64) {
                const int i = base + lane;
                bool pass = false, mine = false;
                int r = 0, c = 0;
                if(i < box) {
                    r = tr + i / side - nt; c = tc + i % side - nt;
                    if(r >= 0 && c >= 0 && r < M.h * 64 && c < M.w * 64) {                        // M_Tile_RelativeDesc
                        mine = dq_island(M, L, r, c) == src_iid;
                        if(cap_binds || mine) pass = circle_hits_tile(M, Q.dst_x, Q.dst_z, Q.range, r, c);
                    }
                }
                if(cap_binds) {
                    const unsigned long long b = __ballot(pass);
                    const int rank = seen + __popcll(b & ((1ull << lane) - 1ull));
                    seen += __popcll(b);
                    pass = pass && rank < OQ_CAP;
                }
                if(pass && mine) {
                    // the tile's corner and its distance from the source, nav.c:5109-5116
                    const float x = M.map_x - (float)c * 4.0f;
                    const float z = M.map_z + (float)r * 4.0f;
                    const uint32_t len = __float_as_uint(len2f(Q.src_x - x, Q.src_z - z));
                    if(len < best_len) { best_len = len; best_i = (uint32_t)i; }
                }
            }
#pragma unroll
            for(int d = 32; d >= 1; d >>= 1) {
                const uint32_t ol = (uint32_t)__shfl_xor((int)best_len, d), oi = (uint32_t)__shfl_xor((int)best_i, d);
                if(ol < best_len || (ol == best_len && oi < best_i)) { best_len = ol; best_i = oi; }
            }
            best_i = (uint32_t)uni<64>((int)best_i);
            if(best_i != 0xffffffffu) {
                dx = M.map_x - (float)(tc + (int)best_i % side - nt) * 4.0f;
                dz = M.map_z + (float)(tr + (int)best_i / side - nt) * 4.0f;
            }else{
                status |= NAVHIP_OQ_NO_TILE;                                                      // nav.c:5124: the target
            }
        }
        if(Q.flags & NAVHIP_OQ_REACHABLE) {
            // ---- N_ClosestReachableDest(layer, src, (dx, dz)), nav.c:4106-4123; a tile's corner is on the map
            dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, dx, dz, &tr, &tc);
            if(src_iid != dq_island(M, L, tr, tc)) {
                int ar = 0, ac = 0;
                const int rc = dq_flood_first<false>(M, L, tr, tc, (uint32_t)src_iid, fr, ring, &ar, &ac);
                if(rc < 0 || (rc > 0 && (dq_abs(ar - tr) > DQ_R || dq_abs(ac - tc) > DQ_R))) {
                    host = true;
                }else if(rc == 0) {
                    dx = Q.src_x; dz = Q.src_z;          // nav.c:4117.  Never reached: the source's own tile is a hit
                }else{
                    dx = M.map_x - ((float)ac + 0.5f) * 4.0f;
                    dz = M.map_z + ((float)ar + 0.5f) * 4.0f;
                }
            }
        }
        if(!host) {
            // ---- n_dest_id (nav.c:848-853) of the answer's tile
            dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, dx, dz, &tr, &tc);
            id = ((uint32_t)(tr >> 6) << 26) | ((uint32_t)(tc >> 6) << 20) | ((uint32_t)(tr & 63) << 14) | ((uint32_t)(tc & 63) << 8)
               | ((uint32_t)Q.layer << 4) | (uint32_t)Q.faction;
        }
    }
    if(lane == 0) {
        out_dest_xz[2 * qi] = host ? __int_as_float(0x7fc00000) : dx; out_dest_xz[2 * qi + 1] = host ? 0.0f : dz;
        out_dest_id[qi] = host ? 0u : id;
        out_status[qi] = host ? NAVHIP_OQ_HOST : status;
    }
}

#define OQ_FAIL(why) nh_fail(ctx, NAVHIP_ERR_ARG, "navhip_order_queries: ", why)

static uint32_t oq_island_layers(const navhip_ctx *ctx)
{
    uint32_t m = 0;
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++) if(ctx->layers[l].islands) m |= 1u << l;
    return m;
}

extern "C" {

int navhip_order_queries_dev(navhip_ctx *ctx, const navhip_order_query *q, int n, float map_pos_x, float map_pos_z,
                             float *out_dest_xz, uint32_t *out_dest_id, uint8_t *out_status, void *stream)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    if(n < 0) return OQ_FAIL("a negative count");
    if(n > 0 && (!q || !out_dest_xz || !out_dest_id || !out_status)) return OQ_FAIL("a missing array");
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // (the islands plane is read as uploaded: no derived rows, no scratch, one launch)
    const dq_map M = dq_map_of(ctx, map_pos_x, map_pos_z);
    hipLaunchKernelGGL(k_order_query, dim3(n), dim3(64), 0, s, M, oq_island_layers(ctx), q, n, out_dest_xz, out_dest_id, out_status);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_order_queries(navhip_ctx *ctx, const navhip_order_query *q, int n, float map_pos_x, float map_pos_z,
                         float *out_dest_xz, uint32_t *out_dest_id, uint8_t *out_status)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    if(n < 0) return OQ_FAIL("a negative count");
    if(n > 0 && (!q || !out_dest_xz || !out_dest_id || !out_status)) return OQ_FAIL("a missing array");
    // every row, before anything is launched
    static const char *const why[] = {"", "flags name an unknown query", "no such layer", "its layer has no resident islands plane",
                                      "no such faction (0..14, or 15 for none)", "a NaN coordinate or range",
                                      "the source is outside the map", "the destination is outside the map",
                                      "the range is above 128 (ceil(range / 4) > 32 tiles)"};
    const uint32_t island_layers = oq_island_layers(ctx);
    for(int i = 0; i < n; i++) {
        const int bad = oq_row_refusal(ctx->w, ctx->h, map_pos_x, map_pos_z, island_layers, q[i]);
        if(bad != OQ_ROW_OK) return OQ_FAIL("query " + std::to_string(i) + ": " + why[bad]);
    }
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const navhip_order_query *d_q;
    float *d_dest; uint32_t *d_id; uint8_t *d_status;
    const size_t rows = (size_t)n;
    nh_plan P;
    P.in(q, sizeof(navhip_order_query) * rows, 0, (void**)&d_q);
    P.out(P.scratch(8 * rows, (void**)&d_dest), out_dest_xz, 8, 0, rows);
    P.out(P.scratch(4 * rows, (void**)&d_id), out_dest_id, 4, 0, rows);
    P.out(P.scratch(rows, (void**)&d_status), out_status, 1, 0, rows);
    int rc = P.reserve(ctx, NH_STAGE_CALL0);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = navhip_order_queries_dev(ctx, d_q, n, map_pos_x, map_pos_z, d_dest, d_id, d_status, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

}   // extern "C"
