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
#include "stage_plan.h"
#include "lane_group.h"
#include "nav_flood.h"        // the floods themselves: dq_map, dq_candidate, dq_flood
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

static_assert(sizeof(navhip_dest_query) == 16, "navhip_dest_query must stay 16 bytes");

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

#define DQ_FAIL(why) nh_fail(ctx, NAVHIP_ERR_ARG, "navhip_dest_queries: ", why)

extern "C" {

int navhip_dest_queries_dev(navhip_ctx *ctx, const navhip_dest_query *q, int n, float map_pos_x, float map_pos_z,
                            float *out_nearest_xz, int32_t *out_tiles_off, int16_t *out_tiles, int tiles_cap,
                            uint8_t *out_status, void *stream)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    if(n < 0 || tiles_cap < 0) return DQ_FAIL("a negative count");
    if(!out_tiles_off || (n > 0 && (!q || !out_nearest_xz || !out_status)) || (tiles_cap > 0 && !out_tiles))
        return DQ_FAIL("a missing array");
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
    const dq_map M = dq_map_of(ctx, map_pos_x, map_pos_z);
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
    if(n < 0 || tiles_cap < 0) return DQ_FAIL("a negative count");
    if(!out_tiles_off || (n > 0 && (!q || !out_nearest_xz || !out_status)) || (tiles_cap > 0 && !out_tiles))
        return DQ_FAIL("a missing array");
    // every record, before anything is launched
    for(int i = 0; i < n; i++) {
        const std::string row = "query " + std::to_string(i);
        const uint32_t known = NAVHIP_DQ_NEAREST | NAVHIP_DQ_TILES;
        if(!(q[i].flags & known) || (q[i].flags & ~known)) return DQ_FAIL(row + ": flags name no query or an unknown one");
        if(q[i].layer < 0 || q[i].layer >= NAVHIP_NAV_LAYER_MAX) return DQ_FAIL(row + ": no such layer");
        const navhip_layer &L = ctx->layers[q[i].layer];
        if(!L.cost || !L.blockers) return DQ_FAIL(row + ": its layer has no resident cost / blockers planes");
        if((q[i].flags & NAVHIP_DQ_TILES) && !L.islands) return DQ_FAIL(row + ": its layer has no resident islands plane");
        int r, c;
        if(!dq_tile_for_point(ctx->w, ctx->h, map_pos_x, map_pos_z, q[i].x, q[i].z, &r, &c))
            return DQ_FAIL(row + ": the position is outside the map");
    }
    if(n == 0) { out_tiles_off[0] = 0; return NAVHIP_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the lists come back through a device array of the full size: the caller's cap is tested against the real total
    // (the plan lays the arena out and uploads; the answers come down by hand, in the two steps below)
    const navhip_dest_query *d_q;
    float *d_nearest; int32_t *d_off; int16_t *d_tiles; uint8_t *d_status;
    const size_t full = (size_t)DQ_MAX_TILES * (size_t)n;
    nh_plan P;
    P.in(q, sizeof(navhip_dest_query) * (size_t)n, 0, (void**)&d_q);
    P.scratch(8 * (size_t)n, (void**)&d_nearest); P.scratch(4 * ((size_t)n + 1), (void**)&d_off);
    P.scratch(4 * full, (void**)&d_tiles); P.scratch((size_t)n, (void**)&d_status);
    int rc = P.reserve(ctx, NH_STAGE_CALL0);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = navhip_dest_queries_dev(ctx, d_q, n, map_pos_x, map_pos_z, d_nearest, d_off, d_tiles, (int)full, d_status, s);
    if(rc) return rc;
    std::vector<int32_t> off((size_t)n + 1);
    HIPCHK(ctx, hipMemcpyAsync(off.data(), d_off, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    if(off[n] > tiles_cap)
        return DQ_FAIL("tiles_cap " + std::to_string(tiles_cap) + " is below the " + std::to_string(off[n]) + " tiles of the answer");
    HIPCHK(ctx, hipMemcpyAsync(out_nearest_xz, d_nearest, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    if(off[n] > 0) HIPCHK(ctx, hipMemcpyAsync(out_tiles, d_tiles, 4 * (size_t)off[n], hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(out_status, d_status, (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    memcpy(out_tiles_off, off.data(), 4 * ((size_t)n + 1));
    return NAVHIP_OK;
}

}   // extern "C"
