// seek_seed_kernels.hip -- the seed tiles of the enemy-seek and surround fields from the device-resident snapshot (gfx950):
// the game-side half of field_update_enemies (field.c:1537) and field_update_entity (:1612), whose grid half is
// k_region_field (region_kernels.hip, out_mode 1).  navhip_build_seek_fields[_dev] run the two behind each other on one stream.
//
// Reference semantics, in the order of the call:
//   field_enemies_initial_frontier :1209
//     field_chunk_bounds :863        the chunk's box in floats; widened by half its length + SEARCH_BUFFER (16) per side (:1232)
//     G_Pos_EntsInRect position.c:302  bg_ent_inrange_rect (bitmap_grid.h:1274): _bg_cell_extent refuses a rectangle that misses
//                                    the grid; every cell of the clamped extent is scanned, and an entity lives in the clamped
//                                    cell of its own coordinates, so membership is BG_SCALE_F(coordinate) against BG_SCALE_F(bound),
//                                    inclusive; at most MAX_ENTS_PER_CHUNK (4 096) in the grid's cell order -- beyond: the host's;
//                                    then filter_garrisoned
//     field_enemy_ent :963, ent_dying  another faction, COMBATABLE, at war by the diplomacy table, visible, not dying
//     M_Tile_AllUnderCircle tile.c:687, then one M_Tile_Contour (:759) of EVERYTHING so far for layer >= 3X3, >= 5X5, >= 7X7
//                                    (enum comparisons: water and air layers take all three), all into tds[512]
//     has_enemy[dr][dc]              the tiles with M_Tile_Distance from `base` inside [0, 128)^2; the frontier is its set bits
//   field_entity_initial_frontier :1317  the target's circle; contours for layer == 3X3, >= 5X5, >= 7X7; the in-region tiles
//
// k_seek_seeds   one 256-thread workgroup per request, the 128 x 128 bitmap (2 KB) in LDS.  The lanes sweep the entity arrays
//                256 at a time; a wave rasterises each of its 64 entities that passes into a 64 x 64 bit window centred on the
//                entity's tile (lane = window row, circle_window.h) and ORs the window's rows into the bitmap: OR is order
//                free, so the bitmap does not depend on scheduling.  The set bits are compacted by a workgroup prefix sum
//                into a row-major list of (abs_r, abs_c) pairs, 64 KB of arena per request, and the request's row of the
//                navhip_region_req table is filled.  A row the device does not decide gets NAVHIP_SK_HOST and a region request
//                that reads and writes nothing (a 2 x 2 region off the map, no seed).
#include <hip/hip_runtime.h>
#include <math.h>
#include "navhip_internal.h"
#include "stage_plan.h"
#include "agent_types.h"
#include "agent_math.h"         // bg_scale
#include "wave_bits.h"
#include "circle_window.h"      // cap_rowmajor, contour_of
#include "circle_tiles.h"       // circle_hits_tile
#include <string>

static_assert(sizeof(navhip_seek_req) == 12, "navhip_seek_req must stay 12 bytes");

#define SK_RDIM        128                  /* FIELD_RES_R * 2: the padded region */
#define SK_MAX_SEEDS   (SK_RDIM * SK_RDIM)  /* seed pairs of arena per request */
#define SK_MAX_ENTS    4096                 /* MAX_ENTS_PER_CHUNK, field.c:64 */
#define SK_TDS         512                  /* tds[512], field.c:1260, :1332 */
#define SK_SEARCH_BUFFER 16.0f              /* field.c:65 */
#define SK_POS_LIMIT   4194304.0f           /* 2^22: BG_SCALE_F of anything at or beyond it does not fit 31 bits */

struct sk_params {
    int       w, h;
    float     map_x, map_z;
    int32_t   origin_x, origin_y;       // the grid of the position index (bitmap_grid.h:968-990)
    int       grid_w, grid_h;
    int       n_ents;
    const float    *pos_xz, *radius;
    const uint32_t *flags;
    const int32_t  *faction;
    const uint8_t  *exclude;
    uint16_t  enemy_mask[16];
    uint32_t  layer_ok;                 // bit l: cost_base and blockers of layer l are resident
};

// contours a request's layer adds to a circle (field.c:1272-1280 against :1345-1353)
__device__ __forceinline__ int sk_contours(int kind, int layer)
{
    const int first = kind == NAVHIP_SEEK_ENEMIES ? (layer >= 1) : (layer == 1);
    return first + (layer >= 2) + (layer >= 3);
}

// Can the window hold the circle?  q = radius / 4 as the reference divides (float by int); false for a NaN radius too
__device__ __forceinline__ bool sk_radius_fits(float radius, int ncont, int *ntiles)
{
    const float q = radius / 4;
    if(!(q <= 31.0f)) return false;
    const int nt = q < -1.0f ? -1 : (int)ceil((double)q);               // tile.c:698; below 0: no tile at all
    *ntiles = nt;
    return nt + ncont <= 31;
}

// One wave: the tiles of a circle and `ncont` contours, capped as tds[512] caps them, ORed into the region's bitmap
// (bits[r * 4 + c / 32] bit c % 32 of region tile (r, c)).  A centre off the map yields nothing (tile.c:691-693).
__device__ inline void sk_raster(const sk_params &P, float cx, float cz, float radius, int ntiles, int ncont,
                                 int base_r, int base_c, uint32_t *bits, int lane)
{
    // M_Tile_DescForPoint2D (tile.c:547) of the centre
    const float width = (float)(P.w * 256), height = (float)(P.h * 256);
    if(cx > P.map_x || cx < P.map_x - width) return;
    if(cz < P.map_z || cz > P.map_z + height) return;
    int chunk_r = (int)(fabsf(P.map_z - cz) / 256.0f), chunk_c = (int)(fabsf(P.map_x - cx) / 256.0f);
    chunk_r = min(max(chunk_r, 0), P.h - 1);
    chunk_c = min(max(chunk_c, 0), P.w - 1);
    const float bx = P.map_x - (float)(chunk_c * 256), bz = P.map_z + (float)(chunk_r * 256);
    int tile_r = (int)(fabsf(bz - cz) / 4.0f), tile_c = (int)(fabsf(bx - cx) / 4.0f);
    tile_r = min(max(tile_r, 0), 63);
    tile_c = min(max(tile_c, 0), 63);
    const int cen_r = chunk_r * 64 + tile_r, cen_c = chunk_c * 64 + tile_c;

    // window row of this lane, and the in-map columns of that row
    const int abs_r = cen_r - 32 + lane;
    const bool row_ok = abs_r >= 0 && abs_r < P.h * 64;
    uint64_t inmap = 0;
    if(row_ok) {
        const int lo = max(0, 32 - cen_c), hi = min(63, P.w * 64 - 1 - cen_c + 32);
        if(hi >= lo) inmap = (hi - lo == 63) ? ~0ull : (((1ull << (hi - lo + 1)) - 1ull) << lo);
    }
    // M_Tile_AllUnderCircle: dr, dc in [-ntiles, ntiles], row-major, cap 512
    uint64_t tds = 0;
    const int dr = lane - 32;
    if(row_ok && dr >= -ntiles && dr <= ntiles) {
        for(int dc = -ntiles; dc <= ntiles; dc++) {
            const int b = 32 + dc;
            if(b < 0 || b > 63 || !((inmap >> b) & 1)) continue;        // M_Tile_RelativeDesc fails
            if(circle_hits_tile(P, cx, cz, radius, abs_r, cen_c + dc)) tds |= 1ull << b;
        }
    }
    uint64_t all = cap_rowmajor(tds, SK_TDS, lane);
    for(int k = 0; k < ncont; k++) {
        // ntds so far (wave sum), then M_Tile_Contour of everything so far into the room that is left
        int ntds = __popcll(all);
#pragma unroll
        for(int d = 1; d < 64; d <<= 1) ntds += __shfl_xor(ntds, d);
        all |= cap_rowmajor(contour_of(all, inmap), SK_TDS - ntds, lane);
    }
    // M_Tile_Distance from base inside [0, 128)^2: window column b is region column b + s
    const int rr = abs_r - base_r, s = cen_c - 32 - base_c;
    if(!all || rr < 0 || rr >= SK_RDIM || s <= -64 || s >= SK_RDIM) return;
    uint64_t lo, hi;
    if(s >= 64)     { lo = 0; hi = all << (s - 64); }
    else if(s > 0)  { lo = all << s; hi = all >> (64 - s); }
    else if(s == 0) { lo = all; hi = 0; }
    else            { lo = all >> (-s); hi = 0; }
    uint32_t *row = bits + rr * 4;
    if((uint32_t)lo)         atomicOr(&row[0], (uint32_t)lo);
    if((uint32_t)(lo >> 32)) atomicOr(&row[1], (uint32_t)(lo >> 32));
    if((uint32_t)hi)         atomicOr(&row[2], (uint32_t)hi);
    if((uint32_t)(hi >> 32)) atomicOr(&row[3], (uint32_t)(hi >> 32));
}

__global__ __launch_bounds__(256) void k_seek_seeds(sk_params P, const navhip_seek_req *reqs, int n, int16_t *arena,
                                                    navhip_region_req *rreqs, uint8_t *out_status, uint8_t *seed_bits)
{
    __shared__ uint32_t bits[SK_RDIM * 4];          // 2 KB: has_enemy
    __shared__ int s_host, s_members, s_wsum[4];
    const int ri = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if(ri >= n) return;
    const navhip_seek_req rq = reqs[ri];
    for(int i = t; i < SK_RDIM * 4; i += 256) bits[i] = 0;
    if(t == 0) { s_host = 0; s_members = 0; }
    __syncthreads();

    const int kind = rq.kind, layer = rq.layer, cr = rq.chunk_r, cc = rq.chunk_c;
    // rows that are not decided here, by the request alone (uniform over the workgroup)
    bool host = kind > NAVHIP_SEEK_ENTITY || layer >= NAVHIP_NAV_LAYER_MAX || !((P.layer_ok >> (layer & 31)) & 1u)
             || P.w < 2 || P.h < 2 || cr < 0 || cr >= P.h || cc < 0 || cc >= P.w;
    if(!host && kind == NAVHIP_SEEK_ENEMIES) host = rq.faction_id < 0 || rq.faction_id > 15;
    if(!host && kind == NAVHIP_SEEK_ENTITY)  host = rq.target_uid < 0 || rq.target_uid >= P.n_ents;
    // the region: field.c:1567-1572
    const int base_r = cr > 0 ? (cr - 1) * 64 + 32 : 0, base_c = cc > 0 ? (cc - 1) * 64 + 32 : 0;
    const int ncont = host ? 0 : sk_contours(kind, layer);

    if(!host && kind == NAVHIP_SEEK_ENTITY) {
        if(wave == 0) {
            const int e = rq.target_uid;
            const float x = P.pos_xz[2 * e], z = P.pos_xz[2 * e + 1], radius = P.radius[e];
            int ntiles = 0;
            const bool ok = !(P.flags[e] & NAVHIP_ENTITY_FLAG_BUILDING) && fabsf(x) < SK_POS_LIMIT && fabsf(z) < SK_POS_LIMIT
                         && sk_radius_fits(radius, ncont, &ntiles);
            if(!ok) { if(lane == 0) s_host = 1; }
            else sk_raster(P, x, z, radius, ntiles, ncont, base_r, base_c, bits, lane);
        }
    }else if(!host) {
        // field_chunk_bounds :863 and the widened rectangle :1232-1235, in float as written there
        const float x_max = P.map_x + (float)(-(cc * 256)), x_min = x_max - 256.0f;
        const float z_min = P.map_z + (float)(cr * 256),    z_max = z_min + 256.0f;
        const float xlen = x_max - x_min, zlen = z_max - z_min;
        const int32_t imnx = bg_scale(x_min - xlen / 2.0f - SK_SEARCH_BUFFER), imxx = bg_scale(x_max + xlen / 2.0f + SK_SEARCH_BUFFER);
        const int32_t imny = bg_scale(z_min - zlen / 2.0f - SK_SEARCH_BUFFER), imxy = bg_scale(z_max + zlen / 2.0f + SK_SEARCH_BUFFER);
        // _bg_cell_extent, bitmap_grid.h:1236: a rectangle that misses the grid finds nobody
        const int32_t span_x = (int32_t)((uint32_t)P.grid_w << 12), span_y = (int32_t)((uint32_t)P.grid_h << 12);
        const bool hits_grid = !(imxx < P.origin_x || imxy < P.origin_y || imnx >= P.origin_x + span_x || imny >= P.origin_y + span_y);
        const int fid = rq.faction_id;
        const uint32_t enemies = P.enemy_mask[fid];
        for(int e0 = 0; hits_grid && e0 < P.n_ents; e0 += 256) {
            const int e = e0 + t;
            bool member = false, source = false, undecided = false;
            float x = 0.0f, z = 0.0f, radius = 0.0f;
            int ntiles = 0;
            if(e < P.n_ents) {
                x = P.pos_xz[2 * e]; z = P.pos_xz[2 * e + 1];
                const bool plain = fabsf(x) < SK_POS_LIMIT && fabsf(z) < SK_POS_LIMIT;     // false for NaN and infinity
                if(plain) {
                    const int32_t ix = bg_scale(x), iy = bg_scale(z);
                    member = ix >= imnx && ix <= imxx && iy >= imny && iy <= imxy;
                }
                if(member || !plain) {
                    const uint32_t fl = P.flags[e];
                    const int fac = P.faction[e];
                    const bool passes = !(fl & NAVHIP_ENTITY_FLAG_GARRISONED) && fac != fid && (fl & NAVHIP_ENTITY_FLAG_COMBATABLE)
                                     && fac >= 0 && fac <= 15 && ((enemies >> fac) & 1u) && !(P.exclude && P.exclude[e]);
                    if(passes) {
                        radius = P.radius[e];
                        if(!plain || (fl & NAVHIP_ENTITY_FLAG_BUILDING) || !sk_radius_fits(radius, ncont, &ntiles)) undecided = true;
                        else source = true;
                    }
                }
            }
            const uint64_t mm = __ballot(member);
            if(lane == 0 && mm) atomicAdd(&s_members, __popcll(mm));
            if(undecided) s_host = 1;
            uint64_t ms = __ballot(source);
            while(ms) {
                const int b = __builtin_ctzll(ms);
                ms &= ms - 1;
                sk_raster(P, __shfl(x, b), __shfl(z, b), __shfl(radius, b), __shfl(ntiles, b), ncont, base_r, base_c, bits, lane);
            }
        }
    }
    __syncthreads();
    host = host || s_host || s_members > SK_MAX_ENTS;

    // ---- the frontier: the set bits in row-major order ------------------------------------------
    const uint32_t w0 = bits[2 * t], w1 = bits[2 * t + 1];
    const int cnt = host ? 0 : __popc(w0) + __popc(w1);
    int incl = cnt;
#pragma unroll
    for(int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if(lane >= d) incl += o;
    }
    if(lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int before = incl - cnt, total = 0;
    for(int k = 0; k < 4; k++) { if(k < wave) before += s_wsum[k]; total += s_wsum[k]; }
    if(!host) {
        int16_t *out = arena + (size_t)ri * SK_MAX_SEEDS * 2 + (size_t)before * 2;
        for(int half = 0; half < 2; half++) {
            uint32_t m = half ? w1 : w0;
            const int r = (2 * t + half) >> 2, c0 = ((2 * t + half) & 3) * 32;
            while(m) {
                const int b = __builtin_ctz(m);
                m &= m - 1;
                out[0] = (int16_t)(base_r + r); out[1] = (int16_t)(base_c + c0 + b);
                out += 2;
            }
        }
        if(seed_bits) {
            uint8_t *sb = seed_bits + (size_t)ri * (SK_RDIM * SK_RDIM / 8) + 8 * t;
            for(int k = 0; k < 4; k++) { sb[k] = (uint8_t)(w0 >> (8 * k)); sb[4 + k] = (uint8_t)(w1 >> (8 * k)); }
        }
    }
    if(t == 0) {
        navhip_region_req rr = {};
        rr.out_mode = 1;
        if(host || total == 0) {
            // nothing to integrate: a region off the map that reads no plane and reaches no tile of the slot
            rr.base_abs_r = -30000; rr.base_abs_c = -30000; rr.rdim = 2; rr.cdim = 2;
        }else{
            rr.layer = (uint8_t)layer;
            rr.base_abs_r = (int16_t)base_r; rr.base_abs_c = (int16_t)base_c;
            rr.rdim = SK_RDIM; rr.cdim = SK_RDIM;
            rr.roff = (uint16_t)(cr > 0 ? 32 : 0); rr.coff = (uint16_t)(cc > 0 ? 32 : 0);      // field.c:1596-1597
            rr.seed_begin = (uint32_t)ri * SK_MAX_SEEDS; rr.seed_count = (uint32_t)total;
        }
        rreqs[ri] = rr;
        out_status[ri] = host ? NAVHIP_SK_HOST : 0;
    }
}

#define SK_FAIL(why) nh_fail(ctx, NAVHIP_ERR_INVALID, "navhip_build_seek_fields: ", why)

// the checks both forms make before anything is launched
static int sk_check(navhip_ctx *ctx, const navhip_world *w, const navhip_seek_game *g, const void *reqs, int n,
                    const void *inout, size_t stride, const void *status)
{
    if(n < 0) return SK_FAIL("a negative count");
    if(!w || !g) return SK_FAIL("a missing array (world or game)");
    if(w->n_ents < 0) return SK_FAIL("a negative n_ents");
    if(stride < NH_CELLS) return SK_FAIL("a stride below 4096");
    if(n > 0 && (!reqs || !inout || !status)) return SK_FAIL("a missing array (reqs, inout or out_status)");
    if(w->n_ents > 0 && (!w->pos_xz || !w->radius || !w->flags || !g->faction))
        return SK_FAIL("a missing array (pos_xz, radius, flags or faction)");
    return NAVHIP_OK;
}

extern "C" {

int navhip_build_seek_fields_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_seek_game *g,
                                 const navhip_seek_req *dev_reqs, int n, uint8_t *dev_inout, size_t stride,
                                 uint8_t *dev_status, uint8_t *dev_seed_bits, void *stream)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    int rc = sk_check(ctx, w, g, dev_reqs, n, dev_inout, stride, dev_status);
    if(rc) return rc;
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;

    sk_params P;
    P.w = ctx->w; P.h = ctx->h; P.map_x = w->map_pos_x; P.map_z = w->map_pos_z;
    // bg_ent_init, bitmap_grid.h:968-990
    P.origin_x = (int32_t)lrintf(w->grid_xmin * 256.0f); P.origin_y = (int32_t)lrintf(w->grid_zmin * 256.0f);
    const int32_t span_x = (int32_t)lrintf(w->grid_xmax * 256.0f) - P.origin_x, span_y = (int32_t)lrintf(w->grid_zmax * 256.0f) - P.origin_y;
    if(span_x < 0 || span_y < 0) return SK_FAIL("grid bounds with max below min");
    P.grid_w = (int)(((uint32_t)span_x + 4095u) >> 12); P.grid_h = (int)(((uint32_t)span_y + 4095u) >> 12);
    if(P.grid_w < 1) P.grid_w = 1;
    if(P.grid_h < 1) P.grid_h = 1;
    P.n_ents = w->n_ents; P.pos_xz = w->pos_xz; P.radius = w->radius; P.flags = w->flags;
    P.faction = g->faction; P.exclude = g->exclude;
    for(int f = 0; f < 16; f++) P.enemy_mask[f] = g->enemy_mask[f];
    P.layer_ok = 0;
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++)
        if(ctx->layers[l].cost && ctx->layers[l].blockers) P.layer_ok |= 1u << l;

    // the region requests, then the seed pairs
    const size_t req_bytes = nh_up256((size_t)n * sizeof(navhip_region_req));
    rc = nh_ensure(ctx, ctx->seek_scratch, req_bytes + (size_t)n * SK_MAX_SEEDS * 4);
    if(rc) return rc;
    navhip_region_req *d_rreqs = (navhip_region_req*)ctx->seek_scratch.p;
    int16_t *d_arena = (int16_t*)((char*)ctx->seek_scratch.p + req_bytes);
    hipLaunchKernelGGL(k_seek_seeds, dim3(n), dim3(256), 0, s, P, dev_reqs, n, d_arena, d_rreqs, dev_status, dev_seed_bits);
    HIPCHK(ctx, hipGetLastError());
    return navhip_build_region_fields_dev(ctx, d_rreqs, n, SK_RDIM, d_arena, nullptr, dev_inout, stride, s);
}

int navhip_build_seek_fields(navhip_ctx *ctx, const navhip_world *w, const navhip_seek_game *g,
                             const navhip_seek_req *reqs, int n, uint8_t *inout, size_t stride,
                             uint8_t *out_status, uint8_t *out_seed_bits)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    int rc = sk_check(ctx, w, g, reqs, n, inout, stride, out_status);
    if(rc) return rc;
    for(int i = 0; i < n; i++)
        if(reqs[i].kind > NAVHIP_SEEK_ENTITY || reqs[i].layer >= NAVHIP_NAV_LAYER_MAX)
            return SK_FAIL("malformed request " + std::to_string(i) + " (a kind above 1 or no such layer)");
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t ne = (size_t)w->n_ents, bytes = (size_t)n * stride, sb_bytes = (size_t)n * (SK_RDIM * SK_RDIM / 8);
    navhip_world d;
    navhip_seek_game dg = *g;
    const navhip_seek_req *d_reqs;
    uint8_t *d_inout, *d_status, *d_bits = nullptr;
    // the three arrays of the snapshot in the world's own slots (which drops a resident snapshot), the rest in one arena
    rc = nh_stage_world(ctx, w, &d, s, {offsetof(navhip_world, pos_xz), offsetof(navhip_world, radius), offsetof(navhip_world, flags)});
    if(rc) return rc;
    nh_plan P;
    P.in(reqs, (size_t)n * sizeof(navhip_seek_req), 0, (void**)&d_reqs);
    if(g->faction) P.in(g->faction, ne * 4, 16, (void**)&dg.faction);
    if(g->exclude) P.in(g->exclude, ne, 16, (void**)&dg.exclude);
    P.out(P.in(inout, bytes, 0, (void**)&d_inout), inout, 1, 0, bytes);       // the slots travel with what they hold
    P.out(P.scratch((size_t)n, (void**)&d_status), out_status, 1, 0, (size_t)n);
    // (rows that come back NAVHIP_SK_HOST keep what the caller's seed rows hold: they travel too)
    if(out_seed_bits) P.out(P.in(out_seed_bits, sb_bytes, 0, (void**)&d_bits), out_seed_bits, 1, 0, sb_bytes);
    rc = P.reserve(ctx, NH_STAGE_CALL0);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = navhip_build_seek_fields_dev(ctx, &d, &dg, d_reqs, n, d_inout, stride, d_status, d_bits, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

}   // extern "C"
