// arrival_build_kernels.hip -- the FIRST build of an arrival zone, the `!built` branch of G_Arrival_UpdateFlock
// (arrival.c:784-848), on the device: the gate (:785-788, arrival_near_goal :377), arrival_zone_radius (:363), the snapped
// centre (:801, N_ClosestPathable nav.c:4126), arrival_approach_axis (:236), arrival_build_slots (:181) over
// N_ClosestConnectedPathableTiles (nav.c:4192) and N_TileKeysForPositions (nav.c:4304), arrival_thin_centered_slots (:196),
// the clear-line filter (:810-817), the centre of mass with its snap and N_DestIDForPos (:819-830, nav.c:3367) and
// arrival_order_slots_far_near (:231).  The tail (:839-847: rings, counters, arrival_realloc_slots) is k_arrival_flock's
// first-build mode, launched behind this kernel on the same arrays.  Kernel AND its C entry points (include/navhip.h:
// navhip_arrival_zone_build[_dev]).
//
// One workgroup of four waves per zone; everything of the zone lives in LDS until the last HOST decision (the snap of
// the centre of mass) has been made, then the outputs are written.
//   - The two N_ClosestPathable floods are nav_flood.h's dq_flood on wave 0.
//   - The best-first flood pops by float priority with ties everywhere (every symmetric tile pair of a centre on a tile
//     centre), and the ties decide the order of out[] and which tiles of the last ring make the budget: ONE lane replays
//     the heap of pqueue.h operation for operation (pq_heap.h) with the visited bitmap of a window around the centre tile
//     in LDS.  The other lanes wait.
//   - The three sorts are rank sorts: element i goes to the number of elements that come before it, an element of equal
//     key and lower index included -- a stable order by construction, which is what glibc's qsort (a merge sort for
//     arrays of this size) gives the reference.  n * n comparisons spread over 256 lanes: n <= 4 096.
//   - The thinning pass is serial over the candidates and parallel over the kept slots: wave 0, a ballot per candidate.
//   - The centre of mass is an ORDERED float sum: lane 0.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <string>
#include "navhip_internal.h"
#include "agent_internal.h"
#include "agent_math.h"
#include "lane_group.h"
#include "nav_flood.h"          // dq_map, dq_probe, dq_tile_for_point, dq_delta, dq_flood: N_ClosestPathable
#include "arrival_region.h"     // af_key, af_zone_radius, af_region_area, sk_segment_within
#include "pq_heap.h"
#include "stage_plan.h"

#define AB_CAP      NAVHIP_ARRIVAL_MAX_SLOTS
#define AB_THREADS  256
#define AB_WIN      NAVHIP_AB_WINDOW_R            /* |dr|, |dc| <= AB_WIN around the centre tile                          */
#define AB_SIDE     256                           /* bits per row of the visited bitmap: 2 * AB_WIN + 1 <= AB_SIDE        */
#define AB_HEAP     NAVHIP_AB_HEAP_NODES
static_assert(2 * AB_WIN + 1 <= AB_SIDE, "the window must fit the bitmap");

// 32 + 32 + 16 + 48 + 8 + 4 + 2 KiB = 142 KiB of the 160 KiB a workgroup can have on gfx950
struct ab_lds {
    uint64_t keys[AB_CAP];                                      // region_keys, ascending
    float    slot_x[AB_CAP], slot_z[AB_CAP];                    // the slots, in the order of the phase
    union {
        uint32_t ftile[AB_CAP];                                 // the flood's out[] as absolute tiles (r << 16 | c)
        float    skey[AB_CAP];                                  // the float key of a slot sort
    } a;
    union {
        struct { float prio[AB_HEAP + 2]; uint32_t tile[AB_HEAP + 2]; } heap;
        uint64_t raw[AB_CAP];                                   // td_keys in flood order
        struct { float x[AB_CAP], z[AB_CAP]; int32_t band[AB_CAP]; } tmp;
    } u;
    uint32_t visited[AB_SIDE * AB_SIDE / 32];
    uint16_t fr[2][DQ_FRONTIER];                                // dq_flood's frontier and ring words
    uint32_t ring[DQ_FRONTIER];
    float    stage_x[AB_THREADS], stage_z[AB_THREADS];
    float    sum_x, sum_z, centre_x, centre_z, com_x, com_z;
    int32_t  n, kept, host;
    uint32_t com_dest_id;
};

// N_ClosestPathable(p) ? snapped : p, on one wave.  false: the reference asserts (p is NaN or off the map), or the flood
// leaves dq_flood's window.
__device__ bool ab_closest_pathable(const dq_map &M, const dq_layer &Ld, ab_lds &L, float px, float pz, float *ox, float *oz)
{
    int sr = 0, sc = 0;
    if(!dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, px, pz, &sr, &sc)) return false;
    *ox = px; *oz = pz;
    if(dq_probe(M, Ld, sr, sc) == 1u) return true;                              // nav.c:4141-4144
    int ar = 0, ac = 0;
    const int rc = dq_flood<false>(M, Ld, sr, sc, 0, L.fr, L.ring, &ar, &ac, nullptr, nullptr);
    if(rc < 0) return false;
    if(rc > 0) {                                                                // M_Tile_Bounds .x / .z (tile.c:356)
        *ox = (M.map_x - (float)((ac >> 6) * 256)) - (float)((ac & 63) * 4);
        *oz = (M.map_z + (float)((ar >> 6) * 256)) + (float)((ar & 63) * 4);
    }
    return true;
}

// the rows of a zone that is not built go out as they came in (out may alias in: every element is read and written by one
// lane); rooms: the zone's ranges lie inside the shared arrays
__device__ void ab_repeat(const navhip_arrival_build_in &in, const navhip_arrival_build_out &out, int zi, const navhip_arrival_zone &Z,
                          const navhip_arrival_flock &S, bool rooms, bool members, uint8_t status)
{
    const int tid = (int)threadIdx.x;
    if(rooms) {
        for(int i = Z.slot_begin + tid; i < Z.slot_end; i += AB_THREADS) {
            const float x = in.slots_xz[2 * i], z = in.slots_xz[2 * i + 1];
            const int32_t r = in.slot_ring[i];
            out.slots_xz[2 * i] = x; out.slots_xz[2 * i + 1] = z; out.slot_ring[i] = r;
        }
        for(int k = Z.key_begin + tid; k < Z.key_end; k += AB_THREADS) { const uint64_t v = in.region_keys[k]; out.region_keys[k] = v; }
    }
    if(members)
        for(int m = S.member_begin + tid; m < S.member_end; m += AB_THREADS) {
            const uint8_t sub = in.substate[m], valid = in.sink_valid[m];
            const float sx = in.sink_xz[2 * m], sz = in.sink_xz[2 * m + 1];
            out.substate[m] = sub; out.sink_valid[m] = valid;
            out.sink_xz[2 * m] = sx; out.sink_xz[2 * m + 1] = sz;
        }
    if(tid == 0) { out.zones[zi] = Z; out.flocks[zi] = S; out.status[zi] = status; }
}

__global__ __launch_bounds__(AB_THREADS) void k_arrival_build(nh_step_params P, dq_map M, navhip_arrival_build_in in, navhip_arrival_build_out out)
{
    __shared__ ab_lds L;
    const int zi = (int)blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    navhip_arrival_zone Z = in.zones[zi];
    navhip_arrival_flock S = in.flocks[zi];
    const int mb = S.member_begin, me = S.member_end;
    const float tx = in.target_xz[2 * zi], tz = in.target_xz[2 * zi + 1];

    // ---- what cannot even be asked
    const bool rooms = Z.slot_begin >= 0 && Z.slot_end >= Z.slot_begin && Z.slot_end <= in.n_slots
                    && Z.key_begin >= 0 && Z.key_end >= Z.key_begin && Z.key_end <= in.n_keys;
    const bool members = mb >= 0 && me >= mb && me <= in.nm;
    const bool layer_ok = S.layer >= 0 && S.layer < NAVHIP_NAV_LAYER_MAX;
    const dq_layer Ld = M.layers[layer_ok ? S.layer : 0];
    bool host = !rooms || !members || !layer_ok || !Ld.probemask || !P.map.layers[layer_ok ? S.layer : 0].blockers
             || S.phase != NAVHIP_ARRIVAL_PHASE_INACTIVE || !(S.unit_radius > 0.0f && S.unit_radius < INFINITY);
    bool bad_uid = false, near = false;
    if(members)
        for(int m = mb + tid; m < me; m += AB_THREADS) {
            const int uid = in.uid[m];
            if(uid < 0 || uid >= P.n_ents) { bad_uid = true; continue; }
            near = near || vlen(mkv(tx - P.pos_xz[2 * uid], tz - P.pos_xz[2 * uid + 1])) < 150.0f;    // ARRIVAL_FIELD_PLAN_RADIUS
        }
    host = __syncthreads_or(bad_uid || host) != 0;
    near = __syncthreads_or(near) != 0;
    if(host) { ab_repeat(in, out, zi, Z, S, rooms, members, NAVHIP_AB_HOST); return; }
    // ---- the gate, arrival.c:785-788
    if(S.total_members < 4 || !near) { ab_repeat(in, out, zi, Z, S, true, true, NAVHIP_AB_WAIT); return; }

    const int radius = af_zone_radius(S.total_members, S.unit_radius);
    const int area = af_region_area(radius);
    const int slot_room = Z.slot_end - Z.slot_begin, key_room = Z.key_end - Z.key_begin;
    if(key_room < area || slot_room < (S.total_members < area ? S.total_members : area)) {
        ab_repeat(in, out, zi, Z, S, true, true, NAVHIP_AB_HOST);
        return;
    }

    // ---- the centre (:801) on wave 0; the bitmap and the sums meanwhile
    for(int i = tid; i < AB_SIDE * AB_SIDE / 32; i += AB_THREADS) L.visited[i] = 0u;
    if(tid == 0) { L.sum_x = 0.0f; L.sum_z = 0.0f; L.host = 0; L.n = 0; L.kept = 0; }
    __syncthreads();
    if(wave == 0) {
        float cx = 0.0f, cz = 0.0f;
        const bool ok = ab_closest_pathable(M, Ld, L, tx, tz, &cx, &cz);
        if(lane == 0) { L.centre_x = cx; L.centre_z = cz; if(!ok) L.host = 1; }
    }
    __syncthreads();
    if(L.host) { ab_repeat(in, out, zi, Z, S, true, true, NAVHIP_AB_HOST); return; }
    const v2 centre = mkv(L.centre_x, L.centre_z);

    // ---- arrival_approach_axis (:236): the member positions summed IN MEMBER ORDER -- runs of AB_THREADS members are
    // fetched by the lanes, lane 0 adds each run in order
    for(int base = mb; base < me; base += AB_THREADS) {
        const int m = base + tid;
        if(m < me) {
            const int uid = in.uid[m];
            L.stage_x[tid] = P.pos_xz[2 * uid]; L.stage_z[tid] = P.pos_xz[2 * uid + 1];
        }
        __syncthreads();
        if(tid == 0) {
            float sx = L.sum_x, sz = L.sum_z;
            const int n = me - base < AB_THREADS ? me - base : AB_THREADS;
            for(int j = 0; j < n; j++) { sx = sx + L.stage_x[j]; sz = sz + L.stage_z[j]; }
            L.sum_x = sx; L.sum_z = sz;
        }
        __syncthreads();
    }
    v2 axis;
    {
        const float inv = nh_fdiv(1.0f, (float)(me - mb));                      // PFM_Vec2_Scale(&centroid, 1.0f / n, &centroid)
        const v2 d = mkv(tx - L.sum_x * inv, tz - L.sum_z * inv);
        axis = vlen(d) > CP_EPS ? vnormal(d) : mkv(0.0f, 1.0f);                 // EPSILON 1.0f / 1024
    }

    // ---- N_ClosestConnectedPathableTiles (nav.c:4192), maxout = area, max_radius = 0: one lane
    if(tid == 0) {
        int cr = 0, cc = 0, n = 0, bad = 0;
        if(dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, centre.x, centre.z, &cr, &cc)) {
            const int max_r = M.h * 64, max_c = M.w * 64;
            pq_heap H;
            H.prio = L.u.heap.prio; H.data = L.u.heap.tile; H.size = 0; H.cap = AB_HEAP;
            L.visited[(128 * AB_SIDE + 128) >> 5] |= 1u << ((128 * AB_SIDE + 128) & 31);
            pq_heap_push(H, 0.0f, (128u << 8) | 128u);                          // the centre tile, blocked or not
            while(H.size > 0 && n < area && !bad) {
                const uint32_t t = pq_heap_pop(H);
                const int dr = (int)(t >> 8) - 128, dc = (int)(t & 255u) - 128;
                const int r = cr + dr, c = cc + dc;
                if(dq_probe(M, Ld, r, c) == 1u) {                               // !n_tile_blocked, nav.c:235
                    L.a.ftile[n++] = ((uint32_t)r << 16) | (uint32_t)c;
                    if(n == area) break;                                        // (the pushes behind the last tile change nothing)
                }
                for(int j = 1; j <= 8; j++) {                                   // the reference's delta order: nav_flood.h
                    int ddr, ddc;
                    dq_delta<true>(j, &ddr, &ddc);
                    const int nr = r + ddr, nc = c + ddc, ndr = dr + ddr, ndc = dc + ddc;
                    if(nr < 0 || nr >= max_r || nc < 0 || nc >= max_c) continue;            // M_Tile_RelativeDesc
                    if(ndr < -AB_WIN || ndr > AB_WIN || ndc < -AB_WIN || ndc > AB_WIN) { bad = 1; break; }
                    const int bit = (ndr + 128) * AB_SIDE + (ndc + 128);
                    if((L.visited[bit >> 5] >> (bit & 31)) & 1u) continue;
                    L.visited[bit >> 5] |= 1u << (bit & 31);
                    if(dq_probe(M, Ld, nr, nc) != 1u) continue;                 // visited, never pushed
                    const float px = M.map_x - ((float)nc + 0.5f) * 4.0f;
                    const float pz = M.map_z + ((float)nr + 0.5f) * 4.0f;
                    const float dx = px - centre.x, dz = pz - centre.z;
                    if(!pq_heap_push(H, dx * dx + dz * dz, ((uint32_t)(ndr + 128) << 8) | (uint32_t)(ndc + 128))) { bad = 1; break; }
                }
            }
        }
        L.n = n; L.host = bad;
    }
    __syncthreads();
    if(L.host) { ab_repeat(in, out, zi, Z, S, true, true, NAVHIP_AB_HOST); return; }
    const int n = L.n;

    // ---- the tile centres (nav.c:4248) and N_TileKeysForPositions (nav.c:4304): td_key of every tile, ascending
    for(int i = tid; i < n; i += AB_THREADS) {
        const int r = (int)(L.a.ftile[i] >> 16), c = (int)(L.a.ftile[i] & 0xffffu);
        L.slot_x[i] = M.map_x - ((float)c + 0.5f) * 4.0f;
        L.slot_z[i] = M.map_z + ((float)r + 0.5f) * 4.0f;
        L.u.raw[i] = af_key(r >> 6, c >> 6, r & 63, c & 63);
    }
    __syncthreads();
    for(int i = tid; i < n; i += AB_THREADS) {
        const uint64_t k = L.u.raw[i];
        int rank = 0;
        for(int j = 0; j < n; j++) rank += L.u.raw[j] < k ? 1 : 0;
        L.keys[rank] = k;
    }
    __syncthreads();

    // ---- arrival_thin_centered_slots (:196): nearest the pushed-forward reference first, ties in flood order
    {
        const v2 ref = mkv(centre.x + axis.x * 8.0f, centre.z + axis.z * 8.0f);     // (ARRIVAL_ZONE_PAD - 1) * tile_dim
        for(int i = tid; i < n; i += AB_THREADS) {
            const v2 d = mkv(L.slot_x[i] - ref.x, L.slot_z[i] - ref.z);
            L.a.skey[i] = vdot(d, d);
        }
        __syncthreads();
        for(int i = tid; i < n; i += AB_THREADS) {
            const float k = L.a.skey[i];
            int rank = 0;
            for(int j = 0; j < n; j++) {
                const float o = L.a.skey[j];
                rank += (o < k || (!(o > k) && j < i)) ? 1 : 0;
            }
            L.u.tmp.x[rank] = L.slot_x[i]; L.u.tmp.z[rank] = L.slot_z[i];
        }
        __syncthreads();
        for(int i = tid; i < n; i += AB_THREADS) { L.slot_x[i] = L.u.tmp.x[i]; L.slot_z[i] = L.u.tmp.z[i]; }
        __syncthreads();
    }
    if(wave == 0) {
        const float spacing = 1.85f * S.unit_radius, sp2 = spacing * spacing;      // ARRIVAL_SLOT_SPACING
        int kept = 0;
        for(int i = 0; i < n && kept < S.total_members; i++) {
            const v2 cand = mkv(L.slot_x[i], L.slot_z[i]);
            bool close = false;
            for(int j = lane; j < kept; j += 64) {
                const v2 d = mkv(cand.x - L.slot_x[j], cand.z - L.slot_z[j]);
                close = close || vdot(d, d) < sp2;
            }
            if(__ballot(close) != 0ull) continue;
            if(lane == 0) { L.slot_x[kept] = cand.x; L.slot_z[kept] = cand.z; }
            kept++;
            wave_sync();
        }
        if(lane == 0) L.kept = kept;
    }
    __syncthreads();

    // ---- the clear-line filter (:810-817), order preserved
    int kept = L.kept;
    for(int i = tid; i < kept; i += AB_THREADS)
        L.u.tmp.band[i] = sk_segment_within(P, centre, mkv(L.slot_x[i], L.slot_z[i]), L.keys, n) ? 1 : 0;
    __syncthreads();
    if(wave == 0) {
        int cnt = 0;
        for(int base = 0; base < kept; base += 64) {
            const int i = base + lane;
            const bool on = i < kept && L.u.tmp.band[i] != 0;
            const unsigned long long mask = __ballot(on);
            if(on) {
                const int at = cnt + __popcll(mask & ((1ull << lane) - 1ull));
                L.u.tmp.x[at] = L.slot_x[i]; L.u.tmp.z[at] = L.slot_z[i];
            }
            cnt += __popcll(mask);
        }
        if(lane == 0) L.kept = cnt;
    }
    __syncthreads();
    const int num = L.kept;
    for(int i = tid; i < num; i += AB_THREADS) { L.slot_x[i] = L.u.tmp.x[i]; L.slot_z[i] = L.u.tmp.z[i]; }
    __syncthreads();

    // ---- the centre of mass (:819-830): sums in slot order on one lane, then its snap and its dest id on wave 0
    if(tid == 0) {
        float cx = 0.0f, cz = 0.0f;
        for(int i = 0; i < num; i++) { cx = cx + L.slot_x[i]; cz = cz + L.slot_z[i]; }
        if(num > 0) { cx = nh_fdiv(cx, (float)num); cz = nh_fdiv(cz, (float)num); }
        L.com_x = cx; L.com_z = cz;
    }
    __syncthreads();
    if(wave == 0) {
        float cx = 0.0f, cz = 0.0f;
        int r = 0, c = 0;
        const bool ok = ab_closest_pathable(M, Ld, L, L.com_x, L.com_z, &cx, &cz)
                     && dq_tile_for_point(M.w, M.h, M.map_x, M.map_z, cx, cz, &r, &c);
        if(lane == 0) {
            L.com_x = cx; L.com_z = cz;
            if(!ok) L.host = 1;
            L.com_dest_id = ((uint32_t)((r >> 6) & 0x3f) << 26) | ((uint32_t)((c >> 6) & 0x3f) << 20) | ((uint32_t)(r & 0x3f) << 14)       // n_dest_id, nav.c:839
                          | ((uint32_t)(c & 0x3f) << 8) | ((uint32_t)(S.layer & 0xf) << 4) | (uint32_t)NAVHIP_FACTION_ID_NONE;
        }
    }
    __syncthreads();
    if(L.host) { ab_repeat(in, out, zi, Z, S, true, true, NAVHIP_AB_HOST); return; }

    // ---- arrival_order_slots_far_near (:231, slot_cmp_far_banded :130) around the centre: the deeper band first, lateral
    // inside a band, ties in the order the filter left
    {
        const float band_w = 1.85f * S.unit_radius;
        const v2 perp = mkv(-axis.z, axis.x);
        for(int i = tid; i < num; i += AB_THREADS) {
            const v2 r = mkv(L.slot_x[i] - centre.x, L.slot_z[i] - centre.z);
            L.u.tmp.band[i] = (int)floorf(nh_fdiv(vdot(r, axis), band_w));
            L.a.skey[i] = vdot(r, perp);
        }
        __syncthreads();
        float *sx = out.slots_xz + 2 * (size_t)Z.slot_begin;
        int32_t *ring = out.slot_ring + Z.slot_begin;
        for(int i = tid; i < num; i += AB_THREADS) {
            const int b = L.u.tmp.band[i];
            const float k = L.a.skey[i];
            int rank = 0;
            for(int j = 0; j < num; j++) {
                const int ob = L.u.tmp.band[j];
                const float o = L.a.skey[j];
                rank += (ob > b || (ob == b && (o < k || (!(o > k) && j < i)))) ? 1 : 0;
            }
            sx[2 * rank] = L.slot_x[i]; sx[2 * rank + 1] = L.slot_z[i];
            ring[rank] = 0;                                                    // (the tail's first pass ranks them)
        }
    }

    // ---- the zone as :791-794 and :839-846 leave it in front of arrival_realloc_slots
    uint64_t *keys = out.region_keys + Z.key_begin;
    for(int k = tid; k < n; k += AB_THREADS) keys[k] = L.keys[k];
    for(int m = mb + tid; m < me; m += AB_THREADS) {
        const uint8_t sub = in.substate[m], valid = in.sink_valid[m];
        const float sx = in.sink_xz[2 * m], sz = in.sink_xz[2 * m + 1];
        out.substate[m] = sub; out.sink_valid[m] = valid;
        out.sink_xz[2 * m] = sx; out.sink_xz[2 * m + 1] = sz;
    }
    if(tid == 0) {
        Z.centre_x = centre.x; Z.centre_z = centre.z;
        Z.unit_radius = S.unit_radius; Z.radius = radius; Z.layer = S.layer;
        Z.fill_frac = 0.0f; Z.active_row = 0; Z.num_rows = 0;
        Z.slot_end = Z.slot_begin + num; Z.key_end = Z.key_begin + n;
        S.phase = NAVHIP_ARRIVAL_PHASE_FILLING;
        S.realloc_counter = 0; S.stall_counter = 0; S.prev_occ = 0;
        S.row_height = 1.85f * S.unit_radius;
        out.zones[zi] = Z; out.flocks[zi] = S;
        out.axis_xz[2 * zi] = axis.x; out.axis_xz[2 * zi + 1] = axis.z;
        out.com_xz[2 * zi] = L.com_x; out.com_xz[2 * zi + 1] = L.com_z;
        out.com_dest_id[zi] = L.com_dest_id;
        out.status[zi] = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// C entry points
// ---------------------------------------------------------------------------------------------
namespace {

#define AB_FAIL(why) nh_fail(ctx, NAVHIP_ERR_ARG, name, why)     /* inside the check below: `name` is the form's */
// The one argument check of both forms; host_arrays: the arrays can be read here, so what lies IN them is checked too.
int ab_check(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_build_in *in, const navhip_arrival_build_out *out, bool host_arrays)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    const char *name = host_arrays ? "navhip_arrival_zone_build: " : "navhip_arrival_zone_build_dev: ";
    if(!w || !in || !out) return AB_FAIL("a missing argument");
    if(in->nm < 0) return AB_FAIL("nm < 0");
    if(in->n_zones < 0 || in->n_slots < 0 || in->n_keys < 0 || w->n_ents < 0) return AB_FAIL("a negative count");
    if(in->n_zones == 0) return NAVHIP_OK;
    if(!in->zones || !in->flocks || !in->target_xz) return AB_FAIL("a missing array: zones, flocks or target_xz");
    if(!out->zones || !out->flocks || !out->status || !out->axis_xz || !out->com_xz || !out->com_dest_id)
        return AB_FAIL("a missing array: zones, flocks, status, axis_xz, com_xz or com_dest_id of navhip_arrival_build_out");
    if(in->n_slots > 0 && (!in->slots_xz || !in->slot_ring || !out->slots_xz || !out->slot_ring)) return AB_FAIL("a missing array: slots_xz or slot_ring");
    if(in->n_keys > 0 && (!in->region_keys || !out->region_keys)) return AB_FAIL("a missing array: region_keys");
    if(in->nm > 0) {
        if(!w->pos_xz) return AB_FAIL("a missing array: world->pos_xz");
        if(!in->uid || !in->settled || !in->substate || !in->sink_valid || !in->sink_xz) return AB_FAIL("a missing array of the members");
        if(!out->substate || !out->sink_valid || !out->sink_xz) return AB_FAIL("a missing array of the members of navhip_arrival_build_out");
    }
    if(!host_arrays) return NAVHIP_OK;
    for(int z = 0; z < in->n_zones; z++) {
        const navhip_arrival_zone &Z = in->zones[z];
        const navhip_arrival_flock &S = in->flocks[z];
        const std::string zn = "zone " + std::to_string(z);
        if(const char *fault = nh_zone_fault(Z, &S, in->n_slots, in->n_keys, in->nm, nullptr)) return AB_FAIL(zn + fault);
        // room is asked of a zone the kernel would go on to build: one it answers NAVHIP_AB_HOST or NAVHIP_AB_WAIT in front
        // of its own room test (a layer without planes, a uid outside the world, nobody near the goal) needs none
        if(S.phase != NAVHIP_ARRIVAL_PHASE_INACTIVE || S.total_members < 4 || !(S.unit_radius > 0.0f && S.unit_radius < INFINITY)) continue;
        if(S.layer < 0 || S.layer >= NAVHIP_NAV_LAYER_MAX || !ctx->layers[S.layer].cost || !ctx->layers[S.layer].blockers) continue;
        bool bad_uid = false, near = false;
        for(int m = S.member_begin; m < S.member_end; m++) {
            const int uid = in->uid[m];
            if(uid < 0 || uid >= w->n_ents) { bad_uid = true; break; }
            const float dx = in->target_xz[2 * z] - w->pos_xz[2 * uid], dz = in->target_xz[2 * z + 1] - w->pos_xz[2 * uid + 1];
            near = near || sqrtf(dx * dx + dz * dz) < 150.0f;                   // arrival_near_goal, as the kernel computes it
        }
        if(bad_uid || !near) continue;
        const int area = af_region_area(af_zone_radius(S.total_members, S.unit_radius));
        const int slots = S.total_members < area ? S.total_members : area;
        if(Z.key_end - Z.key_begin < area || Z.slot_end - Z.slot_begin < slots)
            return AB_FAIL(zn + ": too little room: it needs " + std::to_string(area) + " keys and " + std::to_string(slots) + " slots");
    }
    return NAVHIP_OK;
}

// the two structs of the host form, row by row (stage_plan.h)
const nh_row ab_in_rows[] = {
    NH_ROW(navhip_arrival_build_in, zones, sizeof(navhip_arrival_zone), NH_LEN_ZONE, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_build_in, flocks, sizeof(navhip_arrival_flock), NH_LEN_ZONE, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_build_in, target_xz, 8, NH_LEN_ZONE, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_build_in, slots_xz, 8, NH_LEN_SLOT, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_build_in, slot_ring, 4, NH_LEN_SLOT, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_build_in, region_keys, 8, NH_LEN_KEY, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_build_in, uid, 4, NH_LEN_MEMBER, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_build_in, settled, 1, NH_LEN_MEMBER, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_build_in, substate, 1, NH_LEN_MEMBER, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_build_in, sink_valid, 1, NH_LEN_MEMBER, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_build_in, sink_xz, 8, NH_LEN_MEMBER, NH_ON_ALWAYS),
};
// (axis, com and dest id of a row that is not built are not written: they go up, and back as they came)
const nh_row ab_out_rows[] = {
    NH_ROW_OUT_PAD(navhip_arrival_build_out, zones, sizeof(navhip_arrival_zone), NH_LEN_ZONE, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_build_out, flocks, sizeof(navhip_arrival_flock), NH_LEN_ZONE, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_build_out, slots_xz, 8, NH_LEN_SLOT, NH_ON_ALWAYS, 16),  NH_ROW_OUT_PAD(navhip_arrival_build_out, slot_ring, 4, NH_LEN_SLOT, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_build_out, region_keys, 8, NH_LEN_KEY, NH_ON_ALWAYS, 16),  NH_ROW_IO(navhip_arrival_build_out, axis_xz, 8, NH_LEN_ZONE, NH_ON_ALWAYS, 16),
    NH_ROW_IO(navhip_arrival_build_out, com_xz, 8, NH_LEN_ZONE, NH_ON_ALWAYS, 16),  NH_ROW_IO(navhip_arrival_build_out, com_dest_id, 4, NH_LEN_ZONE, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_build_out, substate, 1, NH_LEN_MEMBER, NH_ON_ALWAYS, 16),  NH_ROW_OUT_PAD(navhip_arrival_build_out, sink_valid, 1, NH_LEN_MEMBER, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_build_out, sink_xz, 8, NH_LEN_MEMBER, NH_ON_ALWAYS, 16),  NH_ROW_OUT_PAD(navhip_arrival_build_out, status, 1, NH_LEN_ZONE, NH_ON_ALWAYS, 16),
};
NH_COVERS(ab_in_rows, navhip_arrival_build_in, 16);         // n_zones, nm, n_slots, n_keys
NH_COVERS(ab_out_rows, navhip_arrival_build_out, 0);

}   // namespace

extern "C" {

int navhip_arrival_zone_build_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_build_in *in,
                                  const navhip_arrival_build_out *out, void *stream)
{
    int rc = ab_check(ctx, w, in, out, false);
    if(rc || in->n_zones == 0) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    rc = nh_refresh_derived(ctx, s);              // the probemask rows of uploads since the last build
    if(rc) return rc;
    nh_step_params P;
    nh_step_params_init(ctx, w, &P);
    P.pos_xz = w->pos_xz;
    const dq_map M = dq_map_of(ctx, w->map_pos_x, w->map_pos_z);
    hipLaunchKernelGGL(k_arrival_build, dim3(in->n_zones), dim3(AB_THREADS), 0, s, P, M, *in, *out);
    HIPCHK(ctx, hipGetLastError());
    // ---- the tail (:839-847): k_arrival_flock on what the build left, for the zones it built
    navhip_arrival_flock_in fi = {};
    fi.n_zones = in->n_zones; fi.nm = in->nm; fi.n_slots = in->n_slots; fi.n_keys = in->n_keys;
    fi.zones = out->zones; fi.flocks = out->flocks;
    fi.slots_xz = out->slots_xz; fi.slot_ring = out->slot_ring; fi.region_keys = out->region_keys;
    fi.uid = in->uid; fi.settled = in->settled;
    fi.substate = out->substate; fi.sink_valid = out->sink_valid; fi.sink_xz = out->sink_xz;
    navhip_arrival_flock_out fo = {};
    fo.zones = out->zones; fo.flocks = out->flocks; fo.slot_ring = out->slot_ring;
    fo.substate = out->substate; fo.sink_valid = out->sink_valid; fo.sink_xz = out->sink_xz; fo.status = out->status;
    nh_launch_arrival_first_realloc(P, fi, fo, out->status, s);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_arrival_zone_build(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_build_in *in, const navhip_arrival_build_out *out)
{
    int rc = ab_check(ctx, w, in, out, true);
    if(rc || in->n_zones == 0) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    nh_dims D;
    D.len[NH_LEN_UNIT] = (size_t)w->n_ents; D.len[NH_LEN_ZONE] = (size_t)in->n_zones; D.len[NH_LEN_MEMBER] = (size_t)in->nm;
    D.len[NH_LEN_SLOT] = (size_t)in->n_slots; D.len[NH_LEN_KEY] = (size_t)in->n_keys;
    D.pad = 16;                                                             // (no input array of a slot-less or member-less call is empty; the result rows pad themselves)
    nh_plan P;
    navhip_world d = *w;
    navhip_arrival_build_in di = *in;
    navhip_arrival_build_out dout = {};
    P.in(in->nm ? w->pos_xz : nullptr, D.len[NH_LEN_UNIT] * 8, D.pad, (void**)&d.pos_xz);    // (no members: the positions do not travel)
    nh_plan_rows(P, ab_in_rows, in, &di, D);
    nh_plan_rows(P, ab_out_rows, out, &dout, D);
    rc = P.reserve(ctx, NH_STAGE_CALL0);
    if(!rc) rc = P.upload(ctx, s);
    if(rc) return rc;
    // (a built zone writes its new ranges only: what the rooms hold behind them goes back as it came)
    const size_t ns = D.len[NH_LEN_SLOT], nkeys = D.len[NH_LEN_KEY];
    if(ns) HIPCHK(ctx, hipMemcpyAsync(dout.slots_xz, di.slots_xz, ns * 8, hipMemcpyDeviceToDevice, s));
    if(ns) HIPCHK(ctx, hipMemcpyAsync(dout.slot_ring, di.slot_ring, ns * 4, hipMemcpyDeviceToDevice, s));
    if(nkeys) HIPCHK(ctx, hipMemcpyAsync(dout.region_keys, di.region_keys, nkeys * 8, hipMemcpyDeviceToDevice, s));
    rc = navhip_arrival_zone_build_dev(ctx, &d, &di, &dout, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

}   // extern "C"
