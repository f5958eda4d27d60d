// arrival_flock_kernels.hip -- the built-zone branch of G_Arrival_UpdateFlock (arrival.c:767-853) on the device: the
// all-settled arm, arrival_zone_radius (:363), the realloc period, and arrival_realloc_slots (:391-516) with
// arrival_compute_geodesic_rings (:257-302) over N_RegionGeodesicDist (nav.c:4389-4460).  The first build of a zone
// (:784-848) is arrival_build_kernels.hip's, which launches this kernel for its tail (first_build below).  Kernel AND
// its C entry points (include/navhip.h: navhip_arrival_flock_update[_dev]).
//
// One workgroup of four waves per zone.  The zone's keys, BFS distances, slots, slot rings, occupied bits and per-ring
// counters live in LDS (the reference caps keys and slots at ARRIVAL_MAX_SLOTS = 4 096 each).  Every part of the rule
// but two is independent of evaluation order -- BFS distances are unique, occupied[] is an OR, every sink is an argmin
// of its own -- and is spread over the lanes; the entry centroid is an ORDERED float sum and the frontier a scalar
// epilogue: both run on lane 0.  The member-by-slot searches take a wave per member: the lanes stride over the slots
// with the key (float bits of dd, slot index), the wave takes the minimum -- the reference's strict `<` from INFINITY
// (the earliest of equal dd, never a dd that is not < INFINITY).
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <string>
#include "navhip_internal.h"
#include "agent_internal.h"
#include "agent_math.h"
#include "arrival_region.h"     // af_key, af_key_index, af_zone_radius
#include "stage_plan.h"

#define AF_CAP      4096        /* ARRIVAL_MAX_SLOTS, arrival.h:47: slots, keys and so rows of a zone           */
#define AF_THREADS  256
#define AF_WAVES    (AF_THREADS / 64)

struct af_lds {
    uint64_t keys[AF_CAP];              // the zone's region_keys, ascending
    float    slot_x[AF_CAP], slot_z[AF_CAP];
    int32_t  cap[AF_CAP], occ[AF_CAP];  // per ring
    int16_t  dist[AF_CAP];              // BFS distance per key, -1 = unreached
    uint16_t ring[AF_CAP];              // slot_ring
    uint32_t occupied[AF_CAP / 32];     // one bit per slot
    float    stage_x[AF_THREADS], stage_z[AF_THREADS];   // a run of members' positions for the ordered sum
    uint8_t  stage_on[AF_THREADS];
    uint32_t red_key[AF_WAVES];
    int32_t  red_at[AF_WAVES];
    float    entry_x, entry_z;
    int32_t  entry_cnt, maxd, total_occ, crowd;
    int32_t  active_row, num_rows;
};

// the least (key, index) of a wave, on every lane
__device__ __forceinline__ void af_wave_min(uint32_t &key, int &at)
{
#pragma unroll
    for(int d = 32; d >= 1; d >>= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)key, d);
        const int      oi = __shfl_xor(at, d);
        if(ok < key || (ok == key && oi < at)) { key = ok; at = oi; }
    }
}

// index of the key of the point's tile, -1 off the map or off the region (arrival_in_region, arrival.c:153: the walk of
// N_SegmentWithinRegion from a point to itself is its tile)
__device__ __forceinline__ int af_point_key(const nh_step_params &P, float x, float z, const uint64_t *keys, int num)
{
    tiledesc t;
    if(num == 0 || !tile_for_point(P, x, z, t)) return -1;
    return af_key_index(keys, num, af_key(t.chunk_r, t.chunk_c, t.tile_r, t.tile_c));
}

// a member's rows go out as they came in (out may alias in: every row is read and written by one lane)
__device__ __forceinline__ void af_copy_member(const navhip_arrival_flock_in &in, const navhip_arrival_flock_out &out, int m)
{
    const uint8_t sub = in.substate[m], valid = in.sink_valid[m];
    const float sx = in.sink_xz[2 * m], sz = in.sink_xz[2 * m + 1];
    out.substate[m] = sub; out.sink_valid[m] = valid;
    out.sink_xz[2 * m] = sx; out.sink_xz[2 * m + 1] = sz;
}

// first_build (or null): the status row of navhip_arrival_zone_build behind whose kernel this one runs -- the tail of the
// `!built` branch (arrival.c:839-847).  A zone that kernel built (status 0, phase FILLING, counters and fill_frac 0) takes
// the realloc below without the all-settled arm and without the counter; any other zone of that call is not touched.
__global__ __launch_bounds__(AF_THREADS) void k_arrival_flock(nh_step_params P, navhip_arrival_flock_in in, navhip_arrival_flock_out out,
                                                              const uint8_t *first_build)
{
    __shared__ af_lds L;
    const int zi = (int)blockIdx.x;
    if(first_build && first_build[zi] != 0) return;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    navhip_arrival_zone Z = in.zones[zi];
    navhip_arrival_flock S = in.flocks[zi];
    const int M = Z.slot_end - Z.slot_begin, nk = Z.key_end - Z.key_begin;
    const int mb = S.member_begin, me = S.member_end;
    const float *slots_xz = in.slots_xz + 2 * (size_t)Z.slot_begin;
    const int32_t *ring_in = in.slot_ring + Z.slot_begin;
    int32_t *ring_out = out.slot_ring + Z.slot_begin;

    // ---- what the device does not decide: every output repeats its input
    const bool layer_ok = S.layer >= 0 && S.layer < NAVHIP_NAV_LAYER_MAX;
    bool host = S.phase != NAVHIP_ARRIVAL_PHASE_FILLING || M < 0 || M > AF_CAP || nk < 0 || nk > AF_CAP
             || !layer_ok || !P.map.layers[layer_ok ? S.layer : 0].blockers
             || Z.num_rows < 0 || Z.num_rows > AF_CAP || (Z.num_rows > 0 && (Z.active_row < 0 || Z.active_row >= Z.num_rows));
    bool bad_uid = false, unsettled = false;
    for(int m = mb + tid; m < me; m += AF_THREADS) {
        const int uid = in.uid[m];
        bad_uid = bad_uid || uid < 0 || uid >= P.n_ents;
        unsettled = unsettled || in.settled[m] == 0;
    }
    host = __syncthreads_or(bad_uid || host) != 0;
    const bool all_settled = __syncthreads_or(unsettled) == 0;

    bool realloc = false;
    if(!host && first_build) {
        realloc = M > 0;                                                    // (:840: num_rows >= 1 with a slot, 0 without)
    }else if(!host && !all_settled) {
        Z.layer = S.layer;
        Z.radius = af_zone_radius(S.total_members, S.unit_radius);
        Z.unit_radius = S.unit_radius;
        if(++S.realloc_counter >= 4) {                                      // ARRIVAL_REALLOC_PERIOD
            S.realloc_counter = 0;
            realloc = !(M == 0 || Z.num_rows == 0);
        }
    }else if(!host) {
        S.phase = NAVHIP_ARRIVAL_PHASE_DONE;
    }

    if(!realloc) {
        for(int i = tid; i < M; i += AF_THREADS) { const int32_t r = ring_in[i]; ring_out[i] = r; }
        for(int m = mb + tid; m < me; m += AF_THREADS) af_copy_member(in, out, m);
        if(tid == 0) {
            out.zones[zi] = Z; out.flocks[zi] = S;
            out.status[zi] = host ? NAVHIP_AF_HOST : 0;
        }
        return;
    }

    // ---- arrival_realloc_slots (arrival.c:391)
    const uint16_t *blockers = P.map.layers[Z.layer].blockers;
    const uint64_t *g_keys = in.region_keys + Z.key_begin;
    for(int k = tid; k < nk; k += AF_THREADS) { L.keys[k] = g_keys[k]; L.dist[k] = -1; }
    for(int i = tid; i < M; i += AF_THREADS) {
        L.slot_x[i] = slots_xz[2 * i]; L.slot_z[i] = slots_xz[2 * i + 1];
        L.ring[i] = (uint16_t)ring_in[i];
    }
    for(int i = tid; i < AF_CAP / 32; i += AF_THREADS) L.occupied[i] = 0u;
    if(tid == 0) {
        L.entry_x = 0.0f; L.entry_z = 0.0f; L.entry_cnt = 0; L.maxd = -1; L.total_occ = 0; L.crowd = 0;
        L.active_row = Z.active_row; L.num_rows = Z.num_rows;
    }
    __syncthreads();

    if(Z.fill_frac < 0.25f) {                                               // ARRIVAL_REORIENT_FREEZE
        // ---- arrival_compute_geodesic_rings (:257).  entry: the unsettled members' positions summed IN MEMBER ORDER --
        // runs of AF_THREADS members are fetched by the lanes, lane 0 adds each run in order
        for(int base = mb; base < me; base += AF_THREADS) {
            const int m = base + tid;
            L.stage_on[tid] = 0;
            if(m < me && in.settled[m] == 0) {
                const int uid = in.uid[m];
                L.stage_x[tid] = P.pos_xz[2 * uid]; L.stage_z[tid] = P.pos_xz[2 * uid + 1];
                L.stage_on[tid] = 1;
            }
            __syncthreads();
            if(tid == 0) {
                float ex = L.entry_x, ez = L.entry_z;
                int cnt = L.entry_cnt;
                const int n = me - base < AF_THREADS ? me - base : AF_THREADS;
                for(int j = 0; j < n; j++) {
                    if(!L.stage_on[j]) continue;
                    ex = ex + L.stage_x[j]; ez = ez + L.stage_z[j];
                    cnt++;
                }
                L.entry_x = ex; L.entry_z = ez; L.entry_cnt = cnt;
            }
            __syncthreads();
        }
        float ex = Z.centre_x, ez = Z.centre_z;
        if(L.entry_cnt > 0) {
            const float inv = 1.0f / (float)L.entry_cnt;                    // PFM_Vec2_Scale(&entry, 1.0f / cnt, &entry)
            ex = L.entry_x * inv; ez = L.entry_z * inv;
        }

        // ---- N_RegionGeodesicDist (nav.c:4389).  The source: the key whose tile centre is nearest the entry, the earliest
        // of equal ones, key 0 when no distance is < INFINITY
        uint32_t best = 0xffffffffu;
        int at = 0x7fffffff;
        for(int k = tid; k < nk; k += AF_THREADS) {
            const uint64_t key = L.keys[k];
            const int chunk_r = (int)((key >> 48) & 0xffff), chunk_c = (int)((key >> 32) & 0xffff);
            const int tile_r = (int)((key >> 16) & 0xffff), tile_c = (int)(key & 0xffff);
            const float cx = P.map_x - ((float)(chunk_c * 64 + tile_c) + 0.5f) * 4.0f;
            const float cz = P.map_z + ((float)(chunk_r * 64 + tile_r) + 0.5f) * 4.0f;
            const float dx = cx - ex, dz = cz - ez;
            const float dd = dx * dx + dz * dz;
            if(!(dd < INFINITY)) continue;
            const uint32_t bits = nh_f2u(dd);
            if(bits < best) { best = bits; at = k; }
        }
        af_wave_min(best, at);
        if(lane == 0) { L.red_key[wave] = best; L.red_at[wave] = at; }
        __syncthreads();
        if(tid == 0 && nk > 0) {
            uint32_t b = L.red_key[0];
            int a = L.red_at[0];
            for(int w = 1; w < AF_WAVES; w++)
                if(L.red_key[w] < b || (L.red_key[w] == b && L.red_at[w] < a)) { b = L.red_key[w]; a = L.red_at[w]; }
            L.dist[b == 0xffffffffu ? 0 : a] = 0;
        }
        __syncthreads();

        // the flood, level by level: a key at `level` reaches its four neighbours (M_Tile_RelativeDesc: across chunk
        // borders, none beyond the map's edge); two lanes that reach one key store the same number
        const int max_r = P.map.h * 64, max_c = P.map.w * 64;
        for(int level = 0; level < AF_CAP; level++) {
            int grew = 0;
            for(int k = tid; k < nk; k += AF_THREADS) {
                if(L.dist[k] != level) continue;
                const uint64_t key = L.keys[k];
                const int r = (int)((key >> 48) & 0xffff) * 64 + (int)((key >> 16) & 0xffff);
                const int c = (int)((key >> 32) & 0xffff) * 64 + (int)(key & 0xffff);
#pragma unroll
                for(int d = 0; d < 4; d++) {
                    const int nr = r + (d == 2 ? -1 : d == 3 ? 1 : 0), nc = c + (d == 0 ? -1 : d == 1 ? 1 : 0);
                    if(nr < 0 || nr >= max_r || nc < 0 || nc >= max_c) continue;
                    const int ni = af_key_index(L.keys, nk, af_key(nr / 64, nc / 64, nr % 64, nc % 64));
                    if(ni < 0 || L.dist[ni] >= 0) continue;
                    L.dist[ni] = (int16_t)(level + 1);
                    grew = 1;
                }
            }
            if(!__syncthreads_or(grew)) break;
        }

        // a slot's distance is its tile's: -1 off the map, off the region or unreached; the deepest SLOT sets the rows
        int my_max = -1;
        for(int i = tid; i < M; i += AF_THREADS) {
            const int idx = af_point_key(P, L.slot_x[i], L.slot_z[i], L.keys, nk);
            const int g = idx >= 0 ? (int)L.dist[idx] : -1;
            L.cap[i] = g;                                                   // (parked: the counters are cleared below)
            my_max = g > my_max ? g : my_max;
        }
        if(my_max >= 0) atomicMax(&L.maxd, my_max);
        __syncthreads();
        int maxd = L.maxd;
        if(maxd < 0) maxd = 0;
        int ring_w = (int)(S.row_height / 4.0f + 0.5f);
        if(ring_w < 1) ring_w = 1;
        const int num_rows = maxd / ring_w + 1;
        for(int i = tid; i < M; i += AF_THREADS) {
            const int g = L.cap[i] >= 0 ? L.cap[i] : 0;                     // unreachable -> deepest ring
            int r = (maxd - g) / ring_w;
            if(r < 0) r = 0;
            if(r >= num_rows) r = num_rows - 1;
            L.ring[i] = (uint16_t)r;
        }
        if(tid == 0) { L.num_rows = num_rows; L.active_row = 0; }
        __syncthreads();
    }
    const int R = L.num_rows;
    for(int r = tid; r < R; r += AF_THREADS) { L.cap[r] = 0; L.occ[r] = 0; }
    __syncthreads();

    // ---- cap[], and the slots a blocker sits on
    for(int i = tid; i < M; i += AF_THREADS) {
        const int r = L.ring[i];
        if(r < R) atomicAdd(&L.cap[r], 1);
        tiledesc t;
        if(tile_for_point(P, L.slot_x[i], L.slot_z[i], t) && blockers[tile_index(P, t)] > 0)
            atomicOr(&L.occupied[i >> 5], 1u << (i & 31));
    }
    // ---- every settled member marks the slot nearest to it, of all M (a wave per member)
    for(int m = mb + wave; m < me; m += AF_WAVES) {
        if(in.settled[m] == 0) continue;
        const int uid = in.uid[m];
        const float px = P.pos_xz[2 * uid], pz = P.pos_xz[2 * uid + 1];
        uint32_t best = 0xffffffffu;
        int at = 0x7fffffff;
        for(int i = lane; i < M; i += 64) {
            const float dx = L.slot_x[i] - px, dz = L.slot_z[i] - pz;
            const float dd = dx * dx + dz * dz;
            if(!(dd < INFINITY)) continue;
            const uint32_t bits = nh_f2u(dd);
            if(bits < best) { best = bits; at = i; }
        }
        af_wave_min(best, at);
        if(lane == 0 && best != 0xffffffffu) atomicOr(&L.occupied[at >> 5], 1u << (at & 31));
    }
    __syncthreads();
    // ---- occ[], fill_frac's numerator, the crowd
    for(int i = tid; i < M; i += AF_THREADS) {
        if(!((L.occupied[i >> 5] >> (i & 31)) & 1u)) continue;
        const int r = L.ring[i];
        if(r < R) { atomicAdd(&L.occ[r], 1); atomicAdd(&L.total_occ, 1); }
    }
    int crowd = 0;
    for(int m = mb + tid; m < me; m += AF_THREADS) {
        if(in.settled[m] != 0) continue;
        const int uid = in.uid[m];
        if(af_point_key(P, P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1], L.keys, nk) >= 0) crowd++;
    }
    if(crowd) atomicAdd(&L.crowd, crowd);
    __syncthreads();

    // ---- the frontier (:462-476), on one lane
    if(tid == 0) {
        int active_row = L.active_row;
        const bool rising = L.occ[active_row] > S.prev_occ;
        bool advanced = false;
        while(active_row < R - 1 && (float)L.occ[active_row] >= 1.0f * (float)L.cap[active_row]) {   // ARRIVAL_ROW_FILL_THRESH
            active_row++;
            advanced = true;
        }
        if(advanced || rising || L.crowd == 0) {
            S.stall_counter = 0;
        }else if(++S.stall_counter >= 20 && active_row < R - 1) {          // ARRIVAL_ROW_STALL_TICKS / ARRIVAL_REALLOC_PERIOD
            active_row++;
            S.stall_counter = 0;
        }
        S.prev_occ = L.occ[active_row];
        L.active_row = active_row;
        Z.fill_frac = nh_fdiv((float)L.total_occ, (float)M);
        Z.active_row = active_row;
        Z.num_rows = R;
        out.zones[zi] = Z; out.flocks[zi] = S;
        out.status[zi] = 0;
    }
    __syncthreads();
    const int active_row = L.active_row;
    for(int i = tid; i < M; i += AF_THREADS) ring_out[i] = (int32_t)L.ring[i];

    // ---- the sinks (:478-511): a wave per member
    for(int m = mb + wave; m < me; m += AF_WAVES) {
        if(in.settled[m] != 0) {
            if(lane == 0) af_copy_member(in, out, m);
            continue;
        }
        const int uid = in.uid[m];
        const float px = P.pos_xz[2 * uid], pz = P.pos_xz[2 * uid + 1];
        int substate = in.substate[m];
        float sx = in.sink_xz[2 * m], sz = in.sink_xz[2 * m + 1];
        int valid = 0;
        if(af_point_key(P, px, pz, L.keys, nk) >= 0) {
            if(substate < 2) substate += 2;                                 // unit_commit, arrival.c:102
            uint32_t best = 0xffffffffu;
            int at = 0x7fffffff;
            for(int i = lane; i < M; i += 64) {
                if((L.occupied[i >> 5] >> (i & 31)) & 1u) continue;
                if((int)L.ring[i] > active_row) continue;
                const float dx = L.slot_x[i] - px, dz = L.slot_z[i] - pz;
                const float dd = dx * dx + dz * dz;
                if(!(dd < INFINITY)) continue;
                const uint32_t bits = nh_f2u(dd);
                if(bits < best) { best = bits; at = i; }
            }
            af_wave_min(best, at);
            if(best != 0xffffffffu) { sx = L.slot_x[at]; sz = L.slot_z[at]; valid = 1; }
        }
        if(lane == 0) {
            out.substate[m] = (uint8_t)substate; out.sink_valid[m] = (uint8_t)valid;
            out.sink_xz[2 * m] = sx; out.sink_xz[2 * m + 1] = sz;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// C entry points
// ---------------------------------------------------------------------------------------------
void nh_launch_arrival_first_realloc(const nh_step_params &P, const navhip_arrival_flock_in &in, const navhip_arrival_flock_out &out,
                                     const uint8_t *first_build, hipStream_t s)
{
    hipLaunchKernelGGL(k_arrival_flock, dim3(in.n_zones), dim3(AF_THREADS), 0, s, P, in, out, first_build);
}

namespace {

#define AF_FAIL(why) nh_fail(ctx, NAVHIP_ERR_ARG, name, why)     /* inside the check below: `name` is the form's */
// The one argument check of both forms; host_arrays: the arrays can be read here, so what lies IN them is checked too.
int af_check(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_flock_in *in, const navhip_arrival_flock_out *out, bool host_arrays)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    const char *name = host_arrays ? "navhip_arrival_flock_update: " : "navhip_arrival_flock_update_dev: ";
    if(!w || !in || !out) return AF_FAIL("a missing argument");
    if(in->nm < 0) return AF_FAIL("nm < 0");
    if(in->n_zones < 0 || in->n_slots < 0 || in->n_keys < 0 || w->n_ents < 0) return AF_FAIL("a negative count");
    if(in->n_zones == 0) return NAVHIP_OK;
    if(!in->zones || !in->flocks) return AF_FAIL("a missing array: zones or flocks");
    if(!out->zones || !out->flocks || !out->status) return AF_FAIL("a missing array: zones, flocks or status of navhip_arrival_flock_out");
    if(in->n_slots > 0 && (!in->slots_xz || !in->slot_ring || !out->slot_ring)) return AF_FAIL("a missing array: slots_xz or slot_ring");
    if(in->n_keys > 0 && !in->region_keys) return AF_FAIL("a missing array: region_keys");
    if(in->nm > 0) {
        if(!w->pos_xz) return AF_FAIL("a missing array: world->pos_xz");
        if(!in->uid || !in->settled || !in->substate || !in->sink_valid || !in->sink_xz) return AF_FAIL("a missing array of the members");
        if(!out->substate || !out->sink_valid || !out->sink_xz) return AF_FAIL("a missing array of the members of navhip_arrival_flock_out");
    }
    if(!host_arrays) return NAVHIP_OK;
    for(int z = 0; z < in->n_zones; z++)
        if(const char *fault = nh_zone_fault(in->zones[z], &in->flocks[z], in->n_slots, in->n_keys, in->nm, in->region_keys))
            return AF_FAIL("zone " + std::to_string(z) + fault);
    return NAVHIP_OK;
}

// the two structs of the host form, row by row (stage_plan.h)
const nh_row af_in_rows[] = {
    NH_ROW(navhip_arrival_flock_in, zones, sizeof(navhip_arrival_zone), NH_LEN_ZONE, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_flock_in, flocks, sizeof(navhip_arrival_flock), NH_LEN_ZONE, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_flock_in, slots_xz, 8, NH_LEN_SLOT, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_flock_in, slot_ring, 4, NH_LEN_SLOT, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_flock_in, region_keys, 8, NH_LEN_KEY, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_flock_in, uid, 4, NH_LEN_MEMBER, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_flock_in, settled, 1, NH_LEN_MEMBER, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_flock_in, substate, 1, NH_LEN_MEMBER, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_flock_in, sink_valid, 1, NH_LEN_MEMBER, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_flock_in, sink_xz, 8, NH_LEN_MEMBER, NH_ON_ALWAYS),
};
const nh_row af_out_rows[] = {
    NH_ROW_OUT_PAD(navhip_arrival_flock_out, zones, sizeof(navhip_arrival_zone), NH_LEN_ZONE, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_flock_out, flocks, sizeof(navhip_arrival_flock), NH_LEN_ZONE, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_flock_out, slot_ring, 4, NH_LEN_SLOT, NH_ON_ALWAYS, 16),  NH_ROW_OUT_PAD(navhip_arrival_flock_out, substate, 1, NH_LEN_MEMBER, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_flock_out, sink_valid, 1, NH_LEN_MEMBER, NH_ON_ALWAYS, 16),  NH_ROW_OUT_PAD(navhip_arrival_flock_out, sink_xz, 8, NH_LEN_MEMBER, NH_ON_ALWAYS, 16),
    NH_ROW_OUT_PAD(navhip_arrival_flock_out, status, 1, NH_LEN_ZONE, NH_ON_ALWAYS, 16),
};
NH_COVERS(af_in_rows, navhip_arrival_flock_in, 16);         // n_zones, nm, n_slots, n_keys
NH_COVERS(af_out_rows, navhip_arrival_flock_out, 0);

}   // namespace

extern "C" {

int navhip_arrival_flock_update_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_flock_in *in,
                                    const navhip_arrival_flock_out *out, void *stream)
{
    const int rc = af_check(ctx, w, in, out, false);
    if(rc || in->n_zones == 0) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    nh_step_params P;
    nh_step_params_init(ctx, w, &P);
    P.pos_xz = w->pos_xz;
    hipLaunchKernelGGL(k_arrival_flock, dim3(in->n_zones), dim3(AF_THREADS), 0, stream ? (hipStream_t)stream : ctx->stream, P, *in, *out,
                       (const uint8_t*)nullptr);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_arrival_flock_update(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_flock_in *in, const navhip_arrival_flock_out *out)
{
    int rc = af_check(ctx, w, in, out, true);
    if(rc || in->n_zones == 0) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    nh_dims D;
    D.len[NH_LEN_UNIT] = (size_t)w->n_ents; D.len[NH_LEN_ZONE] = (size_t)in->n_zones; D.len[NH_LEN_MEMBER] = (size_t)in->nm;
    D.len[NH_LEN_SLOT] = (size_t)in->n_slots; D.len[NH_LEN_KEY] = (size_t)in->n_keys;
    D.pad = 16;                                                             // (no input array of a slot-less or member-less call is empty; the result rows pad themselves)
    nh_plan P;
    navhip_world d = *w;
    navhip_arrival_flock_in di = *in;
    navhip_arrival_flock_out dout = {};
    P.in(in->nm ? w->pos_xz : nullptr, D.len[NH_LEN_UNIT] * 8, D.pad, (void**)&d.pos_xz);    // (no members: the positions do not travel)
    nh_plan_rows(P, af_in_rows, in, &di, D);
    nh_plan_rows(P, af_out_rows, out, &dout, D);
    rc = P.reserve(ctx, NH_STAGE_CALL0);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = navhip_arrival_flock_update_dev(ctx, &d, &di, &dout, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

}   // extern "C"
