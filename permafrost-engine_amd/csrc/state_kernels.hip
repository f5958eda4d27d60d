// state_kernels.hip -- more of entity_compute_update (movement.c:2303) on the device, SURVEY section 8(f4):
// the heading gate (:2319-2336), the arrival arm (k_state_update with k_arrived_compact), the arms of the state switch
// that k_state_update does not cover except
// STATE_SURROUND_ENTITY (:2423-2437, :2569-2668), adjacent_settled_count (:982) and the arrival overlay's settle rule
// (G_Arrival_ShouldSettle, arrival.c:946) with what it calls: N_SegmentWithinRegion (nav.c:4326) over
// M_Tile_LineSupercoverTilesSorted (tile.c:430), arrival_near_region / arrival_near_open_slot
// (arrival.c:158, :326), and the overlay's desired velocity (G_Arrival_DesiredVelocity, arrival.c:862; k_arrival_velocity).
// Kernels AND their C entry points (include/navhip.h): this translation unit was
// added after the round's profiles were taken and touches no other (profiles/README.md, `files`); its
// device scratch is ONE staging slot of the context, carved up per call.
//
// Everything here is decision logic on a few hundred bytes per unit: HBM-latency bound, one row of 16
// lanes per unit where a loop can be shared (the slots of a zone, the pad ring of arrival_near_region), a
// thread per unit elsewhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "navhip_internal.h"
#include "agent_internal.h"
#include "agent_math.h"
#include "lane_group.h"
#include "arrival_region.h"
#include "stage_plan.h"

#define SK_QUERY_R   30.0f       /* SEPARATION_NEIGHB_RADIUS, movement.c:428                            */
#define SK_QUERY_MAX 128         /* near_ents[128], movement.c:997                                      */

// ---------------------------------------------------------------------------------------------
// the heading gate, a thread per unit
// ---------------------------------------------------------------------------------------------
// PFM_Quat_PitchDiff (pf_math.c:677) turns (1, 0, 0) by both quaternions and takes atan2(det, dot) of the
// x/z parts: the turned front of q is (1 - 2y^2 - 2z^2, 2xz + 2wy) (PFM_Mat4x4_RotFromQuat :324, column 0).
// dir_quat_from_velocity (movement.c:1411) is the rotation about Y by atan2(v.z, v.x) - pi/2, whose turned
// front is (cos a, sin a) = (v.z, -v.x) / |v|.  |angle| > tol  <=>  cos(angle) < cos(tol): no trigonometry,
// and the comparison in double with a margin that is a hundred times the float path's error.
__global__ __launch_bounds__(256) void k_heading_gate(nh_step_params P, int begin, int end, const float *pos_xz, const float *vel_xz,
                                                      const uint8_t *state, const float *radius, const uint32_t *flags,
                                                      navhip_gate_in in, float *out_vel, float *out_new_pos, uint8_t *out_gate)
{
    const int i = begin + blockIdx.x * 256 + threadIdx.x;
    if(i >= end) return;
    v2 nv = mkv(in.new_vel_xz[2 * i], in.new_vel_xz[2 * i + 1]);
    const int st = state[i];
    uint8_t gate = 0;
    const bool gated_state = st == NAVHIP_STATE_MOVING || st == NAVHIP_STATE_SEEK_ENEMIES
                          || st == NAVHIP_STATE_SURROUND_ENTITY || st == NAVHIP_STATE_ENTER_ENTITY_RANGE;
    if(gated_state && vlen(nv) > CP_EPS) {
        const v2 vdes = mkv(in.vdes_xz[2 * i], in.vdes_xz[2 * i + 1]);
        const v2 h = vlen(vdes) > CP_EPS ? vdes : nv;                       // intended_heading, :2286
        const double qx = in.next_rot[4 * i], qy = in.next_rot[4 * i + 1], qz = in.next_rot[4 * i + 2],
                     qw = in.next_rot[4 * i + 3];
        const double d1x = 1.0 - 2.0 * qy * qy - 2.0 * qz * qz, d1z = 2.0 * qx * qz + 2.0 * qw * qy;
        const double d2x = (double)h.z, d2z = -(double)h.x;
        const double l1 = sqrt(d1x * d1x + d1z * d1z), l2 = sqrt(d2x * d2x + d2z * d2z);
        const bool rolling = vlen(mkv(vel_xz[2 * i], vel_xz[2 * i + 1])) > CP_EPS;
        // cos(90 deg), cos(10 deg)
        const double cos_tol = rolling ? 0.0 : 0.98480775301220805936674302458952;
        if(!(l1 * l2 > 1e-9)) {
            gate = NAVHIP_GATE_HOST;                                        // not a yaw: the host's float path decides
        }else{
            const double c = (d1x * d2x + d1z * d2z) / (l1 * l2);
            if(fabs(c - cos_tol) < 1e-4) gate = NAVHIP_GATE_HOST;
            else if(c < cos_tol) { gate = NAVHIP_GATE_TURN; nv = mkv(0.0f, 0.0f); }
        }
    }
    out_vel[2 * i] = nv.x; out_vel[2 * i + 1] = nv.z;
    const v2 pos = mkv(pos_xz[2 * i], pos_xz[2 * i + 1]);
    v2 np = mkv(pos.x + nv.x, pos.z + nv.z);                                // new_pos_for_vel, :1820
    if(in.interp_from_xz && P.hz < 20 && !(flags[i] & NAVHIP_ENTITY_FLAG_GARRISONED)) {
        // a rate below 20 Hz: the position the rest of entity_compute_update tests is the first interpolated position
        // of an accepted move (:2356-2377), pos + vel of a refused one
        const int layer = nav_layer_for(flags[i], radius[i]);
        if(!P.map.layers[layer].cost) gate |= NAVHIP_GATE_HOST;
        else if(vlen(nv) > 0.0f && pos_pathable(P, layer, np.x, np.z)
             && (pos_blocked(P, layer, pos.x, pos.z) || !pos_blocked(P, layer, np.x, np.z))) {
            const float fr = in.interp_step[i];
            if(!(fabs(1.0 - (double)fr) < (double)(1.0f / 1024.0f))) {      // interpolate_positions, :2222
                const float fx = in.interp_from_xz[2 * i], fz = in.interp_from_xz[2 * i + 1];
                float dx = np.x - fx, dz = np.z - fz;
                dx = dx * fr; dz = dz * fr;
                np = mkv(fx + dx, fz + dz);
            }
        }
    }
    out_new_pos[2 * i] = np.x; out_new_pos[2 * i + 1] = np.z;
    out_gate[i] = gate;
}

// ---------------------------------------------------------------------------------------------
// the arrival arm of entity_compute_update (movement.c:2303; see include/navhip.h): a row of 16 lanes
// per unit -- the scalar tests on every lane, the flock-mate scan (:953) shared by the lanes
// ---------------------------------------------------------------------------------------------
// the ARRIVED members of every flock, compacted to the front of the flock's range of the member list (any order)
__global__ __launch_bounds__(256) void k_arrived_compact(nh_step_params P, float4 *arrived, int32_t *arrived_n)
{
    __shared__ int count;
    const int f = blockIdx.x;
    if(threadIdx.x == 0) count = 0;
    __syncthreads();
    const int b = P.flock_offsets[f], e = P.flock_offsets[f + 1];
    for(int k0 = b; k0 < e; k0 += 256) {
        const int k = k0 + (int)threadIdx.x;
        int m = -1;
        if(k < e) { m = P.flock_members[k]; if(P.state[m] != NAVHIP_STATE_ARRIVED) m = -1; }
        const uint64_t bal = __ballot(m >= 0);
        int base = 0;
        if((threadIdx.x & 63) == 0 && bal) base = atomicAdd(&count, __popcll(bal));
        base = __shfl(base, 0);
        if(m >= 0) {
            const int at = b + base + __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull));
            // (the scratch holds n_ents rows -- an entity belongs to at most one flock; a device-side member list that
            // breaks that promise loses rows of the scan instead of writing past the buffer)
            if(at < P.n_ents) arrived[at] = make_float4(P.pos_xz[2 * m], P.pos_xz[2 * m + 1], P.radius[m], __int_as_float(m));
        }
    }
    __syncthreads();
    if(threadIdx.x == 0) arrived_n[f] = count;
}

__global__ __launch_bounds__(256) void k_state_update(nh_step_params P, navhip_state_in in, const float4 *arrived,
                                                      const int32_t *arrived_n, uint8_t *out_state, uint8_t *out_flags)
{
    typedef grp<16> g;
    const int uid = P.work_begin + ((blockIdx.x * 256 + threadIdx.x) >> 4);
    const int gl = g::lane();
    if(uid >= P.work_end) return;
    const int state = P.state[uid];
    uint8_t flags = 0, next = (uint8_t)state;
    const int flock = P.flock[uid];
    const uint32_t eflags = P.flags[uid];
    const float radius = P.radius[uid];
    const int layer = nav_layer_for(eflags, radius);
    bool decided = false;
    if(eflags & NAVHIP_ENTITY_FLAG_GARRISONED) {                           // :2344-2351
        if(!state_is_still(state)) { flags = NAVHIP_SU_SET_STATE; next = NAVHIP_STATE_ARRIVED; }
        decided = true;
    }else if(state == NAVHIP_STATE_SEEK_ENEMIES || state == NAVHIP_STATE_ARRIVED) {
        decided = true;                                                    // :2521-2528, :2643: no transition
    }else if((state != NAVHIP_STATE_MOVING && state != NAVHIP_STATE_MOVING_IN_FORMATION) || flock < 0
          || (in.skip && in.skip[uid]) || !P.map.layers[layer].cost || in.flock_layer[flock] != layer) {
        flags = NAVHIP_SU_HOST;
        decided = true;
    }
    if(!decided) {
        const v2 np = mkv(in.new_pos_xz[2 * uid], in.new_pos_xz[2 * uid + 1]);
        const v2 target = mkv(P.flock_target_xz[2 * flock], P.flock_target_xz[2 * flock + 1]);
        if(pos_pathable(P, layer, np.x, np.z)) {                           // :2437
            // ---- arrived(uid, new_pos), :2170
            const float thresh = radius * 1.5f;
            bool arr = vlen(vsub(target, np)) < thresh;
            if(!arr) {
                // N_IsAdjacentToImpassable, nav.c:4745: a 4-neighbour tile that n_tile_blocked (:235)
                tiledesc t;
                bool adj = false;
                if(tile_for_point(P, np.x, np.z, t)) {
                    const int ar = t.chunk_r * 64 + t.tile_r, ac = t.chunk_c * 64 + t.tile_c;
                    const int dr[4] = {-1, 0, 0, 1}, dc[4] = {0, -1, 1, 0};
#pragma unroll
                    for(int k = 0; k < 4; k++) {
                        const int r = ar + dr[k], c = ac + dc[k];
                        if(r < 0 || c < 0 || r >= P.map.h * 64 || c >= P.map.w * 64) continue;      // M_Tile_RelativeDesc
                        tiledesc a;
                        a.chunk_r = r >> 6; a.chunk_c = c >> 6; a.tile_r = r & 63; a.tile_c = c & 63;
                        adj = adj || tile_probe(P, layer, a) != 1u;          // impassable or blocked
                    }
                }
                if(adj) {
                    // N_IsMaximallyClose, nav.c:4727-4740: any of the destination's closest island tiles
                    // within the threshold (centre as the reference computes it: map_pos -/+ tile * 4)
                    bool close = false;
                    for(int k = in.flock_tiles_off[flock] + gl; k < in.flock_tiles_off[flock + 1]; k += 16) {
                        const float cx = P.map_x - (float)in.flock_tiles[2 * k + 1] * 4.0f;
                        const float cz = P.map_z + (float)in.flock_tiles[2 * k] * 4.0f;
                        close = close || vlen(vsub(mkv(cx, cz), np)) <= thresh;
                    }
                    arr = g::any(close);
                }
            }
            if(!arr) {
                const v2 nearest = mkv(in.flock_nearest_xz[2 * flock], in.flock_nearest_xz[2 * flock + 1]);
                if(nearest.x == nearest.x) arr = vlen(vsub(nearest, np)) < thresh;                   // :2187-2192
            }
            if(!arr) {
                // ---- a flock mate that touches us has arrived, :2480-2497 (positions and states of the
                // snapshot: adjacent_flock_members reads the tick's tables).  An existence test -- order does not
                // matter --, so the row scans the ARRIVED members only: k_arrived_compact has put {x, z, radius, uid}
                // of those, flock by flock, where the flock's member list starts (a fresh world: none; the scan of
                // every member cost 405 us per 100 000 units, nine tenths of the state pass)
                const v2 me = mkv(P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1]);
                bool hit = false;
                const int b = P.flock_offsets[flock], e = min(b + arrived_n[flock], P.n_ents);
                for(int k0 = b; k0 < e && !g::any(hit); k0 += 16) {
                    const int k = k0 + gl;
                    if(k < e) {
                        const float4 a = arrived[k];
                        if(__float_as_int(a.w) != uid)
                            hit = vlen(vsub(me, mkv(a.x, a.y))) <= radius + a.z + 5.0f;                  // ADJACENCY_SEP_DIST
                    }
                }
                arr = g::any(hit);
            }
            if(arr) {
                flags = NAVHIP_SU_SET_STATE | NAVHIP_SU_BLOCK; next = NAVHIP_STATE_ARRIVED;
            }else{
                const v2 vdes = mkv(in.vdes_xz[2 * uid], in.vdes_xz[2 * uid + 1]);
                if(vlen(vdes) < 1.0f / 1024.0f) {                          // :2508
                    flags = NAVHIP_SU_SET_STATE | NAVHIP_SU_BLOCK; next = NAVHIP_STATE_WAITING;
                }
            }
        }
    }
    if(gl == 0) { out_state[uid] = next; out_flags[uid] = flags; }
}

static void nh_launch_state_update(const nh_step_params &P, const navhip_state_in &in, float4 *d_arrived, int32_t *d_arrived_n,
                                   uint8_t *d_state, uint8_t *d_flags, hipStream_t s)
{
    const int n = P.work_end - P.work_begin;
    if(n <= 0) return;
    if(P.n_flocks > 0)
        hipLaunchKernelGGL(k_arrived_compact, dim3(P.n_flocks), dim3(256), 0, s, P, d_arrived, d_arrived_n);
    hipLaunchKernelGGL(k_state_update, dim3((n + 15) / 16), dim3(256), 0, s, P, in, (const float4*)d_arrived,
                       (const int32_t*)d_arrived_n, d_state, d_flags);
}

// ---------------------------------------------------------------------------------------------
// the arms that flags, a counter, an angle or a distance decide (formation members on the move, ARRIVING_TO_CELL, the
// wait timer, the end of TURNING, ENTER_ENTITY_RANGE): a thread per unit, after k_state_update
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_state_aux(nh_step_params P, const float *pos_xz, const float *radius, const uint32_t *flags,
                                                   const uint8_t *state, navhip_state_aux_in in, uint8_t *io_state,
                                                   uint8_t *io_flags, int32_t *out_ticks)
{
    const int i = P.work_begin + blockIdx.x * 256 + threadIdx.x;
    if(i >= P.work_end) return;
    const int st = state[i];
    int ticks = in.wait_ticks_left[i];
    const uint32_t ef = flags[i];
    const int layer = nav_layer_for(ef, radius[i]);
    const uint8_t *cost = P.map.layers[layer].cost;
    const bool ours = st == NAVHIP_STATE_WAITING || st == NAVHIP_STATE_ARRIVING_TO_CELL || (st == NAVHIP_STATE_TURNING && in.ent_rot)
                   || (st == NAVHIP_STATE_ENTER_ENTITY_RANGE && in.range_target && in.range_target[i] >= -1)
                   || (st == NAVHIP_STATE_SURROUND_ENTITY && in.surround_target && in.surround_target[i] >= -1 && P.hz == 20)
                   || ((st == NAVHIP_STATE_MOVING || st == NAVHIP_STATE_MOVING_IN_FORMATION) && (in.fstate[i] & NAVHIP_FS_MEMBER));
    if(ours && !(ef & NAVHIP_ENTITY_FLAG_GARRISONED) && cost) {                 // (:2344 returns before everything)
        const uint8_t fs = in.fstate[i];
        tiledesc t;
        const bool pathable = tile_for_point(P, in.new_pos_xz[2 * i], in.new_pos_xz[2 * i + 1], t)
                           && cost[tile_index(P, t)] != NAVHIP_COST_IMPASSABLE;   // :2437
        uint8_t next = (uint8_t)st, fl = 0;
        bool decided = true;
        if(pathable) {
            if(st == NAVHIP_STATE_WAITING) {                                    // :2630-2644
                ticks--;
                if(ticks == 0) { next = in.wait_prev[i]; fl = NAVHIP_SU_SET_MOVING; }
            }else if(st == NAVHIP_STATE_ENTER_ENTITY_RANGE) {                   // :2569-2604
                const int tgt = in.range_target[i];
                if(tgt < 0) { next = NAVHIP_STATE_ARRIVED; fl = NAVHIP_SU_SET_STATE | NAVHIP_SU_BLOCK; }
                else{
                    const v2 np = mkv(in.new_pos_xz[2 * i], in.new_pos_xz[2 * i + 1]);
                    const v2 tp = mkv(pos_xz[2 * tgt], pos_xz[2 * tgt + 1]);
                    bool stop = vlen(vsub(np, tp)) <= in.target_range[i];
                    if(!stop) {
                        // N_IsAdjacentToImpassable (nav.c:4747): a 4-neighbour tile that is impassable or blocked ...
                        const nh_layer_view &L = P.map.layers[layer];
                        const int ar = t.chunk_r * 64 + t.tile_r, ac = t.chunk_c * 64 + t.tile_c;
                        const int dr[4] = {-1, 0, 0, 1}, dc[4] = {0, -1, 1, 0};
                        bool adj = false;
#pragma unroll
                        for(int k = 0; k < 4; k++) {
                            const int r = ar + dr[k], c = ac + dc[k];
                            if(r < 0 || c < 0 || r >= P.map.h * 64 || c >= P.map.w * 64) continue;
                            tiledesc a;
                            a.chunk_r = r >> 6; a.chunk_c = c >> 6; a.tile_r = r & 63; a.tile_c = c & 63;
                            const size_t idx = tile_index(P, a);
                            adj = adj || cost[idx] == NAVHIP_COST_IMPASSABLE || (L.blockers && L.blockers[idx] > 0);
                        }
                        // ... and N_IsMaximallyClose(new_pos, target, 0.0f) (nav.c:4707): the position IS the centre of one
                        // of the target's closest island tiles
                        if(adj) {
                            const int row = in.range_tiles_row[i];
                            for(int k = in.range_tiles_off[row]; k < in.range_tiles_off[row + 1] && !stop; k++) {
                                const float cx = P.map_x - (float)in.range_tiles[2 * k + 1] * 4.0f;
                                const float cz = P.map_z + (float)in.range_tiles[2 * k] * 4.0f;
                                stop = vlen(vsub(mkv(cx, cz), np)) <= 0.0f;
                            }
                        }
                    }
                    if(stop) { next = NAVHIP_STATE_WAITING; fl = NAVHIP_SU_SET_STATE | NAVHIP_SU_BLOCK; }
                    else if(vlen(vsub(tp, mkv(in.target_prev_xz[2 * i], in.target_prev_xz[2 * i + 1]))) > 5.0f)
                        fl = NAVHIP_SU_SET_DEST;
                }
            }else if(st == NAVHIP_STATE_SURROUND_ENTITY) {                      // :2509-2567
                const int tgt = in.surround_target[i];
                const uint8_t sq = in.surround_query[i];
                const int flock = P.flock[i];
                if(tgt >= 0 && (sq & NAVHIP_SQ_HOST)) decided = false;           // (navhip_surround_queries left the row to the host)
                else if(tgt < 0 || (sq & NAVHIP_SQ_ADJACENT)) { next = NAVHIP_STATE_ARRIVED; fl = NAVHIP_SU_SET_STATE | NAVHIP_SU_BLOCK; }
                else if(flock < 0) decided = false;                             // (the reference asserts a flock)
                else{
                    const v2 np = mkv(in.new_pos_xz[2 * i], in.new_pos_xz[2 * i + 1]);
                    const v2 me = mkv(pos_xz[2 * i], pos_xz[2 * i + 1]);
                    const v2 tp = mkv(pos_xz[2 * tgt], pos_xz[2 * tgt + 1]);
                    v2 dest = mkv(in.surround_nearest_prev_xz[2 * i], in.surround_nearest_prev_xz[2 * i + 1]);
                    const v2 delta = vsub(tp, mkv(in.surround_target_prev_xz[2 * i], in.surround_target_prev_xz[2 * i + 1]));
                    bool gone = false;
                    if(vlen(delta) > CP_EPS || vlen(mkv(P.vel_xz[2 * i], P.vel_xz[2 * i + 1])) < CP_EPS) {
                        // the host asked M_NavClosestReachableAdjacentPosFrom from both positions this tick can test:
                        // pos + new velocity [0] and pos [1] (the gate halted the unit; equal when the velocity is zero)
                        const int c = (np.x == me.x && np.z == me.z) ? 1 : 0;
                        if(!(sq & (NAVHIP_SQ_HAS_DEST_0 << c))) gone = true;
                        else dest = mkv(in.surround_dest_xz[4 * i + 2 * c], in.surround_dest_xz[4 * i + 2 * c + 1]);
                    }
                    if(gone) { next = NAVHIP_STATE_ARRIVED; fl = NAVHIP_SU_SET_STATE | NAVHIP_SU_BLOCK; }
                    else{
                        in.out_surround_dest_xz[2 * i] = dest.x; in.out_surround_dest_xz[2 * i + 1] = dest.z;
                        fl = NAVHIP_SU_SURROUND_PREV;
                        const v2 diff = vsub(mkv(P.flock_target_xz[2 * flock], P.flock_target_xz[2 * flock + 1]), dest);
                        if(vlen(diff) > CP_EPS) { fl |= NAVHIP_SU_SURROUND_DEST | NAVHIP_SU_SET_STATE; next = NAVHIP_STATE_SURROUND_ENTITY; }
                        else if(vlen(mkv(in.vdes_xz[2 * i], in.vdes_xz[2 * i + 1])) < CP_EPS) {
                            fl |= NAVHIP_SU_SET_STATE | NAVHIP_SU_BLOCK; next = NAVHIP_STATE_WAITING;
                        }
                    }
                }
            }else if(st == NAVHIP_STATE_TURNING) {                              // :2606-2628
                // |PFM_Quat_PitchDiff(rot, target_dir)| <= 5 degrees, as the heading gate compares: the turned fronts of
                // both quaternions, the cosine in double, a margin around cos(5 deg)
                const float *a = in.ent_rot + 4 * i, *b = in.target_dir + 4 * i;
                const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
                const double d1x = 1.0 - 2.0 * ay * ay - 2.0 * az * az, d1z = 2.0 * ax * az + 2.0 * aw * ay;
                const double d2x = 1.0 - 2.0 * by * by - 2.0 * bz * bz, d2z = 2.0 * bx * bz + 2.0 * bw * by;
                const double l = sqrt(d1x * d1x + d1z * d1z) * sqrt(d2x * d2x + d2z * d2z);
                const double cos5 = 0.99619469809174553229501040247389;
                if(!(l > 1e-9)) decided = false;
                else{
                    const double c = (d1x * d2x + d1z * d2z) / l;
                    // (the cosine is flat at 5 degrees: a margin of 1e-5 is 0.007 degrees, and still 250 times the
                    // float path's error there)
                    if(fabs(c - cos5) < 1e-5) decided = false;                  // the host's float path decides
                    else if(c > cos5) { next = NAVHIP_STATE_ARRIVED; fl = NAVHIP_SU_SET_STATE | NAVHIP_SU_BLOCK; }
                }
            }else if(st == NAVHIP_STATE_ARRIVING_TO_CELL) {                     // :2645-2668
                if(!(fs & NAVHIP_FS_MEMBER)) { next = NAVHIP_STATE_MOVING; fl = NAVHIP_SU_SET_STATE; }
                else if(!(fs & NAVHIP_FS_READY)) { }
                else if(!(fs & NAVHIP_FS_IN_RANGE)) { next = NAVHIP_STATE_MOVING_IN_FORMATION; fl = NAVHIP_SU_SET_STATE; }
                else if(fs & NAVHIP_FS_ARRIVED) { next = NAVHIP_STATE_TURNING; fl = NAVHIP_SU_SET_STATE | NAVHIP_SU_TARGET_DIR; }
            }else{                                                              // a formation member on the move, :2423-2437
                if(!(fs & NAVHIP_FS_READY)) { }
                else if((fs & NAVHIP_FS_ASSIGNED) && (fs & NAVHIP_FS_IN_RANGE)) { next = NAVHIP_STATE_ARRIVING_TO_CELL; fl = NAVHIP_SU_SET_STATE; }
                else decided = false;                                           // falls through to the arrival arm: k_state_update's answer
            }
        }
        if(decided) { io_state[i] = next; io_flags[i] = fl; }
    }
    out_ticks[i] = ticks;
}

// the resident pass: move_work_out.ent_des_v of a unit = the direction its host gave the step, or -- where that was NaN:
// "sample on the device" -- the direction the step sampled (what move_hip.c's scatter leaves in the work item)
__global__ __launch_bounds__(256) void k_pick_vdes(int begin, int end, const float *given, const float *sampled, float *out)
{
    const int i = begin + blockIdx.x * 256 + threadIdx.x;
    if(i >= end) return;
    float x = given ? given[2 * i] : __int_as_float(0x7fc00000), z = given ? given[2 * i + 1] : 0.0f;
    if(x != x) { x = sampled ? sampled[2 * i] : 0.0f; z = sampled ? sampled[2 * i + 1] : 0.0f; }
    out[2 * i] = x; out[2 * i + 1] = z;
}

// the fused pass (navhip_state_pass): a unit whose gate is the host's to decide is the host's altogether
__global__ __launch_bounds__(256) void k_gate_host_rows(int begin, int end, const uint8_t *gate, const uint8_t *state,
                                                        const int32_t *in_ticks, uint8_t *io_state, uint8_t *io_flags,
                                                        int32_t *out_ticks)
{
    const int i = begin + blockIdx.x * 256 + threadIdx.x;
    if(i >= end || !(gate[i] & NAVHIP_GATE_HOST)) return;
    io_state[i] = state[i]; io_flags[i] = NAVHIP_SU_HOST;
    if(out_ticks) out_ticks[i] = in_ticks[i];
}

// sparse rows of the three arms with per-unit arrays (navhip_state_aux_in.sparse_units): row k of every given array
// goes to row units[k] of its dense twin, which the arm kernels read as before; a thread per listed unit
struct sk_sparse_rows {
    int n; const int32_t *units;
    const float *er, *td; float *d_er, *d_td;
    const int32_t *rt; const float *rr, *rp; const int32_t *row; int32_t *d_rt; float *d_rr, *d_rp; int32_t *d_row;
    const int32_t *stgt; const uint8_t *sq; const float *stp, *snp, *sd; int32_t *d_stgt; uint8_t *d_sq; float *d_stp, *d_snp, *d_sd;
};
__global__ __launch_bounds__(256) void k_sparse_rows(sk_sparse_rows S)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if(k >= S.n) return;
    const int i = S.units[k];
    if(S.er) {
        for(int c = 0; c < 4; c++) { S.d_er[4 * i + c] = S.er[4 * k + c]; S.d_td[4 * i + c] = S.td[4 * k + c]; }
    }
    if(S.rt) {
        S.d_rt[i] = S.rt[k]; S.d_rr[i] = S.rr[k]; S.d_row[i] = S.row[k];
        S.d_rp[2 * i] = S.rp[2 * k]; S.d_rp[2 * i + 1] = S.rp[2 * k + 1];
    }
    if(S.stgt) {
        S.d_stgt[i] = S.stgt[k]; S.d_sq[i] = S.sq[k];
        for(int c = 0; c < 2; c++) { S.d_stp[2 * i + c] = S.stp[2 * k + c]; S.d_snp[2 * i + c] = S.snp[2 * k + c]; }
        for(int c = 0; c < 4; c++) S.d_sd[4 * i + c] = S.sd[4 * k + c];
    }
}
__global__ __launch_bounds__(256) void k_sparse_gather2(int n, const int32_t *units, const float *dense, float *rows)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if(k >= n) return;
    rows[2 * k] = dense[2 * units[k]]; rows[2 * k + 1] = dense[2 * units[k] + 1];
}

// ---------------------------------------------------------------------------------------------
// adjacent_settled_count: the ids of the spatial query (k_spatial_query, the reference's visiting order,
// capped) -> the count, a thread per unit
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gather_query(int nq, const int32_t *uids, const float *pos_xz, float *query)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if(q >= nq) return;
    query[2 * q] = pos_xz[2 * uids[q]]; query[2 * q + 1] = pos_xz[2 * uids[q] + 1];
}

// a row of 16 lanes per unit: the candidates of a query are independent tests (a count, no order) -- a thread per unit
// walked its 128 ids one dependent gather after the other (167 us for 3 400 units)
__global__ __launch_bounds__(256) void k_settled_count(int nq, const int32_t *uids, const float *pos_xz,
                                                       const float *radius, const uint32_t *flags,
                                                       const uint8_t *state, const int32_t *q_counts,
                                                       const uint32_t *q_ids, int32_t *out)
{
    const int q = (blockIdx.x * 256 + threadIdx.x) >> 4, gl = threadIdx.x & 15;
    const bool live = q < nq;
    const int uid = live ? uids[q] : 0;
    const float r_uid = radius[uid];
    const bool wide = 2.0f * r_uid + 5.0f > SK_QUERY_R;                     // search_radius, :995
    const v2 pos = mkv(pos_xz[2 * uid], pos_xz[2 * uid + 1]);
    const uint32_t my_air = flags[uid] & NAVHIP_ENTITY_FLAG_AIR;
    int count = 0;
    const uint32_t *ids = q_ids + (size_t)(live ? q : 0) * SK_QUERY_MAX;
    const int n = (live && !wide) ? q_counts[q] : 0;
    for(int k = gl; k < n; k += 16) {
        const int c = (int)ids[k];
        const uint32_t f = flags[c];
        if(f & NAVHIP_ENTITY_FLAG_GARRISONED) continue;                     // filter_garrisoned, position.c:384
        if(c == uid || !(f & NAVHIP_ENTITY_FLAG_MOVABLE) || (f & NAVHIP_ENTITY_FLAG_AIR) != my_air) continue;
        if(state[c] != NAVHIP_STATE_ARRIVED) continue;
        const v2 cp = mkv(pos_xz[2 * c], pos_xz[2 * c + 1]);
        if(vlen(vsub(pos, cp)) <= r_uid + radius[c] + 5.0f) count++;         // ADJACENCY_SEP_DIST
    }
#pragma unroll
    for(int d = 1; d < 16; d <<= 1) count += __shfl_xor(count, d);
    if(live && gl == 0) out[q] = wide ? -1 : count;
}

// ---------------------------------------------------------------------------------------------
// G_Arrival_ShouldSettle, a row of 16 lanes per unit
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sk_row_any(bool p)                          // over the 16 lanes of the unit's row
{
    // (wave64: the ballot is 64 bits, a row its 16-bit field at lane & 48 -- gfx950 only, like everything here)
    return ((__ballot(p) >> (threadIdx.x & 48)) & 0xffffull) != 0ull;
}

// sk_key, sk_keys_contain, sk_segment_within, sk_in_region: arrival_region.h (shared with arrival_build_kernels.hip)

__global__ __launch_bounds__(256) void k_arrival_settle(nh_step_params P, const float *vel_xz, const float *radius_of,
                                                        navhip_settle_in in, navhip_settle_out out)
{
    const int q = (blockIdx.x * 256 + threadIdx.x) >> 4;
    const int gl = (int)(threadIdx.x & 15);
    if(q >= in.nq) return;
    const int uid = in.uid[q];
    const navhip_arrival_zone Z = in.zones[in.zone[q]];
    const uint64_t *keys = in.region_keys + Z.key_begin;
    const int num_region = Z.key_end - Z.key_begin;
    const v2 np = mkv(in.new_pos_xz[2 * q], in.new_pos_xz[2 * q + 1]);
    const v2 vel = mkv(vel_xz[2 * uid], vel_xz[2 * uid + 1]);
    const float radius = radius_of[uid];
    const int nsettled = in.nsettled[q];
    int substate = in.substate[q], stuck = in.stuck[q];
    bool anchored = in.progress_anchored[q] != 0;
    v2 anchor = mkv(in.progress_anchor_xz[2 * q], in.progress_anchor_xz[2 * q + 1]);
    const bool sink_valid = in.sink_valid[q] != 0;
    const v2 sink = mkv(in.sink_xz[2 * q], in.sink_xz[2 * q + 1]);

    const bool in_region = sk_in_region(P, np, keys, num_region);
    // arrival_near_region (arrival.c:158): the ring of pad tiles around the position, shared by the lanes
    bool near_region = in_region;
    if(!in_region) {
        int pad = (int)ceilf(Z.unit_radius / 4.0f);
        if(pad < 1) pad = 1;
        const int side = 2 * pad + 1;
        bool hit = false;
        for(int k = gl; k < side * side; k += 16) {
            const int dz = k / side - pad, dx = k % side - pad;
            if(dx == 0 && dz == 0) continue;
            hit = hit || sk_in_region(P, mkv(np.x + (float)dx * 4.0f, np.z + (float)dz * 4.0f), keys, num_region);
        }
        near_region = sk_row_any(hit);
    }
    // arrival_near_open_slot (arrival.c:326), tolerance radius * ARRIVAL_SINK_TOLERANCE: any slot of an active
    // row within it that no blocker stands on
    bool at_sink = false;
    if(in_region) {
        const float tol = radius * 1.5f, tol2 = tol * tol;
        bool hit = false;
        const nh_layer_view &L = P.map.layers[Z.layer];
        for(int k = Z.slot_begin + gl; k < Z.slot_end; k += 16) {
            if(in.slot_ring[k] > Z.active_row) continue;
            const v2 s = mkv(in.slots_xz[2 * k], in.slots_xz[2 * k + 1]);
            const v2 d = vsub(s, np);
            if(vdot(d, d) > tol2) continue;
            tiledesc t;
            bool blocked = false;
            if(L.blockers && tile_for_point(P, s.x, s.z, t)) blocked = L.blockers[tile_index(P, t)] > 0;
            hit = hit || !blocked;
        }
        at_sink = sk_row_any(hit);
    }
    int settle_contacts = 3;                                                // ARRIVAL_SETTLE_CONTACTS
    if(Z.fill_frac >= 0.90f) settle_contacts = 2;                          // (as the reference has it, :959-962)
    else if(Z.fill_frac >= 0.75f) settle_contacts = 3;
    const bool reachable_slot = sink_valid && sk_segment_within(P, np, sink, keys, num_region);
    const bool fill_done = Z.active_row >= Z.num_rows - 1;
    bool advancing = false;
    if(sink_valid) advancing = vdot(vel, vsub(sink, np)) > 0.0f;
    // unit_armed / unit_arm (arrival.c:96, :110): APPROACH 0, APPROACH_ARMED 1, SEEK 2, SEEK_ARMED 3
    bool armed = substate == 1 || substate == 3;
    if(!armed) {
        const v2 order = mkv(in.order_pos_xz[2 * q], in.order_pos_xz[2 * q + 1]);
        if(vlen(vsub(np, order)) > 4.0f) { substate += 1; armed = true; }    // ARRIVAL_ENGAGE_DIST
    }
    const bool by_prop = armed && !at_sink && in_region && nsettled >= settle_contacts
                      && (reachable_slot ? !advancing : fill_done);
    const float settle_range = ((float)Z.radius * 4.0f + radius) * 1.875f;  // ARRIVAL_SETTLE_RANGE
    const v2 to_centre = vsub(np, mkv(Z.centre_x, Z.centre_z));
    const bool within_settle_range = vdot(to_centre, to_centre) <= settle_range * settle_range;
    const bool stuck_eligible = nsettled >= 1 && (near_region || within_settle_range);
    if(!at_sink && stuck_eligible && armed) {
        if(!anchored) { anchor = np; anchored = true; stuck = 0; }
        if(vlen(vsub(np, anchor)) > 1.875f) { anchor = np; stuck = 0; }      // ARRIVAL_STUCK_DISP
        else stuck++;
    }
    const bool by_stuck = !at_sink && !by_prop && stuck_eligible && stuck >= 12;   // ARRIVAL_STUCK_LIMIT
    const bool by_contact = armed && !at_sink && near_region && !reachable_slot && nsettled >= 1
                         && Z.fill_frac >= 0.90f;
    if(gl == 0) {
        out.settle[q] = (at_sink || by_prop || by_stuck || by_contact) ? 1 : 0;
        out.substate[q] = (uint8_t)substate;
        out.progress_anchor_xz[2 * q] = anchor.x; out.progress_anchor_xz[2 * q + 1] = anchor.z;
        out.progress_anchored[q] = anchored ? 1 : 0;
        out.stuck[q] = stuck;
    }
}

// ---------------------------------------------------------------------------------------------
// G_Arrival_DesiredVelocity (arrival.c:862-944), a row of 16 lanes per unit: the scalar tests on every lane, the pad ring
// of arrival_near_region and the slot scans shared by the lanes
// ---------------------------------------------------------------------------------------------
// arrival_nearest_slot (arrival.c:344) / arrival_nearest_open_slot (:304, with the blockers plane): the slot at or behind
// the frontier of least dd, the EARLIEST of equal ones (the reference's strict `<` from best = INFINITY: a dd that is not
// < INFINITY never wins).  dd >= 0, so its float bits order as it does: each lane keeps the least (bits, index) of its
// stride, the row takes the minimum.  -1 = none.
__device__ int av_nearest_slot(const nh_step_params &P, const navhip_arrival_zone &Z, const float *slots_xz, const int32_t *slot_ring,
                               v2 from, const uint16_t *blockers, int gl)
{
    uint32_t best = 0xffffffffu;
    int at = 0x7fffffff;
    for(int k = Z.slot_begin + gl; k < Z.slot_end; k += 16) {
        if(slot_ring[k] > Z.active_row) continue;
        const v2 s = mkv(slots_xz[2 * k], slots_xz[2 * k + 1]);
        if(blockers) {
            tiledesc t;
            if(tile_for_point(P, s.x, s.z, t) && blockers[tile_index(P, t)] > 0) continue;
        }
        const v2 d = vsub(s, from);
        const float dd = vdot(d, d);
        if(!(dd < INFINITY)) continue;
        const uint32_t key = nh_f2u(dd);
        if(key < best) { best = key; at = k; }
    }
#pragma unroll
    for(int d = 8; d >= 1; d >>= 1) {
        const uint32_t ok = (uint32_t)__shfl_xor((int)best, d);
        const int      oi = __shfl_xor(at, d);
        if(ok < best || (ok == best && oi < at)) { best = ok; at = oi; }
    }
    return best == 0xffffffffu ? -1 : at;
}

__device__ __forceinline__ v2 av_heading(v2 v)                              // "if(PFM_Vec2_Len(&v) > EPSILON) PFM_Vec2_Normal(&v, &v)"
{
    return vlen(v) > CP_EPS ? vnormal(v) : v;
}

__global__ __launch_bounds__(256) void k_arrival_velocity(nh_step_params P, int n_com_rows, int n_zone_rows,
                                                          navhip_arrival_vel_in in, navhip_arrival_vel_out out)
{
    const int q = (blockIdx.x * 256 + threadIdx.x) >> 4;
    const int gl = (int)(threadIdx.x & 15);
    if(q >= in.nq) return;
    const int uid = in.uid[q], zi = in.zone[q];
    int substate = in.substate[q], los_hyst = in.los_hyst[q];
    bool sink_valid = in.sink_valid[q] != 0, los_latched = in.los_latched[q] != 0;
    v2 sink = mkv(in.sink_xz[2 * q], in.sink_xz[2 * q + 1]);
    const float nan = nh_u2f(0x7fc00000u);
    v2 vdes = mkv(nan, nan);
    uint32_t status = 0;

    // ---- what the device does not decide: the row goes back as it came
    const bool listed = uid >= 0 && uid < P.n_ents && zi >= 0 && zi < in.n_zones && substate <= 3;
    navhip_arrival_zone Z = {};
    v2 pos = mkv(nan, nan);
    tiledesc tp = {};
    bool host = !listed;
    if(listed) {
        Z = in.zones[zi];
        pos = mkv(P.pos_xz[2 * uid], P.pos_xz[2 * uid + 1]);
        host = !(pos.x == pos.x) || !(pos.z == pos.z) || !tile_for_point(P, pos.x, pos.z, tp)
            || Z.layer < 0 || Z.layer >= NAVHIP_NAV_LAYER_MAX || !P.map.layers[Z.layer].blockers
            || in.zone_row[zi] < -1 || in.zone_row[zi] >= n_zone_rows || in.com_row[zi] < -1 || in.com_row[zi] >= n_com_rows;
    }
    if(host) {
        status = NAVHIP_AV_HOST;
    }else{
        const uint64_t *keys = in.region_keys + Z.key_begin;
        const int num_region = Z.key_end - Z.key_begin;
        const uint16_t *blockers = P.map.layers[Z.layer].blockers;
        const v2 centre = mkv(Z.centre_x, Z.centre_z);

        // arrival_near_region (arrival.c:158): the tile, then the ring of pad tiles around the position
        bool near_region = sk_in_region(P, pos, keys, num_region);
        if(!near_region) {
            int pad = (int)ceilf(Z.unit_radius / 4.0f);
            if(pad < 1) pad = 1;
            const int side = 2 * pad + 1;
            bool hit = false;
            for(int k = gl; k < side * side; k += 16) {
                const int dz = k / side - pad, dx = k % side - pad;
                if(dx == 0 && dz == 0) continue;
                hit = hit || sk_in_region(P, mkv(pos.x + (float)dx * 4.0f, pos.z + (float)dz * 4.0f), keys, num_region);
            }
            near_region = sk_row_any(hit);
        }
        if(near_region && substate < 2) substate += 2;                      // unit_commit, arrival.c:102

        if(substate >= 2) {
            // ---- SEEK / SEEK_ARMED (:877-908)
            if(sink_valid) {
                tiledesc ts;
                if(tile_for_point(P, sink.x, sink.z, ts) && blockers[tile_index(P, ts)] > 0) {
                    const int k = av_nearest_slot(P, Z, in.slots_xz, in.slot_ring, pos, blockers, gl);
                    sink_valid = k >= 0;
                    if(sink_valid) sink = mkv(in.slots_xz[2 * k], in.slots_xz[2 * k + 1]);
                }
            }
            if(sink_valid && sk_segment_within(P, pos, sink, keys, num_region)) {
                vdes = av_heading(vsub(sink, pos));
            }else{
                const int k = av_nearest_slot(P, Z, in.slots_xz, in.slot_ring, pos, nullptr, gl);
                vdes = mkv(0.0f, 0.0f);
                if(k >= 0) vdes = av_heading(vsub(mkv(in.slots_xz[2 * k], in.slots_xz[2 * k + 1]), pos));
            }
        }else{
            // ---- APPROACH / APPROACH_ARMED (:909-941).  N_DesiredGroupArrivalVelocity (nav.c:3561): N_FlowDir of the byte
            // under the unit in the chunk field of the zone's mapping row; a sink inside the disc is an open slot
            bool zone_ok = false, at_slot = false;
            v2 zvel = mkv(0.0f, 0.0f);
            tiledesc tc;
            const int zrow = in.zone_row[zi];
            if(zrow >= 0 && P.region_field_slot && P.field_pool && tile_for_point(P, centre.x, centre.z, tc)) {
                const int slot = P.region_field_slot[(size_t)zrow * (P.map.w * P.map.h) + tp.chunk_r * P.map.w + tp.chunk_c];
                if(slot >= 0) {
                    const int dir = P.field_pool[((size_t)slot << 12) + tp.tile_r * 64 + tp.tile_c] & 0xf;
                    zone_ok = true;
                    zvel = flow_dir_vec(dir);
                    if(dir == NAVHIP_FD_NONE) {
                        const int dr = (tp.chunk_r * 64 + tp.tile_r) - (tc.chunk_r * 64 + tc.tile_r);     // M_Tile_Distance, tile.c:414
                        const int dc = (tp.chunk_c * 64 + tp.tile_c) - (tc.chunk_c * 64 + tc.tile_c);
                        at_slot = dr * dr + dc * dc <= Z.radius * Z.radius;
                    }
                }
            }
            if(zone_ok && !at_slot && vlen(zvel) > CP_EPS) {
                vdes = zvel;
            }else{
                if((in.has_dest_los[q] != 0) == los_latched) los_hyst = 0;  // the LOS debounce, :925-930
                else if(++los_hyst >= 12) { los_latched = in.has_dest_los[q] != 0; los_hyst = 0; }   // ARRIVAL_LOS_HYST
                if(los_latched) {
                    vdes = av_heading(vsub(centre, pos));
                }else{
                    uint32_t st = 0;
                    vdes = sample_flow(P, in.com_row[zi], pos, st);
                    if(st) { status = NAVHIP_AV_COM_MISS; vdes = mkv(nan, nan); }
                }
            }
        }
    }
    if(gl == 0) {
        if(out.vdes_xz) { out.vdes_xz[2 * q] = vdes.x; out.vdes_xz[2 * q + 1] = vdes.z; }
        if(out.dense_vdes_xz && uid >= 0 && uid < P.n_ents) { out.dense_vdes_xz[2 * uid] = vdes.x; out.dense_vdes_xz[2 * uid + 1] = vdes.z; }
        out.status[q] = (uint8_t)status;
        out.substate[q] = (uint8_t)substate;
        out.sink_valid[q] = host ? in.sink_valid[q] : (sink_valid ? 1 : 0);
        out.sink_xz[2 * q] = sink.x; out.sink_xz[2 * q + 1] = sink.z;
        out.los_latched[q] = host ? in.los_latched[q] : (los_latched ? 1 : 0);
        out.los_hyst[q] = los_hyst;
    }
}

// ---------------------------------------------------------------------------------------------
// C entry points
// ---------------------------------------------------------------------------------------------
namespace {

// the lengths and groups of this unit's structs beside the shared ones (stage_plan.h)
enum { SK_PER_TILE = NH_LEN_OWN, SK_PER_RANGE_ROW_PLUS1, SK_PER_RANGE_TILE,
       SK_PER_ARM_ROW,          // a row per unit -- with sparse rows, per LISTED unit
       SK_PER_LISTED, SK_LEN_END };
enum { SK_SKIP = NH_ON_OWN, SK_TURN, SK_RANGE, SK_SURROUND, SK_INTERP, SK_SPARSE, SK_AUX, SK_ON_END };
static_assert(SK_LEN_END <= NH_LEN_COUNT && SK_ON_END <= NH_ON_COUNT, "nh_dims has no room for this unit's own lengths and groups");

// the structs of the state pass and of the settle calls: one list each (stage_plan.h)
const nh_row sk_gate_rows[] = {
    NH_ROW(navhip_gate_in, next_rot, 16, NH_LEN_UNIT, NH_ON_ALWAYS),  NH_ROW(navhip_gate_in, new_vel_xz, 8, NH_LEN_UNIT, NH_ON_ALWAYS),
    NH_ROW(navhip_gate_in, vdes_xz, 8, NH_LEN_UNIT, NH_ON_ALWAYS),  NH_ROW(navhip_gate_in, interp_from_xz, 8, NH_LEN_UNIT, SK_INTERP),
    NH_ROW(navhip_gate_in, interp_step, 4, NH_LEN_UNIT, SK_INTERP),
};
const nh_row sk_state_rows[] = {
    NH_ROW(navhip_state_in, new_pos_xz, 8, NH_LEN_UNIT, NH_ON_ALWAYS),  NH_ROW(navhip_state_in, vdes_xz, 8, NH_LEN_UNIT, NH_ON_ALWAYS),
    NH_ROW(navhip_state_in, skip, 1, NH_LEN_UNIT, SK_SKIP),  NH_ROW(navhip_state_in, flock_layer, 1, NH_LEN_FLOCK, NH_ON_ALWAYS),
    NH_ROW(navhip_state_in, flock_nearest_xz, 8, NH_LEN_FLOCK, NH_ON_ALWAYS),
    NH_ROW(navhip_state_in, flock_tiles_off, 4, NH_LEN_FLOCK_PLUS1, NH_ON_ALWAYS),
    NH_ROW(navhip_state_in, flock_tiles, 4, SK_PER_TILE, NH_ON_ALWAYS),
};
const nh_row sk_aux_rows[] = {
    NH_ROW(navhip_state_aux_in, fstate, 1, NH_LEN_UNIT, NH_ON_ALWAYS),  NH_ROW(navhip_state_aux_in, wait_ticks_left, 4, NH_LEN_UNIT, NH_ON_ALWAYS),
    NH_ROW(navhip_state_aux_in, wait_prev, 1, NH_LEN_UNIT, NH_ON_ALWAYS),  NH_ROW(navhip_state_aux_in, new_pos_xz, 8, NH_LEN_UNIT, NH_ON_ALWAYS),
    NH_ROW(navhip_state_aux_in, ent_rot, 16, SK_PER_ARM_ROW, SK_TURN),  NH_ROW(navhip_state_aux_in, target_dir, 16, SK_PER_ARM_ROW, SK_TURN),
    NH_ROW(navhip_state_aux_in, range_target, 4, SK_PER_ARM_ROW, SK_RANGE),
    NH_ROW(navhip_state_aux_in, target_range, 4, SK_PER_ARM_ROW, SK_RANGE),
    NH_ROW(navhip_state_aux_in, target_prev_xz, 8, SK_PER_ARM_ROW, SK_RANGE),
    NH_ROW(navhip_state_aux_in, range_tiles_row, 4, SK_PER_ARM_ROW, SK_RANGE),
    NH_ROW(navhip_state_aux_in, range_tiles_off, 4, SK_PER_RANGE_ROW_PLUS1, SK_RANGE),
    NH_ROW_PAD(navhip_state_aux_in, range_tiles, 4, SK_PER_RANGE_TILE, SK_RANGE, 4),
    NH_ROW(navhip_state_aux_in, surround_target, 4, SK_PER_ARM_ROW, SK_SURROUND),
    NH_ROW(navhip_state_aux_in, surround_query, 1, SK_PER_ARM_ROW, SK_SURROUND),
    NH_ROW(navhip_state_aux_in, surround_target_prev_xz, 8, SK_PER_ARM_ROW, SK_SURROUND),
    NH_ROW(navhip_state_aux_in, surround_nearest_prev_xz, 8, SK_PER_ARM_ROW, SK_SURROUND),
    NH_ROW(navhip_state_aux_in, surround_dest_xz, 16, SK_PER_ARM_ROW, SK_SURROUND),
    NH_ROW(navhip_state_aux_in, vdes_xz, 8, NH_LEN_UNIT, SK_SURROUND),
    NH_ROW_OUT_RANGE(navhip_state_aux_in, out_surround_dest_xz, 8, NH_LEN_UNIT, SK_SURROUND),
    NH_ROW(navhip_state_aux_in, sparse_units, 4, SK_PER_LISTED, SK_SPARSE),
};
const nh_row sk_pass_out_rows[] = {
    NH_ROW_OUT_RANGE(navhip_state_pass_out, state, 1, NH_LEN_UNIT, NH_ON_ALWAYS),  NH_ROW_OUT_RANGE(navhip_state_pass_out, flags, 1, NH_LEN_UNIT, NH_ON_ALWAYS),
    NH_ROW_OUT_RANGE(navhip_state_pass_out, gate, 1, NH_LEN_UNIT, NH_ON_ALWAYS),  NH_ROW_OUT_RANGE(navhip_state_pass_out, new_pos_xz, 8, NH_LEN_UNIT, NH_ON_ALWAYS),
    NH_ROW_OUT_RANGE(navhip_state_pass_out, vel_xz, 8, NH_LEN_UNIT, NH_ON_ALWAYS),  NH_ROW_OUT_RANGE(navhip_state_pass_out, wait_ticks_left, 4, NH_LEN_UNIT, SK_AUX),
};
const nh_row sk_settle_in_rows[] = {
    NH_ROW(navhip_settle_in, zones, sizeof(navhip_arrival_zone), NH_LEN_ZONE, NH_ON_ALWAYS),
    NH_ROW_PAD(navhip_settle_in, slots_xz, 8, NH_LEN_SLOT, NH_ON_ALWAYS, 8),  NH_ROW_PAD(navhip_settle_in, slot_ring, 4, NH_LEN_SLOT, NH_ON_ALWAYS, 4),
    NH_ROW_PAD(navhip_settle_in, region_keys, 8, NH_LEN_KEY, NH_ON_ALWAYS, 8),  NH_ROW(navhip_settle_in, uid, 4, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_settle_in, zone, 4, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW(navhip_settle_in, new_pos_xz, 8, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_settle_in, nsettled, 4, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW(navhip_settle_in, substate, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_settle_in, sink_valid, 1, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW(navhip_settle_in, sink_xz, 8, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_settle_in, order_pos_xz, 8, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW(navhip_settle_in, progress_anchor_xz, 8, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_settle_in, progress_anchored, 1, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW(navhip_settle_in, stuck, 4, NH_LEN_QUERY, NH_ON_ALWAYS),
};
const nh_row sk_settle_out_rows[] = {
    NH_ROW_OUT(navhip_settle_out, settle, 1, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW_OUT(navhip_settle_out, substate, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW_OUT(navhip_settle_out, progress_anchor_xz, 8, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW_OUT(navhip_settle_out, progress_anchored, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW_OUT(navhip_settle_out, stuck, 4, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW_OUT(navhip_settle_out, nsettled, 4, NH_LEN_QUERY, NH_ON_ALWAYS),
};
NH_COVERS(sk_gate_rows, navhip_gate_in, 0);
NH_COVERS(sk_state_rows, navhip_state_in, 0);
NH_COVERS(sk_aux_rows, navhip_state_aux_in, 16);            // n_range_rows, n_sparse: 4 bytes and 4 of padding each
NH_COVERS(sk_pass_out_rows, navhip_state_pass_out, 0);
NH_COVERS(sk_settle_in_rows, navhip_settle_in, 8);          // n_zones, nq
NH_COVERS(sk_settle_out_rows, navhip_settle_out, 0);

// the two structs of navhip_arrival_velocity
const nh_row av_in_rows[] = {
    NH_ROW(navhip_arrival_vel_in, zones, sizeof(navhip_arrival_zone), NH_LEN_ZONE, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_vel_in, slots_xz, 8, NH_LEN_SLOT, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_vel_in, slot_ring, 4, NH_LEN_SLOT, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_vel_in, region_keys, 8, NH_LEN_KEY, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_vel_in, zone_row, 4, NH_LEN_ZONE, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_vel_in, com_row, 4, NH_LEN_ZONE, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_vel_in, uid, 4, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_vel_in, zone, 4, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_vel_in, has_dest_los, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_vel_in, substate, 1, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_vel_in, sink_valid, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_vel_in, sink_xz, 8, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW(navhip_arrival_vel_in, los_latched, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW(navhip_arrival_vel_in, los_hyst, 4, NH_LEN_QUERY, NH_ON_ALWAYS),
};
const nh_row av_out_rows[] = {
    NH_ROW_OUT(navhip_arrival_vel_out, vdes_xz, 8, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW_OUT(navhip_arrival_vel_out, status, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW_OUT(navhip_arrival_vel_out, substate, 1, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW_OUT(navhip_arrival_vel_out, sink_valid, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW_OUT(navhip_arrival_vel_out, sink_xz, 8, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW_OUT(navhip_arrival_vel_out, los_latched, 1, NH_LEN_QUERY, NH_ON_ALWAYS),
    NH_ROW_OUT(navhip_arrival_vel_out, los_hyst, 4, NH_LEN_QUERY, NH_ON_ALWAYS),  NH_ROW_OUT(navhip_arrival_vel_out, dense_vdes_xz, 8, NH_LEN_QUERY, NH_ON_DEV_ONLY),
};
NH_COVERS(av_in_rows, navhip_arrival_vel_in, 16);           // n_zones, nq, n_slots, n_keys
NH_COVERS(av_out_rows, navhip_arrival_vel_out, 0);

bool sk_work_range(const navhip_world *w, int *b, int *e)
{
    *b = w->work_begin; *e = w->work_end;
    if(*b == 0 && *e == 0) *e = w->n_ents;
    return *b >= 0 && *e <= w->n_ents && *b <= *e;
}

nh_dims sk_dims_of(const navhip_world *w, int b, int e)
{
    nh_dims D;
    D.len[NH_LEN_UNIT] = D.len[SK_PER_ARM_ROW] = (size_t)w->n_ents;
    D.len[NH_LEN_FLOCK] = (size_t)(w->n_flocks > 0 ? w->n_flocks : 0);
    D.len[NH_LEN_FLOCK_PLUS1] = D.len[NH_LEN_FLOCK] + 1;
    D.lo = (size_t)b; D.cnt = (size_t)(e - b);
    return D;
}

// ---- one argument check per struct: the host-buffer calls, the passes and the _dev entry points all use them --------
bool sk_csr_ok(const int32_t *off, size_t rows)
{
    for(size_t r = 0; r < rows; r++)
        if(off[r] < 0 || off[r + 1] < off[r]) return false;
    return true;
}

// the snapshot arrays the gate reads, its three inputs; the interpolated position of a rate below 20 Hz: both arrays,
// the movement rate, and what names the unit's nav layer
bool sk_check_gate(const navhip_world *w, const navhip_gate_in *in)
{
    if(!w->pos_xz || !w->vel_xz || !w->state || !in->next_rot || !in->new_vel_xz || !in->vdes_xz) return false;
    if((in->interp_from_xz != nullptr) != (in->interp_step != nullptr)) return false;
    if(w->hz != 20 && w->hz != 10 && w->hz != 5 && w->hz != 1 && w->hz != 0) return false;
    return !in->interp_from_xz || (w->radius && w->flags);
}

// navhip_state_in inside a pass (new_pos_xz and vdes_xz are the gate's); navhip_state_update_dev checks this and those two
bool sk_check_state(const navhip_world *w, const navhip_state_in *in)
{
    return w->pos_xz && w->radius && w->flags && w->state && w->flock
        && (w->n_flocks <= 0 || (w->flock_target_xz && w->flock_offsets && w->flock_members && in->flock_layer && in->flock_nearest_xz
                                 && in->flock_tiles_off && in->flock_tiles));
}

enum sk_aux_caller {
    SK_AUX_ALONE,       // navhip_state_update_aux[_dev]: every array is the caller's
    SK_PASS,            // navhip_state_pass: new_pos_xz, vdes_xz and the snapshot of the surround arm are the pass's own
    SK_PASS_RESIDENT,   // navhip_state_pass_resident: that, sparse rows are allowed, and range arrays without a range_target are
                        // ignored, not refused, as that call always has
};
bool sk_check_aux(const navhip_world *w, const navhip_state_aux_in *in, sk_aux_caller by)
{
    if(!w->radius || !w->flags || !w->state || !in->fstate || !in->wait_ticks_left || !in->wait_prev
    || (by == SK_AUX_ALONE && !in->new_pos_xz) || (in->ent_rot != nullptr) != (in->target_dir != nullptr)) return false;
    // sparse rows are navhip_state_pass_resident's
    if(by != SK_PASS_RESIDENT && (in->sparse_units != nullptr || in->n_sparse != 0)) return false;
    // the six enter-range inputs come together, with the positions of the snapshot
    const int range = (in->range_target != nullptr) + (in->target_range != nullptr) + (in->target_prev_xz != nullptr)
                    + (in->range_tiles_row != nullptr) + (in->range_tiles_off != nullptr) + (in->range_tiles != nullptr);
    if(!(by == SK_PASS_RESIDENT && !in->range_target) && range != 0 && !(range == 6 && w->pos_xz && in->n_range_rows >= 0)) return false;
    // the surround inputs come together, with the snapshot arrays the arm reads (a pass supplies vdes and those itself:
    // its caller gives the five query arrays and the output)
    const int query = (in->surround_query != nullptr) + (in->surround_target_prev_xz != nullptr) + (in->surround_nearest_prev_xz != nullptr)
                    + (in->surround_dest_xz != nullptr) + (in->out_surround_dest_xz != nullptr);
    if(in->surround_target && query != 5) return false;
    if(by != SK_AUX_ALONE) return true;
    if(!in->surround_target) return query == 0 && !in->vdes_xz;
    return in->vdes_xz && w->pos_xz && w->vel_xz && w->flock && (w->n_flocks == 0 || w->flock_target_xz);
}

// The per-unit rows of the enter-range and surround arms, rows [v0, v1) of their arrays; fills in which arms are given and how
// long the range tables are.  hw: the snapshot where the host has it; NULL in the resident pass, where states and flocks
// are on the device: then every row with a range target is checked whatever its unit's state, row 0 passes when there
// are no rows at all (what a unit of another state holds), and a surround unit's flock is not looked at.
bool sk_check_arm_rows(const navhip_state_aux_in *in, int n_ents, const navhip_world *hw, size_t v0, size_t v1, nh_dims *D)
{
    D->on[SK_TURN] = in->ent_rot != nullptr; D->on[SK_RANGE] = in->range_target != nullptr; D->on[SK_SURROUND] = in->surround_target != nullptr;
    if(in->range_target) {
        const size_t rows = (size_t)in->n_range_rows;
        if(!sk_csr_ok(in->range_tiles_off, rows)) return false;
        D->len[SK_PER_RANGE_ROW_PLUS1] = rows + 1;
        D->len[SK_PER_RANGE_TILE] = rows ? (size_t)in->range_tiles_off[rows] : 0;
        for(size_t i = v0; i < v1; i++) {
            const int32_t t = in->range_target[i], r = in->range_tiles_row[i];
            if(t >= n_ents) return false;
            if(t >= 0 && (!hw || hw->state[i] == NAVHIP_STATE_ENTER_ENTITY_RANGE) && (r < 0 || (size_t)r >= (hw || rows ? rows : 1))) return false;
        }
    }
    if(in->surround_target)
        for(size_t i = v0; i < v1; i++) {
            const int32_t t = in->surround_target[i];
            if(t >= n_ents) return false;
            if(hw && hw->state[i] == NAVHIP_STATE_SURROUND_ENTITY && t >= -1 && hw->flock[i] >= hw->n_flocks) return false;
        }
    return true;
}

// what every settle call needs of its two structs (nsettled aside: navhip_arrival_settle_resident can count on the device)
bool sk_check_settle(const navhip_settle_in *in, const navhip_settle_out *out)
{
    return in->zones && in->n_zones >= 1 && in->uid && in->zone && in->new_pos_xz && in->substate && in->sink_valid && in->sink_xz
        && in->order_pos_xz && in->progress_anchor_xz && in->progress_anchored && in->stuck && out->settle && out->substate
        && out->progress_anchor_xz && out->progress_anchored && out->stuck;
}

#define AV_FAIL(why) nh_fail(ctx, NAVHIP_ERR_ARG, name, why)     /* inside the check below: `name` is the form's */
// The one argument check of navhip_arrival_velocity and navhip_arrival_velocity_dev; host_arrays: the arrays can be read
// here (the host form), so what lies IN them is checked too.  Fills in the two mapping tables, the pool and how many rows
// each table has.  The reason of a refusal goes to last_error.
struct av_tables { const int32_t *com_slot, *zone_slot; const uint8_t *pool; int n_com_rows, n_zone_rows; bool resident; };
int av_check(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_vel_in *in, const navhip_arrival_vel_out *out,
             bool host_arrays, av_tables *T)
{
    if(!ctx) return NAVHIP_ERR_ARG;
    const char *name = host_arrays ? "navhip_arrival_velocity: " : "navhip_arrival_velocity_dev: ";
    if(!w || !in || !out) return AV_FAIL("a missing argument");
    if(in->nq < 0) return AV_FAIL("nq < 0");
    if(in->n_zones < 0 || in->n_slots < 0 || in->n_keys < 0 || w->n_ents < 0) return AV_FAIL("a negative count");
    if(in->nq == 0) return NAVHIP_OK;
    if(!w->pos_xz) return AV_FAIL("a missing array: world->pos_xz");
    if(in->n_zones > 0 && (!in->zones || !in->zone_row || !in->com_row)) return AV_FAIL("a missing array: zones, zone_row or com_row");
    if((in->n_slots > 0 && (!in->slots_xz || !in->slot_ring)) || (in->n_keys > 0 && !in->region_keys))
        return AV_FAIL("a missing array: slots_xz, slot_ring or region_keys");
    if(!in->uid || !in->zone || !in->has_dest_los || !in->substate || !in->sink_valid || !in->sink_xz || !in->los_latched || !in->los_hyst)
        return AV_FAIL("a missing array of navhip_arrival_vel_in");
    if(!out->status || !out->substate || !out->sink_valid || !out->sink_xz || !out->los_latched || !out->los_hyst)
        return AV_FAIL("a missing array of navhip_arrival_vel_out");
    if(host_arrays ? (!out->vdes_xz || out->dense_vdes_xz) : (!out->vdes_xz && !out->dense_vdes_xz))
        return AV_FAIL(host_arrays ? "vdes_xz missing, or dense_vdes_xz given to the host form" : "neither vdes_xz nor dense_vdes_xz");
    T->resident = w->n_field_slots == NAVHIP_POOL_RESIDENT;
    if(T->resident) {
        if(!ctx->pool) return AV_FAIL("NAVHIP_POOL_RESIDENT without a resident pool");
        T->com_slot = T->zone_slot = nh_pool_map(ctx); T->pool = nh_pool_fields(ctx);
        T->n_com_rows = T->n_zone_rows = nh_pool_dests(ctx);
    }else{
        T->com_slot = w->flock_field_slot; T->zone_slot = w->region_field_slot; T->pool = w->field_pool;
        T->n_com_rows = T->com_slot && w->n_flocks > 0 ? w->n_flocks : 0;
        T->n_zone_rows = T->zone_slot && w->n_region_rows > 0 ? w->n_region_rows : 0;
        if((T->n_com_rows || T->n_zone_rows) && (!T->pool || w->n_field_slots < 1)) return AV_FAIL("a mapping table without field_pool");
    }
    if(!host_arrays) return NAVHIP_OK;
    for(int z = 0; z < in->n_zones; z++) {
        const navhip_arrival_zone &Z = in->zones[z];
        const std::string zn = "zone " + std::to_string(z);
        if(const char *fault = nh_zone_fault(Z, nullptr, in->n_slots, in->n_keys, 0, in->region_keys)) return AV_FAIL(zn + fault);
        if(Z.layer < 0 || Z.layer >= NAVHIP_NAV_LAYER_MAX) return AV_FAIL(zn + ": layer outside the map's");
        if(in->zone_row[z] < -1 || in->zone_row[z] >= T->n_zone_rows) return AV_FAIL(zn + ": zone_row outside region_field_slot");
        if(in->com_row[z] < -1 || in->com_row[z] >= T->n_com_rows) return AV_FAIL(zn + ": com_row outside flock_field_slot");
    }
    return NAVHIP_OK;
}

}   // namespace

extern "C" {

int navhip_heading_gate_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_gate_in *in, float *out_vel,
                            float *out_new_pos, uint8_t *out_gate, void *stream)
{
    if(!ctx || !w || !in || !out_vel || !out_new_pos || !out_gate || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    if(w->n_ents == 0) return NAVHIP_OK;
    int b, e;
    if(!sk_check_gate(w, in) || !sk_work_range(w, &b, &e)) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if(in->interp_from_xz) {
        // (the accept test of the interpolated position probes the derived row masks: rebuilt here if a plane changed)
        int rc = nh_refresh_derived(ctx, ctx->stream);
        if(rc) return rc;
    }
    nh_step_params P;
    nh_step_params_init(ctx, w, &P);
    if(e > b)
        hipLaunchKernelGGL(k_heading_gate, dim3((e - b + 255) / 256), dim3(256), 0, stream ? (hipStream_t)stream : ctx->stream,
                           P, b, e, w->pos_xz, w->vel_xz, w->state, w->radius, w->flags, *in, out_vel, out_new_pos, out_gate);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_heading_gate(navhip_ctx *ctx, const navhip_world *w, const navhip_gate_in *in, float *out_vel,
                        float *out_new_pos, uint8_t *out_gate)
{
    if(!ctx || !w || !in || !out_vel || !out_new_pos || !out_gate || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    if(w->n_ents == 0) return NAVHIP_OK;
    int b, e;
    if(!sk_check_gate(w, in) || !sk_work_range(w, &b, &e)) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    nh_dims D = sk_dims_of(w, b, e);
    D.on[SK_INTERP] = in->interp_from_xz != nullptr;
    const size_t n = (size_t)w->n_ents;
    nh_plan P;
    navhip_world d = nh_device_world(w);
    navhip_gate_in di = {};
    nh_plan_world(P, w, &d, D, {NH_W(pos_xz), NH_W(vel_xz), NH_W(state)});
    if(D.on[SK_INTERP]) nh_plan_world(P, w, &d, D, {NH_W(radius), NH_W(flags)});
    nh_plan_rows(P, sk_gate_rows, in, &di, D);
    float *d_vel, *d_pos; uint8_t *d_gate;
    P.out(P.scratch(n * 8, (void**)&d_vel), out_vel, 8, D.lo, D.cnt);
    P.out(P.scratch(n * 8, (void**)&d_pos), out_new_pos, 8, D.lo, D.cnt);
    P.out(P.scratch(n, (void**)&d_gate), out_gate, 1, D.lo, D.cnt);
    int rc = P.reserve(ctx, NH_STAGE_STATE_ARENA);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = navhip_heading_gate_dev(ctx, &d, &di, d_vel, d_pos, d_gate, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

// k_state_update and k_arrived_compact on device arrays
int navhip_state_update_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_state_in *in, uint8_t *out_state,
                            uint8_t *out_flags, void *stream)
{
    if(!ctx || !w || !in || !out_state || !out_flags || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    if(w->n_ents == 0) return NAVHIP_OK;
    if(!sk_check_state(w, in) || !in->new_pos_xz || !in->vdes_xz) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = nh_refresh_derived(ctx, ctx->stream);
    if(rc) return rc;
    nh_step_params P;
    nh_step_params_init(ctx, w, &P);
    P.n_flocks = w->n_flocks;
    if(!sk_work_range(w, &P.work_begin, &P.work_end)) return NAVHIP_ERR_INVALID;
    P.pos_xz = w->pos_xz; P.radius = w->radius; P.flags = w->flags; P.state = w->state; P.flock = w->flock;
    P.flock_target_xz = w->flock_target_xz; P.flock_offsets = w->flock_offsets; P.flock_members = w->flock_members;
    // (scratch of the arrived-flock-mate rule: the ARRIVED members of every flock, compacted -- every entity belongs to at
    // most one flock)
    rc = nh_ensure_buf(ctx, ctx->state_arrived, 16 * (size_t)w->n_ents);
    if(!rc) rc = nh_ensure_buf(ctx, ctx->state_arrived_n, 4 * (size_t)(w->n_flocks > 0 ? w->n_flocks : 1));
    if(rc) return rc;
    nh_launch_state_update(P, *in, (float4*)ctx->state_arrived.p, (int32_t*)ctx->state_arrived_n.p, out_state, out_flags,
                           stream ? (hipStream_t)stream : ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_state_update(navhip_ctx *ctx, const navhip_world *w, const navhip_state_in *in, uint8_t *out_state, uint8_t *out_flags)
{
    if(!ctx || !w || !in || !out_state || !out_flags) return NAVHIP_ERR_INVALID;
    if(w->n_ents <= 0) return w->n_ents == 0 ? NAVHIP_OK : NAVHIP_ERR_INVALID;
    if(w->n_flocks > 0 && (!w->flock_offsets || !in->flock_tiles_off)) return NAVHIP_ERR_INVALID;
    int b, e;
    if(!sk_work_range(w, &b, &e)) return NAVHIP_ERR_INVALID;
    nh_dims D = sk_dims_of(w, b, e);
    const size_t n = (size_t)w->n_ents, F = D.len[NH_LEN_FLOCK];
    D.len[SK_PER_TILE] = F ? (size_t)in->flock_tiles_off[F] : 0;
    if(F && (size_t)w->flock_offsets[F] > n) {     // (an entity belongs to at most one flock: the scratch of the arrived-mate rule is sized by it)
        ctx->last_error = "navhip_state_update: more flock members than entities";
        return NAVHIP_ERR_INVALID;
    }
    D.on[SK_SKIP] = in->skip != nullptr;
    // (no destination has island tiles: the kernel still wants a pointer of its own -- nothing is read from it, and none
    // need be given)
    D.pad = 4;
    // (what is staged below is never NULL on the device: an array the caller left out is refused here)
    if(!in->new_pos_xz || !in->vdes_xz
    || (F && (!in->flock_layer || !in->flock_nearest_xz || (!in->flock_tiles && D.len[SK_PER_TILE])))) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // the arrays of the snapshot that k_state_update reads: the world's own staging slots (nh_world_rows)
    navhip_world d;
    int rc = nh_stage_world(ctx, w, &d, s, {NH_W(pos_xz), NH_W(radius), NH_W(flags), NH_W(state), NH_W(flock), NH_W(flock_target_xz),
                                            NH_W(flock_offsets), NH_W(flock_members)});
    if(rc) return rc;
    // navhip_state_in and the two results: one copy per row
    nh_plan P;
    navhip_state_in di = {};
    nh_plan_rows(P, sk_state_rows, in, &di, D);
    uint8_t *d_state, *d_flags;
    P.out(P.scratch(n, (void**)&d_state), out_state, 1, D.lo, D.cnt);
    P.out(P.scratch(n, (void**)&d_flags), out_flags, 1, D.lo, D.cnt);
    rc = P.reserve(ctx, NH_STAGE_STATE_ARENA);
    if(!rc) rc = P.upload(ctx, s);
    nh_async_invalidate_static(ctx);
    if(!rc) rc = navhip_state_update_dev(ctx, &d, &di, d_state, d_flags, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

int navhip_state_update_aux_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_state_aux_in *in, uint8_t *io_state,
                                uint8_t *io_flags, int32_t *out_ticks, void *stream)
{
    if(!ctx || !w || !in || !io_state || !io_flags || !out_ticks || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    if(w->n_ents == 0) return NAVHIP_OK;
    int b, e;
    if(!sk_check_aux(w, in, SK_AUX_ALONE) || !sk_work_range(w, &b, &e)) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    nh_step_params P;
    nh_step_params_init(ctx, w, &P);
    P.work_begin = b; P.work_end = e;
    if(in->surround_target) { P.flock = w->flock; P.flock_target_xz = w->flock_target_xz; P.vel_xz = w->vel_xz; P.n_flocks = w->n_flocks; }
    if(e > b)
        hipLaunchKernelGGL(k_state_aux, dim3((e - b + 255) / 256), dim3(256), 0, stream ? (hipStream_t)stream : ctx->stream,
                           P, w->pos_xz, w->radius, w->flags, w->state, *in, io_state, io_flags, out_ticks);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_state_update_aux(navhip_ctx *ctx, const navhip_world *w, const navhip_state_aux_in *in, uint8_t *io_state,
                            uint8_t *io_flags, int32_t *out_ticks)
{
    if(!ctx || !w || !in || !io_state || !io_flags || !out_ticks || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    if(w->n_ents == 0) return NAVHIP_OK;
    int b, e;
    if(!sk_check_aux(w, in, SK_AUX_ALONE) || !sk_work_range(w, &b, &e)) return NAVHIP_ERR_INVALID;
    nh_dims D = sk_dims_of(w, b, e);
    if(!sk_check_arm_rows(in, w->n_ents, w, (size_t)b, (size_t)e, &D)) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)w->n_ents;
    nh_plan P;
    navhip_world d = nh_device_world(w);
    navhip_state_aux_in di = {};
    if(D.on[SK_RANGE]) di.n_range_rows = in->n_range_rows;
    nh_plan_world(P, w, &d, D, {NH_W(radius), NH_W(flags), NH_W(state)});
    // (only the enter-range and surround arms read positions)
    if(D.on[SK_RANGE] || D.on[SK_SURROUND]) nh_plan_world(P, w, &d, D, {NH_W(pos_xz)});
    if(D.on[SK_SURROUND]) {
        nh_plan_world(P, w, &d, D, {NH_W(vel_xz), NH_W(flock)});
        nh_plan_world(P, w, &d, D, {NH_W(flock_target_xz)}, 0, 8);
    }
    nh_plan_rows(P, sk_aux_rows, in, &di, D);
    uint8_t *d_state, *d_flags; int32_t *d_ticks;
    P.out(P.in(io_state, n, 0, (void**)&d_state), io_state, 1, D.lo, D.cnt);
    P.out(P.in(io_flags, n, 0, (void**)&d_flags), io_flags, 1, D.lo, D.cnt);
    P.out(P.scratch(n * 4, (void**)&d_ticks), out_ticks, 4, D.lo, D.cnt);
    int rc = P.reserve(ctx, NH_STAGE_STATE_ARENA);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = navhip_state_update_aux_dev(ctx, &d, &di, d_state, d_flags, d_ticks, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

// gate -> state update on the gate's positions -> aux (da != NULL) -> the rows the gate leaves to the host; r: the device
// twins of the results.  units / ns / listed_dest: sparse rows with a surround arm, whose positions go back per listed unit.
static int sk_run_passes(navhip_ctx *ctx, const navhip_world *d, int b, int e, const navhip_gate_in &dg, navhip_state_in ds,
                         navhip_state_aux_in *da, const navhip_state_pass_out &r, const int32_t *units, size_t ns,
                         float *listed_dest, hipStream_t s)
{
    int rc = navhip_heading_gate_dev(ctx, d, &dg, r.vel_xz, r.new_pos_xz, r.gate, s);
    if(rc) return rc;
    ds.new_pos_xz = r.new_pos_xz; ds.vdes_xz = dg.vdes_xz;
    rc = navhip_state_update_dev(ctx, d, &ds, r.state, r.flags, s);
    if(rc) return rc;
    if(da) {
        da->new_pos_xz = r.new_pos_xz;
        if(da->surround_target) da->vdes_xz = dg.vdes_xz;
        rc = navhip_state_update_aux_dev(ctx, d, da, r.state, r.flags, r.wait_ticks_left, s);
        if(rc) return rc;
    }
    if(e > b) {
        hipLaunchKernelGGL(k_gate_host_rows, dim3((e - b + 255) / 256), dim3(256), 0, s, b, e, (const uint8_t*)r.gate, d->state,
                           da ? da->wait_ticks_left : (const int32_t*)nullptr, r.state, r.flags, r.wait_ticks_left);
        HIPCHK(ctx, hipGetLastError());
        if(units && ns) {
            hipLaunchKernelGGL(k_sparse_gather2, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, (int)ns, units,
                               (const float*)da->out_surround_dest_xz, listed_dest);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    return NAVHIP_OK;
}

int navhip_state_pass(navhip_ctx *ctx, const navhip_world *w, const navhip_state_pass_in *in, const navhip_state_pass_out *out)
{
    if(!ctx || !w || !in || !out || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    if(w->n_ents == 0) return NAVHIP_OK;
    const navhip_gate_in &G = in->gate;
    const navhip_state_in &T = in->state;
    const navhip_state_aux_in &X = in->aux;
    const bool aux = X.fstate != nullptr;
    int b, e;
    // (a negative flock count never got past the offsets below)
    if(w->n_flocks < 0 || !sk_check_gate(w, &G) || !sk_check_state(w, &T) || (aux && !sk_check_aux(w, &X, SK_PASS))
    || !out->state || !out->flags || !out->gate || !out->new_pos_xz || (aux && !out->wait_ticks_left) || !sk_work_range(w, &b, &e))
        return NAVHIP_ERR_INVALID;
    nh_dims D = sk_dims_of(w, b, e);
    const size_t n = (size_t)w->n_ents, F = D.len[NH_LEN_FLOCK];
    // (offsets that are not a CSR become a huge size_t below -- INVALID, not NOMEM)
    if(!sk_csr_ok(w->flock_offsets, F) || !sk_csr_ok(T.flock_tiles_off, F) || (F && (size_t)w->flock_offsets[F] > n)
    || (aux && !sk_check_arm_rows(&X, w->n_ents, w, (size_t)b, (size_t)e, &D))) return NAVHIP_ERR_INVALID;
    D.len[SK_PER_TILE] = F ? (size_t)T.flock_tiles_off[F] : 0;
    D.on[SK_SKIP] = T.skip != nullptr; D.on[SK_INTERP] = G.interp_from_xz != nullptr; D.on[SK_AUX] = aux;
    D.pad = 8;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    nh_plan P;
    navhip_world d = nh_device_world(w);
    navhip_gate_in dg = {}; navhip_state_in ds = {}; navhip_state_aux_in da = {}; navhip_state_pass_out r = {};
    if(D.on[SK_RANGE]) da.n_range_rows = X.n_range_rows;
    // the snapshot, once
    nh_plan_world(P, w, &d, D, {NH_W(pos_xz), NH_W(vel_xz), NH_W(radius), NH_W(flags), NH_W(state), NH_W(flock), NH_W(flock_target_xz),
                                 NH_W(flock_offsets), NH_W(flock_members)}, F ? (size_t)w->flock_offsets[F] : 0);
    nh_plan_rows(P, sk_gate_rows, &G, &dg, D);
    nh_plan_rows(P, sk_state_rows, &T, &ds, D, {offsetof(navhip_state_in, new_pos_xz), offsetof(navhip_state_in, vdes_xz)});
    if(aux) nh_plan_rows(P, sk_aux_rows, &X, &da, D, {offsetof(navhip_state_aux_in, new_pos_xz), offsetof(navhip_state_aux_in, vdes_xz)});
    nh_plan_rows(P, sk_pass_out_rows, out, &r, D);
    int rc = P.reserve(ctx, NH_STAGE_STATE_ARENA);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = sk_run_passes(ctx, &d, b, e, dg, ds, aux ? &da : nullptr, r, nullptr, 0, nullptr, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

int navhip_state_pass_resident(navhip_ctx *ctx, const navhip_state_pass_in *in, const navhip_state_pass_out *out)
{
    if(!ctx || !in || !out) return NAVHIP_ERR_INVALID;
    navhip_world d; navhip_step_out so;
    if(!nh_async_resident(ctx, &d, &so)) {
        ctx->last_error = "navhip_state_pass_resident: no completed host-buffer step is resident on the device";
        return NAVHIP_ERR_INVALID;
    }
    const navhip_state_in &T = in->state;
    const navhip_state_aux_in &X = in->aux;
    const bool aux = X.fstate != nullptr, su = aux && X.surround_target != nullptr;
    const size_t n = (size_t)d.n_ents;
    if(n == 0) return NAVHIP_OK;
    navhip_gate_in G = in->gate;                                // (its new_vel_xz and vdes_xz are the step's own outputs)
    G.new_vel_xz = so.vel_xz; G.vdes_xz = so.vdes_xz ? so.vdes_xz : d.vdes_xz;
    int b, e;
    if(!sk_check_gate(&d, &G) || !sk_check_state(&d, &T) || (aux && !sk_check_aux(&d, &X, SK_PASS_RESIDENT))
    || !out->state || !out->flags || !out->gate || !out->new_pos_xz || (aux && !out->wait_ticks_left) || !sk_work_range(&d, &b, &e))
        return NAVHIP_ERR_INVALID;
    // sparse rows: the arrays of the three arms hold a row per LISTED unit (ns of them), the device lays them out
    const bool sp = aux && X.sparse_units != nullptr;
    if((X.sparse_units == nullptr && X.n_sparse != 0) || X.n_sparse < 0 || (X.sparse_units && !aux)) return NAVHIP_ERR_INVALID;
    const size_t ns = sp ? (size_t)X.n_sparse : 0;
    for(size_t k = 0; k < ns; k++)
        if(X.sparse_units[k] < b || X.sparse_units[k] >= e) return NAVHIP_ERR_INVALID;
    nh_dims D = sk_dims_of(&d, b, e);
    const size_t F = D.len[NH_LEN_FLOCK];
    // (the checks of the arms walk the rows of their arrays: the listed units', or the slab's)
    if(!sk_csr_ok(T.flock_tiles_off, F)
    || (aux && !sk_check_arm_rows(&X, d.n_ents, nullptr, sp ? 0 : (size_t)b, sp ? ns : (size_t)e, &D))) return NAVHIP_ERR_INVALID;
    D.len[SK_PER_TILE] = F ? (size_t)T.flock_tiles_off[F] : 0;
    D.on[SK_SKIP] = T.skip != nullptr; D.on[SK_INTERP] = G.interp_from_xz != nullptr; D.on[SK_AUX] = aux; D.on[SK_SPARSE] = sp;
    D.pad = 8;
    if(sp) { D.len[SK_PER_ARM_ROW] = ns; D.len[SK_PER_LISTED] = ns; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // ---- inputs: one device slab; pageable arrays are packed into the pinned slab and cross the bus as ONE transfer,
    // pinned ones (navhip_host_alloc) are transferred in place.  Results: rows [b, e) of each, likewise
    nh_plan I, R;
    navhip_gate_in dg = {}; navhip_state_in ds = {}; navhip_state_aux_in da = {}, dense = {}; navhip_state_pass_out r = {};
    if(D.on[SK_RANGE]) da.n_range_rows = X.n_range_rows;
    nh_plan_rows(I, sk_gate_rows, &G, &dg, D, {offsetof(navhip_gate_in, new_vel_xz), offsetof(navhip_gate_in, vdes_xz)});
    nh_plan_rows(I, sk_state_rows, &T, &ds, D, {offsetof(navhip_state_in, new_pos_xz), offsetof(navhip_state_in, vdes_xz)});
    if(aux) nh_plan_rows(I, sk_aux_rows, &X, &da, D, {offsetof(navhip_state_aux_in, new_pos_xz), offsetof(navhip_state_aux_in, vdes_xz),
                                                  offsetof(navhip_state_aux_in, out_surround_dest_xz)});
    // (sparse: the dense twins the arm kernels read, filled on the device)
    if(sp) for(const nh_row &t : sk_aux_rows) if(t.len == SK_PER_ARM_ROW && D.on[t.group]) I.scratch(n * t.elem, &nh_member(&dense, t.off));
    nh_plan_rows(R, sk_pass_out_rows, out, &r, D);
    float *d_vdes, *d_sdest = nullptr, *d_listed = nullptr;     // (sparse: the surround positions of the listed units)
    R.scratch(n * 8, (void**)&d_vdes);
    if(su) { const int k = R.scratch(n * 8, (void**)&d_sdest); if(!sp) R.out(k, X.out_surround_dest_xz, 8, D.lo, D.cnt); }
    if(su && sp) R.out(R.scratch(ns * 8, (void**)&d_listed), X.out_surround_dest_xz, 8, 0, ns);
    I.pack(); R.pack();
    int rc = nh_async_slabs(ctx, I.in_bytes, R.out_bytes, &I.h_in, &R.h_out);
    if(!rc) rc = I.reserve(ctx, NH_STAGE_PASS_IN);
    if(!rc) rc = R.reserve(ctx, NH_STAGE_PASS_OUT);
    if(!rc) rc = I.upload(ctx, s);
    if(rc) return rc;
    // ---- sparse rows -> the dense arrays of the arms (targets default to "the host's", rotations and queries to zero)
    const int32_t *units = da.sparse_units;
    da.sparse_units = nullptr;
    if(sp) {
        sk_sparse_rows SR;
        memset(&SR, 0, sizeof(SR));
        SR.n = (int)ns; SR.units = units;
        // (the rows become the kernel's source, their dense twin takes their place in front of the arm kernels)
#define SK_DENSE(member, rows_, dense_) (SR.rows_ = da.member, SR.dense_ = (decltype(SR.dense_))dense.member, da.member = dense.member)
        if(D.on[SK_TURN]) {
            SK_DENSE(ent_rot, er, d_er); SK_DENSE(target_dir, td, d_td);
            HIPCHK(ctx, hipMemsetAsync(SR.d_er, 0, n * 16, s)); HIPCHK(ctx, hipMemsetAsync(SR.d_td, 0, n * 16, s));
        }
        if(D.on[SK_RANGE]) {
            SK_DENSE(range_target, rt, d_rt); SK_DENSE(target_range, rr, d_rr); SK_DENSE(target_prev_xz, rp, d_rp);
            SK_DENSE(range_tiles_row, row, d_row);
            HIPCHK(ctx, hipMemsetAsync(SR.d_rt, 0xfe, n * 4, s)); HIPCHK(ctx, hipMemsetAsync(SR.d_row, 0, n * 4, s));
        }
        if(su) {
            SK_DENSE(surround_target, stgt, d_stgt); SK_DENSE(surround_query, sq, d_sq); SK_DENSE(surround_target_prev_xz, stp, d_stp);
            SK_DENSE(surround_nearest_prev_xz, snp, d_snp); SK_DENSE(surround_dest_xz, sd, d_sd);
            HIPCHK(ctx, hipMemsetAsync(SR.d_stgt, 0xfe, n * 4, s)); HIPCHK(ctx, hipMemsetAsync(SR.d_sq, 0, n, s));
            HIPCHK(ctx, hipMemsetAsync(d_sdest, 0, n * 8, s));
        }
#undef SK_DENSE
        if(ns) {
            hipLaunchKernelGGL(k_sparse_rows, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s, SR);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    // ---- the three passes on the resident snapshot
    if(e > b) hipLaunchKernelGGL(k_pick_vdes, dim3((e - b + 255) / 256), dim3(256), 0, s, b, e, d.vdes_xz, (const float*)so.vdes_xz, d_vdes);
    dg.new_vel_xz = so.vel_xz; dg.vdes_xz = d_vdes;
    da.out_surround_dest_xz = d_sdest;
    rc = sk_run_passes(ctx, &d, b, e, dg, ds, aux ? &da : nullptr, r, su && sp ? units : nullptr, ns, d_listed, s);
    if(!rc) rc = R.download(ctx, s);
    return rc;
}

static int sk_settled_count(navhip_ctx *ctx, const navhip_world *w, int nq, const int32_t *uids, int32_t *out_counts, bool use_resident)
{
    if(!ctx || !w || nq < 0 || w->n_ents < 0 || (nq > 0 && (!uids || !out_counts))) return NAVHIP_ERR_INVALID;
    if(nq == 0) return NAVHIP_OK;
    if(!use_resident && (!w->pos_xz || !w->radius || !w->flags || !w->state)) return NAVHIP_ERR_INVALID;
    for(int q = 0; q < nq; q++)
        if(uids[q] < 0 || uids[q] >= w->n_ents) return NAVHIP_ERR_INVALID;
    // the spatial index over the snapshot, the circle queries and the count, all on the device: the ids of the queries
    // (the reference's visiting order, capped) never leave HBM -- only the uids go up and the counts come back
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    navhip_world d; navhip_step_out so;
    const bool resident = use_resident && nh_async_resident(ctx, &d, &so) && d.n_ents == w->n_ents && d.pos_xz && d.radius && d.flags && d.state;
    if(use_resident && !resident) {
        ctx->last_error = "navhip_settled_count_resident: no completed host-buffer step of this size is resident on the device";
        return NAVHIP_ERR_INVALID;
    }
    nh_plan P;
    if(!resident) {
        // (a snapshot the velocity pass left on the device is read in place: the tick's tables are the same)
        d = *w;
        nh_plan_world(P, w, &d, sk_dims_of(w, 0, 0), {NH_W(pos_xz), NH_W(radius), NH_W(flags), NH_W(state)});
    }
    d.grid_xmin = w->grid_xmin; d.grid_xmax = w->grid_xmax; d.grid_zmin = w->grid_zmin; d.grid_zmax = w->grid_zmax;
    int32_t *d_uid, *d_cnt, *d_out; float *d_q; uint32_t *d_ids;
    P.in(uids, (size_t)nq * 4, 0, (void**)&d_uid);
    P.scratch((size_t)nq * 8, (void**)&d_q); P.scratch((size_t)nq * 4, (void**)&d_cnt); P.scratch((size_t)nq * SK_QUERY_MAX * 4, (void**)&d_ids);
    P.out(P.scratch((size_t)nq * 4, (void**)&d_out), out_counts, 4, 0, (size_t)nq);
    int rc = P.reserve(ctx, NH_STAGE_STATE_ARENA);
    if(!rc) rc = P.upload(ctx, s);
    if(rc) return rc;
    hipLaunchKernelGGL(k_gather_query, dim3((nq + 255) / 256), dim3(256), 0, s, nq, (const int32_t*)d_uid, d.pos_xz, d_q);
    rc = nh_spatial_query_dev(ctx, &d, d_q, nq, SK_QUERY_R, SK_QUERY_MAX, d_cnt, d_ids, s);
    if(rc) return rc;
    hipLaunchKernelGGL(k_settled_count, dim3((nq + 15) / 16), dim3(256), 0, s, nq, (const int32_t*)d_uid,
                       d.pos_xz, d.radius, d.flags, d.state, (const int32_t*)d_cnt, (const uint32_t*)d_ids, d_out);
    HIPCHK(ctx, hipGetLastError());
    return P.download(ctx, s);
}

int navhip_settled_count(navhip_ctx *ctx, const navhip_world *w, int nq, const int32_t *uids, int32_t *out_counts)
{
    return sk_settled_count(ctx, w, nq, uids, out_counts, false);
}

int navhip_settled_count_resident(navhip_ctx *ctx, const navhip_world *w, int nq, const int32_t *uids, int32_t *out_counts)
{
    return sk_settled_count(ctx, w, nq, uids, out_counts, true);
}

int navhip_arrival_settle_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_settle_in *in,
                              const navhip_settle_out *out, void *stream)
{
    if(!ctx || !w || !in || !out || in->nq < 0 || in->n_zones < 0 || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    if(in->nq == 0) return NAVHIP_OK;
    if(!w->vel_xz || !w->radius || !in->nsettled || !sk_check_settle(in, out)) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    nh_step_params P;
    nh_step_params_init(ctx, w, &P);
    hipLaunchKernelGGL(k_arrival_settle, dim3((in->nq + 15) / 16), dim3(256), 0, stream ? (hipStream_t)stream : ctx->stream,
                       P, w->vel_xz, w->radius, *in, *out);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

static int sk_arrival_settle(navhip_ctx *ctx, const navhip_world *w, const navhip_settle_in *in, const navhip_settle_out *out, bool use_resident)
{
    if(!ctx || !w || !in || !out || in->nq < 0 || in->n_zones < 0 || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    if(in->nq == 0) return NAVHIP_OK;
    const bool count_here = in->nsettled == nullptr;          // (adjacent_settled_count on the resident snapshot too)
    if(count_here && !use_resident) return NAVHIP_ERR_INVALID;
    navhip_world rw; navhip_step_out rso;
    const bool resident = use_resident && nh_async_resident(ctx, &rw, &rso) && rw.n_ents == w->n_ents && rw.vel_xz && rw.radius
                       && (!count_here || (rw.pos_xz && rw.flags && rw.state));
    if(use_resident && !resident) {
        ctx->last_error = "navhip_arrival_settle_resident: no completed host-buffer step of this size is resident on the device";
        return NAVHIP_ERR_INVALID;
    }
    if((!resident && (!w->vel_xz || !w->radius)) || !sk_check_settle(in, out)) return NAVHIP_ERR_INVALID;
    const size_t nq = (size_t)in->nq, nz = (size_t)in->n_zones;
    size_t n_slots = 0, n_keys = 0;
    for(size_t z = 0; z < nz; z++) {
        const navhip_arrival_zone &Z = in->zones[z];
        if(Z.slot_begin < 0 || Z.slot_end < Z.slot_begin || Z.key_begin < 0 || Z.key_end < Z.key_begin
        || Z.layer < 0 || Z.layer >= NAVHIP_NAV_LAYER_MAX) return NAVHIP_ERR_INVALID;
        if((size_t)Z.slot_end > n_slots) n_slots = (size_t)Z.slot_end;
        if((size_t)Z.key_end > n_keys) n_keys = (size_t)Z.key_end;
    }
    if((n_slots > 0 && (!in->slots_xz || !in->slot_ring)) || (n_keys > 0 && !in->region_keys)) return NAVHIP_ERR_INVALID;
    for(size_t q = 0; q < nq; q++)
        if(in->uid[q] < 0 || in->uid[q] >= w->n_ents || in->zone[q] < 0 || in->zone[q] >= in->n_zones) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    nh_dims D = sk_dims_of(w, 0, 0);
    D.len[NH_LEN_ZONE] = nz; D.len[NH_LEN_SLOT] = n_slots; D.len[NH_LEN_KEY] = n_keys; D.len[NH_LEN_QUERY] = nq;
    nh_plan P;
    navhip_world d = *w;
    // (the snapshot the velocity half left on the device is read in place: movestate.velocity and the radii are the tick's)
    if(resident) { d.vel_xz = rw.vel_xz; d.radius = rw.radius; }
    else nh_plan_world(P, w, &d, D, {NH_W(vel_xz), NH_W(radius)});
    // (the inputs of the arm side by side, the results at the end: a context with an asynchronous step path owns
    // page-locked slabs, and each region then crosses the bus once)
    navhip_settle_in di = *in;
    navhip_settle_out dout = {};
    const int first_in = (int)P.rows.size();
    nh_plan_rows(P, sk_settle_in_rows, in, &di, D, {offsetof(navhip_settle_in, nsettled)});
    if(!count_here) P.in(in->nsettled, nq * 4, 0, (void**)&di.nsettled);
    float *d_q; int32_t *d_cnt; uint32_t *d_ids;
    const int end_in = P.scratch(count_here ? nq * 8 : 0, (void**)&d_q);
    P.scratch(count_here ? nq * 4 : 0, (void**)&d_cnt); P.scratch(count_here ? nq * SK_QUERY_MAX * 4 : 0, (void**)&d_ids);
    const int first_out = (int)P.rows.size();
    nh_plan_rows(P, sk_settle_out_rows, out, &dout, D, {offsetof(navhip_settle_out, nsettled)});
    if(count_here) P.out(P.scratch(nq * 4, (void**)&di.nsettled), out->nsettled, 4, 0, nq);
    P.region(ctx, first_in, end_in, first_out);
    int rc = P.reserve(ctx, NH_STAGE_STATE_ARENA);
    if(!rc) rc = P.upload(ctx, s);
    if(rc) return rc;
    if(count_here) {
        navhip_world dq = rw;
        dq.grid_xmin = w->grid_xmin; dq.grid_xmax = w->grid_xmax; dq.grid_zmin = w->grid_zmin; dq.grid_zmax = w->grid_zmax;
        hipLaunchKernelGGL(k_gather_query, dim3((in->nq + 255) / 256), dim3(256), 0, s, in->nq, di.uid, rw.pos_xz, d_q);
        rc = nh_spatial_query_dev(ctx, &dq, d_q, in->nq, SK_QUERY_R, SK_QUERY_MAX, d_cnt, d_ids, s);
        if(rc) return rc;
        hipLaunchKernelGGL(k_settled_count, dim3((in->nq + 15) / 16), dim3(256), 0, s, in->nq, di.uid,
                           rw.pos_xz, rw.radius, rw.flags, rw.state, (const int32_t*)d_cnt, (const uint32_t*)d_ids, (int32_t*)di.nsettled);
        HIPCHK(ctx, hipGetLastError());
    }
    rc = navhip_arrival_settle_dev(ctx, &d, &di, &dout, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

int navhip_arrival_settle(navhip_ctx *ctx, const navhip_world *w, const navhip_settle_in *in, const navhip_settle_out *out)
{
    return sk_arrival_settle(ctx, w, in, out, false);
}

int navhip_arrival_settle_resident(navhip_ctx *ctx, const navhip_world *w, const navhip_settle_in *in, const navhip_settle_out *out)
{
    return sk_arrival_settle(ctx, w, in, out, true);
}

int navhip_arrival_velocity_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_vel_in *in,
                                const navhip_arrival_vel_out *out, void *stream)
{
    av_tables T = {};
    const int rc = av_check(ctx, w, in, out, false, &T);
    if(rc || in->nq == 0) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    nh_step_params P;
    nh_step_params_init(ctx, w, &P);
    P.pos_xz = w->pos_xz;
    P.flock_field_slot = T.com_slot; P.region_field_slot = T.zone_slot; P.field_pool = T.pool;
    hipLaunchKernelGGL(k_arrival_velocity, dim3((in->nq + 15) / 16), dim3(256), 0, stream ? (hipStream_t)stream : ctx->stream,
                       P, T.n_com_rows, T.n_zone_rows, *in, *out);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_arrival_velocity(navhip_ctx *ctx, const navhip_world *w, const navhip_arrival_vel_in *in, const navhip_arrival_vel_out *out)
{
    av_tables T = {};
    int rc = av_check(ctx, w, in, out, true, &T);
    if(rc || in->nq == 0) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t nchunks = (size_t)ctx->nchunks;
    nh_dims D = sk_dims_of(w, 0, 0);
    D.len[NH_LEN_ZONE] = (size_t)in->n_zones; D.len[NH_LEN_SLOT] = (size_t)in->n_slots; D.len[NH_LEN_KEY] = (size_t)in->n_keys;
    D.len[NH_LEN_QUERY] = (size_t)in->nq;
    D.pad = 16;                                                             // (no array of a zone-less or slot-less call is empty)
    nh_plan P;
    navhip_world d = nh_device_world(w);
    nh_plan_world(P, w, &d, D, {NH_W(pos_xz)});
    if(!T.resident) {
        // the world's own tables, as the step stages them (rows of -1 .. : see navhip_world)
        if(T.n_com_rows) P.in(w->flock_field_slot, (size_t)T.n_com_rows * nchunks * 4, D.pad, (void**)&d.flock_field_slot);
        if(T.n_zone_rows) P.in(w->region_field_slot, (size_t)T.n_zone_rows * nchunks * 4, D.pad, (void**)&d.region_field_slot);
        if(T.n_com_rows || T.n_zone_rows) P.in(w->field_pool, (size_t)w->n_field_slots * NH_CELLS, D.pad, (void**)&d.field_pool);
    }
    navhip_arrival_vel_in di = *in;
    navhip_arrival_vel_out dout = {};
    nh_plan_rows(P, av_in_rows, in, &di, D);
    nh_plan_rows(P, av_out_rows, out, &dout, D);
    rc = P.reserve(ctx, NH_STAGE_STATE_ARENA);
    if(!rc) rc = P.upload(ctx, s);
    if(rc) return rc;
    rc = navhip_arrival_velocity_dev(ctx, &d, &di, &dout, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

}   // extern "C"
