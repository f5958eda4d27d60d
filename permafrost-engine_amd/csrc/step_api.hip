// step_api.hip -- the host side of the agent step (no kernel lives here): its scratch, the schedule of a tick's launches
// over the caller's stream and the two side streams, the prefetch that starts the snapshot-only
// part early, and the host-buffer entry points that stage a world and run a step on it -- or a spatial query, a region
// lookup, a batch of ClearPath problems: the test utilities over the agent kernels.
#include "navhip_internal.h"
#include "agent_internal.h"
#include "agent_thread.h"
#include <cmath>

#include <algorithm>
#include <cstring>
#include <initializer_list>

// ---------------------------------------------------------------------------------------------
// the step's scratch (ctx->step.buf, enum nh_step_buf)
// ---------------------------------------------------------------------------------------------
// What a buffer holds after a FRESH allocation, before any kernel has written it.  The kernels keep it so afterwards.
enum sb_fresh : uint8_t {
    SB_ANYTHING,        // written before it is read
    SB_ZEROED,          // counters the kernels return to zero themselves
    SB_EMPTY_BOXES,     // the two slab boxes start empty (INT_MIN); afterwards every build re-initialises its successor's
};
struct sb_need { nh_step_buf buf; size_t bytes; sb_fresh fresh; };

// the buffers of one group, grown in the order they are listed; what a fresh one must hold is enqueued on s
template<size_t N> static int step_bufs_ensure(navhip_ctx *ctx, const sb_need (&needs)[N], hipStream_t s)
{
    for(const sb_need &n : needs) {
        nh_buf &b = ctx->step.buf[n.buf];
        const void *old = b.p;
        int rc = nh_ensure_buf(ctx, b, n.bytes);
        if(rc) return rc;
        if(b.p == old) continue;
        if(n.fresh == SB_ZEROED) HIPCHK(ctx, hipMemsetAsync(b.p, 0, b.cap, s));
        if(n.fresh == SB_EMPTY_BOXES) HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)b.p, (int)0x80000000, 8, s));
    }
    return NAVHIP_OK;
}
template<class T> static T *step_buf(const navhip_ctx *ctx, nh_step_buf b) { return (T*)ctx->step.buf[b].p; }

// the spatial hash over n entities and ncells cells
static int hash_ensure(navhip_ctx *ctx, size_t n, size_t ncells, hipStream_t s)
{
    const sb_need needs[] = {
        {NH_SB_ENT_CELL, 4 * n, SB_ANYTHING},               {NH_SB_ENT_RANK, 4 * n, SB_ANYTHING},
        {NH_SB_CELL_COUNT, 4 * ncells, SB_ZEROED},          {NH_SB_CELL_START, 4 * (ncells + 1), SB_ANYTHING},
        {NH_SB_TMP_ID, 4 * n, SB_ANYTHING},                 {NH_SB_BLOCK_SUM, 4 * ((ncells + NH_SCAN_T - 1) / NH_SCAN_T), SB_ANYTHING},
        {NH_SB_SLAB_BOX, 48, SB_EMPTY_BOXES},               // (two boxes of four + the length of the slab's list of walks)
        {NH_SB_REC_A, 16 * n, SB_ANYTHING},                 {NH_SB_REC_V, 8 * n, SB_ANYTHING},
        {NH_SB_POOL_OF, 4 * n, SB_ANYTHING},
    };
    return step_bufs_ensure(ctx, needs, s);
}

static nh_spatial_scratch hash_scratch(const navhip_ctx *ctx)
{
    return {step_buf<int32_t>(ctx, NH_SB_ENT_CELL), step_buf<int32_t>(ctx, NH_SB_ENT_RANK), step_buf<int32_t>(ctx, NH_SB_CELL_COUNT),
            step_buf<int32_t>(ctx, NH_SB_CELL_START), step_buf<int32_t>(ctx, NH_SB_TMP_ID), step_buf<int32_t>(ctx, NH_SB_BLOCK_SUM),
            step_buf<int32_t>(ctx, NH_SB_SLAB_BOX), 0, step_buf<float4>(ctx, NH_SB_REC_A), step_buf<float2>(ctx, NH_SB_REC_V),
            step_buf<int32_t>(ctx, NH_SB_POOL_OF), {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}};
}

// the neighbour walk and the work lists of a step over n_ents entities
static int walk_ensure(navhip_ctx *ctx, int n_ents, nh_nbr *NB, nh_worklists *WL, hipStream_t s)
{
    const size_t n = (size_t)n_ents;
    const int cap = nh_worklist_cap(n_ents);
    const sb_need needs[] = {
        {NH_SB_SEP, 8 * n, SB_ANYTHING},                    {NH_SB_CNT, 4 * n, SB_ZEROED},
        {NH_SB_REC, 4 * (size_t)(64 * 5) * n, SB_ANYTHING}, {NH_SB_MIDREC, sizeof(nh_mid_rec) * n, SB_ANYTHING},
        {NH_SB_WL_COUNT, 4 * 2 * NH_WL_COUNTERS, SB_ZEROED},
        {NH_SB_WL_IDS, 4 * (size_t)NH_WL_LISTS * NH_WL_SUB * cap, SB_ANYTHING},
    };
    int rc = step_bufs_ensure(ctx, needs, s);
    if(rc) return rc;
    NB->sep = step_buf<float2>(ctx, NH_SB_SEP); NB->cnt = step_buf<uint32_t>(ctx, NH_SB_CNT); NB->rec = step_buf<float>(ctx, NH_SB_REC);
    NB->stride = 64 * 5;
    WL->count = step_buf<int32_t>(ctx, NH_SB_WL_COUNT); WL->ids = step_buf<int32_t>(ctx, NH_SB_WL_IDS); WL->cap = cap;
    return NAVHIP_OK;
}

// the cohesion term: its force per entity; its plan, where a new buffer or another flock count has no lane grouping yet
static int coh_ensure(navhip_ctx *ctx, int n_ents, int n_flocks, int n_members, hipStream_t s)
{
    nh_step_state &st = ctx->step;
    const sb_need needs[] = {{NH_SB_COH, (size_t)n_ents * 2 * sizeof(float), SB_ANYTHING},
                             {NH_SB_COH_PLAN, nh_cohesion_scratch_bytes(n_flocks, n_members), SB_ANYTHING}};
    const void *old = st.buf[NH_SB_COH_PLAN].p;
    int rc = step_bufs_ensure(ctx, needs, s);
    if(rc) return rc;
    if(st.buf[NH_SB_COH_PLAN].p != old || st.coh_flocks != n_flocks || st.coh_members != n_members) {
        // (scratch may still be in use by a regrouping on a side stream: order behind it)
        if(st.aux[1] && s != st.aux[1]) {
            HIPCHK(ctx, hipEventRecord(st.ev_regroup, st.aux[1]));
            HIPCHK(ctx, hipStreamWaitEvent(s, st.ev_regroup, 0));
        }
        HIPCHK(ctx, nh_cohesion_scratch_reset(step_buf<int32_t>(ctx, NH_SB_COH_PLAN), n_flocks, n_members, s));
        st.coh_flocks = n_flocks; st.coh_members = n_members; st.coh_parity = 0;
        st.scratch_moves++;
    }
    return NAVHIP_OK;
}

// bg_<name>_init geometry, bitmap_grid.h:959-990
static bool grid_geometry(const navhip_world *w, nh_grid *g)
{
    int32_t ox = (int32_t)lrintf(w->grid_xmin * 256.0f), oy = (int32_t)lrintf(w->grid_zmin * 256.0f);
    int32_t span_x = (int32_t)lrintf(w->grid_xmax * 256.0f) - ox;
    int32_t span_y = (int32_t)lrintf(w->grid_zmax * 256.0f) - oy;
    if(span_x <= 0 || span_y <= 0) return false;
    g->origin_x = ox; g->origin_y = oy;
    g->grid_w = (int)(((uint32_t)span_x + 4095u) >> 12);
    g->grid_h = (int)(((uint32_t)span_y + 4095u) >> 12);
    if(g->grid_w < 1) g->grid_w = 1;
    if(g->grid_h < 1) g->grid_h = 1;
    return true;
}

static int spatial_build(navhip_ctx *ctx, const navhip_world *w, nh_grid *g, hipStream_t s,
                         int slab_begin = 0, int slab_end = -1, bool with_records = true)
{
    if(!grid_geometry(w, g)) {
        ctx->last_error = "agent step: empty spatial-grid bounds";
        return NAVHIP_ERR_INVALID;
    }
    int rc = hash_ensure(ctx, (size_t)w->n_ents, (size_t)g->grid_w * g->grid_h, s);
    if(rc) return rc;
    nh_spatial_scratch S = hash_scratch(ctx);
    // (a query index holds positions only)
    if(with_records) S.src = nh_pack_src{w->vel_xz, w->radius, w->flags, w->state, w->arrival_sink_xz, w->arrival_flags};
    g->n = w->n_ents;
    if(slab_end < 0) slab_end = w->n_ents;
    // (the two slab boxes alternate between the builds that USE one: such a build cleans the other)
    if(slab_begin > 0 || slab_end < w->n_ents) S.box_parity = (int)(ctx->step.sp_builds++ & 1u);
    nh_launch_spatial_build(*g, w->pos_xz, S, slab_begin, slab_end, s);
    return NAVHIP_OK;
}

static int step_check_world(navhip_ctx *ctx, const navhip_world *w)
{
    if(!w || w->n_ents < 0 || (w->hz != 20 && w->hz != 10 && w->hz != 5 && w->hz != 1))
        return NAVHIP_ERR_INVALID;
    if(w->n_ents == 0) return NAVHIP_OK;
    if(w->n_ents >= (1 << 24)) {            // pool records carry the uid in 24 bits
        ctx->last_error = "agent step: more than 2^24 entities";
        return NAVHIP_ERR_INVALID;
    }
    if((w->arrival_flags != nullptr) != (w->arrival_sink_xz != nullptr)) return NAVHIP_ERR_INVALID;
    if(!w->pos_xz || !w->vel_xz || !w->radius || !w->max_speed || !w->speed || !w->flags
    || !w->state || !w->has_dest_los || !w->flock
    || (w->n_flocks > 0 && (!w->flock_target_xz || !w->flock_offsets || !w->flock_members)))
        return NAVHIP_ERR_INVALID;
    if(!ctx->layers[0].cost && !ctx->layers[4].cost && !ctx->layers[8].cost) {
        ctx->last_error = "agent step: no cost_base plane uploaded";
        return NAVHIP_ERR_NOT_UPLOADED;
    }
    return NAVHIP_OK;
}

static int step_fill_params(navhip_ctx *ctx, const navhip_world *w, nh_step_params *Pp)
{
    nh_step_params &P = *Pp;
    memset(&P, 0, sizeof(P));
    int rc_masks = nh_refresh_derived(ctx, ctx->stream);      // the tile probes read the derived row masks
    if(rc_masks) return rc_masks;
    nh_fill_map_view(ctx, &P.map);
    P.map_x = w->map_pos_x; P.map_z = w->map_pos_z;
    P.n_ents = w->n_ents; P.n_flocks = w->n_flocks; P.hz = w->hz;
    P.n_members = w->n_ents;          // every entity belongs to at most one flock
    P.work_begin = w->work_begin; P.work_end = w->work_end;
    if(P.work_begin == 0 && P.work_end == 0) P.work_end = w->n_ents;
    if(P.work_begin < 0 || P.work_end > w->n_ents || P.work_begin > P.work_end)
        return NAVHIP_ERR_INVALID;
    // (the cohesion term's lane grouping, carried from tick to tick: see k_coh_bin)
    if(P.work_begin == 0 && P.work_end == w->n_ents) P.members_key = 0;
    else if(w->static_epoch)                          P.members_key = (int)((w->static_epoch & 0x3fffffffu) | 0x40000000u);
    else                                              P.members_key = (int)(0x80000000u | ++ctx->step.coh_unique);
    P.pos_xz = w->pos_xz; P.vel_xz = w->vel_xz; P.radius = w->radius; P.max_speed = w->max_speed;
    P.speed = w->speed; P.flags = w->flags; P.state = w->state; P.has_dest_los = w->has_dest_los;
    P.flock = w->flock; P.vdes_xz = w->vdes_xz; P.flock_target_xz = w->flock_target_xz;
    P.flock_offsets = w->flock_offsets; P.flock_members = w->flock_members;
    P.flock_field_slot = w->flock_field_slot; P.field_pool = w->field_pool;
    if(w->n_field_slots == NAVHIP_POOL_RESIDENT) {
        // sample the context's resident pool: row = flock index of the (dest, chunk) -> slot table
        if(!ctx->pool || w->n_flocks > nh_pool_dests(ctx)) {
            ctx->last_error = "agent step: NAVHIP_POOL_RESIDENT without a pool that has a row per flock";
            return NAVHIP_ERR_INVALID;
        }
        P.flock_field_slot = nh_pool_map(ctx); P.field_pool = nh_pool_fields(ctx);
    }
    P.form_ready = w->form_ready; P.cell_pos_xz = w->cell_pos_xz;
    P.form_cohesion_xz = w->form_cohesion_xz; P.form_align_xz = w->form_align_xz;
    P.form_drag_xz = w->form_drag_xz;
    P.arrival_sink_xz = w->arrival_sink_xz; P.arrival_flags = w->arrival_flags;
    P.los_pool = w->los_pool; P.flock_los_slot = w->flock_los_slot; P.los_pos_xz = w->los_pos_xz;
    if((P.los_pool != nullptr) != (P.flock_los_slot != nullptr)) return NAVHIP_ERR_INVALID;
    P.region_row = w->region_row; P.region_field_slot = w->region_field_slot;
    if(P.region_row && w->n_field_slots == NAVHIP_POOL_RESIDENT) {
        // rows of the resident pool's mapping table (the caller keeps its region rows behind the flock rows)
        if(w->n_region_rows > nh_pool_dests(ctx)) {
            ctx->last_error = "agent step: more region rows than the resident pool's mapping table has";
            return NAVHIP_ERR_INVALID;
        }
        P.region_field_slot = nh_pool_map(ctx);
    }else if(P.region_row && !P.region_field_slot) {
        ctx->last_error = "agent step: region_row given without region_field_slot";
        return NAVHIP_ERR_INVALID;
    }
    if(P.form_ready && (!P.cell_pos_xz || !P.form_cohesion_xz || !P.form_align_xz || !P.form_drag_xz)) {
        ctx->last_error = "agent step: form_ready given without the other formation arrays";
        return NAVHIP_ERR_INVALID;
    }
    return NAVHIP_OK;
}

// what a prefetch is started for (nh_prefetch_key): the step that follows joins it only for the very same snapshot
static nh_prefetch_key prefetch_key(const navhip_world *w, const nh_step_params &P)
{
    nh_prefetch_key k;
    memset(&k, 0, sizeof(k));           // (compared as bytes: padding included)
    k.pos_xz = w->pos_xz; k.vel_xz = w->vel_xz; k.radius = w->radius; k.flags = w->flags;
    k.state = w->state; k.flock_members = w->flock_members; k.flock_offsets = w->flock_offsets;
    k.arrival_flags = w->arrival_flags; k.arrival_sink_xz = w->arrival_sink_xz;
    k.n_ents = w->n_ents; k.n_flocks = w->n_flocks; k.hz = w->hz;
    k.work_begin = P.work_begin; k.work_end = P.work_end;
    k.origin_x = P.grid.origin_x; k.origin_y = P.grid.origin_y;
    k.grid_w = P.grid.grid_w; k.grid_h = P.grid.grid_h;
    return k;
}

static bool prefetch_key_matches(const navhip_ctx *ctx, const navhip_world *w, const nh_step_params &P)
{
    const nh_prefetch_key k = prefetch_key(w, P);
    return memcmp(&k, &ctx->step.pre.key, sizeof(k)) == 0;
}

// the side streams of the agent step (snapshot-only work beside the field builds; the ClearPath launches beside each
// other) and the words in device memory they hand over through (nh_handover).  The streams are the process's (nh_streams_for): borrowed, and chosen for the stream the
// step's main chain runs on -- the ones whose hardware queues sit on other pipes than that stream's.
int nh_ensure_side_streams(navhip_ctx *ctx, hipStream_t main)
{
    if(ctx->step.aux[0] && ctx->step.aux_main == main) return NAVHIP_OK;
    hipStream_t st[NH_STREAM_FIXED];
    int rc = nh_streams_for(ctx, main, st);
    if(rc) return rc;
    if(!ctx->step.ev_regroup) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->step.ev_regroup, hipEventDisableTiming));
    if(ctx->step.aux[0] && (ctx->step.aux[0] != st[NH_STREAM_SIDE0] || ctx->step.aux[1] != st[NH_STREAM_SIDE1])) {
        // another caller stream than last time: whatever the old side streams still hold is waited for
        for(auto a : ctx->step.aux) HIPCHK(ctx, hipStreamSynchronize(a));
        ctx->step.pre.valid = false; ctx->step.regroup_pending = false;
    }
    ctx->step.aux[0] = st[NH_STREAM_SIDE0]; ctx->step.aux[1] = st[NH_STREAM_SIDE1]; ctx->step.aux_main = main;
    return nh_handover_ensure(ctx);
}

// The lane regrouping of the cohesion term (five small launches behind k_cohesion) is for the NEXT tick's launch
// and only has to be spatially coherent: agents move about one world unit per tick and a group's box is compared
// against a 904-unit reach, so a grouping serves many ticks.  It is rebuilt on the two ticks after anything it was
// built for changes (entity / flock / member counts, work range, membership key) and every NH_COH_REGROUP_EVERY-th
// tick otherwise; k_cohesion checks on the device that the grouping it is given fits (else: the identity).
#define NH_COH_REGROUP_EVERY 8
// a jam: the list lengths of the last step, in pinned memory without a wait -- 8 192 workgroup searches and more
static bool step_in_a_jam(navhip_ctx *ctx)
{
    int32_t lists[6];
    return navhip_step_lists_peek(ctx, lists) == NAVHIP_OK && lists[4] >= 8192;
}

static bool coh_regroup_due(navhip_ctx *ctx, const nh_step_params &P)
{
    const int64_t key[4] = {((int64_t)P.n_ents << 32) | (uint32_t)P.n_flocks, (int64_t)P.n_members,
                            ((int64_t)P.work_begin << 32) | (uint32_t)P.work_end, (int64_t)P.members_key};
    if(memcmp(key, ctx->step.coh_regroup_key, sizeof(key)) != 0) {
        memcpy(ctx->step.coh_regroup_key, key, sizeof(key));
        ctx->step.coh_regroup_age = 0;
    }
    const int age = ctx->step.coh_regroup_age++;
    // In a jam -- the list lengths of the last step, in pinned memory without a wait: 8 192 workgroup searches and more --
    // the regrouping stays on every tick: the crowded world measured 3-4 % SLOWER without its five small launches on the
    // side stream although every kernel takes the same time under the tracer (profiles/archive/r04_ab_regroup_cadence.txt; launch
    // timing against the persistent searches, profiles/HISTORY.md 3.7).  Kept as measured.
    const bool jam = step_in_a_jam(ctx);
    // (a slab step whose caller gave no static_epoch carries a never-repeating key: k_cohesion could not accept a
    // grouping made for it -- the five launches would be wasted)
    if(P.members_key < 0) return false;
    return jam || age < 2 || age % NH_COH_REGROUP_EVERY == 0;
}

// ---------------------------------------------------------------------------------------------
// staging of a world (array by array through nh_stage_in, navhip_api.hip)
// ---------------------------------------------------------------------------------------------
// the world's arrays, staged row by row of nh_world_rows; `only`: just these members (their offsets)
int nh_stage_world(navhip_ctx *ctx, const navhip_world *w, navhip_world *d, hipStream_t s, std::initializer_list<size_t> only)
{
    *d = *w;
    const size_t F = (size_t)w->n_flocks;
    const size_t nmembers = (F > 0 && w->flock_offsets) ? (size_t)w->flock_offsets[F] : 0;
    const bool resident = w->n_field_slots == NAVHIP_POOL_RESIDENT;
    for(const nh_world_row &r : nh_world_rows) {
        if(resident && (r.flags & NH_ROW_NOT_RESIDENT)) continue;
        if(only.size() && std::find(only.begin(), only.end(), r.off) == only.end()) continue;
        int rc = nh_stage_in(ctx, r.slot, nh_member(w, r.off), nh_world_row_bytes(r, w, (size_t)ctx->nchunks, nmembers),
                          (const void**)&nh_member(d, r.off), s);
        if(rc) return rc;
    }
    return NAVHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// the schedule of a tick's launches
// ---------------------------------------------------------------------------------------------
// NH_HO_NBR stored behind the front of the last prefetch, if nobody has yet
static void signal_front_done(navhip_ctx *ctx)
{
    if(ctx->step.join0_signalled) return;
    nh_handover_signal(ctx, NH_HO_NBR, ctx->step.front_stream);
    ctx->step.join0_signalled = true;
}

extern "C" {

int navhip_agent_prefetch_dev_ex(navhip_ctx *ctx, const navhip_world *w, void *stream, uint32_t flags)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    int rc = step_check_world(ctx, w);
    if(rc) return rc;
    ctx->step.pre.valid = false;
    if(w->n_ents == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    // (a prefetch may be issued on another stream than the step it belongs to -- the exchange stream of a sharded tick --:
    // the side streams stay the ones chosen for the step's stream once there has been a step)
    rc = nh_ensure_side_streams(ctx, ctx->step.aux[0] ? ctx->step.aux_main : s);
    if(rc) return rc;
    nh_step_params P;
    rc = step_fill_params(ctx, w, &P);
    if(rc) return rc;
    nh_nbr NB; nh_worklists WL;
    const unsigned moves0 = ctx->step.scratch_moves;
    rc = coh_ensure(ctx, w->n_ents, w->n_flocks, P.n_members, s);
    if(!rc) rc = walk_ensure(ctx, w->n_ents, &NB, &WL, s);
    if(rc) return rc;
    // (a lane-grouping reset or a zeroed reallocation just went onto `s`: the side streams must start behind it, not
    // behind the end word of the last step -- else the reset could land in the middle of this call's cohesion term or
    // regrouping on aux[1].  Constant counts move nothing, and the hand-over-free start stays.)
    const bool scratch_moved = ctx->step.scratch_moves != moves0;
    // the front of the step (spatial hash -> neighbour walk) is a chain of small launches on the
    // critical path of the tick: NAVHIP_PREFETCH_FRONT_INLINE keeps it on the caller's stream, where it
    // follows the previous step without a cross-stream hand-over (tens of microseconds each)
    hipStream_t front = (flags & NAVHIP_PREFETCH_FRONT_INLINE) ? s : ctx->step.aux[0];
    // The side streams start behind a word in device memory (stream_set.hip: 2-3 us from the store to the waiting stream's
    // next kernel, against 12 us and a packet on the caller's stream for an event).  NAVHIP_PREFETCH_FOLLOWS_STEP: the
    // last step on this stream stored that word when it ended, and the snapshot was final then -- nothing goes in front
    // of the front at all.  Otherwise a one-lane launch stores it now, in FRONT of the first kernel of the front: the
    // cohesion kernel ends last, so it must not start late (profiles/archive/r03_ab_fork_first.txt).
    nh_handover_mode(ctx, step_in_a_jam(ctx));           // (words, or events: under a serialising profiler, in a jam)
    const bool follows = (flags & NAVHIP_PREFETCH_FOLLOWS_STEP) && ctx->step.step_end_on == s && !ctx->ho->by_events
                      && !scratch_moved;
    if(!follows) nh_handover_signal(ctx, NH_HO_START, s);
    ctx->step.start_flag = follows ? NH_HO_END : NH_HO_START;
    ctx->step.start_seq = nh_handover_seq(ctx, ctx->step.start_flag);
    if(front != s) nh_handover_wait(ctx, ctx->step.start_flag, ctx->step.aux[0]);
    nh_handover_wait(ctx, ctx->step.start_flag, ctx->step.aux[1]);
    // side stream 1: cohesion -- enqueued first: it ends last, and a host that is not ahead of the device (the tick after a
    // synchronisation) would otherwise hold it back by the front's six launches
    const bool regroup = nh_launch_cohesion(P, step_buf<int32_t>(ctx, NH_SB_COH_PLAN), step_buf<float>(ctx, NH_SB_COH), &ctx->step.coh_parity,
                                            ctx->step.aux[1]);
    nh_handover_signal(ctx, NH_HO_COH, ctx->step.aux[1]);
    // the front: spatial hash -> neighbour walk (separation force + ClearPath neighbour lists)
    rc = spatial_build(ctx, w, &P.grid, front, P.work_begin, P.work_end);
    if(rc) return rc;
    nh_launch_agent_nbr(P, NB, front);
    // (an inline front is ordered on the caller's stream by itself: that it is done is stored by the step's own wait
    // for the cohesion term, or by a launch of its own when somebody asks before -- navhip_stream_wait_stage)
    ctx->step.join0_signalled = false;
    ctx->step.front_stream = front;
    if(front != s) signal_front_done(ctx);
    ctx->step.snapshot_held = (flags & NAVHIP_PREFETCH_SNAPSHOT_HELD) != 0;
    // (behind the cohesion term's word: the agent step does not wait for next tick's lane grouping; but the
    // caller's stream does, at the end of navhip_agent_step_dev, so that whatever the caller does
    // to the snapshot arrays afterwards is ordered behind the last read of them)
    ctx->step.regroup_pending = false;
    if(regroup && coh_regroup_due(ctx, P)) {
        nh_launch_cohesion_regroup(P, step_buf<int32_t>(ctx, NH_SB_COH_PLAN), &ctx->step.coh_parity, ctx->step.aux[1]);
        HIPCHK(ctx, hipEventRecord(ctx->step.ev_regroup, ctx->step.aux[1]));
        ctx->step.regroup_pending = true;
    }
    HIPCHK(ctx, hipGetLastError());
    ctx->step.pre.valid = true;
    ctx->step.pre.key = prefetch_key(w, P);
    return NAVHIP_OK;
}

int navhip_agent_prefetch_dev(navhip_ctx *ctx, const navhip_world *w, void *stream)
{
    return navhip_agent_prefetch_dev_ex(ctx, w, stream, 0);
}

// behind a step: its list counters on their way to pinned host memory (side stream, after the searches)
static int send_step_lists(navhip_ctx *ctx, int parity_used, hipStream_t fallback, bool on_fallback)
{
    if(!ctx->step.lists_pinned) {
        HIPCHK(ctx, hipHostMalloc((void**)&ctx->step.lists_pinned, sizeof(int32_t) * NH_WL_LISTS * NH_WL_SUB, hipHostMallocDefault));
        memset(ctx->step.lists_pinned, 0, sizeof(int32_t) * NH_WL_LISTS * NH_WL_SUB);
    }
    const int32_t *src = step_buf<const int32_t>(ctx, NH_SB_WL_COUNT) + parity_used * NH_WL_COUNTERS;
    HIPCHK(ctx, hipMemcpyAsync(ctx->step.lists_pinned, src, sizeof(int32_t) * NH_WL_LISTS * NH_WL_SUB, hipMemcpyDeviceToHost,
                               (ctx->step.aux[0] && !on_fallback) ? ctx->step.aux[0] : fallback));
    return NAVHIP_OK;
}

// The tail of every step, joined or not: k_agent_mid and the consumers of its work lists (forked onto side stream 0 unless
// the step is serial), what the fork left for others to wait for, the list counters on their way to the host, the
// other set of counters for the next step.
static int step_tail(navhip_ctx *ctx, const nh_step_params &P, const nh_nbr &NB, const nh_worklists &WL, const nh_step_outs &O,
                     hipStream_t s)
{
    nh_step_state &st = ctx->step;
    const bool serial = st.serial_step;
    bool forked = false;
    if(nh_launch_agent_finish(P, NB, step_buf<float>(ctx, NH_SB_COH), step_buf<nh_mid_rec>(ctx, NH_SB_MIDREC), WL, st.wl_parity, O, s,
                              serial ? nullptr : st.aux[0], ctx, &forked)) {
        st.lists_signalled = forked;
        if(forked) {
            st.step_end_on = ctx->ho->by_events ? nullptr : s;      // (an event is no word: nobody can follow it that way)
            st.step_end_signalled = true;
        }
        int rc = send_step_lists(ctx, st.wl_parity, s, serial);
        st.wl_parity ^= 1;
        if(rc) return rc;
    }
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_agent_step_dev(navhip_ctx *ctx, const navhip_world *w, const navhip_step_out *out,
                          void *stream)
{
    if(!ctx || !out || !out->vel_xz) return NAVHIP_ERR_INVALID;
    int rc = step_check_world(ctx, w);
    if(rc) return rc;
    if(w->n_ents == 0) return NAVHIP_OK;
    if(nh_handover_failed(ctx)) return NAVHIP_ERR_DEVICE;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    ctx->step.step_end_on = nullptr; ctx->step.step_end_signalled = false;

    nh_step_params P;
    rc = step_fill_params(ctx, w, &P);
    if(rc) return rc;
    if(!grid_geometry(w, &P.grid)) {
        ctx->last_error = "agent step: empty spatial-grid bounds";
        return NAVHIP_ERR_INVALID;
    }
    ctx->counters.step_calls++; ctx->counters.agent_steps += (uint64_t)(P.work_end - P.work_begin);
    const bool prof = ctx->step.profiling;
    const bool joined = ctx->step.pre.valid && !prof && !ctx->step.serial_step && prefetch_key_matches(ctx, w, P);
    if(ctx->step.pre.valid && !joined) {
        // a prefetch for another snapshot is in flight on the side streams: let it drain before
        // its scratch buffers are reused
        signal_front_done(ctx);
        nh_handover_wait2(ctx, NH_HO_NBR, NH_HO_COH, s);
        if(ctx->step.regroup_pending) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->step.ev_regroup, 0));
        ctx->step.regroup_pending = false;
    }
    ctx->step.pre.valid = false;
    nh_step_outs O = {out->vel_xz, out->new_pos_xz, out->vdes_xz, out->vpref_xz, out->status};
    nh_nbr NB; nh_worklists WL;
    rc = walk_ensure(ctx, w->n_ents, &NB, &WL, s);
    if(!rc) rc = nh_ensure_side_streams(ctx, s);
    if(rc) return rc;
    if(!joined) nh_handover_mode(ctx, step_in_a_jam(ctx));       // (a joined step keeps the mode its prefetch chose)
    if(joined) {
        // spatial hash + neighbour walk + cohesion were started by navhip_agent_prefetch_dev: join
        const nh_spatial_scratch S = hash_scratch(ctx);
        P.grid.n = w->n_ents;
        P.grid.cell_start = S.cell_start; P.grid.recA = S.recA; P.grid.recV = S.recV; P.grid.pool_of = S.pool_of;
        P.grid.active = nullptr; P.grid.n_active = nullptr;       // (the walk, their only reader, ran with the prefetch)
        // ONE launch on this stream waits for the cohesion term -- and for the front, when that ran elsewhere (the step is
        // issued on another stream than the prefetch); behind an inline front it follows the neighbour walk, and says so
        if(ctx->step.front_stream != s) {
            signal_front_done(ctx);
            nh_handover_wait2(ctx, NH_HO_NBR, NH_HO_COH, s);
        }else{
            nh_handover_wait(ctx, NH_HO_COH, s, ctx->step.join0_signalled ? -1 : NH_HO_NBR);
            ctx->step.join0_signalled = true;
        }
    }else{
        // everything on this stream: spatial hash -> neighbour walk -> cohesion (-> next tick's lane grouping)
        if(prof) {
            for(auto &e : ctx->step.ev) if(!e) HIPCHK(ctx, hipEventCreate(&e));
            HIPCHK(ctx, hipEventRecord(ctx->step.ev[0], s));
        }
        rc = spatial_build(ctx, w, &P.grid, s, P.work_begin, P.work_end);
        if(rc) return rc;
        if(prof) HIPCHK(ctx, hipEventRecord(ctx->step.ev[1], s));
        nh_launch_agent_nbr(P, NB, s);
        if(prof) HIPCHK(ctx, hipEventRecord(ctx->step.ev[2], s));
        rc = coh_ensure(ctx, w->n_ents, w->n_flocks, P.n_members, s);
        if(rc) return rc;
        const bool regroup = nh_launch_cohesion(P, step_buf<int32_t>(ctx, NH_SB_COH_PLAN), step_buf<float>(ctx, NH_SB_COH), &ctx->step.coh_parity, s);
        if(prof) HIPCHK(ctx, hipEventRecord(ctx->step.ev[3], s));
        if(regroup && coh_regroup_due(ctx, P)) nh_launch_cohesion_regroup(P, step_buf<int32_t>(ctx, NH_SB_COH_PLAN), &ctx->step.coh_parity, s);
        if(prof) HIPCHK(ctx, hipEventRecord(ctx->step.ev[4], s));
    }
    rc = step_tail(ctx, P, NB, WL, O, s);
    if(rc) return rc;
    if(joined && ctx->step.regroup_pending && !ctx->step.snapshot_held) {
        HIPCHK(ctx, hipStreamWaitEvent(s, ctx->step.ev_regroup, 0));     // long finished by now
        ctx->step.regroup_pending = false;
    }
    if(prof) { HIPCHK(ctx, hipEventRecord(ctx->step.ev[5], s)); ctx->step.ev_valid = true; }
    return NAVHIP_OK;
}

int navhip_stream_wait_stage(navhip_ctx *ctx, void *stream, int stage)
{
    if(!ctx || !stream || !ctx->step.aux[0]) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if(stage == NAVHIP_STAGE_NEIGHBOURS) {
        if(!ctx->step.front_stream) return NAVHIP_ERR_INVALID;
        // (between the prefetch and its step: a launch of its own behind the walk; after the step: the step's wait for
        // the cohesion term has stored it)
        signal_front_done(ctx);
        nh_handover_wait(ctx, NH_HO_NBR, (hipStream_t)stream);
    }else if(stage == NAVHIP_STAGE_START) {
        if(!ctx->step.front_stream) return NAVHIP_ERR_INVALID;
        nh_handover_wait_for(ctx, ctx->step.start_flag, ctx->step.start_seq, (hipStream_t)stream);  // (not the end of a step enqueued since)
    }else if(stage == NAVHIP_STAGE_END) {
        if(!ctx->step.step_end_signalled) return NAVHIP_ERR_INVALID;  // (the last step ran on one stream: its stream is its end)
        nh_handover_wait(ctx, NH_HO_END, (hipStream_t)stream);
    }else if(stage == NAVHIP_STAGE_LISTS) {
        if(ctx->step.lists_signalled) nh_handover_wait(ctx, NH_HO_MID, (hipStream_t)stream);      // (else: one stream, nothing to wait for)
    }
    else return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_set_profiling(navhip_ctx *ctx, int on)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    ctx->step.profiling = on != 0;
    ctx->step.ev_valid = false;
    return NAVHIP_OK;
}

int navhip_last_step_ms(navhip_ctx *ctx, float out_ms[NAVHIP_STEP_PHASES])
{
    if(!ctx || !out_ms || !ctx->step.ev_valid) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipEventSynchronize(ctx->step.ev[5]));
    for(int i = 0; i < NAVHIP_STEP_PHASES; i++)
        HIPCHK(ctx, hipEventElapsedTime(&out_ms[i], ctx->step.ev[i], ctx->step.ev[i + 1]));
    return NAVHIP_OK;
}

// the counters of a step's work lists -> the six reported: the wave and the heavy list together (17-64 neighbours),
// the retry list not at all
static void sum_step_lists(const volatile int32_t *h, int32_t out_counts[6])
{
    static const int slot_of[NH_WL_LISTS] = {0, 1, 2, 3, 4, 4, 5, -1};
    for(int l = 0; l < 6; l++) out_counts[l] = 0;
    for(int l = 0; l < NH_WL_LISTS; l++)
        for(int sb = 0; sb < NH_WL_SUB; sb++) if(slot_of[l] >= 0) out_counts[slot_of[l]] += h[l * NH_WL_SUB + sb];
}

// the work-list sizes of the last agent step: {light 1..4, wave, full} (waits for the step)
int navhip_last_step_lists(navhip_ctx *ctx, int32_t out_counts[6])
{
    if(!ctx || !out_counts || !ctx->step.buf[NH_SB_WL_COUNT].p) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    const int32_t *src = step_buf<const int32_t>(ctx, NH_SB_WL_COUNT) + (ctx->step.wl_parity ^ 1) * NH_WL_COUNTERS;
    int32_t h[NH_WL_COUNTERS];
    HIPCHK(ctx, hipMemcpy(h, src, sizeof(h), hipMemcpyDeviceToHost));
    sum_step_lists(h, out_counts);
    return NAVHIP_OK;
}

int navhip_step_lists_peek(navhip_ctx *ctx, int32_t out_counts[6])
{
    if(!ctx || !out_counts) return NAVHIP_ERR_INVALID;
    for(int l = 0; l < 6; l++) out_counts[l] = 0;
    if(ctx->step.lists_pinned) sum_step_lists((const volatile int32_t*)ctx->step.lists_pinned, out_counts);
    return NAVHIP_OK;
}

int navhip_agent_step(navhip_ctx *ctx, const navhip_world *w, const navhip_step_out *out)
{
    if(!ctx || !w || !out || !out->vel_xz) return NAVHIP_ERR_INVALID;
    if(w->n_ents <= 0) return w->n_ents == 0 ? NAVHIP_OK : NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    navhip_world d;
    int rc = nh_stage_world(ctx, w, &d, s);
    if(rc) return rc;
    const size_t n = (size_t)w->n_ents;
    navhip_step_out dout = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for(const nh_out_row &o : nh_out_rows) {
        if(!nh_member(out, o.off)) continue;
        rc = nh_stage_reserve(ctx, o.slot, n * o.row_bytes, &nh_member(&dout, o.off));
        if(rc) return rc;
    }
    rc = navhip_agent_step_dev(ctx, &d, &dout, s);
    if(rc) return rc;
    // only the rows of the stepped slab were written: a caller that issues one call per slab into
    // the same output arrays (move_submit_cpu_work, movement.c:3759-3762) keeps its other slabs
    size_t b = (size_t)w->work_begin, e = (size_t)w->work_end;
    if(b == 0 && e == 0) e = n;
    for(const nh_out_row &o : nh_out_rows) {
        char *host = (char*)nh_member(out, o.off);
        if(!host || e <= b) continue;
        const size_t row = o.row_bytes;
        HIPCHK(ctx, hipMemcpyAsync(host + b * row, (char*)nh_member(&dout, o.off) + b * row, (e - b) * row,
                                   hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

}  // extern "C"

// bg_ent insert-all + inrange_circle for nq query points with everything on the device: the index over
// dev_w->pos_xz (positions only), ids in the reference's visiting order into d_ids [nq][maxout], counts into d_counts
int nh_spatial_query_dev(navhip_ctx *ctx, const navhip_world *dev_w, const float *d_query, int nq, float range, int maxout,
                         int32_t *d_counts, uint32_t *d_ids, hipStream_t s)
{
    nh_grid g;
    int rc = spatial_build(ctx, dev_w, &g, s, 0, -1, false);
    if(rc) return rc;
    nh_launch_spatial_query(g, d_query, nq, range, maxout, d_counts, d_ids, s);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

extern "C" {

int navhip_spatial_query(navhip_ctx *ctx, const navhip_world *w, const float *query_xz, int nq,
                         float range, int maxout, int32_t *out_counts, uint32_t *out_ids)
{
    if(!ctx || !w || !w->pos_xz || w->n_ents < 0 || nq < 0 || maxout < 1 || !query_xz
    || !out_counts || !out_ids)
        return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    navhip_world d;
    int rc = nh_stage_world(ctx, w, &d, s, {offsetof(navhip_world, pos_xz)});
    if(rc) return rc;
    const float *dq;
    int32_t *d_counts; uint32_t *d_ids;
    rc = nh_stage_in(ctx, NH_STAGE_CALL0, query_xz, (size_t)nq * 8, (const void**)&dq, s);
    if(!rc) rc = nh_stage_reserve(ctx, NH_STAGE_CALL1, (size_t)nq * 4, (void**)&d_counts);
    if(!rc) rc = nh_stage_reserve(ctx, NH_STAGE_CALL2, (size_t)nq * maxout * 4, (void**)&d_ids);
    if(rc) return rc;
    rc = nh_spatial_query_dev(ctx, &d, dq, nq, range, maxout, d_counts, d_ids, s);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_counts, d_counts, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(out_ids, d_ids, (size_t)nq * maxout * 4,
                               hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

int navhip_region_lookup(navhip_ctx *ctx, int nq, const float *pos_xz, const int32_t *rows,
                         const int32_t *region_field_slot, int n_region_rows, const uint8_t *field_pool,
                         int n_field_slots, const int32_t *centre_abs, const int32_t *radius,
                         float map_pos_x, float map_pos_z, uint8_t *out_dir, uint8_t *out_at_slot)
{
    if(!ctx || nq < 0 || (nq > 0 && (!pos_xz || !rows || !out_dir))) return NAVHIP_ERR_INVALID;
    if((out_at_slot != nullptr) && (!centre_abs || !radius)) return NAVHIP_ERR_INVALID;
    if(nq == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    nh_step_params P;
    memset(&P, 0, sizeof(P));
    nh_fill_map_view(ctx, &P.map);
    P.map_x = map_pos_x; P.map_z = map_pos_z;
    const size_t nchunks = (size_t)ctx->nchunks;
    const bool resident = !region_field_slot && !field_pool;
    if(resident) {
        if(!ctx->pool) { ctx->last_error = "navhip_region_lookup: no table given and no resident pool"; return NAVHIP_ERR_INVALID; }
        P.region_field_slot = nh_pool_map(ctx); P.field_pool = nh_pool_fields(ctx);
        n_region_rows = nh_pool_dests(ctx);
    }else{
        if(!region_field_slot || !field_pool || n_region_rows < 1 || n_field_slots < 1) return NAVHIP_ERR_INVALID;
        // (the slots of the world's own tables: the same data)
        int rc = nh_stage_in(ctx, NH_STAGE_REGION_FIELD_SLOT, region_field_slot, (size_t)n_region_rows * nchunks * 4, (const void**)&P.region_field_slot, s);
        if(!rc) rc = nh_stage_in(ctx, NH_STAGE_FIELD_POOL, field_pool, (size_t)n_field_slots * NH_CELLS, (const void**)&P.field_pool, s);
        if(rc) return rc;
        nh_async_invalidate_static(ctx);
    }
    for(int q = 0; q < nq; q++)
        if(rows[q] < -1 || rows[q] >= n_region_rows) return NAVHIP_ERR_INVALID;
    const float *d_pos; const int32_t *d_rows, *d_cen = nullptr, *d_rad = nullptr;
    uint8_t *d_out = nullptr;
    int rc = nh_stage_in(ctx, NH_STAGE_CALL0, pos_xz, (size_t)nq * 8, (const void**)&d_pos, s);
    if(!rc) rc = nh_stage_in(ctx, NH_STAGE_CALL1, rows, (size_t)nq * 4, (const void**)&d_rows, s);
    if(!rc && out_at_slot) rc = nh_stage_in(ctx, NH_STAGE_CALL2, centre_abs, (size_t)nq * 8, (const void**)&d_cen, s);
    if(!rc && out_at_slot) rc = nh_stage_in(ctx, NH_STAGE_CALL3, radius, (size_t)nq * 4, (const void**)&d_rad, s);
    if(!rc) rc = nh_stage_reserve(ctx, NH_STAGE_CALL4, (size_t)nq * 2, (void**)&d_out);
    if(rc) return rc;
    nh_launch_region_lookup(P, nq, d_pos, d_rows, d_cen, d_rad, d_out, d_out + nq, s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_dir, d_out, (size_t)nq, hipMemcpyDeviceToHost, s));
    if(out_at_slot) HIPCHK(ctx, hipMemcpyAsync(out_at_slot, d_out + nq, (size_t)nq, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

// the ClearPath kernels on nq problems in host arrays; rows: nh_launch_clearpath
static int clearpath_batch(navhip_ctx *ctx, int nq, const float *ent, const float *des_v,
                           const float *dyn, const int32_t *n_dyn, const float *stat,
                           const int32_t *n_stat, float *out, int rows)
{
    if(!ctx || nq < 0 || !ent || !des_v || !dyn || !n_dyn || !stat || !n_stat || !out)
        return NAVHIP_ERR_INVALID;
    if(nq == 0) return NAVHIP_OK;
    for(int i = 0; i < nq; i++) {
        if(n_dyn[i] < 0 || n_dyn[i] > 32 || n_stat[i] < 0 || n_stat[i] > 32) return NAVHIP_ERR_INVALID;
        if(rows == 1 && n_dyn[i] + n_stat[i] > NH_ROW_MAX) return NAVHIP_ERR_INVALID;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const void *d[6];
    const struct { const void *host; size_t bytes; nh_stage_slot slot; } in[6] = {
        {ent, (size_t)nq * 20, NH_STAGE_CALL0},   {des_v, (size_t)nq * 8, NH_STAGE_CALL1},  {dyn, (size_t)nq * 640, NH_STAGE_CALL2},
        {n_dyn, (size_t)nq * 4, NH_STAGE_CALL3},  {stat, (size_t)nq * 640, NH_STAGE_CALL4}, {n_stat, (size_t)nq * 4, NH_STAGE_CALL5}};
    for(int i = 0; i < 6; i++) {
        int rc = nh_stage_in(ctx, in[i].slot, in[i].host, in[i].bytes, &d[i], s);
        if(rc) return rc;
    }
    float *d_out = nullptr;
    int rc = nh_stage_reserve(ctx, NH_STAGE_CALL6, (size_t)nq * 8, (void**)&d_out);
    if(rc) return rc;
    nh_launch_clearpath(nq, (const float*)d[0], (const float*)d[1], (const float*)d[2],
                        (const int32_t*)d[3], (const float*)d[4], (const int32_t*)d[5], d_out, rows, s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, (size_t)nq * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

int navhip_clearpath(navhip_ctx *ctx, int nq, const float *ent, const float *des_v,
                     const float *dyn, const int32_t *n_dyn, const float *stat,
                     const int32_t *n_stat, float *out)
{
    return clearpath_batch(ctx, nq, ent, des_v, dyn, n_dyn, stat, n_stat, out, 0);
}

int navhip_clearpath_rows(navhip_ctx *ctx, int nq, const float *ent, const float *des_v,
                          const float *dyn, const int32_t *n_dyn, const float *stat,
                          const int32_t *n_stat, float *out)
{
    return clearpath_batch(ctx, nq, ent, des_v, dyn, n_dyn, stat, n_stat, out, 1);
}

int navhip_clearpath_team(navhip_ctx *ctx, int nq, const float *ent, const float *des_v,
                          const float *dyn, const int32_t *n_dyn, const float *stat,
                          const int32_t *n_stat, float *out)
{
    return clearpath_batch(ctx, nq, ent, des_v, dyn, n_dyn, stat, n_stat, out, 2);
}

}  // extern "C"
