// los_chain_api.hip -- navhip_los_chain_*: the LOS fields of a set of paths kept current while blockers move.
//
// The reference caches one LOS field per (destination, chunk) along a path (N_FC_PutLOSField, nav.c:1840-1847), drops
// the LOS fields of a dirty chunk together with its flow fields (fieldcache.c:213-227, 526-535) and rebuilds a missing
// one from the cached field of the chunk before it on the path (nav.c:2026-2039, 4042-4047).  A chain is that cache for
// a fixed set of (destination, chunk) slots in a pool the CALLER owns (navhip_world.los_pool samples it; slots never
// move): every slot knows the slot of its predecessor, slots are ordered by their distance from the destination chunk
// (the level), and a level only ever reads the level before -- so a level is one launch, and the order of the launches
// on one stream is the only synchronisation there is.
//   build    every slot, level by level: what navhip_build_los_dev gives level by level, without the gathered copy of the
//            predecessors that entry point needs
//   refresh  behind a blocker batch: one launch marks the slots whose chunk the batch flagged in changed[] (with
//            NAVHIP_LOS_REFRESH_DOWNSTREAM: and everything built from them) and compacts them per level, one launch
//            per level rebuilds them in place.  No host round trip, no allocation: everything is sized at create.
// A slot may carry a faction (an attacking path: tiles blocked by enemies only are passable).  changed[] is passability
// WITHOUT a faction; what it misses -- an ally on tiles an enemy holds already -- is in the layer's fac_changed[], one bit
// per faction whose rows differ, and such a slot is also stale by a bit of a faction that is NOT among its enemies
// (fmask[slot]).  With flags = 0 that is a superset of the reference, whose dirty set (nav.c:1036) knows no faction and
// leaves such fields stale.
// A unit without kernels: they are k_los_field / k_los_mark of los_kernels.hip.
#include "navhip_internal.h"
#include <new>

struct navhip_los_chain {
    navhip_ctx          *ctx;
    void                *slab;            // every device array of the view but the pool, one allocation
    nh_los_chain_view    v;
    std::vector<int32_t> level_begin;     // host copy: the grids of the launches
    hipStream_t          last;            // the stream of the last build / refresh (navhip_los_chain_get_stats waits for it)
    bool                 used;
};

// the checks of navhip_build_los on one request, and those that make a set of requests a chain
static const char *chain_request_error(const navhip_ctx *ctx, const navhip_los_req *reqs, const int32_t *prev_slot,
                                       const std::vector<int32_t> &level, int i)
{
    const navhip_los_req &r = reqs[i];
    const bool has_prev = r.prev_dr != 0 || r.prev_dc != 0;
    if(r.layer >= NAVHIP_NAV_LAYER_MAX || r.chunk_r >= ctx->h || r.chunk_c >= ctx->w || r.target_chunk_r >= ctx->h
    || r.target_chunk_c >= ctx->w || r.target_tile_r >= 64 || r.target_tile_c >= 64)
        return "chunk, target or layer outside the map";
    if(!ctx->layers[r.layer].cost) return "the layer is not resident";
    if(r.faction_id != NAVHIP_FACTION_ID_NONE) {
        if(r.faction_id >= NAVHIP_MAX_FACTIONS) return "faction_id is neither a faction nor NAVHIP_FACTION_ID_NONE";
        if(!ctx->layers[r.layer].fac_changed)
            return "a request with a faction on a layer without a factions plane (no per-faction changed flags to follow)";
    }
    if((prev_slot[i] == -1) != !has_prev) return "prev_slot is -1 exactly for a request without a previous chunk";
    if(!has_prev) {
        if(r.chunk_r != r.target_chunk_r || r.chunk_c != r.target_chunk_c) return "a request without a previous chunk is not on the target's chunk";
    }else{
        if((r.prev_dr == 0) == (r.prev_dc == 0) || r.prev_dr < -1 || r.prev_dr > 1 || r.prev_dc < -1 || r.prev_dc > 1)
            return "the previous chunk is not a neighbour";
        if(prev_slot[i] < 0 || prev_slot[i] >= i) return "prev_slot does not name an earlier slot";
        const navhip_los_req &p = reqs[prev_slot[i]];
        if((int)p.chunk_r != (int)r.chunk_r + r.prev_dr || (int)p.chunk_c != (int)r.chunk_c + r.prev_dc)
            return "the predecessor's chunk is not chunk + (prev_dr, prev_dc)";
        if(p.layer != r.layer || p.target_chunk_r != r.target_chunk_r || p.target_chunk_c != r.target_chunk_c
        || p.target_tile_r != r.target_tile_r || p.target_tile_c != r.target_tile_c)
            return "the predecessor has another layer or target";
        if(p.faction_id != r.faction_id || (r.faction_id != NAVHIP_FACTION_ID_NONE && p.enemies != r.enemies))
            return "the predecessor has another faction or other enemies";
    }
    if(i > 0 && level[i] < level[i - 1]) return "slots are not in level order";
    return nullptr;
}

extern "C" {

int navhip_los_chain_create(navhip_ctx *ctx, const navhip_los_req *reqs, const int32_t *prev_slot, int n, uint8_t *dev_pool,
                            float map_pos_x, float map_pos_z, navhip_los_chain **out)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    if(!reqs || !prev_slot || n <= 0 || !dev_pool || !out) {
        ctx->last_error = "navhip_los_chain_create: no requests, no pool or nowhere to put the chain";
        return NAVHIP_ERR_INVALID;
    }
    std::vector<int32_t> level((size_t)n, 0);
    std::vector<uint32_t> cell((size_t)n);
    std::vector<uint16_t> fmask((size_t)n, 0);
    bool any_faction = false;
    for(int i = 0; i < n; i++) {
        if(prev_slot[i] >= 0 && prev_slot[i] < i) level[i] = level[prev_slot[i]] + 1;
        if(const char *why = chain_request_error(ctx, reqs, prev_slot, level, i)) {
            ctx->last_error = "navhip_los_chain_create: slot " + std::to_string(i) + ": " + why;
            return NAVHIP_ERR_INVALID;
        }
        cell[i] = (uint32_t)reqs[i].layer << 24 | (uint32_t)((int)reqs[i].chunk_r * ctx->w + reqs[i].chunk_c);
        if(reqs[i].faction_id != NAVHIP_FACTION_ID_NONE) { fmask[i] = (uint16_t)(~reqs[i].enemies & 0x7fff); any_faction = true; }
    }
    const int levels = level[n - 1] + 1;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    navhip_los_chain *c = new (std::nothrow) navhip_los_chain();
    if(!c) return NAVHIP_ERR_NOMEM;
    c->ctx = ctx;
    c->level_begin.assign((size_t)levels + 1, n);
    for(int i = n - 1; i >= 0; i--) c->level_begin[level[i]] = i;
    c->level_begin[0] = 0;
    // one slab: requests | prev_slot | cell | level_begin | list | count | stats | stale | overflow | fmask (with a faction slot)
    const size_t N = (size_t)n;
    const size_t parts[] = {N * sizeof(navhip_los_req), N * 4, N * 4, ((size_t)levels + 1) * 4, N * 4, (size_t)levels * 4,
                            NH_LCS_COUNT * 4, N, N, any_faction ? N * 2 : 0};
    size_t off[sizeof(parts) / sizeof(parts[0]) + 1] = {0};
    for(size_t k = 0; k < sizeof(parts) / sizeof(parts[0]); k++) off[k + 1] = off[k] + nh_up256(parts[k]);
    const size_t total = off[sizeof(parts) / sizeof(parts[0])];
    auto fail = [&](const char *what, int rc) { ctx->last_error = what; navhip_los_chain_destroy(c); return rc; };
    if(hipMalloc(&c->slab, total) != hipSuccess) { c->slab = nullptr; return fail("navhip_los_chain_create: device memory", NAVHIP_ERR_NOMEM); }
    char *base = (char*)c->slab;
    if(hipMemset(base, 0, total) != hipSuccess
    || hipMemcpy(base + off[0], reqs, parts[0], hipMemcpyHostToDevice) != hipSuccess
    || hipMemcpy(base + off[1], prev_slot, parts[1], hipMemcpyHostToDevice) != hipSuccess
    || hipMemcpy(base + off[2], cell.data(), parts[2], hipMemcpyHostToDevice) != hipSuccess
    || hipMemcpy(base + off[3], c->level_begin.data(), parts[3], hipMemcpyHostToDevice) != hipSuccess
    || (any_faction && hipMemcpy(base + off[9], fmask.data(), parts[9], hipMemcpyHostToDevice) != hipSuccess))
        return fail("navhip_los_chain_create: copy to the device", NAVHIP_ERR_DEVICE);
    c->v = nh_los_chain_view{(const navhip_los_req*)(base + off[0]), (const int32_t*)(base + off[1]), (const uint32_t*)(base + off[2]),
                             any_faction ? (const uint16_t*)(base + off[9]) : nullptr, (const int32_t*)(base + off[3]), dev_pool, (uint8_t*)(base + off[7]), (uint8_t*)(base + off[8]),
                             (int32_t*)(base + off[4]), (int32_t*)(base + off[5]), (int32_t*)(base + off[6]), n, levels,
                             map_pos_x, map_pos_z};
    *out = c;
    return NAVHIP_OK;
}

int navhip_los_chain_build(navhip_los_chain *c, void *stream)
{
    if(!c) return NAVHIP_ERR_INVALID;
    navhip_ctx *ctx = c->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    ctx->counters.los_fields += (uint64_t)c->v.slots;
    for(int L = 0; L < c->v.levels; L++)
        nh_launch_los_chain_level(ctx, c->v, c->level_begin[L], c->level_begin[L + 1] - c->level_begin[L], s);
    c->last = s; c->used = true;
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_los_chain_refresh(navhip_los_chain *c, uint32_t flags, void *stream)
{
    if(!c) return NAVHIP_ERR_INVALID;
    navhip_ctx *ctx = c->ctx;
    if(flags & ~(uint32_t)NAVHIP_LOS_REFRESH_DOWNSTREAM) { ctx->last_error = "navhip_los_chain_refresh: unknown flag"; return NAVHIP_ERR_INVALID; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    nh_launch_los_chain_mark(ctx, c->v, (flags & NAVHIP_LOS_REFRESH_DOWNSTREAM) != 0, s);
    for(int L = 0; L < c->v.levels; L++)
        nh_launch_los_chain_stale(ctx, c->v, L, c->level_begin[L], c->level_begin[L + 1] - c->level_begin[L], s);
    c->last = s; c->used = true;
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_los_chain_get_stats(navhip_los_chain *c, navhip_los_chain_stats *out)
{
    if(!c || !out) return NAVHIP_ERR_INVALID;
    navhip_ctx *ctx = c->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if(c->used) HIPCHK(ctx, hipStreamSynchronize(c->last));
    int32_t st[NH_LCS_COUNT];
    HIPCHK(ctx, hipMemcpy(st, c->v.stats, sizeof(st), hipMemcpyDeviceToHost));
    out->slots = c->v.slots; out->levels = c->v.levels;
    out->stale = st[NH_LCS_STALE]; out->rebuilt = st[NH_LCS_REBUILT]; out->redone = st[NH_LCS_REDONE];
    return NAVHIP_OK;
}

void navhip_los_chain_destroy(navhip_los_chain *c)
{
    if(!c) return;
    hipSetDevice(c->ctx->device);
    if(c->used && nh_streams_alive(c->ctx->device)) hipStreamSynchronize(c->last);
    if(c->slab) hipFree(c->slab);
    delete c;
}

}  // extern "C"
