// navhip_api.hip -- the map state behind the C ABI of libnavhip.so (include/navhip.h): the context, the planes of every
// nav layer resident in HBM with the row masks derived from them, the blockers, and the chunk / LOS / region field builds
// through device or host buffers, with the two field ids.
#include "navhip_internal.h"
#include <cmath>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <new>
#include <vector>

// The planes of a layer (resident from their first upload: for the reference's maximum 64x64-chunk map 64 MB cost + 128 MB
// blockers + 128 MB local islands + 960 MB factions, a fraction of the 288 GB part), one row per NAVHIP_PLANE_* in the order
// of their numbers: the member of navhip_layer, bytes per cell, whether an upload leaves the derived masks stale, whether
// a fresh allocation is zeroed (a cost plane is not: it appears with its first upload) ...
struct plane_row { size_t off; size_t cell_bytes; bool dirties, zeroed; };
static const plane_row plane_rows[] = {
    {offsetof(navhip_layer, cost),          1,                   true,  false},  // u8  [chunks][64][64]     nav_chunk.cost_base     nav_data.h:123
    {offsetof(navhip_layer, blockers),      2,                   true,  true},   // u16 [chunks][64][64]     nav_chunk.blockers      nav_data.h:134
    {offsetof(navhip_layer, local_islands), 2,                   false, true},   // u16 [chunks][64][64]     nav_chunk.local_islands nav_data.h:157
    {offsetof(navhip_layer, factions),      NAVHIP_MAX_FACTIONS, true,  true},   // u8  [chunks][15][64][64] nav_chunk.factions      nav_data.h:141
    {offsetof(navhip_layer, islands),       2,                   false, true},   // u16 [chunks][64][64]     global island ids
};
static_assert(std::size(plane_rows) == NAVHIP_PLANE_COUNT && NAVHIP_PLANE_COST_BASE == 0 && NAVHIP_PLANE_BLOCKERS == 1
           && NAVHIP_PLANE_LOCAL_ISLANDS == 2 && NAVHIP_PLANE_FACTIONS == 3 && NAVHIP_PLANE_ISLANDS == 4,
              "plane_rows: one row per NAVHIP_PLANE_*, indexed by it");
// ... and its derived device arrays (struct navhip_layer says what each holds): bytes per chunk, whether the array exists
// only beside the factions plane, whether a fresh one is zeroed (the flags the kernels raise; the rows of a factions plane
// that is all zero until its first upload)
struct derived_row { size_t off; size_t chunk_bytes; bool with_factions, zeroed; };
static const derived_row derived_rows[] = {
    {offsetof(navhip_layer, passmask),    64 * sizeof(uint64_t),                       false, false},
    {offsetof(navhip_layer, probemask),   128 * sizeof(uint64_t),                      false, false},
    {offsetof(navhip_layer, unit_cost),   1,                                           false, false},
    {offsetof(navhip_layer, touched),     1,                                           false, true},
    {offsetof(navhip_layer, changed),     1,                                           false, true},
    {offsetof(navhip_layer, facmask),     NAVHIP_MAX_FACTIONS * 64 * sizeof(uint64_t), true,  true},
    {offsetof(navhip_layer, facany),      sizeof(uint16_t),                            true,  true},
    {offsetof(navhip_layer, fac_changed), sizeof(uint16_t),                            true,  true},
    {offsetof(navhip_layer, fac_touched), sizeof(uint32_t),                            true,  true},
};

static void *&plane_slot(navhip_layer &L, int plane) { return nh_member(&L, plane_rows[plane].off); }
static size_t plane_bytes(const navhip_ctx *ctx, int plane) { return (size_t)ctx->nchunks * NH_CELLS * plane_rows[plane].cell_bytes; }
static bool check_layer_plane(const navhip_ctx *ctx, int layer, int plane)
{
    return ctx && layer >= 0 && layer < NAVHIP_NAV_LAYER_MAX && plane >= 0 && plane < NAVHIP_PLANE_COUNT;
}

// Device buffers grown on demand, and the staging path of every host-buffer entry point of the library (this unit,
// step_api.hip, submit_api.hip, state_kernels.hip): nh_ensure -- b holds at least `need` bytes, contents are not kept;
// nh_ensure_buf -- the step's scratch and the staging slots: at least 16 bytes, and a buffer that moved is counted
// (scratch_moves); nh_stage_reserve -- a staging slot of `bytes`; nh_stage_in -- a host array copied to its slot on s
// (*dst: the device copy, NULL stays NULL).  What a slot in front of NH_STAGE_CALL0 held may have been the asynchronous
// step's (its attribute tables, its resident snapshot): writing one tells it so.
int nh_ensure(navhip_ctx *ctx, nh_buf &b, size_t need)
{
    if(b.cap >= need) return NAVHIP_OK;
    if(b.p) HIPCHK(ctx, hipFree(b.p));
    b = nh_buf();
    const size_t want = need + need / 2;
    HIPCHK(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return NAVHIP_OK;
}

int nh_ensure_buf(navhip_ctx *ctx, nh_buf &b, size_t need)
{
    const void *old = b.p;
    int rc = nh_ensure(ctx, b, need ? need : 16);
    if(b.p != old) ctx->step.scratch_moves++;
    return rc;
}

int nh_stage_reserve(navhip_ctx *ctx, nh_stage_slot slot, size_t bytes, void **dev)
{
    int rc = nh_ensure_buf(ctx, ctx->stage[slot], bytes);
    if(rc) return rc;
    *dev = ctx->stage[slot].p;
    return NAVHIP_OK;
}

int nh_stage_in(navhip_ctx *ctx, nh_stage_slot slot, const void *host, size_t bytes, const void **dst, hipStream_t s)
{
    if(slot < NH_STAGE_CALL0) nh_async_invalidate_static(ctx);
    *dst = nullptr;
    if(!host) return NAVHIP_OK;
    int rc = nh_stage_reserve(ctx, slot, bytes, (void**)dst);
    if(rc) return rc;
    if(bytes) HIPCHK(ctx, hipMemcpyAsync((void*)*dst, host, bytes, hipMemcpyHostToDevice, s));
    return NAVHIP_OK;
}

// rebuild passmask / probemask / unit_cost / facmask of chunks whose cost, blockers or factions changed (after an upload: the
// device-side blocker updates refresh their chunks themselves).  Whatever it launches has completed when it
// returns, so consumers on any stream may follow.
int nh_refresh_derived(navhip_ctx *ctx, hipStream_t s)
{
    bool launched = false;
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++) {
        navhip_layer &L = ctx->layers[l];
        if(!L.any_dirty || !L.cost) continue;
        std::vector<uint32_t> list;
        for(int i = 0; i < ctx->nchunks; i++)
            if(L.dirty[i]) list.push_back((uint32_t)i);
        if(!list.empty()) {
            if((int)list.size() == ctx->nchunks) {
                nh_launch_derive(ctx, l, nullptr, ctx->nchunks, s);
            }else{
                int rc = nh_ensure(ctx, ctx->d_dirty_list, list.size() * sizeof(uint32_t));
                if(rc) return rc;
                HIPCHK(ctx, hipMemcpyAsync(ctx->d_dirty_list.p, list.data(),
                                           list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
                nh_launch_derive(ctx, l, (const uint32_t*)ctx->d_dirty_list.p, (int)list.size(), s);
                HIPCHK(ctx, hipStreamSynchronize(s));   // list buffer is reused per layer
            }
            HIPCHK(ctx, hipGetLastError());
            launched = true;
        }
        memset(L.dirty, 0, ctx->nchunks);
        L.any_dirty = false;
    }
    if(launched) HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

// a device array of a layer that does not exist yet
static int layer_array(navhip_ctx *ctx, void *&p, size_t bytes, bool zeroed)
{
    if(p) return NAVHIP_OK;
    HIPCHK(ctx, hipMalloc(&p, bytes));
    if(zeroed) HIPCHK(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream));
    return NAVHIP_OK;
}

// The layer is about to hold `plane`: the plane, the host's dirty marks and the derived arrays, each made where it is
// missing -- a preparation that ran out of memory half way is finished by the next one, and the dirty marks, made first,
// are there for every upload that gets as far as marking.
static int layer_prepare(navhip_ctx *ctx, int layer, int plane)
{
    navhip_layer &L = ctx->layers[layer];
    if(!L.dirty && !(L.dirty = (uint8_t*)calloc(ctx->nchunks, 1))) return NAVHIP_ERR_NOMEM;
    int rc = layer_array(ctx, plane_slot(L, plane), plane_bytes(ctx, plane), plane_rows[plane].zeroed);
    for(const derived_row &d : derived_rows)
        if(!rc && (!d.with_factions || L.factions))
            rc = layer_array(ctx, nh_member(&L, d.off), (size_t)ctx->nchunks * d.chunk_bytes, d.zeroed);
    return rc;
}

// Chunks [chunk0, chunk0 + n) of a plane from host memory (who: the entry point, for last_error).  A whole-plane upload
// (navhip_upload_plane: [0, nchunks)) SETS the layer's nonunit_costs, so it can go back to false; a chunk upload
// (navhip_upload_chunk: one chunk) can only raise it.
static int upload_chunks(navhip_ctx *ctx, int layer, int plane, int chunk0, int n, bool whole, const void *host, size_t bytes,
                         const char *who)
{
    const size_t per = NH_CELLS * plane_rows[plane].cell_bytes;
    if(bytes != (size_t)n * per) {
        ctx->last_error = std::string(who) + ": size mismatch";
        return NAVHIP_ERR_INVALID;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = layer_prepare(ctx, layer, plane);
    if(rc) return rc;
    navhip_layer &L = ctx->layers[layer];
    HIPCHK(ctx, hipMemcpyAsync((char*)plane_slot(L, plane) + (size_t)chunk0 * per, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // caller may reuse `host` immediately
    if(plane_rows[plane].dirties) {
        memset(L.dirty + chunk0, 1, n);
        L.any_dirty = true;
    }
    if(plane == NAVHIP_PLANE_COST_BASE) {
        // does the layer hold costs other than 1 / impassable?  (The reference's cost writers produce no
        // others, nav.c:339-342,416; a host that does sends its requests to the relaxation kernel, whose
        // launch is then sized for real work instead of for an empty list.)
        const uint8_t *c = (const uint8_t*)host;
        bool other = false;
        for(size_t i = 0; i < bytes && !other; i++) other = c[i] != 1 && c[i] != NAVHIP_COST_IMPASSABLE;
        L.nonunit_costs = other || (!whole && L.nonunit_costs);
    }
    return NAVHIP_OK;
}

// request i is built into slot dev_slots[i] of dev_inout_dirs when dev_slots is given (navhip_pool_build)
static int build_fields_on(navhip_ctx *ctx, const navhip_field_req *dev_reqs, int n, uint8_t *dev_inout_dirs,
                           float *dev_out_integ, const int32_t *dev_slots, hipStream_t s)
{
    int rc = nh_refresh_derived(ctx, s);
    if(rc) return rc;
    // work list of the generic kernel: the header is zero between launches (the kernel resets it)
    const void *old_list = ctx->gen_list.p;
    rc = nh_ensure_buf(ctx, ctx->gen_list, ((size_t)n + NH_GEN_HEADER) * sizeof(int32_t));
    if(rc) return rc;
    if(ctx->gen_list.p != old_list) HIPCHK(ctx, hipMemsetAsync(ctx->gen_list.p, 0, NH_GEN_HEADER * sizeof(int32_t), s));
    // scratch of the classing pass: zero when it is (re)allocated, kept zero between builds by the builds themselves
    if(n > ctx->classes.cap) {
        const int cap = (n + n / 2 + 1) & ~1;
        ctx->classes = {};
        rc = nh_ensure_buf(ctx, ctx->field_classes, nh_field_classes_bytes(cap));
        if(rc) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->field_classes.p, 0, nh_field_classes_bytes(cap), s));
        ctx->classes.cap = cap;
    }
    ctx->last_fields.gen_slot = nh_launch_fields(ctx, dev_reqs, n, dev_inout_dirs, dev_out_integ, (int32_t*)ctx->gen_list.p,
                                                 (int32_t*)ctx->field_classes.p, s, dev_slots);
    ctx->last_fields.n = n; ctx->last_fields.stream = s;
    HIPCHK(ctx, hipGetLastError());
    ctx->counters.field_calls++; ctx->counters.chunk_fields += (uint64_t)n;
    return NAVHIP_OK;
}

int navhip_build_fields_slots_dev(navhip_ctx *ctx, const navhip_field_req *dev_reqs, int n, uint8_t *dev_fields,
                                  const int32_t *dev_slots, hipStream_t s)
{
    if(n == 0) return NAVHIP_OK;
    return build_fields_on(ctx, dev_reqs, n, dev_fields, nullptr, dev_slots, s);
}

extern "C" {

int navhip_ctx_create(navhip_ctx **out, int chunk_w, int chunk_h, int device)
{
    if(!out || chunk_w < 1 || chunk_h < 1 || chunk_w > 64 || chunk_h > 64)   // 6-bit chunk ids, nav.c:841-848
        return NAVHIP_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if(hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) {
        fprintf(stderr, "navhip: no usable HIP device (count=%d, asked for %d); this library has "
                        "no CPU fallback\n", ndev, device);
        return NAVHIP_ERR_DEVICE;
    }
    navhip_ctx *ctx = new (std::nothrow) navhip_ctx();
    if(!ctx) return NAVHIP_ERR_NOMEM;
    ctx->device = device;
    ctx->w = chunk_w; ctx->h = chunk_h; ctx->nchunks = chunk_w * chunk_h;
    if(hipSetDevice(device) != hipSuccess
    || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return NAVHIP_ERR_DEVICE;
    }
    *out = ctx;
    return NAVHIP_OK;
}

void navhip_ctx_destroy(navhip_ctx *ctx)
{
    if(!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    navhip_comm_destroy(ctx);
    if(ctx->step.lists_pinned) hipHostFree(ctx->step.lists_pinned);
    navhip_pool_destroy(ctx);
    nh_async_destroy(ctx);
    for(navhip_layer &L : ctx->layers) {
        for(const plane_row &p : plane_rows) hipFree(nh_member(&L, p.off));
        for(const derived_row &d : derived_rows) hipFree(nh_member(&L, d.off));
        free(L.dirty);
    }
    nh_ctx_each_buf(ctx, [](nh_buf &b) { hipFree(b.p); });
    for(auto &e : ctx->step.ev) if(e) hipEventDestroy(e);
    if(nh_streams_alive(ctx->device))
        for(auto &a : ctx->step.aux) if(a) hipStreamSynchronize(a);   // (borrowed: the process's own set, csrc/stream_set.hip)
    nh_handover_destroy(ctx);
    if(ctx->step.ev_regroup) hipEventDestroy(ctx->step.ev_regroup);
    nh_streams_forget(ctx->device, ctx->stream);
    hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *navhip_last_error(const navhip_ctx *ctx) { return ctx ? ctx->last_error.c_str() : ""; }
int   navhip_device(const navhip_ctx *ctx) { return ctx ? ctx->device : -1; }
void *navhip_stream(const navhip_ctx *ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int navhip_sync(navhip_ctx *ctx)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for(auto a : ctx->step.aux) if(a) HIPCHK(ctx, hipStreamSynchronize(a));       // prefetch side streams
    return NAVHIP_OK;
}

int navhip_get_counters(navhip_ctx *ctx, navhip_counters *out, int reset)
{
    if(!ctx || !out) return NAVHIP_ERR_INVALID;
    *out = ctx->counters;
    if(reset) memset(&ctx->counters, 0, sizeof(ctx->counters));
    return NAVHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// planes
// ---------------------------------------------------------------------------------------------
int navhip_upload_plane(navhip_ctx *ctx, int layer, int plane, const void *host, size_t bytes)
{
    if(!check_layer_plane(ctx, layer, plane) || !host) return NAVHIP_ERR_INVALID;
    return upload_chunks(ctx, layer, plane, 0, ctx->nchunks, true, host, bytes, "navhip_upload_plane");
}

int navhip_upload_chunk(navhip_ctx *ctx, int layer, int plane, int chunk_r, int chunk_c,
                        const void *host, size_t bytes)
{
    if(!check_layer_plane(ctx, layer, plane) || !host
    || chunk_r < 0 || chunk_r >= ctx->h || chunk_c < 0 || chunk_c >= ctx->w)
        return NAVHIP_ERR_INVALID;
    return upload_chunks(ctx, layer, plane, chunk_r * ctx->w + chunk_c, 1, false, host, bytes, "navhip_upload_chunk");
}

void *navhip_plane_dev(navhip_ctx *ctx, int layer, int plane)
{
    return check_layer_plane(ctx, layer, plane) ? plane_slot(ctx->layers[layer], plane) : nullptr;
}

int navhip_download_plane(navhip_ctx *ctx, int layer, int plane, void *host, size_t bytes)
{
    if(!check_layer_plane(ctx, layer, plane) || !host) return NAVHIP_ERR_INVALID;
    const void *src = plane_slot(ctx->layers[layer], plane);
    if(!src) return NAVHIP_ERR_NOT_UPLOADED;
    if(bytes != plane_bytes(ctx, plane)) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NAVHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// dynamic obstacles
// ---------------------------------------------------------------------------------------------
int navhip_blockers_circles_dev(navhip_ctx *ctx, const navhip_circle *dev_circles, int n,
                                float map_pos_x, float map_pos_z, void *stream)
{
    if(!ctx || n < 0 || (n > 0 && !dev_circles)) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    ctx->counters.blocker_circles += (uint64_t)n;
    int rc = nh_refresh_derived(ctx, s);          // the "before" masks must be current
    if(rc) return rc;
    bool any = false;
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++) any |= ctx->layers[l].blockers != nullptr;
    if(!any) {
        ctx->last_error = "navhip_blockers_circles: no blockers plane resident";
        return NAVHIP_ERR_NOT_UPLOADED;
    }
    nh_launch_blockers_circles(ctx, dev_circles, n, map_pos_x, map_pos_z, s);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_blockers_circles(navhip_ctx *ctx, const navhip_circle *circles, int n,
                            float map_pos_x, float map_pos_z)
{
    if(!ctx || n < 0 || (n > 0 && !circles)) return NAVHIP_ERR_INVALID;
    for(int i = 0; i < n; i++) {
        const navhip_circle &c = circles[i];
        if(!(c.radius >= 0.0f) || std::ceil((double)(c.radius / 4)) > 28.0
        || (c.delta != 1 && c.delta != -1) || c.faction_id < 0 || c.faction_id >= NAVHIP_MAX_FACTIONS) {
            ctx->last_error = "navhip_blockers_circles: circle " + std::to_string(i)
                            + " outside the device path (radius > 112, delta != +-1 or bad faction)";
            return NAVHIP_ERR_INVALID;
        }
    }
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const navhip_circle *d_circles;
    int rc = nh_stage_in(ctx, NH_STAGE_CALL0, circles, (size_t)n * sizeof(navhip_circle), (const void**)&d_circles, ctx->stream);
    if(!rc) rc = navhip_blockers_circles_dev(ctx, d_circles, n, map_pos_x, map_pos_z, ctx->stream);
    if(rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NAVHIP_OK;
}

int navhip_relabel_local_islands(navhip_ctx *ctx, int layer)
{
    if(!ctx || layer < 0 || layer >= NAVHIP_NAV_LAYER_MAX) return NAVHIP_ERR_INVALID;
    if(!ctx->layers[layer].cost) return NAVHIP_ERR_NOT_UPLOADED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = layer_prepare(ctx, layer, NAVHIP_PLANE_LOCAL_ISLANDS);
    if(rc) return rc;
    rc = nh_refresh_derived(ctx, ctx->stream);
    if(rc) return rc;
    nh_launch_local_islands(ctx, layer, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NAVHIP_OK;
}

int navhip_changed_chunks(navhip_ctx *ctx, int layer, uint8_t *host_flags, int clear)
{
    if(!ctx || !host_flags || layer < 0 || layer >= NAVHIP_NAV_LAYER_MAX) return NAVHIP_ERR_INVALID;
    navhip_layer &L = ctx->layers[layer];
    if(!L.changed) { memset(host_flags, 0, (size_t)ctx->nchunks); return NAVHIP_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(host_flags, L.changed, (size_t)ctx->nchunks, hipMemcpyDeviceToHost,
                               ctx->stream));
    if(clear) HIPCHK(ctx, hipMemsetAsync(L.changed, 0, (size_t)ctx->nchunks, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NAVHIP_OK;
}

int navhip_faction_changed_chunks(navhip_ctx *ctx, int layer, uint16_t *host_flags, int clear)
{
    if(!ctx || !host_flags || layer < 0 || layer >= NAVHIP_NAV_LAYER_MAX) return NAVHIP_ERR_INVALID;
    navhip_layer &L = ctx->layers[layer];
    const size_t bytes = (size_t)ctx->nchunks * sizeof(uint16_t);
    if(!L.fac_changed) { memset(host_flags, 0, bytes); return NAVHIP_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(host_flags, L.fac_changed, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if(clear) HIPCHK(ctx, hipMemsetAsync(L.fac_changed, 0, bytes, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NAVHIP_OK;
}

int navhip_clear_changed(navhip_ctx *ctx, void *stream)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++) {
        const navhip_layer &L = ctx->layers[l];
        if(L.changed) HIPCHK(ctx, hipMemsetAsync(L.changed, 0, (size_t)ctx->nchunks, s));
        if(L.fac_changed) HIPCHK(ctx, hipMemsetAsync(L.fac_changed, 0, (size_t)ctx->nchunks * sizeof(uint16_t), s));
    }
    return NAVHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// region fields
// ---------------------------------------------------------------------------------------------
int navhip_build_region_fields_dev(navhip_ctx *ctx, const navhip_region_req *dev_reqs, int n,
                                   int max_dim, const int16_t *dev_seeds, const int16_t *dev_overlay,
                                   uint8_t *dev_inout, size_t out_stride, void *stream)
{
    if(!ctx || n < 0 || (n > 0 && (!dev_reqs || !dev_inout)) || max_dim < 2 || max_dim > 128)
        return NAVHIP_ERR_INVALID;
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    ctx->counters.region_fields += (uint64_t)n;
    nh_launch_region_fields(ctx, dev_reqs, n, max_dim, dev_seeds, dev_overlay, dev_inout, out_stride, s);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_build_region_fields(navhip_ctx *ctx, const navhip_region_req *reqs, int n,
                               const int16_t *seeds, size_t n_seeds,
                               const int16_t *overlay, size_t n_overlay,
                               uint8_t *inout, size_t out_stride)
{
    if(!ctx || n < 0 || (n > 0 && (!reqs || !inout))) return NAVHIP_ERR_INVALID;
    if(n == 0) return NAVHIP_OK;
    int max_dim = 0;
    bool any_window = false;
    for(int i = 0; i < n; i++) {
        const navhip_region_req &r = reqs[i];
        bool ok = r.layer < NAVHIP_NAV_LAYER_MAX && r.out_mode <= 1 && r.rdim == r.cdim
               && r.rdim >= 2 && r.rdim <= 128 && (r.rdim % 2) == 0
               && (size_t)r.seed_begin + r.seed_count <= n_seeds
               && (size_t)r.overlay_begin + r.overlay_count <= n_overlay
               && (r.seed_count == 0 || seeds) && (r.overlay_count == 0 || overlay);
        if(ok && r.out_mode == 1)
            ok = r.roff + (r.rdim < 64 ? r.rdim : 64) <= r.rdim && r.coff + (r.cdim < 64 ? r.cdim : 64) <= r.cdim
              && out_stride >= NH_CELLS;
        if(ok && r.out_mode == 0) ok = out_stride >= (size_t)r.rdim * r.cdim / 2;
        if(!ok) {
            ctx->last_error = "navhip_build_region_fields: malformed request " + std::to_string(i);
            return NAVHIP_ERR_INVALID;
        }
        if(!ctx->layers[r.layer].cost) return NAVHIP_ERR_NOT_UPLOADED;
        max_dim = r.rdim > max_dim ? r.rdim : max_dim;
        any_window |= r.out_mode == 1;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t out_bytes = (size_t)n * out_stride;
    const navhip_region_req *d_reqs; const int16_t *d_seeds, *d_overlay;
    uint8_t *d_out = nullptr;
    int rc = nh_stage_in(ctx, NH_STAGE_CALL0, reqs, (size_t)n * sizeof(navhip_region_req), (const void**)&d_reqs, s);
    if(!rc) rc = nh_stage_in(ctx, NH_STAGE_CALL1, seeds, n_seeds * 4, (const void**)&d_seeds, s);
    if(!rc) rc = nh_stage_in(ctx, NH_STAGE_CALL2, overlay, n_overlay * 4, (const void**)&d_overlay, s);
    // (the slots a window request writes into travel with what they hold; whole-region slots are fully written)
    if(!rc) rc = any_window ? nh_stage_in(ctx, NH_STAGE_CALL3, inout, out_bytes, (const void**)&d_out, s)
                            : nh_stage_reserve(ctx, NH_STAGE_CALL3, out_bytes, (void**)&d_out);
    if(!rc) rc = navhip_build_region_fields_dev(ctx, d_reqs, n, max_dim, d_seeds, d_overlay, d_out, out_stride, s);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(inout, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// LOS fields
// ---------------------------------------------------------------------------------------------
int navhip_build_los_dev(navhip_ctx *ctx, const navhip_los_req *dev_reqs, int n,
                         const uint8_t *dev_prev_fields, uint8_t *dev_out_fields,
                         float map_pos_x, float map_pos_z, void *stream)
{
    if(!ctx || n < 0 || (n > 0 && (!dev_reqs || !dev_out_fields))) return NAVHIP_ERR_INVALID;
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    ctx->counters.los_fields += (uint64_t)n;
    uint8_t *d_over = nullptr;                 // the per-request overlay of the two launches
    int rc = nh_stage_reserve(ctx, NH_STAGE_LOS_OVERLAY, (size_t)n, (void**)&d_over);
    if(rc) return rc;
    nh_launch_los(ctx, dev_reqs, n, dev_prev_fields, dev_out_fields, d_over, map_pos_x, map_pos_z, s);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

int navhip_build_los(navhip_ctx *ctx, const navhip_los_req *reqs, int n,
                     const uint8_t *prev_fields, uint8_t *out_fields,
                     float map_pos_x, float map_pos_z)
{
    if(!ctx || n < 0 || (n > 0 && (!reqs || !out_fields))) return NAVHIP_ERR_INVALID;
    if(n == 0) return NAVHIP_OK;
    bool any_prev = false;
    for(int i = 0; i < n; i++) {
        const navhip_los_req &r = reqs[i];
        const bool has_prev = r.prev_dr != 0 || r.prev_dc != 0;
        bool ok = r.layer < NAVHIP_NAV_LAYER_MAX && r.chunk_r < ctx->h && r.chunk_c < ctx->w
               && r.target_chunk_r < ctx->h && r.target_chunk_c < ctx->w
               && r.target_tile_r < 64 && r.target_tile_c < 64
               && (!has_prev || ((r.prev_dr == 0) != (r.prev_dc == 0)
                                 && r.prev_dr >= -1 && r.prev_dr <= 1 && r.prev_dc >= -1 && r.prev_dc <= 1))
               && (has_prev || (r.chunk_r == r.target_chunk_r && r.chunk_c == r.target_chunk_c));
        if(!ok) {
            ctx->last_error = "navhip_build_los: malformed request " + std::to_string(i);
            return NAVHIP_ERR_INVALID;
        }
        if(!ctx->layers[r.layer].cost) return NAVHIP_ERR_NOT_UPLOADED;
        any_prev |= has_prev;
    }
    if(any_prev && !prev_fields) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t field_bytes = (size_t)n * NH_CELLS;
    const navhip_los_req *d_reqs; const uint8_t *d_prev;
    uint8_t *d_out = nullptr;
    int rc = nh_stage_in(ctx, NH_STAGE_CALL0, reqs, (size_t)n * sizeof(navhip_los_req), (const void**)&d_reqs, s);
    // (no request with a predecessor: no copy, and NULL for the kernel, which reads a previous field only for such a request)
    if(!rc) rc = nh_stage_in(ctx, NH_STAGE_CALL1, any_prev ? prev_fields : nullptr, field_bytes, (const void**)&d_prev, s);
    if(!rc) rc = nh_stage_reserve(ctx, NH_STAGE_CALL2, field_bytes, (void**)&d_out);
    if(!rc) rc = navhip_build_los_dev(ctx, d_reqs, n, d_prev, d_out, map_pos_x, map_pos_z, s);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_fields, d_out, field_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// chunk fields, field ids
// ---------------------------------------------------------------------------------------------
int nh_validate_field_reqs(navhip_ctx *ctx, const navhip_field_req *reqs, int n)
{
    for(int i = 0; i < n; i++) {
        const navhip_field_req &r = reqs[i];
        bool ok = r.layer < NAVHIP_NAV_LAYER_MAX && r.chunk_r < ctx->h && r.chunk_c < ctx->w
               && (r.type == NAVHIP_TARGET_TILE || r.type == NAVHIP_TARGET_PORTAL
                || r.type == NAVHIP_TARGET_NEAREST_PATHABLE);
        if(ok && r.type != NAVHIP_TARGET_PORTAL)
            ok = r.tile_r < 64 && r.tile_c < 64;
        if(ok && r.type == NAVHIP_TARGET_PORTAL)
            ok = r.port_r0 <= r.port_r1 && r.port_r1 < 64 && r.port_c0 <= r.port_c1 && r.port_c1 < 64
              && r.next_r0 <= r.next_r1 && r.next_r1 < 64 && r.next_c0 <= r.next_c1 && r.next_c1 < 64
              && r.next_chunk_r < ctx->h && r.next_chunk_c < ctx->w;
        if(!ok) {
            ctx->last_error = "navhip_build_fields: malformed request " + std::to_string(i);
            return NAVHIP_ERR_INVALID;
        }
        const navhip_layer &L = ctx->layers[r.layer];
        if(!L.cost || (r.type == NAVHIP_TARGET_PORTAL && !L.local_islands)
        || ((r.flags & NAVHIP_REQ_ISLAND_NEAREST) && (!L.local_islands || !L.islands))) {
            // (a faction request on a layer without a factions plane is served: nobody can be told from an enemy, so no
            // blocker stops it -- both kernels, and the device entry points always did)
            ctx->last_error = "navhip_build_fields: request " + std::to_string(i)
                            + " needs a plane that was never uploaded";
            return NAVHIP_ERR_NOT_UPLOADED;
        }
    }
    return NAVHIP_OK;
}

int navhip_build_fields_dev(navhip_ctx *ctx, const navhip_field_req *dev_reqs, int n,
                            uint8_t *dev_inout_dirs, float *dev_out_integ, void *stream)
{
    if(!ctx || n < 0 || (n > 0 && (!dev_reqs || !dev_inout_dirs))) return NAVHIP_ERR_INVALID;
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return build_fields_on(ctx, dev_reqs, n, dev_inout_dirs, dev_out_integ, nullptr,
                           stream ? (hipStream_t)stream : ctx->stream);
}

int navhip_build_fields(navhip_ctx *ctx, const navhip_field_req *reqs, int n,
                        uint8_t *inout_dirs, float *out_integ)
{
    if(!ctx || n < 0 || (n > 0 && (!reqs || !inout_dirs))) return NAVHIP_ERR_INVALID;
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = nh_validate_field_reqs(ctx, reqs, n);
    if(rc) return rc;
    hipStream_t s = ctx->stream;
    bool any_inout = false;
    for(int i = 0; i < n; i++)      // skipped (IF_CHANGED) slots must come back unchanged too
        any_inout |= (reqs[i].flags & (NAVHIP_REQ_INOUT | NAVHIP_REQ_IF_CHANGED | NAVHIP_REQ_ISLAND_NEAREST)) != 0
                  || reqs[i].type == NAVHIP_TARGET_NEAREST_PATHABLE;
    const size_t dirs_bytes = (size_t)n * NH_CELLS, integ_bytes = dirs_bytes * sizeof(float);
    const navhip_field_req *d_reqs;
    uint8_t *d_dirs = nullptr;
    float *d_integ = nullptr;
    rc = nh_stage_in(ctx, NH_STAGE_CALL0, reqs, (size_t)n * sizeof(navhip_field_req), (const void**)&d_reqs, s);
    if(!rc) rc = any_inout ? nh_stage_in(ctx, NH_STAGE_CALL1, inout_dirs, dirs_bytes, (const void**)&d_dirs, s)
                           : nh_stage_reserve(ctx, NH_STAGE_CALL1, dirs_bytes, (void**)&d_dirs);
    if(!rc && out_integ) rc = nh_stage_reserve(ctx, NH_STAGE_CALL2, integ_bytes, (void**)&d_integ);
    if(!rc) rc = navhip_build_fields_dev(ctx, d_reqs, n, d_dirs, d_integ, s);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(inout_dirs, d_dirs, dirs_bytes, hipMemcpyDeviceToHost, s));
    if(out_integ) HIPCHK(ctx, hipMemcpyAsync(out_integ, d_integ, integ_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

int navhip_set_field_kernel(navhip_ctx *ctx, int mode)
{
    if(!ctx || mode < 0 || mode > 1) return NAVHIP_ERR_INVALID;
    ctx->field_kernel_mode = mode;
    return NAVHIP_OK;
}

int navhip_last_fields_split(navhip_ctx *ctx, int32_t out[2])
{
    if(!ctx || !out) return NAVHIP_ERR_INVALID;
    if(ctx->last_fields.n < 0) {
        ctx->last_error = "navhip_last_fields_split: no chunk-field build yet";
        return NAVHIP_ERR_INVALID;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int32_t generic = ctx->last_fields.n;           // (forced: no list, k_field_generic built every request)
    if(ctx->last_fields.gen_slot >= 0)
        // the counter the two kernels keep anyway: it stays until the launch after the next one zeroes it
        // (the REQUESTS of the classes on the list, two words behind the list's length)
        HIPCHK(ctx, hipMemcpyAsync(&generic, (const int32_t*)ctx->gen_list.p + 2 + ctx->last_fields.gen_slot, sizeof(int32_t),
                                   hipMemcpyDeviceToHost, ctx->last_fields.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->last_fields.stream));
    out[0] = ctx->last_fields.n - generic; out[1] = generic;
    return NAVHIP_OK;
}

uint64_t navhip_flow_field_id(const navhip_field_req *r)
{
    // N_FlowFieldID, field.c:1952-1975
    if(r->type == NAVHIP_TARGET_PORTAL) {
        return (((uint64_t)r->layer)            << 60)
             | (((uint64_t)r->type)             << 56)
             | (((uint64_t)(r->next_iid & 0xf)) << 48)
             | (((uint64_t)(r->port_iid & 0xf)) << 40)
             | (((uint64_t)r->port_r0)          << 34)
             | (((uint64_t)r->port_c0)          << 28)
             | (((uint64_t)r->port_r1)          << 22)
             | (((uint64_t)r->port_c1)          << 16)
             | (((uint64_t)r->chunk_r)          <<  8)
             | (((uint64_t)r->chunk_c)          <<  0);
    }
    return (((uint64_t)r->layer)   << 60)
         | (((uint64_t)r->type)    << 56)
         | (((uint64_t)r->tile_r)  << 24)
         | (((uint64_t)r->tile_c)  << 16)
         | (((uint64_t)r->chunk_r) <<  8)
         | (((uint64_t)r->chunk_c) <<  0);
}

uint64_t navhip_region_field_id(int kind, int layer, int chunk_r, int chunk_c, uint32_t a, int b, int c)
{
    // N_FlowFieldID, field.c:1976-2003
    const uint64_t head = (((uint64_t)layer) << 60) | (((uint64_t)kind) << 56);
    const uint64_t tail = (((uint64_t)chunk_r) << 8) | ((uint64_t)chunk_c);
    if(kind == NAVHIP_FFID_ENEMIES || kind == NAVHIP_FFID_ENTITY)
        return head | (((uint64_t)a) << 24) | tail;
    if(kind == NAVHIP_FFID_ZONE) {
        const uint32_t cen_chunk_r = a / 64u, cen_tile_r = a % 64u;
        const uint32_t cen_chunk_c = (uint32_t)b / 64u, cen_tile_c = (uint32_t)b % 64u;
        return head | (((uint64_t)(c & 0xff)) << 44) | (((uint64_t)(cen_tile_c & 0x3f)) << 38)
             | (((uint64_t)(cen_tile_r & 0x3f)) << 32) | (((uint64_t)(cen_chunk_c & 0xff)) << 24)
             | (((uint64_t)(cen_chunk_r & 0xff)) << 16) | tail;
    }
    return 0;
}

} // extern "C"
