// navhip_api.hip -- the C ABI of libnavhip.so (include/navhip.h): context, map-plane
// residency in HBM, and the host-/device-buffer entry points that launch the kernels.
//
// Data layout in HBM (per nav layer, allocated on first upload; sized for the reference's
// maximum 64x64-chunk map this is 64 MB cost + 128 MB blockers + 128 MB local islands +
// 960 MB factions -- a fraction of the 288 GB part, so everything stays resident):
//   cost          u8  [chunks][64][64]       struct nav_chunk.cost_base      nav_data.h:123
//   blockers      u16 [chunks][64][64]       struct nav_chunk.blockers       nav_data.h:134
//   local_islands u16 [chunks][64][64]       struct nav_chunk.local_islands  nav_data.h:157
//   factions      u8  [chunks][15][64][64]   struct nav_chunk.factions       nav_data.h:141
//   passmask      u64 [chunks][64]           derived: row bitmasks of field_tile_passable
//   probemask     u64 [chunks][64][2]        derived: row bitmasks cost_base != 0xff | blockers > 0 (tile probes)
//   facmask       u64 [chunks][15][64]       derived: row bitmasks factions[f] != 0 (attacking-path fields); with the
//   facany        u16 [chunks]               derived: factions present in the chunk      factions plane only
//   unit_cost     u8  [chunks]               derived: BFS kernel eligibility
#include "navhip_internal.h"
#include "agent_internal.h"
#include "agent_thread.h"
#include <cmath>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <new>
#include <vector>

static size_t plane_elem_bytes(int plane)
{
    switch(plane) {
    case NAVHIP_PLANE_COST_BASE:     return 1;
    case NAVHIP_PLANE_BLOCKERS:      return 2;
    case NAVHIP_PLANE_LOCAL_ISLANDS: return 2;
    case NAVHIP_PLANE_FACTIONS:      return NAVHIP_MAX_FACTIONS;
    case NAVHIP_PLANE_ISLANDS:       return 2;
    default: return 0;
    }
}

static void **plane_slot(navhip_layer &L, int plane)
{
    switch(plane) {
    case NAVHIP_PLANE_COST_BASE:     return (void**)&L.cost;
    case NAVHIP_PLANE_BLOCKERS:      return (void**)&L.blockers;
    case NAVHIP_PLANE_LOCAL_ISLANDS: return (void**)&L.local_islands;
    case NAVHIP_PLANE_FACTIONS:      return (void**)&L.factions;
    case NAVHIP_PLANE_ISLANDS:       return (void**)&L.islands;
    default: return nullptr;
    }
}

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

// the step's scratch and the staging slots: at least 16 bytes, and a buffer that moved is counted (scratch_moves)
int nh_ensure_buf(navhip_ctx *ctx, nh_buf &b, size_t need)
{
    const void *old = b.p;
    int rc = nh_ensure(ctx, b, need ? need : 16);
    if(b.p != old) ctx->step.scratch_moves++;
    return rc;
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
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++) {
        navhip_layer &L = ctx->layers[l];
        hipFree(L.cost); hipFree(L.blockers); hipFree(L.local_islands); hipFree(L.factions);
        hipFree(L.islands);
        hipFree(L.passmask); hipFree(L.probemask); hipFree(L.unit_cost); hipFree(L.touched); hipFree(L.changed);
        hipFree(L.facmask); hipFree(L.facany); hipFree(L.fac_touched);
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

int navhip_stream_beside(navhip_ctx *ctx, void *main_stream, int cu_begin, int cu_count, void **out_stream)
{
    if(!ctx || !out_stream || cu_begin < 0) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = nullptr;
    if(cu_count <= 0) {
        hipStream_t all[NH_STREAM_FIXED];
        int rc = nh_streams_for(ctx, (hipStream_t)main_stream, all);
        if(rc) return rc;
        st = all[NH_STREAM_FIELDS];
    }else{
        st = nh_stream_partial_for(ctx, (hipStream_t)main_stream, cu_begin, cu_count);
        if(!st) return ctx->last_error.empty() ? NAVHIP_ERR_INVALID : NAVHIP_ERR_DEVICE;
    }
    *out_stream = (void*)st;
    return NAVHIP_OK;
}

int navhip_stream_main(navhip_ctx *ctx, void **out_stream)
{
    if(!ctx || !out_stream) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t all[NH_STREAM_FIXED];
    int rc = nh_streams_for(ctx, nullptr, all);
    if(rc) return rc;
    *out_stream = (void*)all[NH_STREAM_MAIN];
    return NAVHIP_OK;
}

int navhip_stream_create_partial(navhip_ctx *ctx, int cu_begin, int cu_count, void **out_stream)
{
    if(cu_count <= 0) return NAVHIP_ERR_INVALID;
    return navhip_stream_beside(ctx, ctx ? (void*)ctx->stream : nullptr, cu_begin, cu_count, out_stream);
}

int navhip_sync(navhip_ctx *ctx)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for(auto a : ctx->step.aux) if(a) HIPCHK(ctx, hipStreamSynchronize(a));       // prefetch side streams
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
        HIPCHK(ctx, hipMemcpyAsync(&generic, (const int32_t*)ctx->gen_list.p + ctx->last_fields.gen_slot, sizeof(int32_t),
                                   hipMemcpyDeviceToHost, ctx->last_fields.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->last_fields.stream));
    out[0] = ctx->last_fields.n - generic; out[1] = generic;
    return NAVHIP_OK;
}

static int layer_prepare(navhip_ctx *ctx, int layer, int plane)
{
    navhip_layer &L = ctx->layers[layer];
    void **slot = plane_slot(L, plane);
    if(!*slot) {
        size_t bytes = (size_t)ctx->nchunks * NH_CELLS * plane_elem_bytes(plane);
        HIPCHK(ctx, hipMalloc(slot, bytes));
        if(plane != NAVHIP_PLANE_COST_BASE)
            HIPCHK(ctx, hipMemsetAsync(*slot, 0, bytes, ctx->stream));
    }
    if(!L.passmask) {
        HIPCHK(ctx, hipMalloc((void**)&L.passmask, (size_t)ctx->nchunks * 64 * sizeof(uint64_t)));
        HIPCHK(ctx, hipMalloc((void**)&L.probemask, (size_t)ctx->nchunks * 128 * sizeof(uint64_t)));
        HIPCHK(ctx, hipMalloc((void**)&L.unit_cost, (size_t)ctx->nchunks));
        HIPCHK(ctx, hipMalloc((void**)&L.touched, (size_t)ctx->nchunks));
        HIPCHK(ctx, hipMalloc((void**)&L.changed, (size_t)ctx->nchunks));
        HIPCHK(ctx, hipMemsetAsync(L.touched, 0, (size_t)ctx->nchunks, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(L.changed, 0, (size_t)ctx->nchunks, ctx->stream));
        L.dirty = (uint8_t*)calloc(ctx->nchunks, 1);
        if(!L.dirty) return NAVHIP_ERR_NOMEM;
    }
    if(L.factions && !L.facmask) {
        // the derived rows of the factions plane (all zero, like the plane itself until its first upload)
        const size_t rows = (size_t)ctx->nchunks * NAVHIP_MAX_FACTIONS * 64 * sizeof(uint64_t);
        HIPCHK(ctx, hipMalloc((void**)&L.facmask, rows));
        HIPCHK(ctx, hipMalloc((void**)&L.facany, (size_t)ctx->nchunks * sizeof(uint16_t)));
        HIPCHK(ctx, hipMalloc((void**)&L.fac_touched, (size_t)ctx->nchunks * sizeof(uint32_t)));
        HIPCHK(ctx, hipMemsetAsync(L.facmask, 0, rows, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(L.facany, 0, (size_t)ctx->nchunks * sizeof(uint16_t), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(L.fac_touched, 0, (size_t)ctx->nchunks * sizeof(uint32_t), ctx->stream));
    }
    return NAVHIP_OK;
}

int navhip_upload_plane(navhip_ctx *ctx, int layer, int plane, const void *host, size_t bytes)
{
    if(!ctx || !host || layer < 0 || layer >= NAVHIP_NAV_LAYER_MAX
    || plane < 0 || plane >= NAVHIP_PLANE_COUNT)
        return NAVHIP_ERR_INVALID;
    size_t want = (size_t)ctx->nchunks * NH_CELLS * plane_elem_bytes(plane);
    if(bytes != want) {
        ctx->last_error = "navhip_upload_plane: size mismatch";
        return NAVHIP_ERR_INVALID;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = layer_prepare(ctx, layer, plane);
    if(rc) return rc;
    navhip_layer &L = ctx->layers[layer];
    HIPCHK(ctx, hipMemcpyAsync(*plane_slot(L, plane), host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // caller may reuse `host` immediately
    if(plane == NAVHIP_PLANE_COST_BASE || plane == NAVHIP_PLANE_BLOCKERS || plane == NAVHIP_PLANE_FACTIONS) {
        memset(L.dirty, 1, ctx->nchunks);
        L.any_dirty = true;
    }
    if(plane == NAVHIP_PLANE_COST_BASE) {
        // does the layer hold costs other than 1 / impassable?  (The reference's cost writers produce no
        // others, nav.c:339-342,416; a host that does sends its requests to the relaxation kernel, whose
        // launch is then sized for real work instead of for an empty list.)
        const uint8_t *c = (const uint8_t*)host;
        bool other = false;
        for(size_t i = 0; i < bytes && !other; i++) other = c[i] != 1 && c[i] != NAVHIP_COST_IMPASSABLE;
        L.nonunit_costs = other;
    }
    return NAVHIP_OK;
}

int navhip_upload_chunk(navhip_ctx *ctx, int layer, int plane, int chunk_r, int chunk_c,
                        const void *host, size_t bytes)
{
    if(!ctx || !host || layer < 0 || layer >= NAVHIP_NAV_LAYER_MAX
    || plane < 0 || plane >= NAVHIP_PLANE_COUNT
    || chunk_r < 0 || chunk_r >= ctx->h || chunk_c < 0 || chunk_c >= ctx->w)
        return NAVHIP_ERR_INVALID;
    size_t per = (size_t)NH_CELLS * plane_elem_bytes(plane);
    if(bytes != per) {
        ctx->last_error = "navhip_upload_chunk: size mismatch";
        return NAVHIP_ERR_INVALID;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = layer_prepare(ctx, layer, plane);
    if(rc) return rc;
    navhip_layer &L = ctx->layers[layer];
    int chunk = chunk_r * ctx->w + chunk_c;
    if(plane == NAVHIP_PLANE_COST_BASE) {
        const uint8_t *c = (const uint8_t*)host;
        for(size_t i = 0; i < per; i++) if(c[i] != 1 && c[i] != NAVHIP_COST_IMPASSABLE) { L.nonunit_costs = true; break; }
    }
    HIPCHK(ctx, hipMemcpyAsync((char*)*plane_slot(L, plane) + (size_t)chunk * per, host, per,
                               hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if(plane == NAVHIP_PLANE_COST_BASE || plane == NAVHIP_PLANE_BLOCKERS || plane == NAVHIP_PLANE_FACTIONS) {
        L.dirty[chunk] = 1;
        L.any_dirty = true;
    }
    return NAVHIP_OK;
}

void *navhip_plane_dev(navhip_ctx *ctx, int layer, int plane)
{
    if(!ctx || layer < 0 || layer >= NAVHIP_NAV_LAYER_MAX || plane < 0 || plane >= NAVHIP_PLANE_COUNT)
        return nullptr;
    return *plane_slot(ctx->layers[layer], plane);
}

int navhip_download_plane(navhip_ctx *ctx, int layer, int plane, void *host, size_t bytes)
{
    if(!ctx || !host || layer < 0 || layer >= NAVHIP_NAV_LAYER_MAX
    || plane < 0 || plane >= NAVHIP_PLANE_COUNT)
        return NAVHIP_ERR_INVALID;
    void *src = *plane_slot(ctx->layers[layer], plane);
    if(!src) return NAVHIP_ERR_NOT_UPLOADED;
    if(bytes != (size_t)ctx->nchunks * NH_CELLS * plane_elem_bytes(plane)) return NAVHIP_ERR_INVALID;
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
    nh_buf &d_circles = ctx->stage[NH_STAGE_CALL0];
    int rc = nh_ensure_buf(ctx, d_circles, (size_t)n * sizeof(navhip_circle));
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_circles.p, circles, (size_t)n * sizeof(navhip_circle),
                               hipMemcpyHostToDevice, ctx->stream));
    rc = navhip_blockers_circles_dev(ctx, (const navhip_circle*)d_circles.p, n, map_pos_x,
                                     map_pos_z, ctx->stream);
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

int navhip_clear_changed(navhip_ctx *ctx, void *stream)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    for(int l = 0; l < NAVHIP_NAV_LAYER_MAX; l++)
        if(ctx->layers[l].changed)
            HIPCHK(ctx, hipMemsetAsync(ctx->layers[l].changed, 0, (size_t)ctx->nchunks, s));
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
    nh_buf &d_reqs = ctx->stage[NH_STAGE_CALL0], &d_seeds = ctx->stage[NH_STAGE_CALL1];
    nh_buf &d_overlay = ctx->stage[NH_STAGE_CALL2], &d_out = ctx->stage[NH_STAGE_CALL3];
    int rc = nh_ensure_buf(ctx, d_reqs, (size_t)n * sizeof(navhip_region_req));
    if(!rc) rc = nh_ensure_buf(ctx, d_seeds, n_seeds * 4);
    if(!rc) rc = nh_ensure_buf(ctx, d_overlay, n_overlay * 4);
    if(!rc) rc = nh_ensure_buf(ctx, d_out, (size_t)n * out_stride);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_reqs.p, reqs, (size_t)n * sizeof(navhip_region_req), hipMemcpyHostToDevice, s));
    if(n_seeds) HIPCHK(ctx, hipMemcpyAsync(d_seeds.p, seeds, n_seeds * 4, hipMemcpyHostToDevice, s));
    if(n_overlay) HIPCHK(ctx, hipMemcpyAsync(d_overlay.p, overlay, n_overlay * 4, hipMemcpyHostToDevice, s));
    if(any_window)
        HIPCHK(ctx, hipMemcpyAsync(d_out.p, inout, (size_t)n * out_stride, hipMemcpyHostToDevice, s));
    rc = navhip_build_region_fields_dev(ctx, (const navhip_region_req*)d_reqs.p, n, max_dim,
                                        (const int16_t*)d_seeds.p, (const int16_t*)d_overlay.p,
                                        (uint8_t*)d_out.p, out_stride, s);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(inout, d_out.p, (size_t)n * out_stride, hipMemcpyDeviceToHost, s));
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
    nh_buf &d_reqs = ctx->stage[NH_STAGE_CALL0], &d_prev = ctx->stage[NH_STAGE_CALL1], &d_out = ctx->stage[NH_STAGE_CALL2];
    int rc = nh_ensure_buf(ctx, d_reqs, (size_t)n * sizeof(navhip_los_req));
    if(!rc) rc = nh_ensure_buf(ctx, d_prev, (size_t)n * NH_CELLS);
    if(!rc) rc = nh_ensure_buf(ctx, d_out, (size_t)n * NH_CELLS);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(d_reqs.p, reqs, (size_t)n * sizeof(navhip_los_req), hipMemcpyHostToDevice, s));
    if(any_prev)
        HIPCHK(ctx, hipMemcpyAsync(d_prev.p, prev_fields, (size_t)n * NH_CELLS, hipMemcpyHostToDevice, s));
    rc = navhip_build_los_dev(ctx, (const navhip_los_req*)d_reqs.p, n, (const uint8_t*)d_prev.p, (uint8_t*)d_out.p,
                              map_pos_x, map_pos_z, s);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_fields, d_out.p, (size_t)n * NH_CELLS, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

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

static int build_fields_on(navhip_ctx *ctx, const navhip_field_req *dev_reqs, int n, uint8_t *dev_inout_dirs,
                           float *dev_out_integ, const int32_t *dev_slots, hipStream_t s)
{
    int rc = nh_refresh_derived(ctx, s);
    if(rc) return rc;
    // work list of the generic kernel: the header is zero between launches (the kernel resets it)
    const void *old_list = ctx->gen_list.p;
    rc = nh_ensure_buf(ctx, ctx->gen_list, ((size_t)n + 2) * sizeof(int32_t));
    if(rc) return rc;
    if(ctx->gen_list.p != old_list) HIPCHK(ctx, hipMemsetAsync(ctx->gen_list.p, 0, 2 * sizeof(int32_t), s));
    ctx->last_fields.gen_slot = nh_launch_fields(ctx, dev_reqs, n, dev_inout_dirs, dev_out_integ, (int32_t*)ctx->gen_list.p,
                                                 s, dev_slots);
    ctx->last_fields.n = n; ctx->last_fields.stream = s;
    HIPCHK(ctx, hipGetLastError());
    ctx->counters.field_calls++; ctx->counters.chunk_fields += (uint64_t)n;
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

}  // extern "C"

// request i is built into slot dev_slots[i] of dev_fields (navhip_pool_build)
int navhip_build_fields_slots_dev(navhip_ctx *ctx, const navhip_field_req *dev_reqs, int n, uint8_t *dev_fields,
                                  const int32_t *dev_slots, hipStream_t s)
{
    if(n == 0) return NAVHIP_OK;
    return build_fields_on(ctx, dev_reqs, n, dev_fields, nullptr, dev_slots, s);
}

int nh_stage_reserve(navhip_ctx *ctx, nh_stage_slot slot, size_t bytes, void **dev)
{
    int rc = nh_ensure_buf(ctx, ctx->stage[slot], bytes);
    if(rc) return rc;
    *dev = ctx->stage[slot].p;
    return NAVHIP_OK;
}

extern "C" {

int navhip_build_fields(navhip_ctx *ctx, const navhip_field_req *reqs, int n,
                        uint8_t *inout_dirs, float *out_integ)
{
    if(!ctx || n < 0 || (n > 0 && (!reqs || !inout_dirs))) return NAVHIP_ERR_INVALID;
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = nh_validate_field_reqs(ctx, reqs, n);
    if(rc) return rc;
    hipStream_t s = ctx->stream;
    nh_buf &d_reqs = ctx->stage[NH_STAGE_CALL0], &d_dirs_buf = ctx->stage[NH_STAGE_CALL1], &d_integ_buf = ctx->stage[NH_STAGE_CALL2];
    rc = nh_ensure_buf(ctx, d_reqs, (size_t)n * sizeof(navhip_field_req));
    if(!rc) rc = nh_ensure_buf(ctx, d_dirs_buf, (size_t)n * NH_CELLS);
    if(!rc && out_integ) rc = nh_ensure_buf(ctx, d_integ_buf, (size_t)n * NH_CELLS * sizeof(float));
    if(rc) return rc;
    uint8_t *d_dirs = (uint8_t*)d_dirs_buf.p;
    float *d_integ = out_integ ? (float*)d_integ_buf.p : nullptr;
    HIPCHK(ctx, hipMemcpyAsync(d_reqs.p, reqs, (size_t)n * sizeof(navhip_field_req),
                               hipMemcpyHostToDevice, s));
    bool any_inout = false;
    for(int i = 0; i < n; i++)      // skipped (IF_CHANGED) slots must come back unchanged too
        any_inout |= (reqs[i].flags & (NAVHIP_REQ_INOUT | NAVHIP_REQ_IF_CHANGED | NAVHIP_REQ_ISLAND_NEAREST)) != 0
                  || reqs[i].type == NAVHIP_TARGET_NEAREST_PATHABLE;
    if(any_inout)
        HIPCHK(ctx, hipMemcpyAsync(d_dirs, inout_dirs, (size_t)n * NH_CELLS,
                                   hipMemcpyHostToDevice, s));
    rc = navhip_build_fields_dev(ctx, (const navhip_field_req*)d_reqs.p, n, d_dirs, d_integ, s);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(inout_dirs, d_dirs, (size_t)n * NH_CELLS,
                               hipMemcpyDeviceToHost, s));
    if(out_integ)
        HIPCHK(ctx, hipMemcpyAsync(out_integ, d_integ, (size_t)n * NH_CELLS * sizeof(float),
                                   hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return NAVHIP_OK;
}

int navhip_get_counters(navhip_ctx *ctx, navhip_counters *out, int reset)
{
    if(!ctx || !out) return NAVHIP_ERR_INVALID;
    *out = ctx->counters;
    if(reset) memset(&ctx->counters, 0, sizeof(ctx->counters));
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

// ---------------------------------------------------------------------------------------------
// ClearPath batches, field ids
// ---------------------------------------------------------------------------------------------
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
