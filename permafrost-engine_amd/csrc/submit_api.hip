// submit_api.hip -- the asynchronous host-buffer agent step and the page-locked memory of its callers.
//
// submit / poll / wait for the per-tick velocity step of a C host (the reference is C99, it has no device pointers),
// staged through pinned memory, so that the nav task can yield between submit and join like the GL path does
// (movement.c:4212-4233).  Host code only: the step itself is step_api.hip.
#include "navhip_internal.h"
#include "agent_internal.h"

#include <cstring>
#include <iterator>
#include <mutex>

struct nh_async {
    bool        pending = false;
    bool        empty = false;   // the submitted world had no entities: nothing is in flight, poll / wait succeed
    hipEvent_t  done = nullptr;
    // pinned staging: one slab for the inputs, one for the outputs
    char  *h_in = nullptr;  size_t h_in_cap = 0;
    char  *h_out = nullptr; size_t h_out_cap = 0;
    struct cp { void *dst; const void *src; size_t bytes; };
    std::vector<cp> finish;          // staging -> caller copies at completion
    // the attribute tables on the device are those of this epoch / entity count / flock count
    uint32_t static_epoch = 0; int32_t static_n = 0, static_f = 0;
    // what the last submitted step left on the device: its snapshot (device addresses) and its outputs -- the state half
    // of the tick reads them in place (navhip_state_pass_resident)
    bool            resident = false;
    navhip_world    d_world = {};
    navhip_step_out d_out = {};
};

// Asking the runtime what kind of memory a pointer names costs microseconds; a host passes the same page-locked arrays
// every tick: the answers for the last few pointers are remembered, under a mutex (the cache is the process's: contexts on
// several threads share it).  An array freed and reallocated pageable at the same address would be answered stale: that
// only changes the copy path taken (a staged copy of pinned memory, or a direct transfer the runtime stages itself),
// never a result; navhip_host_free forgets its pointer.
static struct { const void *p; bool pinned; } s_pin_cache[32];
static int s_pin_next;
static std::mutex s_pin_mu;            // (the cache is the process's)

bool nh_is_pinned(const void *p)
{
    if(!p) return false;
    std::lock_guard<std::mutex> lock(s_pin_mu);
    for(auto &e : s_pin_cache) if(e.p == p) return e.pinned;
    hipPointerAttribute_t a;
    bool r = false;
    if(hipPointerGetAttributes(&a, p) == hipSuccess) r = a.type == hipMemoryTypeHost;
    else (void)hipGetLastError();
    s_pin_cache[s_pin_next] = {p, r};
    s_pin_next = (s_pin_next + 1) % 32;
    return r;
}

static int pinned_grow(navhip_ctx *ctx, char **p, size_t *cap, size_t need)
{
    if(*cap >= need) return NAVHIP_OK;
    if(*p) HIPCHK(ctx, hipHostFree(*p));
    *p = nullptr; *cap = 0;
    const size_t want = need + need / 2 + 4096;
    HIPCHK(ctx, hipHostMalloc((void**)p, want, hipHostMallocDefault));
    *cap = want;
    return NAVHIP_OK;
}

// One array of the submitted world: where it comes from, and -- after submit_layout -- where it lives on the device.
// Pageable arrays are packed into the pinned slab (one memcpy each) and cross the bus as ONE transfer into one device
// slab -- a dozen separate copies cost a dozen hand-overs to the copy engine, more than the bytes --; page-locked ones
// (navhip_host_alloc) are transferred in place into their own staging slots.  The attribute tables keep their own
// device buffers too and stay there while the caller repeats its static_epoch.
struct submit_in {
    const void *host; size_t bytes; nh_stage_slot slot;
    const void **dev;                 // the member of the device-side navhip_world
    bool attr, early, pinned;         // NH_ROW_ATTR | NH_ROW_EARLY | page-locked: classified ONCE per call
    size_t off;                       // in the slab (when !own())
    bool own() const { return attr || pinned; }        // has a staging slot of its own
    bool front() const { return attr || early; }       // read by the front of the step
};
// ... one output: a pageable one lives in the output slab as its rows [b, e) ...
struct submit_out { void **dev; void *host; size_t row; nh_stage_slot slot; bool pinned; size_t off; };
// ... and one call
struct submit_call {
    navhip_ctx *ctx; nh_async *A; hipStream_t s;
    navhip_world d; navhip_step_out dout;          // the device-side snapshot and outputs (ins / outs point into them)
    std::vector<submit_in> ins; submit_out outs[std::size(nh_out_rows)];
    size_t b, e;                                   // the rows the step works on
    bool attrs_resident;                           // the attribute tables on the device are the caller's: not sent
    char *d_slab = nullptr, *d_oslab = nullptr;    // the device slabs of the pageable inputs and outputs
    size_t sent = 0, oneed = 0;                    // input slab handed to the copy engine so far; bytes of the output slab
};

// The arrays the caller gave, each looked at once
static void submit_classify(submit_call &c, const navhip_world *w, const navhip_step_out *out)
{
    const size_t F = (size_t)w->n_flocks;
    const size_t nmembers = (F > 0 && w->flock_offsets) ? (size_t)w->flock_offsets[F] : 0;
    const bool resident = w->n_field_slots == NAVHIP_POOL_RESIDENT;
    c.ins.reserve(std::size(nh_world_rows));
    for(const nh_world_row &r : nh_world_rows) {
        const void *host = nh_member(w, r.off);
        if(!host || (resident && (r.flags & NH_ROW_NOT_RESIDENT))) continue;
        const bool attr = (r.flags & NH_ROW_ATTR) != 0;
        c.ins.push_back({host, nh_world_row_bytes(r, w, (size_t)c.ctx->nchunks, nmembers), r.slot, (const void**)&nh_member(&c.d, r.off),
                         attr, (r.flags & NH_ROW_EARLY) != 0, !attr && nh_is_pinned(host), 0});
    }
    for(size_t k = 0; k < std::size(nh_out_rows); k++) {
        const nh_out_row &o = nh_out_rows[k];
        void *host = (void*)nh_member(out, o.off);
        c.outs[k] = {&nh_member(&c.dout, o.off), host, o.row_bytes, o.slot, nh_is_pinned(host), 0};
    }
}

// Every staged array gets its final device address, before a byte moves.  Inputs: the front rows first, then the late
// ones, in table order.  Outputs: the same -- one device slab, one transfer, for the pageable ones; a page-locked one
// has a slot of its own, all n rows of it.  (A pageable output lives in the slab as its rows [b, e): the kernels index
// by entity, so the array's device address is the slab position minus b rows.)
static int submit_layout(submit_call &c)
{
    size_t need = 0;
    int rc = NAVHIP_OK;
    for(bool front : {true, false})
        for(auto &it : c.ins) {
            if(rc || it.front() != front) continue;
            if(it.own()) rc = nh_stage_reserve(c.ctx, it.slot, it.bytes, (void**)it.dev);
            else { it.off = need; need += nh_up256(it.bytes); }
        }
    for(auto &o : c.outs) if(o.host && !o.pinned) { o.off = c.oneed; c.oneed += nh_up256((c.e - c.b) * o.row); }
    if(!rc) rc = pinned_grow(c.ctx, &c.A->h_in, &c.A->h_in_cap, need);
    if(!rc) rc = pinned_grow(c.ctx, &c.A->h_out, &c.A->h_out_cap, c.oneed);
    if(!rc && need) rc = nh_stage_reserve(c.ctx, NH_STAGE_SUBMIT_IN, need, (void**)&c.d_slab);
    if(!rc && c.oneed) rc = nh_stage_reserve(c.ctx, NH_STAGE_SUBMIT_OUT, c.oneed, (void**)&c.d_oslab);
    for(auto &it : c.ins) if(!it.own()) *it.dev = c.d_slab + it.off;
    for(auto &o : c.outs) {
        if(rc || !o.host) continue;
        if(o.pinned) rc = nh_stage_reserve(c.ctx, o.slot, (size_t)c.d.n_ents * o.row, o.dev);
        else *o.dev = c.d_oslab + o.off - c.b * o.row;
    }
    return rc;
}

// what has been packed into the input slab in front of `upto`, to the copy engine
static int submit_flush(submit_call &c, size_t upto)
{
    if(upto > c.sent) HIPCHK(c.ctx, hipMemcpyAsync(c.d_slab + c.sent, c.A->h_in + c.sent, upto - c.sent, hipMemcpyHostToDevice, c.s));
    c.sent = upto;
    return NAVHIP_OK;
}

// The front rows, or the late ones, on their way
static int submit_send(submit_call &c, bool front)
{
    size_t off = c.sent;
    for(auto &it : c.ins) {
        if(it.front() != front || (it.attr && c.attrs_resident)) continue;
        if(it.own()) {
            if(it.bytes) HIPCHK(c.ctx, hipMemcpyAsync((void*)*it.dev, it.host, it.bytes, hipMemcpyHostToDevice, c.s));
            continue;
        }
        if(it.bytes) memcpy(c.A->h_in + it.off, it.host, it.bytes);
        off = it.off + nh_up256(it.bytes);
        // hand what has been packed to the copy engine about every megabyte: it moves that part while the next one is packed
        if(off - c.sent >= ((size_t)1 << 20)) { int rc = submit_flush(c, off); if(rc) return rc; }
    }
    return submit_flush(c, off);
}

// The outputs on their way back behind the step: page-locked ones in place, the slab into its pinned twin, from where
// async_finish hands the rows out (A->finish)
static int submit_fetch(submit_call &c)
{
    c.A->finish.clear();
    for(auto &o : c.outs) {
        if(!o.host || c.e <= c.b) continue;
        const size_t bytes = (c.e - c.b) * o.row;
        char *dst = (char*)o.host + c.b * o.row;
        if(o.pinned) HIPCHK(c.ctx, hipMemcpyAsync(dst, (char*)*o.dev + c.b * o.row, bytes, hipMemcpyDeviceToHost, c.s));
        else c.A->finish.push_back({dst, c.A->h_out + o.off, bytes});
    }
    if(c.oneed) HIPCHK(c.ctx, hipMemcpyAsync(c.A->h_out, c.d_oslab, c.oneed, hipMemcpyDeviceToHost, c.s));
    return NAVHIP_OK;
}

extern "C" {

void *navhip_host_alloc(size_t bytes)
{
    void *p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void navhip_host_free(void *p)
{
    if(!p) return;
    { std::lock_guard<std::mutex> lock(s_pin_mu); for(auto &e : s_pin_cache) if(e.p == p) e.p = nullptr; }
    hipHostFree(p);
}

int navhip_agent_step_submit(navhip_ctx *ctx, const navhip_world *w, const navhip_step_out *out)
{
    if(!ctx || !w || !out || !out->vel_xz || w->n_ents < 0) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if(!ctx->async) {
        ctx->async = new (std::nothrow) nh_async();
        if(!ctx->async) return NAVHIP_ERR_NOMEM;
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->async->done, hipEventDisableTiming));
    }
    nh_async *A = ctx->async;
    if(A->pending) { ctx->last_error = "navhip_agent_step_submit: a step is already in flight"; return NAVHIP_ERR_INVALID; }
    A->resident = false;
    A->empty = w->n_ents == 0;      // an empty world is a valid tick: submit / poll / wait all succeed
    if(A->empty) { A->finish.clear(); A->pending = true; return NAVHIP_OK; }
    submit_call c = {ctx, A, ctx->stream, *w, {nullptr, nullptr, nullptr, nullptr, nullptr}};
    c.b = (size_t)w->work_begin; c.e = (size_t)w->work_end;
    if(c.b == 0 && c.e == 0) c.e = (size_t)w->n_ents;
    c.attrs_resident = w->static_epoch != 0 && w->static_epoch == A->static_epoch
                       && A->static_n == w->n_ents && A->static_f == w->n_flocks;
    submit_classify(c, w, out);
    // Two phases: what the front of the step reads (positions, velocities, states, the attribute tables) goes first and
    // the front is started on it -- it is handed the final device addresses of the late arrays before their contents
    // arrive --; the rest is packed and transferred while the spatial hash, the neighbour walk and the cohesion term run.
    int rc = submit_layout(c);
    if(!rc) rc = submit_send(c, true);
    if(!rc) rc = navhip_agent_prefetch_dev(ctx, &c.d, c.s);
    if(!rc) rc = submit_send(c, false);
    if(rc) return rc;
    A->static_epoch = w->static_epoch; A->static_n = w->n_ents; A->static_f = w->n_flocks;
    rc = navhip_agent_step_dev(ctx, &c.d, &c.dout, c.s);
    if(!rc) rc = submit_fetch(c);
    if(rc) return rc;
    HIPCHK(ctx, hipEventRecord(A->done, c.s));
    A->pending = true;
    A->d_world = c.d; A->d_out = c.dout; A->resident = true;
    return NAVHIP_OK;
}

static int async_finish(navhip_ctx *ctx)
{
    nh_async *A = ctx->async;
    for(auto &c : A->finish) memcpy(c.dst, c.src, c.bytes);
    A->finish.clear();
    A->pending = false;
    return NAVHIP_OK;
}

int navhip_agent_step_poll(navhip_ctx *ctx)
{
    if(!ctx || !ctx->async || !ctx->async->pending) return NAVHIP_ERR_INVALID;
    if(ctx->async->empty) return async_finish(ctx);
    hipError_t e = hipEventQuery(ctx->async->done);
    if(e == hipErrorNotReady) return 1;
    if(e != hipSuccess) { ctx->last_error = std::string("navhip_agent_step_poll: ") + hipGetErrorString(e); return NAVHIP_ERR_DEVICE; }
    return async_finish(ctx);
}

int navhip_agent_step_wait(navhip_ctx *ctx)
{
    if(!ctx || !ctx->async || !ctx->async->pending) return NAVHIP_ERR_INVALID;
    if(ctx->async->empty) return async_finish(ctx);
    // a step takes a few hundred microseconds: poll for that long (a blocking wait costs a wake-up of
    // tens of microseconds), then block
    for(int spin = 0; spin < 20000; spin++) {
        const hipError_t e = hipEventQuery(ctx->async->done);
        if(e == hipSuccess) return async_finish(ctx);
        if(e != hipErrorNotReady) break;
    }
    HIPCHK(ctx, hipEventSynchronize(ctx->async->done));
    return async_finish(ctx);
}

}  // extern "C"

void nh_async_invalidate_static(navhip_ctx *ctx) { if(ctx->async) { ctx->async->static_epoch = 0; ctx->async->resident = false; } }

// the device-side snapshot and outputs of the last COMPLETED host-buffer step (false: none, or still in flight)
bool nh_async_resident(navhip_ctx *ctx, navhip_world *w, navhip_step_out *o)
{
    nh_async *A = ctx->async;
    if(!A || !A->resident || A->pending || A->empty) return false;
    *w = A->d_world; *o = A->d_out;
    return true;
}

// its two pinned staging slabs, grown to the sizes asked for (the step is complete: nobody reads them)
int nh_async_slabs(navhip_ctx *ctx, size_t in_bytes, size_t out_bytes, char **h_in, char **h_out)
{
    nh_async *A = ctx->async;
    if(!A || A->pending) return NAVHIP_ERR_INVALID;
    int rc = pinned_grow(ctx, &A->h_in, &A->h_in_cap, in_bytes);
    if(!rc) rc = pinned_grow(ctx, &A->h_out, &A->h_out_cap, out_bytes);
    if(rc) return rc;
    *h_in = A->h_in; *h_out = A->h_out;
    return NAVHIP_OK;
}

void nh_async_destroy(navhip_ctx *ctx)
{
    if(!ctx->async) return;
    for(char *p : {ctx->async->h_in, ctx->async->h_out}) if(p) hipHostFree(p);
    hipEventDestroy(ctx->async->done);
    delete ctx->async;
    ctx->async = nullptr;
}
