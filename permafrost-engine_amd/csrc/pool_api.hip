// pool_api.hip -- the resident flow-field pool.
//
// What a C host (the reference is C99, it has no device pointers) needs so that the host-buffer entry points do not move
// the whole field cache over PCIe on every call: a field pool that STAYS in HBM, keyed by the reference's own 64-bit
// flow-field ids (N_FlowFieldID, field.c:1952), with the same put / contains / dest-mapping operations as the reference's
// field cache (N_FC_PutFlowField, N_FC_ContainsFlowField, N_FC_PutDestFFMapping, fieldcache.c); batched builds write
// straight into pool slots.  (The other half of that host's tick, the asynchronous velocity step, is submit_api.hip.)
#include "navhip_internal.h"

#include <list>
#include <unordered_map>

// the field of slot `slot` in a pool's [n_slots][4096] array (constexpr: callable from the host and from the kernels)
static constexpr uint8_t *pool_field(uint8_t *fields, int slot) { return fields + (size_t)slot * NH_CELLS; }

struct nh_pool {
    int       n_slots = 0, n_dests = 0, nchunks = 0;
    uint8_t  *d_fields = nullptr;       // [n_slots][4096]
    int32_t  *d_map = nullptr;          // [n_dests][nchunks] slot of the (dest, chunk) field, -1 = none
    std::vector<int32_t>  h_map;
    std::vector<uint64_t> id_of;        // per slot (valid when used[slot])
    std::vector<uint8_t>  used;
    std::unordered_map<uint64_t, int> slot_of;
    std::list<int> lru;                 // front = most recently used
    std::vector<std::list<int>::iterator> lru_it;   // per slot (lru.end(): not in the list yet)
    std::vector<std::vector<int64_t>> refs;   // per slot: map entries that point at it
    // scratch
    nh_buf d_reqs, d_slots;             // requests and slot lists of a build
    nh_buf d_upd;                       // (index, value) pairs of map updates
    std::vector<int32_t> pending;       // host list of (index, value) map updates not yet on the device
};

__global__ void k_scatter_i32(int32_t *dst, const int32_t *pairs, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if(i < n) dst[pairs[2 * i]] = pairs[2 * i + 1];
}

__global__ void k_copy_field(uint8_t *fields, const int32_t *src_dst, int n)
{
    // one workgroup of 256 threads per 4 KB field: 16 bytes per thread
    const int i = blockIdx.x;
    if(i >= n) return;
    const uint4 *s = (const uint4*)pool_field(fields, src_dst[2 * i]);
    uint4 *d = (uint4*)pool_field(fields, src_dst[2 * i + 1]);
    d[threadIdx.x] = s[threadIdx.x];
}

__global__ void k_zero_fields(uint8_t *fields, const int32_t *slots, int n)
{
    const int i = blockIdx.x;
    if(i >= n) return;
    ((uint4*)pool_field(fields, slots[i]))[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

// `slot` to an end of the LRU list: the front is the most recently used, the back is what the next new id takes
static void pool_lru_move(nh_pool *P, int slot, bool to_front)
{
    if(P->lru_it[slot] != P->lru.end()) P->lru.erase(P->lru_it[slot]);
    P->lru_it[slot] = P->lru.insert(to_front ? P->lru.begin() : P->lru.end(), slot);
}

// drop the field of `slot`, by eviction, invalidation or a failed build: every (dest, chunk) mapping that still points
// at it becomes "no field" (queued for pool_flush_map), its id is registered no more -- no id is ever left registered
// for a slot whose field was not built -- and the slot is free again
static void pool_drop_slot(nh_pool *P, int slot)
{
    if(!P->used[slot]) return;
    for(int64_t e : P->refs[slot]) {
        if(P->h_map[(size_t)e] != slot) continue;
        P->h_map[(size_t)e] = -1;
        P->pending.push_back((int32_t)e); P->pending.push_back(-1);
    }
    P->refs[slot].clear();
    P->slot_of.erase(P->id_of[slot]);
    P->used[slot] = 0;
    pool_lru_move(P, slot, false);     // least recently used again: the next new id takes it first
}

// slot of ff_id, taking the least recently used one when it is new (*fresh = the slot holds nothing of this id yet).
// `pinned`: slots that must not be evicted (used by the batch in flight).
static int pool_slot_for(nh_pool *P, uint64_t id, bool *fresh, const std::vector<uint8_t> *pinned)
{
    auto it = P->slot_of.find(id);
    *fresh = it == P->slot_of.end();
    if(!*fresh) { pool_lru_move(P, it->second, true); return it->second; }
    int slot = -1;
    for(auto r = P->lru.rbegin(); r != P->lru.rend(); ++r)
        if(!pinned || !(*pinned)[*r]) { slot = *r; break; }
    if(slot < 0) return -1;
    pool_drop_slot(P, slot);        // evict what it holds
    P->used[slot] = 1;
    P->id_of[slot] = id;
    P->slot_of[id] = slot;
    pool_lru_move(P, slot, true);
    return slot;
}

static int pool_flush_map(navhip_ctx *ctx, nh_pool *P, hipStream_t s)
{
    if(P->pending.empty()) return NAVHIP_OK;
    // one update per table entry: the scatter kernel applies the pairs in parallel, so two updates of the same entry in
    // one launch (a chunk re-mapped twice between two flushes) would race -- the LAST one is the one that counts
    std::unordered_map<int32_t, size_t> last;
    for(size_t i = 0; i + 1 < P->pending.size(); i += 2) last[P->pending[i]] = i;
    if(last.size() * 2 != P->pending.size()) {
        std::vector<int32_t> uniq;
        for(size_t i = 0; i + 1 < P->pending.size(); i += 2)
            if(last[P->pending[i]] == i) { uniq.push_back(P->pending[i]); uniq.push_back(P->pending[i + 1]); }
        P->pending.swap(uniq);
    }
    const int n = (int)(P->pending.size() / 2);
    int rc = nh_ensure(ctx, P->d_upd, P->pending.size() * sizeof(int32_t));
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(P->d_upd.p, P->pending.data(), P->pending.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_scatter_i32, dim3((n + 255) / 256), dim3(256), 0, s, P->d_map, (const int32_t*)P->d_upd.p, n);
    HIPCHK(ctx, hipStreamSynchronize(s));          // (the host vector is reused)
    P->pending.clear();
    return NAVHIP_OK;
}

// One navhip_pool_build call: what its three steps hand to each other.
struct pool_build_job {
    int n = 0;
    std::vector<navhip_field_req> rq;      // the n requests; the flags of those that land on fresh slots are edited
    std::vector<uint64_t> base;            // per request: the id of the field it starts from, 0 = none
    std::vector<int32_t>  slots;           // per request: its pool slot (valid in front of `end`)
    std::vector<uint8_t>  pinned;          // per pool slot: this call reads or wrote it, nothing evicts it
    int begin = 0, end = 0;                // the sub-batch being cut and issued: requests [begin, end)
    std::vector<int32_t> copies, zeros;    // ... its (base slot, slot) pairs and the slots it starts from zero
    navhip_field_req *d_reqs = nullptr;    // device staging: P->d_reqs, and the three regions of P->d_slots
    int32_t *d_slots = nullptr, *d_copies = nullptr, *d_zeros = nullptr;     // [n] | [2n] | [n]
};

// Plan first, commit nothing: every base must be resident or produced earlier in this call, and the fields the call
// touches (its ids and the resident bases it reads) must fit the pool together -- they stay pinned for the WHOLE
// call, so that no sub-batch evicts what another one reads or wrote (the resident bases from here on, the call's
// own ids as pool_build_cut reaches them)
static int pool_build_plan(navhip_ctx *ctx, const nh_pool *P, const uint64_t *ff_ids, const uint64_t *base_ids, pool_build_job &J)
{
    std::unordered_map<uint64_t, int> seen;          // ids of earlier requests of this call
    std::unordered_map<uint64_t, int> touched;       // distinct ids + resident bases
    J.base.assign(J.n, 0);
    J.pinned.assign(P->n_slots, 0);
    for(int i = 0; i < J.n; i++) {
        const uint64_t b = (base_ids && (J.rq[i].flags & NAVHIP_REQ_INOUT)) ? base_ids[i] : 0;
        if(b && b != ff_ids[i]) {
            auto it = P->slot_of.find(b);
            if(!seen.count(b)) {
                if(it == P->slot_of.end()) { ctx->last_error = "navhip_pool_build: base field not resident"; return NAVHIP_ERR_NOT_UPLOADED; }
                touched[b] = 1;
            }
            if(it != P->slot_of.end()) J.pinned[it->second] = 1;
            J.base[i] = b;
        }
        seen[ff_ids[i]] = i;
        touched[ff_ids[i]] = 1;
    }
    if((int)touched.size() > P->n_slots) { ctx->last_error = "navhip_pool_build: the call touches more fields than the pool has slots"; return NAVHIP_ERR_NOMEM; }
    return NAVHIP_OK;
}

// Cut the sub-batch that starts at J.begin.  A request that reads (base) or rewrites the slot of an EARLIER request
// of the same sub-batch has to wait for it -- the in-place chains of nav.c:1987-2011 -- and so has a request that
// rewrites a field an earlier request of the sub-batch is COPIED from (the copies of a sub-batch run in one launch
// in front of its builds).  On an error J.end is the request that found no slot: [begin, end) hold theirs.
static int pool_build_cut(navhip_ctx *ctx, nh_pool *P, const uint64_t *ff_ids, pool_build_job &J)
{
    std::unordered_map<uint64_t, int> written, copied_from;
    J.copies.clear(); J.zeros.clear();
    for(J.end = J.begin; J.end < J.n; J.end++) {
        const int i = J.end;
        const uint64_t b = J.base[i];
        if(written.count(ff_ids[i]) || (b && written.count(b)) || copied_from.count(ff_ids[i])) break;
        int base_slot = -1;
        if(b) {
            base_slot = P->slot_of.find(b)->second;      // resident by now: planned above
            J.pinned[base_slot] = 1;
            copied_from[b] = 1;
        }
        bool fresh;
        const int slot = pool_slot_for(P, ff_ids[i], &fresh, &J.pinned);
        if(slot < 0) { ctx->last_error = "navhip_pool_build: no evictable slot"; return NAVHIP_ERR_NOMEM; }
        J.pinned[slot] = 1;
        J.slots[i] = slot;
        written[ff_ids[i]] = i;
        navhip_field_req &r = J.rq[i];
        if(base_slot >= 0) { J.copies.push_back(base_slot); J.copies.push_back(slot); }
        if(fresh) r.flags &= ~NAVHIP_REQ_IF_CHANGED;     // (nothing is cached yet; a copy of its base is not the field asked for)
        if(fresh && base_slot < 0) {
            // A new slot still holds the field of the id it was taken from.  An in-place request without a base starts
            // from N_FlowFieldInit; nothing is cached yet, so "only if changed" does not apply (above); and a request
            // the kernel may decline (NAVHIP_REQ_LIVE_IIDS: a portal blocked from end to end) must find
            // N_FlowFieldInit's all-FD_NONE field there, not the evicted one.
            if((r.flags & NAVHIP_REQ_INOUT) && r.type != NAVHIP_TARGET_NEAREST_PATHABLE && !(r.flags & NAVHIP_REQ_ISLAND_NEAREST))
                r.flags &= ~NAVHIP_REQ_INOUT;
            if(r.flags & (NAVHIP_REQ_LIVE_IIDS | NAVHIP_REQ_INOUT)) J.zeros.push_back(slot);
        }
    }
    return NAVHIP_OK;
}

// Issue the sub-batch [J.begin, J.end): the map updates of its evictions, its requests and slots, zero, copy, build;
// complete when it returns
static int pool_build_issue(navhip_ctx *ctx, nh_pool *P, const pool_build_job &J, hipStream_t s)
{
    const int m = J.end - J.begin;
    int rc = pool_flush_map(ctx, P, s);
    if(rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(J.d_reqs + J.begin, &J.rq[J.begin], (size_t)m * sizeof(navhip_field_req), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(J.d_slots + J.begin, &J.slots[J.begin], (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if(!J.zeros.empty()) {
        HIPCHK(ctx, hipMemcpyAsync(J.d_zeros, J.zeros.data(), J.zeros.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_zero_fields, dim3((unsigned)J.zeros.size()), dim3(256), 0, s, P->d_fields, (const int32_t*)J.d_zeros, (int)J.zeros.size());
    }
    if(!J.copies.empty()) {
        HIPCHK(ctx, hipMemcpyAsync(J.d_copies, J.copies.data(), J.copies.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_copy_field, dim3((unsigned)(J.copies.size() / 2)), dim3(256), 0, s, P->d_fields, (const int32_t*)J.d_copies, (int)(J.copies.size() / 2));
    }
    rc = navhip_build_fields_slots_dev(ctx, J.d_reqs + J.begin, m, P->d_fields, J.d_slots + J.begin, s);
    if(rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));       // (host vectors of the next sub-batch reuse the staging)
    return NAVHIP_OK;
}

extern "C" {

int navhip_pool_create(navhip_ctx *ctx, int n_slots, int n_dests)
{
    if(!ctx || n_slots < 1 || n_dests < 1) return NAVHIP_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if((int64_t)n_dests * ctx->nchunks > 0x7fffffffLL) {       // (map updates travel as 32-bit entry indices)
        ctx->last_error = "navhip_pool_create: n_dests x chunks does not fit 31 bits";
        return NAVHIP_ERR_INVALID;
    }
    navhip_pool_destroy(ctx);
    nh_pool *P = new (std::nothrow) nh_pool();
    if(!P) return NAVHIP_ERR_NOMEM;
    P->n_slots = n_slots; P->n_dests = n_dests; P->nchunks = ctx->nchunks;
    ctx->pool = P;
    HIPCHK(ctx, hipMalloc((void**)&P->d_fields, (size_t)n_slots * NH_CELLS));
    HIPCHK(ctx, hipMalloc((void**)&P->d_map, (size_t)n_dests * P->nchunks * sizeof(int32_t)));
    HIPCHK(ctx, hipMemsetAsync(P->d_fields, 0, (size_t)n_slots * NH_CELLS, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(P->d_map, 0xff, (size_t)n_dests * P->nchunks * sizeof(int32_t), ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    P->h_map.assign((size_t)n_dests * P->nchunks, -1);
    P->id_of.assign(n_slots, 0); P->used.assign(n_slots, 0); P->refs.assign(n_slots, {});
    P->lru_it.assign(n_slots, P->lru.end());
    for(int i = 0; i < n_slots; i++) pool_lru_move(P, i, false);
    return NAVHIP_OK;
}

void navhip_pool_destroy(navhip_ctx *ctx)
{
    if(!ctx || !ctx->pool) return;
    nh_pool *P = ctx->pool;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    hipFree(P->d_fields); hipFree(P->d_map);
    for(nh_buf *b : {&P->d_reqs, &P->d_slots, &P->d_upd}) hipFree(b->p);
    delete P;
    ctx->pool = nullptr;
}

int navhip_pool_clear(navhip_ctx *ctx)
{
    if(!ctx || !ctx->pool) return NAVHIP_ERR_INVALID;
    return navhip_pool_create(ctx, ctx->pool->n_slots, ctx->pool->n_dests);      // (by value: create destroys the old pool first)
}

int navhip_pool_contains(navhip_ctx *ctx, uint64_t ff_id)
{
    return ctx && ctx->pool && ctx->pool->slot_of.count(ff_id) ? 1 : 0;
}

int navhip_pool_invalidate(navhip_ctx *ctx, uint64_t ff_id)
{
    if(!ctx || !ctx->pool) return NAVHIP_ERR_INVALID;
    nh_pool *P = ctx->pool;
    auto it = P->slot_of.find(ff_id);
    if(it == P->slot_of.end()) return NAVHIP_OK;               // (lru_flow_remove of an absent key: no-op)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    pool_drop_slot(P, it->second);                             // unregister, least recently used again
    return pool_flush_map(ctx, P, ctx->stream);
}

int navhip_pool_put(navhip_ctx *ctx, uint64_t ff_id, const uint8_t *dirs)
{
    if(!ctx || !ctx->pool || !dirs) return NAVHIP_ERR_INVALID;
    nh_pool *P = ctx->pool;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    bool fresh;
    const int slot = pool_slot_for(P, ff_id, &fresh, nullptr);
    if(slot < 0) return NAVHIP_ERR_NOMEM;
    HIPCHK(ctx, hipMemcpyAsync(pool_field(P->d_fields, slot), dirs, NH_CELLS, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return pool_flush_map(ctx, P, ctx->stream);
}

int navhip_pool_get(navhip_ctx *ctx, uint64_t ff_id, uint8_t *out_dirs)
{
    if(!ctx || !ctx->pool || !out_dirs) return NAVHIP_ERR_INVALID;
    nh_pool *P = ctx->pool;
    auto it = P->slot_of.find(ff_id);
    if(it == P->slot_of.end()) return NAVHIP_ERR_NOT_UPLOADED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(out_dirs, pool_field(P->d_fields, it->second), NH_CELLS, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return NAVHIP_OK;
}

int navhip_pool_map(navhip_ctx *ctx, int n, const int32_t *dest, const uint16_t *chunk_r, const uint16_t *chunk_c, const uint64_t *ff_ids)
{
    if(!ctx || !ctx->pool || n < 0 || (n > 0 && (!dest || !chunk_r || !chunk_c || !ff_ids))) return NAVHIP_ERR_INVALID;
    nh_pool *P = ctx->pool;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for(int i = 0; i < n; i++) {
        if(dest[i] < 0 || dest[i] >= P->n_dests || chunk_r[i] >= ctx->h || chunk_c[i] >= ctx->w) return NAVHIP_ERR_INVALID;
        const int64_t e = (int64_t)dest[i] * P->nchunks + (int)chunk_r[i] * ctx->w + chunk_c[i];
        int slot = -1;                                   // an id that is not resident maps to "no field"
        auto it = P->slot_of.find(ff_ids[i]);
        if(it != P->slot_of.end()) slot = it->second;
        if(P->h_map[(size_t)e] != slot) {
            if(slot >= 0) P->refs[slot].push_back(e);     // (once per change: a host that re-puts its
                                                          // mappings every tick must not grow the list)
            P->h_map[(size_t)e] = slot;
            P->pending.push_back((int32_t)e); P->pending.push_back(slot);
        }
    }
    return pool_flush_map(ctx, P, ctx->stream);
}

int navhip_pool_build(navhip_ctx *ctx, const navhip_field_req *reqs, const uint64_t *ff_ids, const uint64_t *base_ids, int n, uint8_t *out_dirs)
{
    if(!ctx || !ctx->pool || n < 0 || (n > 0 && (!reqs || !ff_ids))) return NAVHIP_ERR_INVALID;
    if(n == 0) return NAVHIP_OK;
    nh_pool *P = ctx->pool;
    if(n > P->n_slots) { ctx->last_error = "navhip_pool_build: more requests than pool slots"; return NAVHIP_ERR_INVALID; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc = nh_validate_field_reqs(ctx, reqs, n);
    if(rc) return rc;
    pool_build_job J;
    J.n = n; J.rq.assign(reqs, reqs + n); J.slots.resize(n);
    rc = pool_build_plan(ctx, P, ff_ids, base_ids, J);
    if(!rc) rc = nh_ensure(ctx, P->d_reqs, (size_t)n * sizeof(navhip_field_req));
    if(!rc) rc = nh_ensure(ctx, P->d_slots, (size_t)n * 4 * sizeof(int32_t));
    if(rc) return rc;
    J.d_reqs = (navhip_field_req*)P->d_reqs.p;
    J.d_slots = (int32_t*)P->d_slots.p; J.d_copies = J.d_slots + n; J.d_zeros = J.d_copies + 2 * (size_t)n;
    for(J.begin = 0; J.begin < n; J.begin = J.end) {
        rc = pool_build_cut(ctx, P, ff_ids, J);
        if(!rc) rc = pool_build_issue(ctx, P, J, s);
        if(rc) {
            // A failure undoes the sub-batch it happened in, ALL of it: a fresh slot was never valid, and a resident
            // field that was being rebuilt in place (or had just received its base copy) may be half written -- it is
            // dropped like navhip_pool_invalidate drops it (the host builds it again on the next miss).  The
            // sub-batches before it were built, synchronised and stay registered.
            hipStreamSynchronize(s);
            for(int i = J.begin; i < J.end; i++) pool_drop_slot(P, J.slots[i]);
            pool_flush_map(ctx, P, s);
            return rc;
        }
    }
    if(out_dirs) {
        // (the fields are built and registered: a failing read-back does not unregister them)
        for(int i = 0; i < n; i++)
            HIPCHK(ctx, hipMemcpyAsync(out_dirs + (size_t)i * NH_CELLS, pool_field(P->d_fields, J.slots[i]), NH_CELLS, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return NAVHIP_OK;
}

}  // extern "C"

const uint8_t *nh_pool_fields(const navhip_ctx *ctx) { return ctx->pool ? ctx->pool->d_fields : nullptr; }
const int32_t *nh_pool_map(const navhip_ctx *ctx) { return ctx->pool ? ctx->pool->d_map : nullptr; }
int nh_pool_dests(const navhip_ctx *ctx) { return ctx->pool ? ctx->pool->n_dests : 0; }
int nh_pool_slots(const navhip_ctx *ctx) { return ctx->pool ? ctx->pool->n_slots : 0; }
