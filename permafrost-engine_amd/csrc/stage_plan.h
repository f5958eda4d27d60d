// stage_plan.h -- the staging plan of the host-buffer entry points: host code only, for the units whose host forms copy
// the caller's arrays up, call their _dev form and copy the answers down (state_kernels.hip, the two arrival units, the
// query, repair and seek units).
#pragma once
#include <string.h>
#include "navhip_internal.h"
#include "agent_types.h"

// One staging slot, planned before it is reserved: input rows (a host source), scratch rows, and the rows of a scratch
// row that go back to the host.  Rows are 256-byte aligned; reserve() gives every row its device address and writes it
// to the member of the device-side struct the row was staged for (`twin`).  How the rows cross the bus is a policy:
//   per row   (default)  one copy per row: every call but the two below
//   region()             rows that lie side by side travel as ONE region, mirrored in the page-locked slabs: the settle calls
//   pack()               page-locked arrays travel in place, pageable ones as ONE block behind the rows: the resident pass
struct nh_plan {
    struct row { size_t off, bytes; const void *src; void **twin; char *dev; bool direct; size_t h_off; };
    struct ret { int row; void *dst; size_t elem, lo, cnt, h_off; bool direct; };   // rows [lo, lo + cnt) of `row` -> dst
    std::vector<row> rows;
    std::vector<ret> rets;
    size_t total = 0;
    size_t in_blk = 0, in_bytes = 0, out_blk = 0, out_bytes = 0;    // the block of each direction: offset in the slot, bytes
    bool gather = false;                                            // pack(): the blocks lie behind the rows
    char *base = nullptr, *h_in = nullptr, *h_out = nullptr;

    static size_t up(size_t bytes) { return nh_up256(bytes); }
    // pad: tail bytes of a row whose array may be empty, so that a kernel is never handed the next row's address as its own
    int in(const void *src, size_t bytes, size_t pad = 0, void **twin = nullptr)
    {
        rows.push_back({total, src ? bytes : 0, src, twin, nullptr, true, 0});
        total += up(bytes + pad);
        return (int)rows.size() - 1;
    }
    int scratch(size_t bytes, void **twin = nullptr, size_t pad = 0) { return in(nullptr, bytes, pad, twin); }
    void out(int row, void *dst, size_t elem, size_t lo, size_t cnt) { if(dst && cnt) rets.push_back({row, dst, elem, lo, cnt, 0, true}); }
    template<class T> T *dev(int r) const { return (T*)rows[r].dev; }

    // input rows [first, end) go up as one region, everything from row first_out on comes down as one -- when the
    // context owns page-locked slabs (an asynchronous step path); per row otherwise
    void region(navhip_ctx *ctx, int first, int end, int first_out)
    {
        const size_t i0 = rows[first].off, o0 = rows[first_out].off;
        if(nh_async_slabs(ctx, rows[end].off - i0, total - o0, &h_in, &h_out) != NAVHIP_OK) return;
        in_blk = i0; in_bytes = rows[end].off - i0; out_blk = o0; out_bytes = total - o0;
        for(int i = first; i < end; i++) { rows[i].direct = false; rows[i].h_off = rows[i].off - i0; }
        for(ret &o : rets) { o.direct = false; o.h_off = rows[o.row].off + o.lo * o.elem - o0; }
    }
    // in_bytes / out_bytes: what the caller asks nh_async_slabs for (h_in, h_out)
    void pack()
    {
        gather = true;
        for(row &r : rows) if(r.bytes && !(r.direct = nh_is_pinned(r.src))) { r.h_off = in_bytes; in_bytes += up(r.bytes); }
        for(ret &o : rets) if(!(o.direct = nh_is_pinned(o.dst))) { o.h_off = out_bytes; out_bytes += up(o.cnt * o.elem); }
        in_blk = total; out_blk = total + in_bytes;
    }
    int reserve(navhip_ctx *ctx, nh_stage_slot slot)
    {
        int rc = nh_stage_reserve(ctx, slot, total + (gather ? in_bytes + out_bytes + 256 : 0), (void**)&base);
        if(rc) return rc;
        for(row &r : rows) {
            r.dev = base + (gather && !r.direct ? in_blk + r.h_off : r.off);
            if(r.twin) *r.twin = r.dev;
        }
        return NAVHIP_OK;
    }
    int upload(navhip_ctx *ctx, hipStream_t s)
    {
        for(const row &r : rows) {
            if(!r.bytes) continue;
            if(r.direct) HIPCHK(ctx, hipMemcpyAsync(r.dev, r.src, r.bytes, hipMemcpyHostToDevice, s));
            else         memcpy(h_in + r.h_off, r.src, r.bytes);
        }
        if(in_bytes) HIPCHK(ctx, hipMemcpyAsync(base + in_blk, h_in, in_bytes, hipMemcpyHostToDevice, s));
        return NAVHIP_OK;
    }
    // the results, and the wait for them
    int download(navhip_ctx *ctx, hipStream_t s)
    {
        for(const ret &o : rets) {
            const char *d = rows[o.row].dev + o.lo * o.elem;
            if(o.direct)    HIPCHK(ctx, hipMemcpyAsync((char*)o.dst + o.lo * o.elem, d, o.cnt * o.elem, hipMemcpyDeviceToHost, s));
            else if(gather) HIPCHK(ctx, hipMemcpyAsync(base + out_blk + o.h_off, d, o.cnt * o.elem, hipMemcpyDeviceToDevice, s));
        }
        if(out_bytes) HIPCHK(ctx, hipMemcpyAsync(h_out, base + out_blk, out_bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        for(const ret &o : rets) if(!o.direct) memcpy((char*)o.dst + o.lo * o.elem, h_out + o.h_off, o.cnt * o.elem);
        return NAVHIP_OK;
    }
};

// Which pointer member of an input / output struct is how large and when it travels: ONE list per struct for every
// host-buffer path of its unit (as nh_world_rows is for navhip_world).  nh_plan_rows walks a list: staging a struct and
// building its device twin is one loop.  The lengths and groups every unit knows are named here; a unit names its own
// from NH_LEN_OWN / NH_ON_OWN on (state_kernels.hip: the tiles of a flock, the rows of an arm, ...).
enum nh_len : uint8_t { NH_LEN_UNIT, NH_LEN_FLOCK, NH_LEN_FLOCK_PLUS1, NH_LEN_QUERY, NH_LEN_ZONE, NH_LEN_SLOT, NH_LEN_KEY,
                        NH_LEN_MEMBER,          // a row per member of the zones' flocks
                        NH_LEN_OWN, NH_LEN_COUNT = NH_LEN_OWN + 6 };
enum nh_group : uint8_t { NH_ON_ALWAYS,
                          NH_ON_DEV_ONLY,       // a member only the _dev form of a call reads: never staged
                          NH_ON_OWN, NH_ON_COUNT = NH_ON_OWN + 8 };
// What a row is: an input; a result that goes back whole (NH_OUT); the rows [D.lo, D.lo + D.cnt) of a per-unit result
// (NH_OUT_RANGE: the work range of the state pass); a result whose row starts as the caller's array (NH_IO: rows the kernel
// leaves alone go back as they came)
enum nh_row_kind : uint8_t { NH_IN, NH_OUT, NH_OUT_RANGE, NH_IO };
struct nh_row { size_t off; uint16_t elem; uint8_t len, group, pad, kind; };
struct nh_dims {
    size_t len[NH_LEN_COUNT] = {};
    bool   on[NH_ON_COUNT] = {true};        // NH_ON_ALWAYS
    size_t pad = 0;                         // at least this much tail padding on every input row
    size_t lo = 0, cnt = 0;                 // the rows of an NH_OUT_RANGE result that go back
};
// pad: tail bytes of the row's own (an array that may be empty, a result row of a call whose counts may be zero)
#define NH_ROW(T, member, elem, len, group) {offsetof(T, member), elem, len, group, 0, NH_IN}
#define NH_ROW_PAD(T, member, elem, len, group, pad) {offsetof(T, member), elem, len, group, pad, NH_IN}
#define NH_ROW_OUT(T, member, elem, len, group) {offsetof(T, member), elem, len, group, 0, NH_OUT}
#define NH_ROW_OUT_PAD(T, member, elem, len, group, pad) {offsetof(T, member), elem, len, group, pad, NH_OUT}
#define NH_ROW_OUT_RANGE(T, member, elem, len, group) {offsetof(T, member), elem, len, group, 0, NH_OUT_RANGE}
#define NH_ROW_IO(T, member, elem, len, group, pad) {offsetof(T, member), elem, len, group, pad, NH_IO}
// a new pointer member breaks the build here until its list has a row for it
#define NH_COVERS(tab, T, scalar_bytes) \
    static_assert(sizeof(T) == sizeof(tab) / sizeof(tab[0]) * sizeof(void*) + (scalar_bytes), #T " changed: does " #tab " cover it?")

static inline bool nh_listed(std::initializer_list<size_t> members, size_t off)
{
    for(size_t m : members) if(m == off) return true;
    return false;
}

// Stage the members of *in whose group is on, and have reserve() point the same members of *twin at the device copies.
// elsewhere: members this caller does not take from *in (another pass produces them on the device): it sets them in *twin.
template<class T, size_t N>
static inline void nh_plan_rows(nh_plan &p, const nh_row (&tab)[N], const T *in, T *twin_of, const nh_dims &D,
                                std::initializer_list<size_t> elsewhere = {})
{
    for(const nh_row &r : tab) {
        if(!D.on[r.group] || nh_listed(elsewhere, r.off)) continue;
        const size_t bytes = D.len[r.len] * r.elem;
        void *host = (void*)nh_member(in, r.off);
        void **twin = &nh_member(twin_of, r.off);
        if(r.kind == NH_IN) p.in(host, bytes, D.pad > r.pad ? D.pad : r.pad, twin);
        else if(r.kind == NH_OUT_RANGE) p.out(p.scratch(bytes, twin), host, r.elem, D.lo, D.cnt);
        else p.out(r.kind == NH_IO ? p.in(host, bytes, r.pad, twin) : p.scratch(bytes, twin, r.pad), host, r.elem, 0, D.len[r.len]);
    }
}

// ... and the listed arrays of the snapshot (nh_world_rows knows their sizes)
static inline void nh_plan_world(nh_plan &p, const navhip_world *w, navhip_world *twin, const nh_dims &D,
                                 std::initializer_list<size_t> members, size_t nmembers = 0, size_t pad = 0)
{
    for(const nh_world_row &r : nh_world_rows) {
        if(!nh_listed(members, r.off)) continue;
        const size_t cnt = r.count == NH_PER_ENT ? D.len[NH_LEN_UNIT] : r.count == NH_PER_FLOCK ? D.len[NH_LEN_FLOCK]
                         : r.count == NH_PER_FLOCK_PLUS1 ? D.len[NH_LEN_FLOCK_PLUS1] : nmembers;
        p.in(nh_member(w, r.off), cnt * r.row_bytes, D.pad > pad ? D.pad : pad, &nh_member(twin, r.off));
    }
}
#define NH_W(member) offsetof(navhip_world, member)

// the scalars of the world, no array: what is not staged must not travel as a host pointer
static inline navhip_world nh_device_world(const navhip_world *w)
{
    navhip_world d = *w;
    for(const nh_world_row &r : nh_world_rows) nh_member(&d, r.off) = nullptr;
    return d;
}

// the step parameters every kernel outside the agent step starts from: the map's planes, its origin, the world's size and rate
static inline void nh_step_params_init(const navhip_ctx *ctx, const navhip_world *w, nh_step_params *P)
{
    memset(P, 0, sizeof(*P));
    nh_fill_map_view(ctx, &P->map);
    P->map_x = w->map_pos_x; P->map_z = w->map_pos_z;
    P->n_ents = w->n_ents; P->hz = w->hz;
}
