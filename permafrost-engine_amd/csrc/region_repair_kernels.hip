// region_repair_kernels.hip -- N_CellArrivalFieldUpdateToNearestPathable (field.c:2603-2710) for region fields, gfx950:
// the second half of cell_field_fixup_task (formation.c:3160), which leads a formation member out of the blocked ground it
// stands on.  The first half, N_CellArrivalFieldCreate, is k_region_field (region_kernels.hip, out_mode 0); the two chain
// on one stream over the same slot.
//
// Reference semantics, in the order of the call:
//   clamped_region :1892            cb = max(base, 0), R = min(base_r + dim, H - 1) - cb_r, C likewise: where the far clamp
//                                   binds, the map's last row / column is not part of the flood
//   field_passable_frontier :1441   FIFO flood from `start` over the clamped region: a passable tile (field_tile_passable:
//                                   no overlay, no enemies) is emitted, any other pushes its 4 neighbours in the order W, E,
//                                   N, S.  visited[] is indexed dr * R + dc (:1431) while dc runs to C - 1: injective for
//                                   C <= R, so the emitted set is the set of passable tiles beside the start's component
//                                   whatever the queue order; for C > R the tiles (dr, dc >= R) and (dr + 1, dc - R) share
//                                   a flag and the emitted set depends on the exact order -- replayed on one lane
//   the seeds :2663                 every emitted tile gets 0
//   field_build_integration_nonpass_region :678
//                                   4-connected Dijkstra over the UNCLAMPED region [base, base + dim)^2, on-map tiles, into
//                                   the tiles for which `field_tile_passable && !overlay_blocked` is false, at the cost_base
//                                   of the tile entered (255 for impassable ground); integers below 2^24, exact in the
//                                   reference's floats: the relaxation's fixpoint (field_cells.h) is the same field
//   the bake :2691                  on-map tiles with a finite, non-zero value get field_flow_dir; every other nibble stays
//
// One 256-thread workgroup per request.  Dynamic LDS, 6 bytes per region tile (96 x 96: 54 KB, 128 x 128: 96 KB): the u32
// integration tile, a byte tile of step costs and a byte tile of marks.  The flood runs before the integration tile holds
// anything, so the serial arm's ring (16-bit entries, at most max(R, C)^2 <= dim^2 of them: every push sets a fresh flag)
// and visited flags live in it.
#include "navhip_internal.h"
#include "stage_plan.h"
#include "field_cells.h"

static_assert(sizeof(navhip_region_repair_req) == 20, "navhip_region_repair_req must stay 20 bytes");

#define RR_MAX_DIM 128
enum : uint8_t { RR_ON_MAP = 1, RR_PASSABLE = 2, RR_OVERLAY = 4, RR_REACHED = 8, RR_EMITTED = 16 };

// the Dijkstra of field.c:678 enters on-map tiles that are not passable or lie under the overlay, at their own cost_base
struct rr_step_cost {
    const uint8_t *pc, *mk;
    __device__ __forceinline__ uint32_t operator()(int i) const
    {
        const uint8_t m = mk[i];
        return (m & RR_ON_MAP) && (!(m & RR_PASSABLE) || (m & RR_OVERLAY)) ? (uint32_t)pc[i] : FIELD_NO_STEP;
    }
};

// Is the row well-formed (the host form refuses the others before the launch)?  One rule for the check and the kernel.
#ifdef NH_HOSTSIM
#define RR_HOST_DEVICE
#else
#define RR_HOST_DEVICE __host__ __device__
#endif
RR_HOST_DEVICE static inline bool rr_row_ok(const navhip_region_repair_req &rq, size_t stride, bool have_overlay)
{
    return rq.dim >= 2 && rq.dim <= RR_MAX_DIM && (rq.dim % 2) == 0 && rq.layer < NAVHIP_NAV_LAYER_MAX
        && stride >= (size_t)rq.dim * rq.dim / 2 && (rq.overlay_count == 0 || have_overlay);
}

__global__ __launch_bounds__(256) void k_region_repair(nh_map_view map, const navhip_region_repair_req *reqs, int n,
                                                       int max_dim, const int16_t *overlay, uint8_t *inout,
                                                       size_t stride, uint8_t *out_status)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int ri = blockIdx.x, t = threadIdx.x;
    if(ri >= n) return;
    const navhip_region_repair_req rq = reqs[ri];
    const int H = map.h * 64, W = map.w * 64;
    const int dim = rq.dim, cells = dim * dim;

    // ---- the rows that are the host's: every thread decides alike, nobody has met a barrier yet ------------------------
    bool host = !rr_row_ok(rq, stride, overlay != nullptr) || dim > max_dim;
    const int sr = rq.start_abs_r, sc = rq.start_abs_c;
    host = host || sr < 0 || sr >= H || sc < 0 || sc >= W
                || rq.centre_abs_r < 0 || rq.centre_abs_r >= H || rq.centre_abs_c < 0 || rq.centre_abs_c >= W;
    const nh_layer_view &L = map.layers[host ? 0 : rq.layer];
    host = host || !L.cost || !L.blockers;
    // base :2654 and clamped_region :1892
    const int base_r = rq.centre_abs_r - dim / 2, base_c = rq.centre_abs_c - dim / 2;
    const int cb_r = max(base_r, 0), cb_c = max(base_c, 0);
    const int R = min(base_r + dim, H - 1) - cb_r, C = min(base_c + dim, W - 1) - cb_c;
    const int off_r = cb_r - base_r, off_c = cb_c - base_c;          // clamped (dr, dc) -> region tile (dr + off_r, dc + off_c)
    host = host || sr - cb_r < 0 || sr - cb_r >= R || sc - cb_c < 0 || sc - cb_c >= C;
    if(!host) {
        const size_t cell = ((size_t)((sr >> 6) * map.w + (sc >> 6)) << 12) + (sr & 63) * 64 + (sc & 63);
        host = L.cost[cell] != NAVHIP_COST_IMPASSABLE && L.blockers[cell] == 0;          // the assert of :1454
    }
    if(host) {
        if(t == 0) out_status[ri] = NAVHIP_RR_HOST;
        return;
    }

    uint32_t *dist = (uint32_t*)smem;                    // [cells]; before the seeds: the ring and the visited flags
    uint8_t *pc = smem + (size_t)cells * 4;              // [cells] cost_base
    uint8_t *mk = pc + cells;                            // [cells] RR_* marks
    uint16_t *ring = (uint16_t*)smem;                    // [<= cells] clamped (dr << 7 | dc)
    uint8_t *visited = smem + (size_t)cells * 2;         // [max(R, C)^2 <= cells], the reference's index
    const bool serial = C > R;
    const int nelems = max(R, C) * max(R, C);

    // ---- stage the planes.  The start's RR_REACHED is set here, by the thread that owns the byte in this loop: the overlay
    // loop below only ORs into bytes it reads behind the barrier, so no other write can lose it -------------------------
    const int si = (sr - base_r) * dim + (sc - base_c);
    for(int i = t; i < cells; i += 256) {
        const int ar = base_r + i / dim, ac = base_c + i % dim;
        uint8_t m = 0, cst = NAVHIP_COST_IMPASSABLE;
        if(ar >= 0 && ar < H && ac >= 0 && ac < W) {                // M_Tile_RelativeDesc: on the map
            const size_t cell = ((size_t)((ar >> 6) * map.w + (ac >> 6)) << 12) + (ar & 63) * 64 + (ac & 63);
            cst = L.cost[cell];
            m = RR_ON_MAP | (cst != NAVHIP_COST_IMPASSABLE && L.blockers[cell] == 0 ? RR_PASSABLE : 0);   // field_tile_passable :117
        }
        pc[i] = cst;
        mk[i] = i == si ? (uint8_t)(m | RR_REACHED) : m;
        if(serial && i < nelems) visited[i] = 0;
    }
    __syncthreads();
    // overlay mask (build_overlay_mask :571) over the unclamped region; tiles outside it are ignored
    for(uint32_t k = t; k < rq.overlay_count; k += 256) {
        const int dr = overlay[2 * ((size_t)rq.overlay_begin + k)] - base_r;
        const int dc = overlay[2 * ((size_t)rq.overlay_begin + k) + 1] - base_c;
        if(dr >= 0 && dr < dim && dc >= 0 && dc < dim) mk[dr * dim + dc] |= RR_OVERLAY;
    }
    __syncthreads();

    // ---- field_passable_frontier ------------------------------------------------------------------------------------------
    if(!serial) {
        // C <= R: the component of non-passable tiles around the start inside the clamped region, to a fixpoint; marks only
        // ever gain RR_REACHED, and a sweep in which no thread set one proves the component complete
        for(;;) {
            int changed = 0;
            for(int i = t; i < cells; i += 256) {
                const int dr = i / dim - off_r, dc = i % dim - off_c;
                if(dr < 0 || dr >= R || dc < 0 || dc >= C) continue;
                if(mk[i] & (RR_PASSABLE | RR_REACHED)) continue;
                const bool beside = (dc > 0     && (mk[i - 1] & RR_REACHED))   || (dc < C - 1 && (mk[i + 1] & RR_REACHED))
                                 || (dr > 0     && (mk[i - dim] & RR_REACHED)) || (dr < R - 1 && (mk[i + dim] & RR_REACHED));
                if(beside) { mk[i] |= RR_REACHED; changed = 1; }
            }
            if(!__syncthreads_or(changed)) break;
        }
        // a passable tile is popped, and emitted, when a tile of the component pushed it (RR_REACHED is never set on one)
        for(int i = t; i < cells; i += 256) {
            const int dr = i / dim - off_r, dc = i % dim - off_c;
            if(dr < 0 || dr >= R || dc < 0 || dc >= C || !(mk[i] & RR_PASSABLE)) continue;
            const bool beside = (dc > 0     && (mk[i - 1] & RR_REACHED))   || (dc < C - 1 && (mk[i + 1] & RR_REACHED))
                             || (dr > 0     && (mk[i - dim] & RR_REACHED)) || (dr < R - 1 && (mk[i + dim] & RR_REACHED));
            if(beside) mk[i] |= RR_EMITTED;
        }
    }else{
        // C > R: the reference's queue on one lane, with its aliased visited index; the others wait at the barrier below
        if(t == 0) {
            int head = 0, tail = 0;
            ring[tail++] = (uint16_t)(((sr - cb_r) << 7) | (sc - cb_c));
            visited[(sr - cb_r) * R + (sc - cb_c)] = 1;
            while(head < tail) {
                const int cur = ring[head++], dr = cur >> 7, dc = cur & 127;
                const int i = (dr + off_r) * dim + dc + off_c;
                if(mk[i] & RR_PASSABLE) { mk[i] |= RR_EMITTED; continue; }
                const int ddr[4] = {0, 0, -1, 1}, ddc[4] = {-1, 1, 0, 0};
#pragma unroll
                for(int k = 0; k < 4; k++) {
                    const int nr = dr + ddr[k], nc = dc + ddc[k];
                    if(nr < 0 || nr >= R || nc < 0 || nc >= C) continue;        // tile_outside_region (on the map: implied)
                    const int vi = nr * R + nc;                                  // visited_idx :1431, stride R
                    if(visited[vi]) continue;
                    visited[vi] = 1;
                    // one push per fresh flag, the start's included: tail <= max(R, C)^2 <= cells, the ring's size
                    ring[tail++] = (uint16_t)((nr << 7) | nc);
                }
            }
        }
    }
    __syncthreads();

    // ---- the seeds: the emitted tiles get 0.  (:2668 skips emitted tiles outside [0, dim)^2 of the unclamped base: the
    // clamped region lies inside it, and the marks are indexed by it, so no such tile exists here) ------------------------
    for(int i = t; i < cells; i += 256) dist[i] = (mk[i] & RR_EMITTED) ? 0u : NH_INF_U32;
    __syncthreads();

    // ---- relaxation to the fixpoint (== the Dijkstra of :678, integer exact) -----------------------------------------
    const field_grid_square g = {dim};
    field_relax_to_fixpoint(g, dist, rr_step_cost{pc, mk});

    // ---- bake: one thread owns one byte, so both nibbles; a nibble is rewritten for an on-map tile with a finite,
    // non-zero value only (:2696-2702) ------------------------------------------------------------------------------------
    uint8_t *o = inout + (size_t)ri * stride;
    for(int j = t; j < cells / 2; j += 256) {
        uint32_t set = 0, keep = 0xff;
        for(int h = 0; h < 2; h++) {
            const int i = 2 * j + h;
            const uint32_t d = dist[i];
            if(!(mk[i] & RR_ON_MAP) || d >= NH_INF_U32 || d == 0) continue;
            const uint32_t dir = field_flow_dir(g, dist, i);
            // set_flow_cell :790: even column -> high nibble, odd column -> low nibble
            set |= h == 0 ? dir << 4 : dir;
            keep &= h == 0 ? 0x0fu : 0xf0u;
        }
        if(keep != 0xff) o[j] = (uint8_t)((o[j] & keep) | set);
    }
    if(t == 0) out_status[ri] = 0;
}

static int nh_launch_region_repair(navhip_ctx *ctx, const navhip_region_repair_req *d_reqs, int n, int max_dim,
                                    const int16_t *d_overlay, uint8_t *d_inout, size_t stride, uint8_t *d_status,
                                    hipStream_t s)
{
    nh_map_view mv;
    nh_fill_map_view(ctx, &mv);
    const size_t lds = (size_t)max_dim * max_dim * 6;
    static nh_lds_once lds_allowed;                 // (a failure is the call's error)
    HIPCHK(ctx, nh_allow_dynamic_lds(lds_allowed, ctx->device, (const void*)k_region_repair, RR_MAX_DIM * RR_MAX_DIM * 6));
    hipLaunchKernelGGL(k_region_repair, dim3(n), dim3(256), lds, s, mv, d_reqs, n, max_dim, d_overlay, d_inout, stride,
                       d_status);
    HIPCHK(ctx, hipGetLastError());
    return NAVHIP_OK;
}

#define RR_FAIL(why) nh_fail(ctx, NAVHIP_ERR_INVALID, "navhip_repair_region_fields: ", why)

extern "C" {

int navhip_repair_region_fields_dev(navhip_ctx *ctx, const navhip_region_repair_req *dev_reqs, int n, int max_dim,
                                    const int16_t *dev_overlay, uint8_t *dev_inout, size_t stride, uint8_t *dev_status,
                                    void *stream)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    if(n < 0) return RR_FAIL("a negative count");
    if(n > 0 && (!dev_reqs || !dev_inout || !dev_status)) return RR_FAIL("a missing array");
    if(max_dim < 2 || max_dim > RR_MAX_DIM || (max_dim % 2) != 0) return RR_FAIL("max_dim is odd or outside 2..128");
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    return nh_launch_region_repair(ctx, dev_reqs, n, max_dim, dev_overlay, dev_inout, stride, dev_status, s);
}

int navhip_repair_region_fields(navhip_ctx *ctx, const navhip_region_repair_req *reqs, int n,
                                const int16_t *overlay, size_t n_overlay, uint8_t *inout, size_t stride,
                                uint8_t *out_status)
{
    if(!ctx) return NAVHIP_ERR_INVALID;
    if(n < 0) return RR_FAIL("a negative count");
    if(n > 0 && (!reqs || !inout || !out_status)) return RR_FAIL("a missing array");
    // every row, before anything is launched
    int max_dim = 2;
    for(int i = 0; i < n; i++) {
        const navhip_region_repair_req &r = reqs[i];
        if(!rr_row_ok(r, stride, overlay != nullptr) || (size_t)r.overlay_begin + r.overlay_count > n_overlay)
            return RR_FAIL("malformed request " + std::to_string(i) + " (dim odd, 0 or above 128; no such layer; a stride"
                                " below dim * dim / 2; an overlay range outside the array)");
        max_dim = r.dim > max_dim ? r.dim : max_dim;
    }
    if(n == 0) return NAVHIP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t bytes = (size_t)n * stride;
    const navhip_region_repair_req *d_reqs; const int16_t *d_overlay = nullptr;
    uint8_t *d_inout, *d_status;
    nh_plan P;
    P.in(reqs, (size_t)n * sizeof(navhip_region_repair_req), 0, (void**)&d_reqs);
    if(overlay) P.in(overlay, n_overlay * 4, 16, (void**)&d_overlay);
    P.out(P.in(inout, bytes, 0, (void**)&d_inout), inout, 1, 0, bytes);       // the slots travel with what they hold
    P.out(P.scratch((size_t)n, (void**)&d_status), out_status, 1, 0, (size_t)n);
    int rc = P.reserve(ctx, NH_STAGE_CALL0);
    if(!rc) rc = P.upload(ctx, s);
    if(!rc) rc = navhip_repair_region_fields_dev(ctx, d_reqs, n, max_dim, d_overlay, d_inout, stride, d_status, s);
    if(!rc) rc = P.download(ctx, s);
    return rc;
}

}   // extern "C"
