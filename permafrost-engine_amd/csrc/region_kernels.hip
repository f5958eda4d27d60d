// region_kernels.hip -- flow fields over arbitrary square tile regions that straddle chunk
// boundaries, gfx950.
//
// Reference semantics (navigation/field.c): field_build_integration_region :582 (4-connected
// Dijkstra over the region in GLOBAL tile coordinates, neighbours via field_neighbours_grid_global
// :252, optional overlay mask of extra blocked tiles), then either
//   field_build_flow_unaligned :800  (whole region, two 4-bit directions per byte, set_flow_cell
//                                     :786) -- N_CellArrivalFieldCreate :2445,
//                                     N_GroupArrivalFieldCreate :2525 (96x96 regions, formation.c:78)
//   field_build_flow_region :763     (a 64x64 window of the region written in place into a chunk
//                                     field) -- field_update_enemies :1537, field_update_entity
//                                     :1615, field_update_zone :1822 (128x128 padded regions).
// The seeds (target tile, open formation slots, enemy / entity / zone footprints) are produced by
// the host's game-side queries and handed over as a tile list.
//
// One 256-thread workgroup per region; u32 integration tile + u8 cost tile in dynamic LDS
// (96x96: 45 KB, 128x128: 80 KB); chaotic min-plus relaxation to the integer-exact fixpoint, then
// the bake with the reference's neighbour priority.
#include "navhip_internal.h"
#include "field_cells.h"

static_assert(sizeof(navhip_region_req) == 32, "navhip_region_req must stay 32 bytes");

__global__ __launch_bounds__(256) void k_region_field(nh_map_view map, const navhip_region_req *reqs,
                                                      int n, const int16_t *seeds, const int16_t *overlay,
                                                      uint8_t *out, size_t out_stride)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int ri = blockIdx.x, t = threadIdx.x;
    if(ri >= n) return;
    const navhip_region_req rq = reqs[ri];
    const int dim = rq.rdim, cells = dim * dim;
    uint32_t *dist = (uint32_t*)smem;                    // [cells]
    uint8_t *pc = smem + (size_t)cells * 4;              // [cells] cost, 0xff = cannot be entered
    const nh_layer_view &L = map.layers[rq.layer];
    const int H = map.h * 64, W = map.w * 64;

    // ---- stage: which region tiles may the wavefront enter, and at what cost -----------------
    for(int i = t; i < cells; i += 256) {
        const int ar = rq.base_abs_r + i / dim, ac = rq.base_abs_c + i % dim;
        uint8_t v = NAVHIP_COST_IMPASSABLE;
        if(ar >= 0 && ar < H && ac >= 0 && ac < W) {                // M_Tile_RelativeDesc: on the map
            const size_t cell = ((size_t)((ar >> 6) * map.w + (ac >> 6)) << 12) + (ar & 63) * 64 + (ac & 63);
            const uint32_t cst = L.cost[cell];
            const uint32_t blk = L.blockers ? L.blockers[cell] : 0;
            // (a job "has a faction" when it names enemies)
            if(field_cell_enterable(L, cell, cst, blk, rq.enemies != 0, rq.enemies)) v = (uint8_t)cst;
        }
        pc[i] = v;
        dist[i] = NH_INF_U32;
    }
    __syncthreads();
    // overlay mask (build_overlay_mask :571): extra blocked tiles, never entered
    for(uint32_t k = t; k < rq.overlay_count; k += 256) {
        const int dr = overlay[2 * (rq.overlay_begin + k)] - rq.base_abs_r;
        const int dc = overlay[2 * (rq.overlay_begin + k) + 1] - rq.base_abs_c;
        if(dr >= 0 && dr < dim && dc >= 0 && dc < dim) pc[dr * dim + dc] = NAVHIP_COST_IMPASSABLE;
    }
    __syncthreads();
    // seeds get 0 unconditionally (pushed without a passability test, e.g. field.c:2497,2577)
    for(uint32_t k = t; k < rq.seed_count; k += 256) {
        const int dr = seeds[2 * (rq.seed_begin + k)] - rq.base_abs_r;
        const int dc = seeds[2 * (rq.seed_begin + k) + 1] - rq.base_abs_c;
        if(dr >= 0 && dr < dim && dc >= 0 && dc < dim) dist[dr * dim + dc] = 0;
    }
    __syncthreads();

    // ---- relaxation to the fixpoint (== Dijkstra distances, integer exact) ---------------------
    const field_grid_square g = {dim};
    field_relax_to_fixpoint(g, dist, field_cost_bytes{pc});

    // ---- bake ---------------------------------------------------------------------------------
    uint8_t *o = out + (size_t)ri * out_stride;
    const bool window = rq.out_mode == 1;
    const int wdim = window ? min(64, dim) : dim;
    const int ncell_out = wdim * (window ? wdim : dim);
    for(int j = t; j < (window ? ncell_out : cells / 2); j += 256) {
        // packed mode: one thread owns one output byte = two horizontally adjacent cells
        const int ncell = window ? 1 : 2;
        uint8_t byte = 0;
        bool keep_byte = false;
        for(int h = 0; h < ncell; h++) {
            int r, c;
            if(window) { r = j / wdim + rq.roff; c = j % wdim + rq.coff; }
            else       { r = (2 * j + h) / dim;  c = (2 * j + h) % dim; }
            const int i = r * dim + c;
            const uint32_t d = dist[i];
            uint32_t dir;
            bool write = true;
            if(d >= NH_INF_U32) {
                dir = NAVHIP_FD_NONE;             // packed: stays 0 (memset); window: left untouched
                write = !window;
            }else if(d == 0) {
                dir = NAVHIP_FD_NONE;
            }else{
                dir = field_flow_dir(g, dist, i);
            }
            if(window) {
                if(write) byte = (uint8_t)dir; else keep_byte = true;
            }else{
                // set_flow_cell :786: even column -> high nibble, odd column -> low nibble
                byte |= (uint8_t)(h == 0 ? dir << 4 : dir);
            }
        }
        if(window) { if(!keep_byte) o[(j / wdim) * 64 + (j % wdim)] = byte; }
        else       o[j] = byte;
    }
}

void nh_launch_region_fields(navhip_ctx *ctx, const navhip_region_req *d_reqs, int n, int max_dim,
                             const int16_t *d_seeds, const int16_t *d_overlay, uint8_t *d_out,
                             size_t out_stride, hipStream_t s)
{
    nh_map_view mv;
    nh_fill_map_view(ctx, &mv);
    const size_t lds = (size_t)max_dim * max_dim * 5;
    static nh_lds_once lds_allowed;                 // (a failure is not looked at here: the launch then fails)
    nh_allow_dynamic_lds(lds_allowed, ctx->device, (const void*)k_region_field, 128 * 128 * 5);
    if(n > 0)
        hipLaunchKernelGGL(k_region_field, dim3(n), dim3(256), lds, s, mv, d_reqs, n, d_seeds,
                           d_overlay, d_out, out_stride);
}
