// field_cells.h -- the reference's rules for ONE cell of a flow or LOS field, for the kernels that work cell by cell out
// of LDS: which tiles a request may enter, the sweep of the min-plus relaxation and the bake of a direction.  Shared by
// field_kernels.hip (k_field_generic), region_kernels.hip (k_region_field) and los_kernels.hip (k_los_field, the
// predicate only).  k_field_bfs states the same rules on bit planes and does not come here.  Free of device variables, so
// any unit may include it.
#pragma once
#include "navhip_internal.h"

// May a request enter the tile `cell` (absolute index into the layer's planes: chunk base + tile) with cost_base `cst`
// and blockers count `blk`?  Without a faction: field_tile_passable, field.c:117.  With one (the CALLER says which of its
// requests have one): field_tile_passable_no_enemies, field.c:179-201 -- blockers do not count on a tile that only
// factions of the `enemies` mask hold; with no factions plane resident nobody holds a tile, and blockers never count.
__device__ __forceinline__ bool field_cell_enterable(const nh_layer_view &L, size_t cell, uint32_t cst, uint32_t blk,
                                                     bool with_faction, uint32_t enemies)
{
    if(cst == NAVHIP_COST_IMPASSABLE) return false;
    if(!with_faction) return blk == 0;
    bool enemies_only = true;
    if(L.factions) {
        // factions[chunk][faction][tile]: 15 tiles of counters per chunk
        const uint8_t *fp = L.factions + (cell >> 12) * ((size_t)NAVHIP_MAX_FACTIONS << 12) + (cell & (NH_CELLS - 1));
        for(int f = 0; f < NAVHIP_MAX_FACTIONS; f++)
            if(fp[(size_t)f << 12] && !(enemies & (1u << f))) { enemies_only = false; break; }
    }
    return enemies_only || blk == 0;
}

// ---- the grid a workgroup of 256 threads relaxes and bakes: thread t owns the cells t, t + 256, ...; cell i lies in row
// i / dim, column i % dim.  The 64 x 64 tile of a chunk: `dim` is a constant, so these are a shift and a mask and the
// sweep a fixed 16 cells per thread.  A square region of `dim` tiles a side known at run time: one divide per cell.
struct field_grid_chunk  { static constexpr int dim = 64, passes = 16, unroll = 4; };
struct field_grid_square { static constexpr int passes = 0, unroll = 1; int dim; };

#define FIELD_NO_STEP 0xffffffffu      /* step_cost: the sweep leaves this cell alone */
// the usual step cost: a tile of staged cost bytes, 0xff = cannot be entered
struct field_cost_bytes {
    const uint8_t *pc;
    __device__ __forceinline__ uint32_t operator()(int i) const { return pc[i] == NAVHIP_COST_IMPASSABLE ? FIELD_NO_STEP : pc[i]; }
};

// Chaotic (in-place) min-plus relaxation to the fixpoint, by the whole workgroup:
//   d[x] = min(d[x], min_{4-nbrs y} d[y] + step_cost(x))   for every x with a step cost.
// Values only decrease and never drop below the true shortest distance, so the fixpoint is the Dijkstra result of
// field_build_integration (field.c:539; field_build_integration_region :582, ..._nonpass :643) bit for bit; a sweep in
// which no thread lowered anything proves every read saw final values.
template <class Grid, class StepCost>
__device__ __forceinline__ void field_relax_to_fixpoint(const Grid &g, uint32_t *dist, StepCost step_cost)
{
    const int dim = g.dim, n = dim * dim;
    for(;;) {
        int changed = 0;
        // (a chunk tile: a constant number of passes, the loop counter uniform; a region: until the cells run out)
#pragma unroll Grid::unroll
        for(int k = 0; Grid::passes ? k < Grid::passes : k * 256 + (int)threadIdx.x < n; k++) {
            const int i = k * 256 + (int)threadIdx.x;
            const uint32_t cst = step_cost(i);
            if(cst == FIELD_NO_STEP) continue;
            const int r = i / dim, c = i % dim;
            uint32_t m = NH_INF_U32;
            if(r > 0)       m = min(m, dist[i - dim]);
            if(r < dim - 1) m = min(m, dist[i + dim]);
            if(c > 0)       m = min(m, dist[i - 1]);
            if(c < dim - 1) m = min(m, dist[i + 1]);
            if(m < NH_INF_U32) {
                const uint32_t nd = m + cst;
                if(nd < dist[i]) { dist[i] = nd; changed = 1; }
            }
        }
        if(!__syncthreads_or(changed)) break;
    }
}

// field_flow_dir, field.c:355-433, of a cell with 0 < dist < NH_INF_U32: the neighbour of least distance, a diagonal
// admitted only when both tiles beside it are finite (:382-400), first match in the order N, S, E, W, NW, NE, SW, SE
// (:405-428).
template <class Grid>
__device__ __forceinline__ uint32_t field_flow_dir(const Grid &g, const uint32_t *dist, int i)
{
    const int dim = g.dim, r = i / dim, c = i % dim;
    const bool n = r > 0, s = r < dim - 1, w = c > 0, e = c < dim - 1;
    const uint32_t I = NH_INF_U32;
    const uint32_t dn = n ? dist[i - dim] : I, ds = s ? dist[i + dim] : I;
    const uint32_t dw = w ? dist[i - 1] : I,   de = e ? dist[i + 1] : I;
    const uint32_t dnw = (n && w) ? dist[i - dim - 1] : I;
    const uint32_t dne = (n && e) ? dist[i - dim + 1] : I;
    const uint32_t dsw = (s && w) ? dist[i + dim - 1] : I;
    const uint32_t dse = (s && e) ? dist[i + dim + 1] : I;
    uint32_t mc = min(min(dn, ds), min(dw, de));
    if(dn < I && dw < I) mc = min(mc, dnw);
    if(dn < I && de < I) mc = min(mc, dne);
    if(ds < I && dw < I) mc = min(mc, dsw);
    if(ds < I && de < I) mc = min(mc, dse);
    if(dn == mc)  return NAVHIP_FD_N;
    if(ds == mc)  return NAVHIP_FD_S;
    if(de == mc)  return NAVHIP_FD_E;
    if(dw == mc)  return NAVHIP_FD_W;
    if(dnw == mc) return NAVHIP_FD_NW;
    if(dne == mc) return NAVHIP_FD_NE;
    if(dsw == mc) return NAVHIP_FD_SW;
    return NAVHIP_FD_SE;
}
