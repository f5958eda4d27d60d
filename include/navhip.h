/* include/navhip.h -- C ABI of libnavhip.so
 *
 * MI355X (gfx950) implementation of permafrost-engine's per-tick navigation
 * hot path: chunk flow-field build (integration sweep + 8-neighbour bake) and
 * the per-agent steering + ClearPath velocity step, behind plain-C entry
 * points that the reference's C host code binds directly (see INTEGRATION.md
 * for the reference-side call sites).  No torch / C++ types cross this
 * boundary: plain pointers, sizes and PODs only.
 *
 * Every entry point cites the reference interface (file:line under the
 * reference's src/) that it replaces or is fed by.
 *
 * Conventions
 *   - all functions return NAVHIP_OK (0) or a negative NAVHIP_ERR_* code; on a
 *     non-zero return the caller falls back to the reference CPU path
 *     (SURVEY.md §8b "Errors");
 *   - "host" pointers are ordinary CPU memory, "dev" pointers are HIP device
 *     memory on the context's GPU; `stream` is a hipStream_t passed as void*
 *     (NULL = the context's own stream);
 *   - plane layouts are the reference's packed upload layouts
 *     (N_CopyCostBasePacked / N_CopyBlockersPacked, nav.c:2432,2470): for one
 *     layer, chunk-row-major, each chunk a raw [64][64] array.
 */
#ifndef NAVHIP_H
#define NAVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAVHIP_OK                 0
#define NAVHIP_ERR_INVALID       -1   /* bad argument                         */
#define NAVHIP_ERR_ARG           NAVHIP_ERR_INVALID   /* the same code, as navhip_dest_queries names it */
#define NAVHIP_ERR_DEVICE        -2   /* HIP runtime error (see last_error)   */
#define NAVHIP_ERR_NOMEM         -3
#define NAVHIP_ERR_NOT_UPLOADED  -4   /* a plane the request needs is missing */

#define NAVHIP_FIELD_RES         64          /* FIELD_RES_R/C      nav_data.h:45-46 */
#define NAVHIP_FIELD_CELLS       4096
#define NAVHIP_COST_IMPASSABLE   0xff        /* COST_IMPASSABLE    nav_data.h:47 */
#define NAVHIP_ISLAND_NONE       0xffff      /* ISLAND_NONE        nav_data.h:48 */
#define NAVHIP_FACTION_ID_NONE   0xf         /* FACTION_ID_NONE    nav_data.h:49 */
#define NAVHIP_MAX_FACTIONS      15          /* MAX_FACTIONS       game.h:48     */
#define NAVHIP_NAV_LAYER_MAX     12          /* enum nav_layer     nav.h:78-92   */

/* enum flow_dir, nav.h:94-104 */
enum { NAVHIP_FD_NONE = 0, NAVHIP_FD_NW, NAVHIP_FD_N, NAVHIP_FD_NE, NAVHIP_FD_W,
       NAVHIP_FD_E, NAVHIP_FD_SW, NAVHIP_FD_S, NAVHIP_FD_SE };

/* field_target.type values, field.h:85-98 (only the chunk-aligned targets), plus the repair build
 * N_FlowFieldUpdateToNearestPathable (field.c:2247), which ignores the field's own target */
enum { NAVHIP_TARGET_PORTAL = 0, NAVHIP_TARGET_TILE = 1, NAVHIP_TARGET_NEAREST_PATHABLE = 2 };

/* per-layer planes held on the device (struct nav_chunk members, nav_data.h:118-158) */
enum {
    NAVHIP_PLANE_COST_BASE     = 0,   /* uint8_t  [64][64] per chunk              */
    NAVHIP_PLANE_BLOCKERS      = 1,   /* uint16_t [64][64] per chunk              */
    NAVHIP_PLANE_LOCAL_ISLANDS = 2,   /* uint16_t [64][64] per chunk              */
    NAVHIP_PLANE_FACTIONS      = 3,   /* uint8_t  [15][64][64] per chunk          */
    NAVHIP_PLANE_ISLANDS       = 4,   /* uint16_t [64][64] per chunk (global island ids,
                                         nav_chunk.islands nav_data.h:150; only read by
                                         NAVHIP_REQ_ISLAND_NEAREST)                */
    NAVHIP_PLANE_COUNT
};

/* navhip_field_req.flags */
#define NAVHIP_REQ_INOUT   0x1   /* update an existing field in place: unreachable cells keep
                                    the bytes already in the output slot (field.c:737-751,
                                    nav.c:1998-2008) instead of starting from N_FlowFieldInit */

#define NAVHIP_REQ_IF_CHANGED 0x2 /* incremental repair: build only when the request's chunk (or, for a
                                    portal target, the next chunk) is flagged changed by the blocker
                                    updates since the last navhip_clear_changed; otherwise the slot
                                    is left untouched (the cached field stays valid, the device image
                                    of N_ApplyDeferredInvalidations, nav.c:2208).  A request with a
                                    faction is also built when the per-faction flags of its own chunk
                                    (navhip_faction_changed_chunks) name a faction that is not among
                                    its enemies: more than the reference's dirty set (nav.c:1036),
                                    which knows no faction and leaves such a field stale */
#define NAVHIP_REQ_LIVE_IIDS  0x4 /* portal targets: re-read port_iid / next_iid on the device from the
                                    CURRENT local_islands plane -- the label of the first tile of the
                                    port / next portal that has one (a blocker leaves ISLAND_NONE); a
                                    portal blocked from end to end leads nowhere: the slot is left
                                    untouched (for request lists that outlive a relabel, as in the
                                    device-resident incremental-repair benchmark) */

#define NAVHIP_REQ_ISLAND_NEAREST 0x8 /* N_FlowFieldUpdateIslandToNearest(aux_iid, ...) (field.c:2307) on
                                    an existing TILE/PORTAL field: the frontier is moved to the tiles
                                    of local island aux_iid nearest (Manhattan) to the target's own
                                    frontier; always in place.  The repair the sampler runs when an
                                    agent's tile is orphaned from its goal by blockers (nav.c:3540) */

/* One chunk-field build: the arguments of
 *   N_FlowFieldUpdate(chunk, priv, faction_id, layer, target, ctx, inout)   field.c:2030
 * with `struct field_target` / `struct portal_desc` (field.h:67-72,85-101) flattened so the
 * record is position independent (portal pointers become endpoint coordinates).  32 bytes. */
typedef struct navhip_field_req {
    uint8_t  layer;          /* enum nav_layer                                         */
    uint8_t  type;           /* NAVHIP_TARGET_TILE / NAVHIP_TARGET_PORTAL              */
    uint8_t  faction_id;     /* NAVHIP_FACTION_ID_NONE, or the pathing faction (an "attacking
                                path": tiles blocked by enemies only are passable, field.c:179).
                                Either way the bit-parallel wave kernel builds the field when
                                every passable cell of the chunk costs 1 (navhip_set_field_kernel) */
    uint8_t  flags;          /* NAVHIP_REQ_*                                           */
    uint16_t enemies;        /* enemies_for_faction(faction_id) bitmask, field.c:166: bit f set =
                                faction f does not block.  Read with a faction only; without a
                                resident factions plane no blocker stops such a request        */
    uint16_t chunk_r, chunk_c;
    uint8_t  tile_r, tile_c;                       /* TARGET_TILE: target.tile;
                                                      NEAREST_PATHABLE: the start tile  */
    uint8_t  port_r0, port_c0, port_r1, port_c1;   /* TARGET_PORTAL: pd.port->endpoints */
    uint8_t  next_r0, next_c0, next_r1, next_c1;   /*                pd.next->endpoints */
    uint16_t next_chunk_r, next_chunk_c;           /*                pd.next->chunk     */
    uint16_t port_iid, next_iid;                   /*                pd.port_iid/next_iid */
    uint16_t aux_iid;                              /* NAVHIP_REQ_ISLAND_NEAREST: local_iid */
    uint16_t _pad;
} navhip_field_req;

typedef struct navhip_ctx navhip_ctx;

/* ---- context / map state (SURVEY.md §8b "Map/state upload") ------------------------------ */

/* Create a context for a map of chunk_w x chunk_h chunks (struct nav_private width/height,
 * nav_private.h:53) on HIP device `device`.  Fails loudly (NAVHIP_ERR_DEVICE) when no GPU is
 * present: there is no CPU fallback inside this library. */
int  navhip_ctx_create(navhip_ctx **out, int chunk_w, int chunk_h, int device);
void navhip_ctx_destroy(navhip_ctx *ctx);
const char *navhip_last_error(const navhip_ctx *ctx);
int  navhip_device(const navhip_ctx *ctx);
/* the context's HIP stream, as void* (hipStream_t) */
void *navhip_stream(const navhip_ctx *ctx);
/* A stream (hipStream_t as void*; the library's, never to be destroyed by the caller) for wide, throughput-bound work --
 * the field builds -- that runs BESIDE the agent step enqueued on `main_stream`.  cu_count > 0: it may only use the
 * compute units [cu_begin, cu_begin + cu_count) (hipExtStreamCreateWithCUMask; the MI355X has 256 CUs in 8 XCDs of 32)
 * and leaves the rest of the chip to the narrow, latency-bound front of the step; cu_count <= 0: every compute unit.
 * The stream has a hardware queue of its own, on a pipe of the command processor that neither `main_stream` nor the
 * step's side streams use (a hand-over between two queues on one pipe costs 100-200 us instead of 12: measured once per
 * process and caller stream, csrc/navhip_api.hip).  One set of such streams exists per process and device: calls with
 * the same arguments return the same stream. */
int  navhip_stream_beside(navhip_ctx *ctx, void *main_stream, int cu_begin, int cu_count, void **out_stream);
/* The library's own stream for the agent chain (what navhip_tick_create runs a tick on when its description names no
 * stream): a hardware queue of its own on the fourth pipe, beside the three of navhip_stream_beside(ctx, <this stream>, ..)
 * and of the step's side streams.  A host that has no reason to run the step on a stream of its own should use this
 * one: the set is the same for every context of the process, so a tick costs the same whatever the process created before. */
int  navhip_stream_main(navhip_ctx *ctx, void **out_stream);
/* navhip_stream_beside(ctx, navhip_stream(ctx), cu_begin, cu_count, out_stream) with cu_count > 0 */
int  navhip_stream_create_partial(navhip_ctx *ctx, int cu_begin, int cu_count, void **out_stream);
/* waits for the context's own stream and for the side streams of navhip_agent_prefetch_dev */
int  navhip_sync(navhip_ctx *ctx);

/* Upload one whole plane of one layer (all chunks).  Replaces N_CopyCostBasePacked /
 * N_CopyBlockersPacked consumers (nav.c:2408-2490): same layout, same sizes. */
int  navhip_upload_plane(navhip_ctx *ctx, int layer, int plane, const void *host, size_t bytes);
/* Upload one chunk of one plane (dirty-chunk update after N_Update, nav.c:2119). */
int  navhip_upload_chunk(navhip_ctx *ctx, int layer, int plane, int chunk_r, int chunk_c,
                         const void *host, size_t bytes);
/* Device pointer of a resident plane (NULL when never uploaded); for zero-copy producers.  The library keeps row
 * masks derived from the cost_base, blockers AND factions planes; it rebuilds them after navhip_upload_plane /
 * navhip_upload_chunk and after navhip_blockers_circles[_dev].  Whoever writes one of these three planes through this
 * pointer re-uploads nothing but has to name the chunks it wrote: one navhip_upload_chunk of the chunk (any of the three
 * planes, e.g. its own read-back) before the next build -- the factions plane is under the same rule as the other two. */
void *navhip_plane_dev(navhip_ctx *ctx, int layer, int plane);

/* Read a resident plane back (tests; host mirrors after device-side blocker updates). */
int  navhip_download_plane(navhip_ctx *ctx, int layer, int plane, void *host, size_t bytes);

/* ---- dynamic obstacles -------------------------------------------- */

/* One N_BlockersIncref (delta = +1) / N_BlockersDecref (delta = -1) call, nav.c:4663,4685:
 * (xz_pos, range, faction_id, flags).  24 bytes. */
typedef struct navhip_circle {
    float    x, z;          /* xz_pos                                                      */
    float    radius;        /* range; the device path takes ceil(radius/4) <= 28 tiles     */
    int32_t  faction_id;    /* 0..14                                                       */
    uint32_t flags;         /* ENTITY_FLAG_AIR selects the air layers, else water + ground */
    int32_t  delta;         /* +1 incref, -1 decref                                        */
} navhip_circle;

/* Apply n incref/decref calls to the resident blockers (+ factions) planes of every resident
 * layer of the affected domains, with the reference's tile sets: tiles under the circle
 * (M_Tile_AllUnderCircle, tile.c:687) on the 1x1 layer, plus 1/2/3 successive contours
 * (M_Tile_Contour, tile.c:759) on the 3x3/5x5/7x7 layers (n_update_blockers_circle_*,
 * nav.c:1051-1133).  Afterwards, on the device and without a host round trip: the derived
 * passability of every touched chunk is rebuilt, chunks whose passability CHANGED are flagged
 * (the dirty_chunks set of n_update_blockers, nav.c:1033-1046, restricted to real changes) and
 * their local-island labels recomputed (n_update_local_islands, nav.c:967).
 * map_pos_x/z: the vec3 map_pos .x/.z handed to every N_* call. */
int  navhip_blockers_circles(navhip_ctx *ctx, const navhip_circle *circles, int n,
                             float map_pos_x, float map_pos_z);
int  navhip_blockers_circles_dev(navhip_ctx *ctx, const navhip_circle *dev_circles, int n,
                                 float map_pos_x, float map_pos_z, void *stream);
/* n_update_local_island_field (nav.c:986) for one layer on the device, from the resident
 * cost_base + blockers planes (allocates the local_islands plane when it was never uploaded). */
int  navhip_relabel_local_islands(navhip_ctx *ctx, int layer);
/* The changed-chunk flags of one layer ([chunk_h*chunk_w] bytes, 1 = passability changed);
 * clear != 0 resets them afterwards. */
int  navhip_changed_chunks(navhip_ctx *ctx, int layer, uint8_t *host_flags, int clear);
/* The per-faction changed flags of one layer ([chunk_h*chunk_w] uint16_t): bit f = since the last navhip_clear_changed
 * a blocker update changed WHICH tiles of the chunk faction f holds (factions[f] != 0, nav_chunk.factions
 * nav_data.h:141) -- what an attacking path that is no enemy of f may cross (field_tile_passable_no_enemies,
 * field.c:179-201) -- whether or not the passability without a faction, and with it the flag above, changed.  Masks, not
 * counters: a second unit on tiles the faction holds already raises nothing, nor do an incref and a decref of one
 * circle in one batch.  Raised by navhip_blockers_circles[_dev] only: uploads raise neither kind of flag.  All zero for
 * a layer without a factions plane.  Runs on the context's stream like navhip_changed_chunks; clear != 0 resets these
 * flags afterwards (and only these: navhip_changed_chunks(.., 1) resets only its own). */
int  navhip_faction_changed_chunks(navhip_ctx *ctx, int layer, uint16_t *host_flags, int clear);
/* Resets both kinds of flags of every layer, asynchronously on `stream` (NULL: the context's). */
int  navhip_clear_changed(navhip_ctx *ctx, void *stream);

/* ---- chunk flow fields ---------------------------------------- */

/* Build n chunk fields.  Replaces the fiber fan-out of field_task (nav.c:2049-2060) joined by
 * N_AwaitAsyncFields (nav.c:3958), and the serial N_FlowFieldInit+N_FlowFieldUpdate pairs inside
 * n_request_path (nav.c:1830-1831,2016-2017).
 *   reqs        host, n records
 *   inout_dirs  host, n * 4096 bytes; slot i is `struct flow_field.field` of request i
 *               (one dir_idx 0..8 per byte, row-major [64][64]).  Read only for requests with
 *               NAVHIP_REQ_INOUT, always written.
 *   out_integ   host, n * 4096 floats or NULL: the integration field (field.c:2059-2077),
 *               INFINITY where unreached.  Debug/parity output; the reference never exposes it. */
int  navhip_build_fields(navhip_ctx *ctx, const navhip_field_req *reqs, int n,
                         uint8_t *inout_dirs, float *out_integ);
/* Same with every buffer resident on the device (no PCIe in the call).  Equal records of one call are built once and the
 * field stored into the slot of each (requests that read their slot -- NAVHIP_REQ_INOUT, the repairs -- excepted); the
 * scratch that finds them belongs to the context: at most ONE chunk-field build of a context (this call,
 * navhip_build_fields, navhip_pool_build, a tick's) may be in flight at a time unless all of them run on one stream. */
int  navhip_build_fields_dev(navhip_ctx *ctx, const navhip_field_req *dev_reqs, int n,
                             uint8_t *dev_inout_dirs, float *dev_out_integ, void *stream);

/* ---- region flow fields ---------------------------------------------------- */

/* One flow field over a square region of nav tiles that may straddle chunks (struct region,
 * field.c; field_build_integration_region field.c:582).  Seeds and overlay-blocked tiles are
 * (abs_r, abs_c) int16 pairs in absolute nav-tile coordinates (chunk * 64 + tile), handed over in
 * two shared arrays.  32 bytes.
 *   out_mode 0  whole region, two 4-bit directions per byte (field_build_flow_unaligned :800):
 *               N_CellArrivalFieldCreate :2445 / N_GroupArrivalFieldCreate :2525; the caller
 *               computes base_abs_* exactly as those functions do (:2475-2488 / :2558-2559)
 *   out_mode 1  the 64x64 window at (roff, coff) of the region written IN PLACE into a chunk field
 *               of one direction per byte (field_build_flow_region :763): field_update_enemies
 *               :1537 / _entity :1615 / _zone :1822, whose frontiers the game side provides */
typedef struct navhip_region_req {
    uint8_t  layer;
    uint8_t  out_mode;
    uint16_t enemies;                 /* 0: field_tile_passable, else ..._no_enemies(enemies)   */
    int16_t  base_abs_r, base_abs_c;  /* region.base; may lie outside the map                   */
    uint16_t rdim, cdim;              /* even, rdim == cdim <= 128                              */
    uint16_t roff, coff;              /* out_mode 1                                             */
    uint32_t seed_begin, seed_count;
    uint32_t overlay_begin, overlay_count;
} navhip_region_req;

/* out: n slots of out_stride bytes (>= rdim*cdim/2 for mode 0, >= 4096 for mode 1).  Mode 0
 * slots are fully written; mode 1 slots are read-modify-write (unreached tiles keep their byte). */
int  navhip_build_region_fields(navhip_ctx *ctx, const navhip_region_req *reqs, int n,
                                const int16_t *seeds, size_t n_seeds,
                                const int16_t *overlay, size_t n_overlay,
                                uint8_t *inout, size_t out_stride);
int  navhip_build_region_fields_dev(navhip_ctx *ctx, const navhip_region_req *dev_reqs, int n,
                                    int max_dim, const int16_t *dev_seeds,
                                    const int16_t *dev_overlay, uint8_t *dev_inout,
                                    size_t out_stride, void *stream);

/* One N_CellArrivalFieldUpdateToNearestPathable(rdim = cdim = dim, layer, start, center, inout, overlay) call
 * (field.c:2603): the pass of cell_field_fixup_task (formation.c:3160) that leads a unit out of the blocked ground it
 * stands on.  Tiles are absolute (chunk * 64 + tile).  The library derives what the reference derives: base = centre -
 * dim / 2 per axis, NOT shifted by a target clamp as N_CellArrivalFieldCreate's is (:2654 against :2483), and the
 * clamped region of the flood (clamped_region :1892; where its far clamp binds, the map's last row or column is not
 * part of the flood).  field_passable_frontier (:1441) floods the blocked ground around `start` over the clamped region
 * and emits the passable tiles beside it -- with the reference's visited index dr * R + dc, which is not injective for a
 * clamped region of more columns than rows (C > R): the FIFO is then replayed operation for operation --; the emitted
 * tiles get 0; field_build_integration_nonpass_region (:678) runs over [base, base + dim)^2 into the tiles that are not
 * passable or lie under the overlay, at the cost_base of the tile entered; every on-map tile with a finite non-zero value
 * gets field_flow_dir (:355), every other nibble keeps what it held.  `enemies` plays no part.  20 bytes. */
typedef struct navhip_region_repair_req {
    uint8_t  layer;
    uint8_t  reserved;                      /* 0 */
    uint16_t dim;                           /* even, 2..128 */
    int16_t  centre_abs_r, centre_abs_c;
    int16_t  start_abs_r, start_abs_c;      /* the unit's tile: not passable */
    uint32_t overlay_begin, overlay_count;  /* a range of the call's overlay array of (abs_r, abs_c) int16 pairs */
} navhip_region_repair_req;
#define NAVHIP_RR_HOST 0x80   /* out_status: not decided here, the slot is untouched and the host decides.  Never a wrong
                                 field.  For: a passable start tile (the reference asserts); a start or centre tile off the
                                 map; a start outside the clamped region (the reference would index its visited array out
                                 of bounds); a layer without resident cost_base and blockers planes; in the resident form,
                                 a row the host form refuses */
/* inout: n slots of `stride` >= dim * dim / 2 bytes, two 4-bit directions per byte as navhip_build_region_fields'
 * out_mode 0 writes them, changed in place.  out_status [n]: 0 or NAVHIP_RR_HOST.
 * NAVHIP_ERR_INVALID, with the reason in navhip_last_error, before anything is launched and with the buffers untouched: a
 * missing array; n < 0; a dim that is odd, 0 or above 128; a layer outside [0, NAVHIP_NAV_LAYER_MAX); a stride below
 * dim * dim / 2; an overlay range outside [0, n_overlay). */
int  navhip_repair_region_fields(navhip_ctx *ctx, const navhip_region_repair_req *reqs, int n,
                                 const int16_t *overlay, size_t n_overlay,
                                 uint8_t *inout, size_t stride, uint8_t *out_status);
/* Every buffer resident on the device, ONE launch on `stream`, no synchronisation: behind navhip_build_region_fields_dev
 * on the same stream and over the same slots this is cell_field_fixup_task.  max_dim: an even bound >= every row's dim
 * (it sizes the launch); a row the host form would refuse, or whose dim exceeds max_dim, comes back NAVHIP_RR_HOST. */
int  navhip_repair_region_fields_dev(navhip_ctx *ctx, const navhip_region_repair_req *dev_reqs, int n, int max_dim,
                                     const int16_t *dev_overlay, uint8_t *dev_inout, size_t stride,
                                     uint8_t *dev_status, void *stream);

/* ---- line-of-sight fields ------------------------------------------------- */

/* One N_LOSFieldCreate(id, chunk_coord, target, priv, map_pos, ctx, out_los, prev_los) call
 * (field.c:2085).  16 bytes.  layer / faction_id are N_DestLayer(id) / N_DestFactionID(id)
 * (nav.c:5052,5057); prev_dr/prev_dc = prev_los->chunk - chunk_coord (0,0: the destination
 * chunk, no previous field). */
typedef struct navhip_los_req {
    uint8_t  layer, faction_id;
    uint16_t enemies;                       /* enemy_faction_from(faction_id), field.c:153 */
    uint16_t chunk_r, chunk_c;
    uint16_t target_chunk_r, target_chunk_c;
    uint8_t  target_tile_r, target_tile_c;
    int8_t   prev_dr, prev_dc;
} navhip_los_req;

/* Build n LOS fields.  A field is 4096 bytes, one per tile, row-major [64][64]:
 * bit 0 = visible, bit 1 = wavefront_blocked (struct LOS_field, field.h:48-54).
 *   prev_fields  host, n * 4096 bytes (slot i = prev_los of request i; ignored for requests
 *                without a previous field) or NULL when no request has one
 *   out_fields   host, n * 4096 bytes
 * Bit-exact with the reference, including the pop order of its binary heap (pqueue.h). */
int  navhip_build_los(navhip_ctx *ctx, const navhip_los_req *reqs, int n,
                      const uint8_t *prev_fields, uint8_t *out_fields,
                      float map_pos_x, float map_pos_z);
int  navhip_build_los_dev(navhip_ctx *ctx, const navhip_los_req *dev_reqs, int n,
                          const uint8_t *dev_prev_fields, uint8_t *dev_out_fields,
                          float map_pos_x, float map_pos_z, void *stream);

/* A resident LOS chain: the LOS fields of a fixed set of (destination, chunk) slots, kept current while blockers move.
 * The reference drops the LOS fields of a dirty chunk together with its flow fields (fieldcache.c:213-227, 526-535) and
 * rebuilds a missing one from the cached field of the chunk before it on the path (nav.c:2026-2039, 4042-4047); a chain
 * does both on the device, behind navhip_blockers_circles[_dev] and from the changed-chunk flags those leave.  A slot
 * may carry a faction (an attacking path): it follows the per-faction flags (navhip_faction_changed_chunks) as well.
 *   reqs, prev_slot  HOST arrays of n entries (copied).  Slot i is field i of dev_pool; prev_slot[i] is the slot of the
 *                    field request i continues (its prev_los), -1 for the destination chunk's own field.  Slots are
 *                    in LEVEL order (level = 0 without a predecessor, else the predecessor's + 1, non-decreasing).
 *   dev_pool         DEVICE, n * 4096 bytes, the caller's: what navhip_world.los_pool points at.  Slots never move.
 * NAVHIP_ERR_INVALID, with the reason in navhip_last_error, unless for every slot: prev_slot[i] == -1 exactly where
 * prev_dr == prev_dc == 0, otherwise 0 <= prev_slot[i] < i; the predecessor's chunk is chunk + (prev_dr, prev_dc) and its
 * layer and target are this slot's; levels do not decrease; the layer is resident -- and where faction_id is not
 * NAVHIP_FACTION_ID_NONE: it is below NAVHIP_MAX_FACTIONS, the layer has a resident factions plane (without one there
 * are no per-faction flags to follow) and the predecessor has the same faction_id and enemies.  Slots with and without
 * a faction may share a chain. */
typedef struct navhip_los_chain navhip_los_chain;
enum { NAVHIP_LOS_REFRESH_DOWNSTREAM = 1u };
typedef struct navhip_los_chain_stats {
    int32_t slots, levels;
    int32_t stale;      /* slots whose own chunk was flagged changed (by either kind of flag), summed over every
                           refresh so far                                                                     */
    int32_t rebuilt;    /* fields the refreshes rebuilt: the same number, plus -- with NAVHIP_LOS_REFRESH_DOWNSTREAM --
                           the fields built from a stale one                                                  */
    int32_t redone;     /* fields a build left to its second launch (more than 1 022 tiles in the frontier)    */
} navhip_los_chain_stats;
int  navhip_los_chain_create(navhip_ctx *ctx, const navhip_los_req *reqs, const int32_t *prev_slot, int n,
                             uint8_t *dev_pool, float map_pos_x, float map_pos_z, navhip_los_chain **out);
/* Every slot, level by level: one pair of launches per level, each field from its predecessor IN the pool (which need
 * not hold anything before).  The bytes navhip_build_los_dev gives level by level.  Asynchronous on `stream`. */
int  navhip_los_chain_build(navhip_los_chain *chain, void *stream);
/* Only what the changed chunks make stale; asynchronous on `stream`, no host round trip, no allocation.
 *   flags 0                              the reference: the fields ON changed chunks are dropped, and each is rebuilt --
 *                                        in level order -- from whatever its predecessor holds then
 *   NAVHIP_LOS_REFRESH_DOWNSTREAM        ... and every field built from a rebuilt one: the pool equals a
 *                                        navhip_los_chain_build on the current planes
 * A slot's chunk is changed when its changed-chunk flag is set, or -- for a slot with a faction -- a per-faction flag of
 * a faction that is not among the slot's enemies: its field reads cost_base, blockers > 0 and, on blocked tiles, the
 * factions rows of non-enemies; the first flag covers the first two, the third only differs when such a row does, and a
 * row of an enemy never matters.  With flags 0 that is a superset of the reference, whose dirty set (nav.c:1036) knows
 * no faction and leaves the field of an attacking path stale when only faction counters moved.
 * Reads the flags and clears nothing: that stays navhip_clear_changed. */
int  navhip_los_chain_refresh(navhip_los_chain *chain, uint32_t flags, void *stream);
/* Waits for the last build / refresh. */
int  navhip_los_chain_get_stats(navhip_los_chain *chain, navhip_los_chain_stats *out);
/* (before the context) */
void navhip_los_chain_destroy(navhip_los_chain *chain);

/* N_FlowFieldID (field.c:1952) for TILE / PORTAL targets: the 64-bit cache key the reference's
 * fieldcache uses; pure bit packing, host side. */
uint64_t navhip_flow_field_id(const navhip_field_req *req);
/* ... and for the region targets (field.h:85-101), whose fields navhip_build_region_fields writes
 * (out_mode 1): kind = the reference's field_target.type,
 *   NAVHIP_FFID_ENEMIES  a = enemies.faction_id
 *   NAVHIP_FFID_ENTITY   a = ent.target (uid)
 *   NAVHIP_FFID_ZONE     a, b = zone.centre in absolute nav tiles (chunk * 64 + tile: row, column),
 *                        c = zone.radius
 * 0 for any other kind. */
enum { NAVHIP_FFID_ENEMIES = 2, NAVHIP_FFID_ENTITY = 4, NAVHIP_FFID_ZONE = 5 };
uint64_t navhip_region_field_id(int kind, int layer, int chunk_r, int chunk_c, uint32_t a, int b, int c);

/* kernel selection override for tests/bench: 0 = auto, 1 = force generic.  Auto: the bit-parallel BFS (one wave per
 * request) builds TILE / PORTAL requests -- with or without a faction, in place or not -- of chunks whose passable cells
 * all cost 1; the generic relaxation (one workgroup per request) builds the requests of chunks with other costs and the
 * two repair builds (NAVHIP_TARGET_NEAREST_PATHABLE, NAVHIP_REQ_ISLAND_NEAREST).  Both are bit-exact. */
int  navhip_set_field_kernel(navhip_ctx *ctx, int mode);
/* How the context's last chunk-field build (navhip_build_fields[_dev], navhip_pool_build) split its requests (waits for
 * that build; its stream must still exist): out[0] = requests the BFS kernel kept (the ones a flag made it skip
 * included), out[1] = requests the generic kernel built.  NAVHIP_ERR_INVALID before the first build. */
int  navhip_last_fields_split(navhip_ctx *ctx, int32_t out[2]);

/* ---- resident flow-field pool (SURVEY.md §8b "Ownership" / the reference's field cache) ------- */

/* A C host has no device pointers: without a device-resident pool every host-buffer call would move
 * the field cache over PCIe again.  The pool keeps chunk fields in HBM under the reference's own
 * 64-bit flow-field ids (N_FlowFieldID, field.c:1952) and mirrors the operations of the reference's
 * cache (fieldcache.c): put / contains / (dest, chunk) -> field mapping; least-recently-used slots
 * are recycled like lru_flow_put (fieldcache.c:411), and mappings that point at a recycled slot drop
 * to "no field".  n_dests = rows of the mapping table; the agent step uses the FLOCK INDEX as row.
 * Called from the nav-tick task only, like the reference's cache (FC_ASSERT_NAV_TASK). */
int  navhip_pool_create(navhip_ctx *ctx, int n_slots, int n_dests);
void navhip_pool_destroy(navhip_ctx *ctx);
int  navhip_pool_clear(navhip_ctx *ctx);                                  /* N_FC_ClearAll              */
int  navhip_pool_contains(navhip_ctx *ctx, uint64_t ff_id);               /* N_FC_ContainsFlowField     */
int  navhip_pool_put(navhip_ctx *ctx, uint64_t ff_id, const uint8_t *dirs);   /* N_FC_PutFlowField: 4096
                                                                              direction bytes from the host */
int  navhip_pool_get(navhip_ctx *ctx, uint64_t ff_id, uint8_t *out_dirs); /* N_FC_FlowFieldAt (a copy)  */
/* lru_flow_remove (the N_FC_Invalidate* family, fieldcache.c:253,520,580) and the eviction of the
 * host cache: the field is dropped and every mapping that points at it becomes "no field" */
int  navhip_pool_invalidate(navhip_ctx *ctx, uint64_t ff_id);
/* Batched N_FlowFieldInit + N_FlowFieldUpdate + N_FC_PutFlowField: request i is built INTO the pool
 * slot of ff_ids[i].  For a NAVHIP_REQ_INOUT request base_ids[i] names the resident field the update
 * starts from (the memcpy of nav.c:1998, the repairs of nav.c:3527-3547); 0 or ff_ids[i] itself = the
 * slot's own content; base_ids may be NULL.  Requests that depend on an earlier request of the same
 * call are ordered behind it.  out_dirs: n * 4096 bytes copied back, or NULL. */
int  navhip_pool_build(navhip_ctx *ctx, const navhip_field_req *reqs, const uint64_t *ff_ids,
                       const uint64_t *base_ids, int n, uint8_t *out_dirs);
/* N_FC_PutDestFFMapping, batched: (dest row, chunk) -> ff_id; an id that is not resident maps to
 * "no field" (the step then reports NAVHIP_ST_FIELD_MISS for agents on that chunk). */
int  navhip_pool_map(navhip_ctx *ctx, int n, const int32_t *dest, const uint16_t *chunk_r,
                     const uint16_t *chunk_c, const uint64_t *ff_ids);
/* navhip_world.n_field_slots value that makes the agent step sample the context's resident pool
 * (field_pool / flock_field_slot are then ignored) */
#define NAVHIP_POOL_RESIDENT (-1)

/* Page-locked host memory: arrays allocated here are transferred by the host-buffer entry points
 * without a staging copy (any other host memory works too, through the library's own pinned slab). */
void *navhip_host_alloc(size_t bytes);
void  navhip_host_free(void *p);

/* ---- per-agent movement step ---------------------------------- */

/* enum move_state, movement.c:113-143 */
enum { NAVHIP_STATE_MOVING = 0, NAVHIP_STATE_MOVING_IN_FORMATION, NAVHIP_STATE_ARRIVED,
       NAVHIP_STATE_SEEK_ENEMIES, NAVHIP_STATE_WAITING, NAVHIP_STATE_SURROUND_ENTITY,
       NAVHIP_STATE_ENTER_ENTITY_RANGE, NAVHIP_STATE_TURNING, NAVHIP_STATE_ARRIVING_TO_CELL };

/* ENTITY_FLAG_* bits the step reads, entity.h:56-82 */
#define NAVHIP_ENTITY_FLAG_MOVABLE      (1u << 3)
#define NAVHIP_ENTITY_FLAG_COMBATABLE   (1u << 4)
#define NAVHIP_ENTITY_FLAG_BUILDING     (1u << 8)
#define NAVHIP_ENTITY_FLAG_WATER        (1u << 14)
#define NAVHIP_ENTITY_FLAG_AIR          (1u << 15)
#define NAVHIP_ENTITY_FLAG_GARRISONED   (1u << 18)
#define NAVHIP_ENTITY_FLAG_COMBAT_HELD  (1u << 21)

/* navhip_step_out.status bits */
#define NAVHIP_ST_MOVED        0x01  /* pos+vel accepted by the position test (movement.c:2356-2358) */
#define NAVHIP_ST_FIELD_MISS   0x02  /* no flow field cached for the agent's chunk: the host must run
                                        the planner (n_request_path, nav.c:3483-3492) and re-step    */
#define NAVHIP_ST_FIELD_NONE   0x04  /* the field has FD_NONE under the agent (nav.c:3495-3554 path)  */
#define NAVHIP_ST_LOS_MISS     0x08  /* NAVHIP_LOS_LOOKUP, but no LOS field is mapped for the agent's chunk   */
#define NAVHIP_ST_UNSUPPORTED  0x80  /* formation state without formation inputs: velocity = 0        */

/* The snapshot the movement tick works on: `struct move_gamestate` + `struct move_work_in` +
 * flock table (movement.c:207-213,264-276,296-312) as structure-of-arrays; uid == array index.
 * All pointers are HOST pointers for navhip_agent_step and DEVICE pointers for
 * navhip_agent_step_dev. */
typedef struct navhip_world {
    int32_t  n_ents;                 /* every entity in the position snapshot                  */
    int32_t  n_flocks;
    int32_t  hz;                     /* movement tick rate: 20/10/5/1 (hz_count, movement.c:2210) */
    int32_t  n_field_slots;          /* slots of field_pool, or NAVHIP_POOL_RESIDENT                */
    const float    *pos_xz;          /* [n][2]  G_Pos_GetXZFrom                                */
    const float    *vel_xz;          /* [n][2]  movestate.velocity (world units per tick)      */
    const float    *radius;          /* [n]     G_GetSelectionRadiusFrom                       */
    const float    *max_speed;       /* [n]     movestate.max_speed                            */
    const float    *speed;           /* [n]     move_work_in.speed                             */
    const uint32_t *flags;           /* [n]     G_FlagsGetFrom                                 */
    const uint8_t  *state;           /* [n]     movestate.state                                */
    const uint8_t  *has_dest_los;    /* [n]     move_work_in.has_dest_los                      */
    const int32_t  *flock;           /* [n]     index into the flock table, -1 = none          */
    const float    *vdes_xz;         /* [n][2]  move_work_in.ent_des_v, or NULL: sample the flow
                                                fields on the device (N_DesiredPointSeekVelocity).
                                                With a non-NULL array, an entry whose x is NaN is
                                                sampled on the device as well                       */
    const float    *flock_target_xz; /* [F][2]  flock.target_xz                                */
    const int32_t  *flock_offsets;   /* [F+1]   CSR offsets into flock_members                 */
    const int32_t  *flock_members;   /* member uids, in kh_foreach order of flock.ents         */
    const int32_t  *flock_field_slot;/* [F][chunks] slot of the (dest,chunk) flow field in
                                                field_pool, -1 = not cached (N_FC_GetDestFFMapping) */
    const uint8_t  *field_pool;      /* [slots][4096] flow fields (one dir_idx per byte)       */
    float    map_pos_x, map_pos_z;   /* vec3 map_pos .x/.z handed to every N_* call            */
    float    grid_xmin, grid_xmax, grid_zmin, grid_zmax;  /* bg_ent_init bounds, position.c:276-283 */
    int32_t  work_begin, work_end;   /* the slab [begin,end) of uids this call computes (the index
                                        slabs of move_submit_cpu_work, movement.c:3759-3762); every
                                        entity still acts as a neighbour (internally only entities
                                        within reach of the slab's queries are indexed, which does
                                        not change any result).  0,0 = all entities               */
    /* Formation inputs, computed by the host's formation module (struct formation_state,
     * movement.c:215-225; move_work_in.cell_pos, :268).  form_ready == NULL: entities in
     * STATE_MOVING_IN_FORMATION / STATE_ARRIVING_TO_CELL are reported NAVHIP_ST_UNSUPPORTED. */
    const uint8_t  *form_ready;      /* [n]     fstate.assignment_ready                          */
    const float    *cell_pos_xz;     /* [n][2]  move_work_in.cell_pos                            */
    const float    *form_cohesion_xz;/* [n][2]  fstate.normal_cohesion_force                     */
    const float    *form_align_xz;   /* [n][2]  fstate.normal_align_force                        */
    const float    *form_drag_xz;    /* [n][2]  fstate.normal_drag_force                         */
    /* Fine-arrival inputs (struct arrival_unit_state, arrival.h:105-128, kept per unit in
     * movestate.arrival; struct arrival_state per flock and nav layer, arrival.h:66-91).  NULL (both):
     * the arrival overlay is inactive for everyone.  The step reads them exactly where the reference
     * does: the seek target of the arrive force is the unit's slot once bits 0 and 1 are set
     * (G_Arrival_SeekTarget, arrival.c:1034; movement.c:1751-1753,1887-1889), and a NEIGHBOUR with bit 0
     * set that stands within 1.5 radii of its slot is a static obstacle for ClearPath
     * (G_Arrival_NeighbourSettling, arrival.c:1042; find_neighbours, movement.c:2815-2817). */
    const float    *arrival_sink_xz; /* [n][2]  movestate.arrival.sink                           */
    const uint8_t  *arrival_flags;   /* [n]     bit 0: substate is SEEK / SEEK_ARMED (unit_committed,
                                                arrival.c:90) and sink_valid; bit 1: the flock's
                                                arrival_state for the unit's nav layer exists and is in
                                                ARRIVAL_PHASE_FILLING                                  */
    /* Per-agent line of sight on the device (compute_los_state movement.c:4129 -> N_HasDestLOS
     * nav.c:4026): an entry of has_dest_los equal to NAVHIP_LOS_LOOKUP is answered from the LOS fields
     * of navhip_build_los -- `visible` of the agent's tile in the (destination, chunk) field.  No field
     * mapped for the chunk: false, and NAVHIP_ST_LOS_MISS is reported so that the host can request the
     * path (nav.c:4041-4047).  All three NULL / 0: every entry of has_dest_los is taken as given. */
    const uint8_t  *los_pool;        /* [slots][4096] LOS fields (bit 0 visible, bit 1 wavefront_blocked) */
    const int32_t  *flock_los_slot;  /* [F][chunks] slot of the (dest, chunk) LOS field, -1 = none       */
    const float    *los_pos_xz;      /* [n][2]  the position the lookup uses: movestate.prev_pos
                                                (movement.c:4137), or NULL = pos_xz                    */
    int32_t  n_los_slots;
    /* Host-buffer calls (navhip_agent_step, _submit) only: a caller that knows that its FLOCK tables --
     * flock, flock_target_xz, flock_offsets, flock_members -- are the ones of its previous call on this
     * context (no entity was added or removed, no flock made, disbanded or re-targeted: G_Move_AddEntity
     * movement.c:4591, G_Move_RemoveEntity :4615, make_flock :789) passes the same nonzero epoch again and
     * those tables are not transferred a second time; 0 = transfer everything (the default).  Everything
     * else always travels: the per-tick state (pos, vel, speed, state, has_dest_los, vdes, formation and
     * arrival inputs) and the per-entity attributes that change without any of those events -- radius,
     * max_speed (MOVE_CMD_SET_MAX_SPEED, movement.c:3226) and flags (ENTITY_FLAG_GARRISONED is toggled
     * outside movement.c).
     * Device-resident calls (navhip_agent_step_dev, _prefetch_dev) read it for one purpose: a caller that steps a
     * uid SLAB (work_begin / work_end) and passes the same nonzero epoch again promises that flock_members is the
     * one of its previous call -- the cohesion term then reuses the lane grouping of the slab's members it made
     * last tick.  0 on a slab call = unknown: the grouping is rebuilt from the flock tables (slower, never wrong).
     * Steps over the whole snapshot do not need it. */
    uint32_t static_epoch;
    /* Region fields sampled on the device: N_DesiredEnemySeekVelocity (nav.c:3603) for STATE_SEEK_ENEMIES and
     * N_DesiredSurroundVelocity (nav.c:3687) for STATE_SURROUND_ENTITY entities that use the surround field
     * (ent_desired_velocity, movement.c:1478-1500).  Those return N_FlowDir of the ONE tile under the entity
     * in the chunk field of an ENEMIES / ENTITY target (navhip_build_region_fields, out_mode 1) -- no blend.
     * region_row[i] >= 0 names the entity's mapping row: a row of region_field_slot ([rows][chunks] slots of
     * field_pool, -1 = not cached), or -- with n_field_slots = NAVHIP_POOL_RESIDENT -- a row of the resident
     * pool's mapping table (navhip_pool_map; rows n_flocks.. are free for this); -1 = the entity samples its
     * flock's point-seek fields as above.  Like there, only entries whose vdes_xz is absent (NULL array or
     * NaN x) are sampled; a missing field / FD_NONE under the entity (the repair builds of nav.c:3652-3683,
     * :3733-3760) is reported as NAVHIP_ST_FIELD_MISS / _NONE.  Both NULL: no region sampling. */
    const int32_t  *region_row;        /* [n] */
    const int32_t  *region_field_slot; /* [n_region_rows][chunks] */
    int32_t  n_region_rows;
} navhip_world;
#define NAVHIP_LOS_LOOKUP 0xff

typedef struct navhip_step_out {
    float   *vel_xz;        /* [n][2]  move_work_out.ent_vel (movement.c:3462-3464); 0 for still ents */
    float   *new_pos_xz;    /* [n][2]  or NULL: pos+vel when accepted, else pos (movement.c:2336-2358) */
    float   *vdes_xz;       /* [n][2]  or NULL: the desired direction used (debug / parity)    */
    float   *vpref_xz;      /* [n][2]  or NULL: preferred velocity before ClearPath (debug / parity) */
    uint8_t *status;        /* [n]     or NULL: NAVHIP_ST_*                                     */
} navhip_step_out;

/* One velocity step for every non-still entity: replaces the WORK_TYPE_CPU / WORK_TYPE_GPU arms of
 * fork_join_velocity_computations (movement.c:4182-4194), i.e. move_velocity_work (:3395) for all
 * work items, plus the position accept test of entity_compute_update (:2336-2358).
 * Host-buffer form: uploads the snapshot, runs, downloads the outputs. */
int  navhip_agent_step(navhip_ctx *ctx, const navhip_world *world, const navhip_step_out *out);
/* Device-resident form (no PCIe in the call), asynchronous on `stream`. */
int  navhip_agent_step_dev(navhip_ctx *ctx, const navhip_world *dev_world,
                           const navhip_step_out *dev_out, void *stream);

/* Asynchronous host-buffer form (SURVEY.md §8b "Threading": the nav task must not block for a tick;
 * the GL path polls a fence once per frame, movement.c:4212-4233): submit stages the inputs through
 * pinned memory and returns at once; poll returns 1 while the step is running and 0 once the outputs
 * are in the caller's arrays (wait blocks until then).  One step in flight per context; the caller's
 * arrays must stay untouched between submit and completion. */
int  navhip_agent_step_submit(navhip_ctx *ctx, const navhip_world *world, const navhip_step_out *out);
int  navhip_agent_step_poll(navhip_ctx *ctx);
int  navhip_agent_step_wait(navhip_ctx *ctx);

/* Optional overlap: start the parts of the step that depend only on the snapshot (the spatial hash
 * and the O(N*F) cohesion term) on the context's own side streams, forked from `stream`, and return
 * at once.  Work enqueued on `stream` afterwards (e.g. the tick's field builds) then runs
 * concurrently with them; the next navhip_agent_step_dev on the same snapshot arrays joins the side
 * streams instead of recomputing.  Purely a scheduling hint: results are identical.
 * The side streams read the snapshot arrays until that step has completed on ITS stream (work the
 * caller enqueues there afterwards is ordered behind the last read); a prefetch that is never
 * followed by a step is drained by navhip_sync. */
int  navhip_agent_prefetch_dev(navhip_ctx *ctx, const navhip_world *dev_world, void *stream);
/* flags: NAVHIP_PREFETCH_FRONT_INLINE  the spatial hash and the neighbour walk stay on `stream` itself
 * (only the cohesion term forks): for a caller that enqueues nothing wide on `stream` between this call
 * and the step -- the chain then follows the previous step on the same stream without a hand-over. */
#define NAVHIP_PREFETCH_FRONT_INLINE 0x1u
/*        NAVHIP_PREFETCH_SNAPSHOT_HELD  the caller leaves the snapshot arrays of this call untouched until
 * its NEXT step on this context has been enqueued (it ping-pongs its position / velocity buffers): the
 * step then does not make the caller's stream wait for the lane regrouping the cohesion stream runs
 * for the next tick -- that work is ordered in front of the next step's cohesion term anyway. */
#define NAVHIP_PREFETCH_SNAPSHOT_HELD 0x2u
/*        NAVHIP_PREFETCH_FOLLOWS_STEP   every array of the snapshot was final when the last navhip_agent_step_dev
 * on `stream` ended, and nothing was enqueued on `stream` since that this call has to follow (a tick loop that
 * ping-pongs the outputs of one step into the snapshot of the next): the side streams then start behind a word the
 * step stored in device memory when it ended, instead of behind an event recorded on `stream` now -- one packet less
 * in front of the spatial hash.  Ignored when the last step did not run on `stream`. */
#define NAVHIP_PREFETCH_FOLLOWS_STEP 0x4u
int  navhip_agent_prefetch_dev_ex(navhip_ctx *ctx, const navhip_world *dev_world, void *stream, uint32_t flags);
/* Scheduling hint for a caller that runs other wide work (the field builds of the NEXT tick, say)
 * beside the agent step: make `stream` wait until the given stage of the step in flight is done, so
 * that the narrow, serial front of the step is not slowed down by it.
 *   NAVHIP_STAGE_START       the moment the last navhip_agent_prefetch_dev was forked from its stream
 *                            (= the previous step on that stream has finished)
 *   NAVHIP_STAGE_NEIGHBOURS  spatial hash + neighbour walk of the last navhip_agent_prefetch_dev
 *   NAVHIP_STAGE_LISTS       preferred velocities + work lists of the last navhip_agent_step_dev
 *   NAVHIP_STAGE_END         the last navhip_agent_step_dev has written its outputs (NAVHIP_ERR_INVALID when that step
 *                            ran on one stream, without side streams: its stream is its end -- order behind that)
 * (NAVHIP_ERR_INVALID when that call has not been made).  The wait is a one-lane kernel on `stream` that ends when the
 * stage's word in device memory has been stored -- no event, no packet on the step's own streams; 2-3 us from the
 * store to the next kernel on `stream` --, or an event wait where the step itself hands over
 * through events: in a jam, under rocprofv3 --pmc, with NAVHIP_HANDOVER=events in the environment. */
#define NAVHIP_STAGE_NEIGHBOURS 0
#define NAVHIP_STAGE_LISTS      1
#define NAVHIP_STAGE_START      2
#define NAVHIP_STAGE_END        3
int  navhip_stream_wait_stage(navhip_ctx *ctx, void *stream, int stage);

/* Per-kernel-group timing of the agent step with HIP events on the launch stream (bench.py's
 * roofline line).  A profiled navhip_agent_step[_dev] runs every kernel group back to back on the
 * caller's stream (no side streams); navhip_last_step_ms then returns, in milliseconds,
 * {spatial-hash build, neighbour walk (k_agent_nbr), k_cohesion, cohesion lane regrouping,
 *  k_agent_mid + the ClearPath searches} (it waits for the step). */
#define NAVHIP_STEP_PHASES 5
int  navhip_set_profiling(navhip_ctx *ctx, int on);
int  navhip_last_step_ms(navhip_ctx *ctx, float out_ms[NAVHIP_STEP_PHASES]);

/* Work counters of the context since creation (or the last reset): what SURVEY.md section 5 asks the shim
 * to expose so that a host can report cells/s and agent-steps/s with its own clock (one chunk field
 * = 4096 cells; host counters, no device synchronisation). */
typedef struct navhip_counters {
    uint64_t field_calls;     /* navhip_build_fields / _dev / pool builds                          */
    uint64_t chunk_fields;    /* chunk-field requests in them                                      */
    uint64_t step_calls;      /* navhip_agent_step / _dev / _submit                                */
    uint64_t agent_steps;     /* work items (work_end - work_begin) in them                        */
    uint64_t los_fields;      /* navhip_build_los requests                                         */
    uint64_t region_fields;   /* navhip_build_region_fields requests                               */
    uint64_t blocker_circles; /* navhip_blockers_circles entries                                   */
} navhip_counters;
int  navhip_get_counters(navhip_ctx *ctx, navhip_counters *out, int reset);
/* How the last agent step split its agents (waits for it): the number of agents whose ClearPath ran
 * on a row of 16 lanes ([0..3]: 1-2, 3-4, 5-8, 9-16 neighbours), on a wave ([4]: 17-64 neighbours),
 * and agents whose whole step ran on a wave ([5]: garrisoned neighbours / wide queries).  Everyone
 * else has no ClearPath neighbour and finished in the thread-per-agent pass. */
int  navhip_last_step_lists(navhip_ctx *ctx, int32_t out_counts[6]);
/* The same without waiting: the counts of the most recent step whose copy has ARRIVED (the library sends them to
 * pinned host memory behind every step, on its side stream) -- one or two steps old, zeros before the first.
 * For a host that adapts its schedule to the crowd: tick.py starts the next tick's field builds with the tick
 * instead of behind the neighbour walk once the workgroup searches ([4]) would starve them of registers. */
int  navhip_step_lists_peek(navhip_ctx *ctx, int32_t out_counts[6]);

/* ClearPath retry statistics of this process since the last reset (diagnostics: bench.py's status
 * histogram): out[k], k = 1..7 = searches that returned in attempt k + 1 of G_ClearPath_NewVelocity's
 * remove_furthest loop (clearpath.c:704-713; [7]: eight or more), out[0] = searches that gave up with a
 * list empty, out[8] = attempts of all retried searches.  Waits for the device. */
int  navhip_debug_cp_attempts(unsigned long long out[9], int reset);

/* ---- more than one GPU: the tick's exchange step for a C host --------- */

/* One process per GPU, one context per process.  The path shards without any data-path collective
 * (requests by destination, uid slabs of the velocity step: movement.c:3759-3762) up to ONE exchange per
 * tick: all ranks need all rows of [new position | velocity] before the next tick's neighbour queries.
 * These entry points call librccl directly (loaded on first use; RCCL over xGMI on an MI355X node), so
 * that the reference's C host does not need torch.distributed.
 *   rank 0 makes the id (ncclGetUniqueId) and hands its 128 bytes to the other ranks by whatever means
 *   the host has (a file, a socket, an environment variable); every rank then calls navhip_comm_init. */
#define NAVHIP_COMM_ID_BYTES 128
int  navhip_comm_unique_id(uint8_t out_id[NAVHIP_COMM_ID_BYTES]);
int  navhip_comm_init(navhip_ctx *ctx, int rank, int world, const uint8_t id[NAVHIP_COMM_ID_BYTES]);
/* The same exchange without RCCL, for bringing the step up on one device or behind a transport of the host's
 * own: the "network" is dev_mailbox, a device buffer laid out like the gathered array ([n][4] floats for
 * navhip_comm_allgather_step_dev, the rows themselves for _rows_dev).  A call deposits this rank's rows there and
 * takes every other rank's rows from there -- the caller has put them in (or moves the mailbox between ranks by
 * whatever means it has).  Packing, slab bounds, the ragged grouping and unpacking are the code RCCL runs behind;
 * the GPU tests drive every rank of a 2-, 3- and 4-rank job through it on one device. */
int  navhip_comm_init_mailbox(navhip_ctx *ctx, int rank, int world, void *dev_mailbox, size_t mailbox_bytes);
void navhip_comm_destroy(navhip_ctx *ctx);
int  navhip_comm_rank(const navhip_ctx *ctx);     /* -1 without a communicator */
int  navhip_comm_world(const navhip_ctx *ctx);    /*  0 without a communicator */
/* The slab results of navhip_agent_step_dev -> every rank, in place, asynchronous on `stream`:
 * bounds[r] .. bounds[r + 1] = the uid slab rank r stepped (bounds[0] = 0, bounds[world] = n_ents).  ONE
 * collective: the rank's rows are packed into [n][4] floats (16 B per agent), all-gathered
 * (ncclAllGather for equal slabs, a group of ncclBroadcast for ragged ones), and the other ranks' rows
 * unpacked into dev_new_pos_xz / dev_vel_xz. */
int  navhip_comm_allgather_step_dev(navhip_ctx *ctx, float *dev_new_pos_xz, float *dev_vel_xz,
                                    const int32_t *bounds, void *stream);
/* The same for any row array (baked 4 KB flow tiles: row_bytes = 4096, bounds over the request stream). */
int  navhip_comm_allgather_rows_dev(navhip_ctx *ctx, void *dev_rows, size_t row_bytes, const int32_t *bounds,
                                    void *stream);

/* ---- the whole tick behind ONE call (host code stays in C: the per-tick orchestration is the library's) ------- */

/* The reference runs its navigation tick from one place: move_do_tick (movement.c:4312) -> navigation_tick_task
 * (:4263-4280): field work, the velocity fork-join, the state fork-join, the snapshot for the next tick.  A navhip_tick
 * is that loop for a device-resident world: every call of navhip_tick_run enqueues, per tick,
 *   - the chunk-field builds of this context's share of the requests (into the pool slot of each request; with a second
 *     pool the fields tick t+1 samples are built DURING tick t on a stream of their own, behind the narrow front of
 *     the step -- the schedule DESIGN.md section 4 describes),
 *   - [dynamic obstacles] the tick's N_BlockersIncref/Decref batch in front of them (incremental repair),
 *   - the velocity step + position accept of the uid slab (navhip_agent_prefetch_dev + navhip_agent_step_dev),
 *   - [a communicator on the context] the slab exchange (navhip_comm_allgather_step_dev) on a stream of its own, which
 *     only the snapshot consumers of the next tick wait for,
 *   - the advance of the snapshot: position / velocity buffers and the two pools ping-pong.
 * Nothing is waited for; the host returns after a few dozen launches.  Results are those of the separate calls, bit for
 * bit: the same kernels on the same buffers in the same order per stream. */
typedef struct navhip_tick navhip_tick;
#define NAVHIP_TICK_SERIAL 0x2u   /* the whole tick on ONE stream: no side streams, no events, the fields in front of
                                     the step of their own tick (field_pool_1 unused).  For small worlds, whose tick is a
                                     chain of short dependent launches: every cross-stream edge costs a barrier packet
                                     (10-20 us once the host runs ahead of the device) and buys no overlap there --
                                     configs[0] 0.27 -> ... ms per tick (profiles/r05_host_overhead_*.txt)              */
#define NAVHIP_TICK_TIME_FIELDS 0x8u /* time the field builds of every fourth tick with two HIP events on the FIELD stream (no
                                     packet on the agent stream): navhip_tick_info.fields_ms / fields_samples -- how long
                                     the builds take INSIDE the tick, beside the agent step they overlap with           */
#define NAVHIP_TICK_OWNS_SNAPSHOT 0x10u /* between two ticks the caller enqueues nothing on the tick's stream that the next
                                     tick has to follow, and writes the snapshot buffers only with the device idle: the side
                                     streams of tick t+1 then start behind a word tick t stored in device memory when it
                                     ended (NAVHIP_PREFETCH_FOLLOWS_STEP) -- inside one navhip_tick_run that is so anyway  */
typedef struct navhip_tick_desc {
    navhip_world world;             /* DEVICE arrays of the snapshot (buffer set 0: pos_xz, vel_xz, field_pool);
                                       work_begin/work_end = this rank's uid slab                                      */
    float    *pos_xz_1, *vel_xz_1;  /* [n][2] buffer set 1: tick t reads set (t & 1) and writes the other               */
    uint8_t  *status;               /* [n] NAVHIP_ST_* or NULL                                                          */
    float    *vdes_xz, *vpref_xz;   /* [n][2] or NULL (debug / parity outputs of navhip_step_out)                       */
    const navhip_field_req *dev_reqs;   /* this rank's chunk-field requests, rebuilt every tick (device)                */
    int32_t   n_reqs;
    int32_t   req_slot0;            /* request i is built into slot req_slot0 + i of the pool                           */
    uint8_t  *field_pool_1;         /* [slots][4096] second pool: the fields of tick t+1 are built during tick t into the
                                       pool tick t does not sample; NULL = built in front of the step of their own tick */
    int32_t   field_cus;            /* compute units the ahead builds may use (the last field_cus of the device); 0 = all */
    int32_t   fields_stage;         /* NAVHIP_STAGE_NEIGHBOURS / NAVHIP_STAGE_START: where in tick t they start         */
    const navhip_circle *dev_moves; /* [n_move_ticks][n_moves] the N_BlockersIncref/Decref batch of every tick, or NULL */
    int32_t   n_moves, n_move_ticks;
    int32_t   move_tick0;           /* the batch of this object's first tick (tick k applies row (move_tick0 + k) % n_move_ticks) */
    const int32_t *bounds;          /* HOST [world + 1] uid slabs of the ranks: the exchange of navhip_comm_allgather_step_dev
                                       through the context's communicator every tick; NULL = no exchange                */
    void     *stream, *field_stream, *comm_stream;   /* hipStream_t or NULL = streams of the library's own              */
    uint32_t  flags;                /* NAVHIP_TICK_*                                                                    */
} navhip_tick_desc;
typedef struct navhip_tick_info {
    int64_t  ticks;                 /* ticks enqueued so far: the current snapshot is buffer set (ticks & 1)            */
    double   host_enqueue_ms;       /* host time spent inside navhip_tick_run since creation                            */
    void    *stream, *field_stream, *comm_stream;
    double   fields_ms;             /* NAVHIP_TICK_TIME_FIELDS: mean duration of the timed field builds that have finished */
    int32_t  fields_samples, _pad;
} navhip_tick_info;
int  navhip_tick_create(navhip_ctx *ctx, const navhip_tick_desc *desc, navhip_tick **out);
/* Enqueue n ticks; asynchronous. */
int  navhip_tick_run(navhip_tick *tick, int n);
/* The two halves for a host with a transport of its own between them (tick.py's torch.distributed exchange):
 * compute = everything up to the exchange of ONE tick, advance = the ping-pong behind the host's exchange. */
int  navhip_tick_compute(navhip_tick *tick);
int  navhip_tick_advance(navhip_tick *tick);
/* A LOS chain for the tick to keep current (NULL: none, the default): every tick that applies a batch of dev_moves
 * enqueues navhip_los_chain_refresh(chain, flags, the tick's stream) behind the batch and in front of the
 * navhip_clear_changed that ends it -- in front of the step that samples the pool.  The chain stays the caller's. */
int  navhip_tick_set_los_chain(navhip_tick *tick, navhip_los_chain *chain, uint32_t flags);
int  navhip_tick_sync(navhip_tick *tick);
int  navhip_tick_get_info(const navhip_tick *tick, navhip_tick_info *out);
void navhip_tick_destroy(navhip_tick *tick);

/* ---- the arrival arm of the movement state machine --------------------------- */

/* entity_compute_update (movement.c:2303) decides, per unit and tick, the next movement state.  Most of it is
 * game logic over host state (orientation and the heading gate, formations, the arrival overlay, surround
 * targets, wait timers) and stays with the host.  The part every point-seeking unit runs every tick is the
 * STATE_MOVING / STATE_MOVING_IN_FORMATION case without a formation and without an active arrival group
 * (:2441-2520) -- and that part is data parallel:
 *   1. garrisoned and not still          -> STATE_ARRIVED, no blocker                       (:2344-2351)
 *   2. new position not pathable         -> no transition                                   (:2437-2438)
 *   3. arrived(uid, new_pos) (:2170): within 1.5 radii of the flock target; or adjacent to an impassable
 *      tile (N_IsAdjacentToImpassable, nav.c:4745) and maximally close to the target (N_IsMaximallyClose,
 *      nav.c:4707: within that distance of one of the destination's closest island tiles); or within it of
 *      N_ClosestPathable(target) (nav.c:4126)                 -> STATE_ARRIVED, blocker
 *   4. a flock mate within radius + radius + 5 has arrived (adjacent_flock_members :953, :2480-2497)
 *                                                             -> STATE_ARRIVED, blocker
 *   5. no guidance: |vdes| < 1/1024                           -> STATE_WAITING, blocker     (:2508-2515)
 * The two nav queries of step 3 depend on the destination only; the host makes them once per flock
 * (flock_nearest_xz, flock_tiles) and the device runs the per-unit tests.  Everything else is reported
 * back as NAVHIP_SU_HOST (the host runs entity_compute_update for that unit as before). */
#define NAVHIP_SU_SET_STATE  0x01   /* UPDATE_SET_STATE: next_state holds the new state                       */
#define NAVHIP_SU_BLOCK      0x02   /* movestate_patch.next_block                                            */
#define NAVHIP_SU_HOST       0x80   /* not decided here: another state, skip[i] != 0 (an active arrival zone:
                                       navhip_arrival_settle; a rate below 20 Hz), or a unit whose nav layer is
                                       not its flock's.  Formation members need not be skipped: see
                                       navhip_state_update_aux                                                 */
typedef struct navhip_state_in {
    const float    *new_pos_xz;       /* [n][2] the position entity_compute_update tests: new_pos_for_vel(uid,
                                                new_vel) (movement.c:2338) -- position + the velocity of the tick
                                                AFTER the heading gate (:2321-2334) -- at 20 Hz; at lower movement
                                                rates the interpolated intermediate position that replaces it
                                                (:2368-2377) -- or mark those units in `skip` (the binding does) */
    const float    *vdes_xz;          /* [n][2] move_work_out.ent_des_v                                        */
    const uint8_t  *skip;             /* [n] or NULL                                                           */
    const uint8_t  *flock_layer;      /* [F]    the nav layer flock_nearest_xz / flock_tiles were made for     */
    const float    *flock_nearest_xz; /* [F][2] N_ClosestPathable(layer, flock.target_xz); x = NaN: none       */
    const int32_t  *flock_tiles_off;  /* [F+1]  CSR offsets into flock_tiles                                   */
    const int16_t  *flock_tiles;      /* [..][2] absolute nav tiles (row, column) of n_closest_island_tiles(
                                                 dest tile, its global island, false), nav.c:4725, in order    */
} navhip_state_in;
/* world: the snapshot of the tick (pos_xz, radius, flags, state, flock, flock tables; uid slab
 * work_begin/work_end as in the step).  out_state / out_flags: [n] bytes, rows of the slab written.
 * Host buffers. */
int  navhip_state_update(navhip_ctx *ctx, const navhip_world *world, const navhip_state_in *in,
                         uint8_t *out_state, uint8_t *out_flags);
/* Everything resident on the device, asynchronous on `stream`. */
int  navhip_state_update_dev(navhip_ctx *ctx, const navhip_world *dev_world, const navhip_state_in *dev_in,
                             uint8_t *dev_out_state, uint8_t *dev_out_flags, void *stream);

/* ---- the two destination queries of arrived() on the device ----------------------------------------------------
 *
 * flock_nearest_xz and flock_tiles above (and range_tiles of navhip_state_aux_in below) are answers of two nav queries
 * that depend on the destination only: N_ClosestPathable(layer, target) (nav.c:4126) and the tiles N_IsMaximallyClose
 * walks (nav.c:4707): n_closest_island_tiles(dest tile, its global island id, ignore_blockers = false) (nav.c:1226,
 * called at :4725).  Both read the blockers, which every unit that stops or starts changes: a host that caches them has
 * to ask again on almost every tick.  These entry points answer them from the resident planes -- the probemask rows
 * (cost_base != 0xff, blockers > 0: n_tile_blocked, nav.c:235), kept current behind navhip_blockers_circles[_dev], and
 * NAVHIP_PLANE_ISLANDS -- bit for bit, the order of the tile list included.  16 bytes. */
typedef struct navhip_dest_query { float x, z; int32_t layer; uint32_t flags; } navhip_dest_query;
#define NAVHIP_DQ_NEAREST  0x1u   /* N_ClosestPathable(layer, (x, z))                                            */
#define NAVHIP_DQ_TILES    0x2u   /* the closest island tiles of (x, z)                                          */
#define NAVHIP_DQ_HOST     0x80   /* out_status: not decided here -- a search that has to visit a tile outside the window
                                     of 127 x 127 tiles centred on the destination's tile (a map that fits the window
                                     never does).  The row's nearest is (NaN, 0) and its tile list is empty, as with
                                     NAVHIP_SU_HOST: the host makes both queries for that row                    */
/* n queries, host buffers.  The outputs have the shapes of navhip_state_in.flock_nearest_xz / .flock_tiles_off /
 * .flock_tiles and navhip_state_aux_in.range_tiles_off / .range_tiles:
 *   out_nearest_xz [n][2]   the answer of NAVHIP_DQ_NEAREST; (NaN, 0) when the reference returns false (nothing on the map
 *                           is free) or the bit was not asked for
 *   out_tiles_off  [n + 1]  CSR offsets into out_tiles
 *   out_tiles      [tiles_cap][2]  absolute nav tiles (row, column) in the reference's output order, at most 256 per
 *                           query (FIELD_RES_R * 2 + FIELD_RES_C * 2, nav.c:4722); empty without NAVHIP_DQ_TILES
 *   out_status     [n]      0 = answered, NAVHIP_DQ_HOST
 * tiles_cap < 256 * n is accepted when the lists fit; when they do not -- known once the queries have run -- the call fails
 * with NAVHIP_ERR_ARG and no output is written.
 * NAVHIP_ERR_ARG, with the reason in navhip_last_error and before anything is launched: flags without a known bit or
 * with an unknown one; a layer without resident cost_base and blockers planes, or -- with NAVHIP_DQ_TILES -- without the
 * islands plane; a position outside the map (the reference asserts there). */
int  navhip_dest_queries(navhip_ctx *ctx, const navhip_dest_query *q, int n, float map_pos_x, float map_pos_z,
                         float *out_nearest_xz, int32_t *out_tiles_off, int16_t *out_tiles, int tiles_cap,
                         uint8_t *out_status);
/* Everything resident on the device, asynchronous on `stream`, no allocation after the first call at a given n: the
 * results can be handed to navhip_state_update_dev as they are.  The records are not readable before the launch: a
 * row the host form would refuse comes back NAVHIP_DQ_HOST.  dev_out_tiles_off always holds the true offsets; tiles
 * beyond tiles_cap are not written (dev_out_tiles_off[n] > tiles_cap says so). */
int  navhip_dest_queries_dev(navhip_ctx *ctx, const navhip_dest_query *dev_q, int n, float map_pos_x, float map_pos_z,
                             float *dev_out_nearest_xz, int32_t *dev_out_tiles_off, int16_t *dev_out_tiles, int tiles_cap,
                             uint8_t *dev_out_status, void *stream);

/* ---- the two unit queries of STATE_SURROUND_ENTITY on the device ---------------------------------------------------
 *
 * navhip_state_aux_in.surround_query / .surround_dest_xz (below) are the answers of M_NavObjAdjacentFrom (map.c:1061 ->
 * n_objects_adjacent, nav.c:1682: do the unit's tiles touch the target's?) and M_NavClosestReachableAdjacentPosFrom
 * (map.c:860 -> n_closest_adjacent_pos, nav.c:1636: the closest reachable tile next to the target, one
 * n_closest_island_tiles flood per tile under the target's circle) from both positions the tick can test.  Both read the
 * blockers; for a MOVABLE target these entry points answer them from the resident planes (probemask rows, islands), bit
 * for bit with the reference.
 *   world          n_ents, pos_xz, radius, flags, map_pos_x / _z
 *   new_vel_xz     [n_ents][2] the ungated velocity of the step (move_work_out.ent_vel)
 *   units, target  [nq] row k concerns unit units[k] and target row target[k] (< 0: no target).  units == NULL is the
 *                  dense form: nq == n_ents and row i is unit i -- the sparse and the dense layouts of
 *                  navhip_state_aux_in
 *   out_query      [nq] NAVHIP_SQ_ADJACENT | NAVHIP_SQ_HAS_DEST_0 | NAVHIP_SQ_HAS_DEST_1 | NAVHIP_SQ_HOST.  No target: 0.
 *                  Touching: NAVHIP_SQ_ADJACENT alone, nothing else is computed.
 *   out_dest_xz    [nq][2][2] the closest position from pos + new velocity ([k][0]) and from pos ([k][1]): the corner of
 *                  the winning tile; 0 where the bit is clear
 * NAVHIP_SQ_HOST is never a wrong answer.  It comes back for: a target row >= n_ents; a target without
 * NAVHIP_ENTITY_FLAG_MOVABLE (a static target is answered by navhip_surround_queries_ex below); ceil(radius / 4) of unit or target
 * above 8 (radius 32); a NaN radius or position; a source off the map (the reference asserts there); a flood of the row
 * that has to push a tile outside the window of 127 x 127 tiles centred on its target tile in front of its answer (the
 * rule of NAVHIP_DQ_HOST).
 * NAVHIP_ERR_ARG, with the reason in navhip_last_error, before anything is launched and with the outputs untouched: a
 * missing array; nq < 0; the dense form with nq != n_ents; a unit row outside [0, n_ents); a unit on a layer
 * (Entity_NavLayerWithRadius of its flags and radius) without resident cost_base, blockers and islands planes. */
#define NAVHIP_SQ_HOST 0x80   /* out_query: not decided here; the row's other bits are 0 and its dest is 0 */
int  navhip_surround_queries(navhip_ctx *ctx, const navhip_world *world, const float *new_vel_xz,
                             const int32_t *units, const int32_t *target, int nq,
                             uint8_t *out_query, float *out_dest_xz);
/* Everything resident on the device (dev_world: a host struct of device pointers), asynchronous on `stream`, no
 * allocation after the first call at a given nq: the dense form's outputs can be handed to navhip_state_update_aux_dev
 * as they are.  The rows are not readable before the launch: a unit row outside the world or on a layer without
 * resident planes comes back NAVHIP_SQ_HOST. */
int  navhip_surround_queries_dev(navhip_ctx *ctx, const navhip_world *dev_world, const float *dev_new_vel_xz,
                                 const int32_t *dev_units, const int32_t *dev_target, int nq,
                                 uint8_t *dev_out_query, float *dev_out_dest_xz, void *stream);

/* ---- the same two queries for a STATIC target (a resource, a storage site, a building) ---------------------------------
 *
 * The reference answers them from the tile list of the target's OBB: N_ObjAdjacentToStaticWith (nav.c:4932) and
 * N_ClosestReachableAdjacentPosStatic (nav.c:4621) call M_Tile_AllUnderObj (tile.c:594) and then the functions above.
 * Buildings do not move: the host computes a building's list once, with the reference's own M_Tile_AllUnderObj, and
 * registers it here.  Nothing rasterises an OBB on the device.
 *
 * navhip_static_targets_set replaces the context's whole table of lists (n_sets == 0 clears it; the table is freed with
 * the context).  tiles_off [n_sets + 1] is a CSR index into tiles[][2], absolute nav tiles (row, column) in the order
 * M_Tile_AllUnderObj returned them, duplicates and all, at most 2048 per list (the reference's tds[2048]; a list the
 * reference truncated is passed truncated).  The library keeps the first occurrence of every tile of a list, in order:
 * a later duplicate can neither win n_closest_adjacent_pos's strict < nor change n_objects_adjacent.
 * NAVHIP_ERR_ARG, with the reason in navhip_last_error and the table as it was: a missing array, non-monotonic offsets, a
 * list longer than 2048, a tile off the map.  The call waits for the context's stream; a query on another stream that
 * still reads the old table is the caller's to wait for. */
int  navhip_static_targets_set(navhip_ctx *ctx, int n_sets, const int32_t *tiles_off, const int16_t *tiles);
/* navhip_surround_queries[_dev] with target_set [nq]: the table row of row k's target when that target has no
 * NAVHIP_ENTITY_FLAG_MOVABLE; ignored for a MOVABLE target.  target_set == NULL is navhip_surround_queries[_dev], bit for
 * bit.  Outputs as above.  A static row is answered in LIST order: of equal lengths the earlier entry of the list wins,
 * whichever tile its answer is.  It comes back NAVHIP_SQ_HOST only for: a set outside the table or an empty table (device
 * form; the host form refuses the call with NAVHIP_ERR_ARG before anything is launched); ceil(radius / 4) of the unit
 * above 8; a NaN radius or position of the unit; a source off the map; a flood that has to leave the window of 127 x 127
 * tiles around the list entry it starts on.  The length of the list is never a reason.  The scratch is sized from nq and
 * the longest registered list: no allocation after the first call at a given nq and table. */
int  navhip_surround_queries_ex(navhip_ctx *ctx, const navhip_world *world, const float *new_vel_xz,
                                const int32_t *units, const int32_t *target, const int32_t *target_set, int nq,
                                uint8_t *out_query, float *out_dest_xz);
int  navhip_surround_queries_ex_dev(navhip_ctx *ctx, const navhip_world *dev_world, const float *dev_new_vel_xz,
                                    const int32_t *dev_units, const int32_t *dev_target, const int32_t *dev_target_set,
                                    int nq, uint8_t *dev_out_query, float *dev_out_dest_xz, void *stream);

/* ---- the nav queries of an order on the device: reachable destination, tile in range ------------------------------------
 *
 * When a SET_DEST or SET_ENTER_RANGE command is carried out (move_process_cmds, movement.c:3246) the reference asks, per
 * unit and on the main thread: M_NavClosestReachableInRange (do_set_enter_range, movement.c:3069-3092; combat.c:491 issues
 * it for every ranged unit that picks a target), M_NavClosestReachableDest and M_NavDestIDForPos[Attacking] (do_set_dest,
 * movement.c:2951-2972; make_flock :804, :845-847 once per flock) and M_NavLocationsReachable (combat.c:486).  One row of
 * these entry points is that chain for one unit, from NAVHIP_PLANE_ISLANDS, bit for bit with the reference:
 *   t = flags & NAVHIP_OQ_IN_RANGE  ? N_ClosestReachableInRange(src, dst, range, layer)  (nav.c:5067)  : dst
 *   d = flags & NAVHIP_OQ_REACHABLE ? N_ClosestReachableDest(layer, src, t)              (nav.c:4085)  : t
 *   out_dest_xz = d;  out_dest_id = faction == 15 (FACTION_ID_NONE) ? N_DestIDForPos(d, layer)
 *                                                                   : N_DestIDForPosAttacking(d, layer, faction)
 * Both flags: the nav part of do_set_enter_range.  NAVHIP_OQ_REACHABLE alone: that of do_set_dest / make_flock.  Neither: a
 * dest id and the reachability bit.  `range` is the value the caller passes to N_ClosestReachableInRange: the arithmetic of
 * movement.c:3080, :3091 and the already-in-range early-out stay the host's.  It is checked on every row, used or not.
 * THE QUERIES READ THE ISLANDS PLANE ONLY, no blockers (the flood of N_ClosestReachableDest runs with ignore_blockers =
 * true): the answers change only when the host uploads a new islands plane.
 * The in-range tile is the CORNER of the winning tile (nav.c:5109-5112), the reachable destination the CENTRE of the first
 * tile of the source's island in the flood's queue order (nav.c:4119-4122).  N_ClosestReachableDest's "no tile found:
 * return xz_src" arm is written, and no world reaches it: the source's own tile is of the source's island, a hit once the
 * flood gets there.  32 bytes. */
typedef struct navhip_order_query { float src_x, src_z, dst_x, dst_z, range; int32_t layer; int32_t faction; uint32_t flags; } navhip_order_query;
#define NAVHIP_OQ_IN_RANGE     0x1u   /* t = N_ClosestReachableInRange(src, dst, range, layer); else t = dst           */
#define NAVHIP_OQ_REACHABLE    0x2u   /* d = N_ClosestReachableDest(layer, src, t); else d = t                         */
#define NAVHIP_OQ_SAME_ISLAND  0x01   /* out_status: N_LocationsReachable(layer, src, dst) of the row's original dst (nav.c:4593) */
#define NAVHIP_OQ_NO_TILE      0x02   /* out_status: the in-range search found no tile of the source's island and returned
                                         the target (nav.c:5124)                                                       */
#define NAVHIP_OQ_HOST         0x80   /* out_status: not decided here; the row's other bits are 0, its dest is (NaN, 0) and
                                         its dest id 0.  Never a wrong answer.  For: a flood of N_ClosestReachableDest whose
                                         answer lies outside the window of 127 x 127 tiles centred on the tile it starts on
                                         (the rule of NAVHIP_DQ_HOST; a map that fits the window never does); in the resident
                                         form, a row the host form refuses                                              */
/* n rows, host buffers.  out_dest_xz [n][2], out_dest_id [n], out_status [n].
 * NAVHIP_ERR_ARG, with the reason in navhip_last_error, before anything is launched and with the outputs untouched: a
 * missing array; n < 0; unknown flag bits; a layer outside [0, NAVHIP_NAV_LAYER_MAX) or without a resident islands plane; a
 * faction outside [0, 15]; a NaN coordinate or range; src or dst (the in-range search's target) off the map (the reference
 * asserts there); ceil(range / 4) > 32 (a range above 128). */
int  navhip_order_queries(navhip_ctx *ctx, const navhip_order_query *q, int n, float map_pos_x, float map_pos_z,
                          float *out_dest_xz, uint32_t *out_dest_id, uint8_t *out_status);
/* Everything resident on the device: ONE launch, asynchronous on `stream`, no allocation at all.  The rows are not readable
 * before the launch: a row the host form would refuse comes back NAVHIP_OQ_HOST. */
int  navhip_order_queries_dev(navhip_ctx *ctx, const navhip_order_query *dev_q, int n, float map_pos_x, float map_pos_z,
                              float *dev_out_dest_xz, uint32_t *dev_out_dest_id, uint8_t *dev_out_status, void *stream);

/* ---- more of entity_compute_update: the heading gate, the arms of the state switch that flags, a
 *      counter, an angle or a distance decide, the arrival overlay's settle rule, and all of it but the last in one call ----
 *
 * The heading gate (movement.c:2319-2336): a unit in STATE_MOVING / SEEK_ENEMIES / SURROUND_ENTITY /
 * ENTER_ENTITY_RANGE (move_gated_by_heading, :2273) whose new velocity is longer than EPSILON does not translate
 * while its facing (movestate.next_rot) is more than MOVE_HEADING_HALT (90 degrees, a unit that is rolling:
 * |movestate.velocity| > EPSILON) or MOVE_HEADING_RESUME (10 degrees, a halted one) off its intended heading
 * (vdes when that is longer than EPSILON, else the new velocity, :2286): its velocity becomes zero and it turns in
 * place (turn_to_move).  The reference measures the angle with float quaternions and atan2
 * (PFM_Quat_PitchDiff, pf_math.c:677; dir_quat_from_velocity, movement.c:1411); the device compares the cosine
 * in double and leaves a unit whose cosine is within 1e-4 of the tolerance's to the host (NAVHIP_GATE_HOST;
 * the float path's error is below 1e-6).  world: n_ents, pos_xz, vel_xz (movestate.velocity), state, work range.
 * out_vel_xz[i] = the velocity after the gate, out_new_pos_xz[i] = new_pos_for_vel (:1820) of it -- what
 * navhip_state_in.new_pos_xz wants at 20 Hz -- out_gate[i] = NAVHIP_GATE_*.  Rows of the slab are written. */
typedef struct navhip_gate_in {
    const float *next_rot;     /* [n][4] movestate.next_rot (x, y, z, w)                            */
    const float *new_vel_xz;   /* [n][2] move_work_out.ent_vel: the velocity the step produced      */
    const float *vdes_xz;      /* [n][2] move_work_out.ent_des_v                                    */
    /* Movement rates below 20 Hz (world->hz = 10 / 5 / 1), both NULL at 20 Hz: entity_compute_update then tests -- in
     * the state switch, in G_Arrival_ShouldSettle -- not pos + vel but the first INTERPOLATED position of the move
     * when the move is accepted (movement.c:2356-2377: |vel| > 0, new position pathable, and not blocked unless the
     * unit already stands on a blocker): interpolate_positions(movestate.next_pos, new_pos, movestate.step) (:2222,
     * float arithmetic; `to` itself when |1 - step| < 1/1024).  out_new_pos_xz receives that position.  Needs
     * world->radius and ->flags (the unit's nav layer); a unit whose layer has no cost plane comes back
     * NAVHIP_GATE_HOST. */
    const float *interp_from_xz;   /* [n][2] movestate.next_pos (x, z)                              */
    const float *interp_step;      /* [n]    movestate.step                                         */
} navhip_gate_in;
#define NAVHIP_GATE_TURN  0x01   /* turn_to_move: the velocity was zeroed, the unit pivots (UPDATE_TURNING_IN_PLACE) */
#define NAVHIP_GATE_HOST  0x80   /* within the margin: not decided, out_vel / out_new_pos hold the UNGATED step     */
int  navhip_heading_gate(navhip_ctx *ctx, const navhip_world *world, const navhip_gate_in *in,
                         float *out_vel_xz, float *out_new_pos_xz, uint8_t *out_gate);
/* Everything resident on the device, asynchronous on `stream`. */
int  navhip_heading_gate_dev(navhip_ctx *ctx, const navhip_world *dev_world, const navhip_gate_in *dev_in,
                             float *dev_out_vel_xz, float *dev_out_new_pos_xz, uint8_t *dev_out_gate, void *stream);

/* The arms of the state switch that flags and a counter decide (movement.c:2423-2437, :2630-2644, :2645-2668): a
 * formation member in STATE_MOVING / MOVING_IN_FORMATION that waits for its assignment or has come within range of its
 * cell (-> ARRIVING_TO_CELL), STATE_ARRIVING_TO_CELL (-> MOVING / MOVING_IN_FORMATION / TURNING), the timer of
 * STATE_WAITING (-> movestate.wait_prev once it runs out), the end of STATE_TURNING (-> ARRIVED) and
 * STATE_ENTER_ENTITY_RANGE.  Called AFTER navhip_state_update on the same slab, with
 * formation members NOT skipped there: a member the flags do not decide keeps the answer of the arrival arm, exactly
 * as the reference falls through to it (:2439).  Rows this call decides are overwritten in inout_state / inout_flags
 * (NAVHIP_SU_HOST cleared); garrisoned units and units whose new position is not pathable (:2437) are left alone /
 * left unchanged as there.  out_wait_ticks_left[i] = movestate.wait_ticks_left after the tick (written for every row
 * of the slab).  world: n_ents, radius, flags, state, map_pos, work range (pos_xz too with the
 * enter-range inputs). */
#define NAVHIP_SU_SET_MOVING  0x04   /* UPDATE_SET_MOVING: the state is movestate.wait_prev (the wait ran out, :2641)     */
#define NAVHIP_SU_TARGET_DIR  0x08   /* UPDATE_SET_TARGET_DIR rides along: next_target_dir = fstate.target_orientation   */
#define NAVHIP_SU_SET_DEST    0x10   /* UPDATE_SET_DEST | UPDATE_SET_TARGET_PREV: next_dest = next_target_prev = the target's
                                        position, next_attack = false (:2597-2602); the state stays                      */
#define NAVHIP_SU_SURROUND_DEST 0x20 /* STATE_SURROUND_ENTITY: UPDATE_SET_DEST | UPDATE_SET_STATE, next_dest =
                                        out_surround_dest_xz[i], next_attack = false, the state stays (:2555-2560)         */
#define NAVHIP_SU_SURROUND_PREV 0x40 /* movestate.surround_target_prev = the target's position, .surround_nearest_prev =
                                        out_surround_dest_xz[i] (the reference writes them inside the switch, :2551-2552)  */
#define NAVHIP_FS_MEMBER      0x01   /* fstate.fid != NULL_FID                                                           */
#define NAVHIP_FS_READY       0x02   /* fstate.assignment_ready                                                          */
#define NAVHIP_FS_ASSIGNED    0x04   /* fstate.assigned_to_cell                                                          */
#define NAVHIP_FS_IN_RANGE    0x08   /* fstate.in_range_of_cell                                                          */
#define NAVHIP_FS_ARRIVED     0x10   /* fstate.arrived_at_cell                                                           */
typedef struct navhip_state_aux_in {
    const uint8_t  *fstate;           /* [n] NAVHIP_FS_* of move_work_in.fstate (struct formation_state, movement.c:215) */
    const int32_t  *wait_ticks_left;  /* [n] movestate.wait_ticks_left                                                   */
    const uint8_t  *wait_prev;        /* [n] movestate.wait_prev                                                         */
    const float    *new_pos_xz;       /* [n][2] as navhip_state_in.new_pos_xz                                            */
    /* STATE_TURNING (:2606-2628), both NULL = its units stay NAVHIP_SU_HOST: the unit has arrived once its rotation is
     * within 5 degrees of movestate.target_dir (cosine compared in double, a unit within 1e-5 of cos 5 deg -- 0.007
     * degrees -- stays the host's); one that keeps turning is decided too (no transition) -- its rotation patch (turn_toward, :2251) is
     * pose bookkeeping the host does for it */
    const float    *ent_rot;          /* [n][4] Entity_GetRot(uid) (x, y, z, w)                                          */
    const float    *target_dir;       /* [n][4] movestate.target_dir                                                     */
    /* STATE_ENTER_ENTITY_RANGE (:2569-2604), all six NULL = its units stay NAVHIP_SU_HOST: no target -> ARRIVED; within
     * movestate.target_range of the target, or next to an impassable tile and on one of the closest island tiles of
     * the target's position (N_IsMaximallyClose with tolerance 0, nav.c:4707) -> WAITING; else, once the target has
     * moved more than 5 units from target_prev_pos, NAVHIP_SU_SET_DEST.  The target's position is world->pos_xz of its
     * row.  Needs the BLOCKERS plane of the units' layers. */
    const int32_t  *range_target;     /* [n] row of movestate.surround_target_uid in the world's arrays; -1 = NULL_UID;
                                             -2 (any value below -1) = leave the unit to the host (a target outside
                                             the snapshot)                                                               */
    const float    *target_range;     /* [n] movestate.target_range                                                      */
    const float    *target_prev_xz;   /* [n][2] movestate.target_prev_pos                                                */
    const int32_t  *range_tiles_row;  /* [n] row of range_tiles_off for the unit: the closest island tiles of ITS target's
                                             position on ITS nav layer (n_closest_island_tiles, nav.c:4725, as flock_tiles
                                             of navhip_state_in)                                                         */
    const int32_t  *range_tiles_off;  /* [rows + 1] CSR offsets into range_tiles                                         */
    const int16_t  *range_tiles;      /* [..][2] absolute nav tiles (row, column)                                        */
    int32_t         n_range_rows;     /* rows of range_tiles_off (host-buffer call: sizes the transfer)                  */
    /* STATE_SURROUND_ENTITY (:2509-2567), surround_target NULL = its units stay NAVHIP_SU_HOST (as do all of them at a
     * rate below 20 Hz).  The two nav queries on the unit-query context are handed over per unit exactly as
     * flock_nearest_xz is for arrived() -- by the host, or by navhip_surround_queries[_dev] above, whose NAVHIP_SQ_HOST
     * rows stay NAVHIP_SU_HOST here --: whether the unit already touches its target (M_NavObjAdjacentFrom, map.c:1061 --
     * or the target is gone), and the closest reachable position next to the target (M_NavClosestReachableAdjacentPosFrom,
     * map.c:860) from BOTH positions the tick can test: pos + new velocity, and pos (the heading gate zeroed the
     * velocity).  The host only needs to fill the query answers for units that reach the query (:2532-2545: the target
     * has moved since surround_target_prev, or the unit stands still).  The device runs the switch: no target / adjacent
     * / no reachable position -> ARRIVED; the position differs from the flock's target -> NAVHIP_SU_SURROUND_DEST with the
     * position in out_surround_dest_xz; no guidance -> WAITING; and reports NAVHIP_SU_SURROUND_PREV where the reference
     * stores surround_target_prev = the target's position, surround_nearest_prev = out_surround_dest_xz[i] (:2551-2552).
     * world: pos_xz, vel_xz (movestate.velocity), flock, flock_target_xz too. */
    const int32_t  *surround_target;  /* [n] row of movestate.surround_target_uid; -1 = NULL_UID; below -1 = leave to the host */
    const uint8_t  *surround_query;   /* [n] NAVHIP_SQ_*                                                                 */
    const float    *surround_target_prev_xz;   /* [n][2] movestate.surround_target_prev                                  */
    const float    *surround_nearest_prev_xz;  /* [n][2] movestate.surround_nearest_prev                                 */
    const float    *surround_dest_xz; /* [n][2][2] the query's answer from pos + new velocity ([i][0]) and from pos ([i][1]) */
    const float    *vdes_xz;          /* [n][2] move_work_out.ent_des_v (the surround arm's no-guidance test)            */
    float          *out_surround_dest_xz;      /* [n][2] written for units flagged NAVHIP_SU_SURROUND_PREV               */
    /* SPARSE ROWS (navhip_state_pass_resident only; NULL / 0 everywhere else).  The three arms above concern a few units
     * in a hundred, and their arrays are 108 bytes per ENTITY.  With sparse_units != NULL every per-unit array of the
     * three arms that is given -- ent_rot, target_dir; range_target, target_range, target_prev_xz, range_tiles_row;
     * surround_target, surround_query, surround_target_prev_xz, surround_nearest_prev_xz, surround_dest_xz,
     * out_surround_dest_xz -- holds ONE ROW PER LISTED UNIT, row k for unit sparse_units[k], instead of one per entity;
     * the device lays them out.  List every unit of the three states that the device is to decide: an unlisted
     * ENTER_ENTITY_RANGE / SURROUND_ENTITY unit is left to the host (as a target below -1), an unlisted TURNING unit is
     * computed from a zero rotation (as a dense row nobody filled would be).  A unit may be listed once. */
    const int32_t  *sparse_units;     /* [n_sparse] rows of the world's arrays, inside the slab                          */
    int32_t         n_sparse;
} navhip_state_aux_in;
#define NAVHIP_SQ_ADJACENT   0x01   /* !entity_exists(target) || M_NavObjAdjacentFrom(map, uid, target, ctx)              */
#define NAVHIP_SQ_HAS_DEST_0 0x02   /* M_NavClosestReachableAdjacentPosFrom(.., pos + new velocity, ..) found a position */
#define NAVHIP_SQ_HAS_DEST_1 0x04   /* ... from pos                                                                      */
/* (NAVHIP_SQ_HOST 0x80, above: the query was not decided on the device; a unit with a target keeps NAVHIP_SU_HOST)        */
int  navhip_state_update_aux(navhip_ctx *ctx, const navhip_world *world, const navhip_state_aux_in *in,
                             uint8_t *inout_state, uint8_t *inout_flags, int32_t *out_wait_ticks_left);
/* Everything resident on the device, asynchronous on `stream`. */
int  navhip_state_update_aux_dev(navhip_ctx *ctx, const navhip_world *dev_world, const navhip_state_aux_in *dev_in,
                                 uint8_t *dev_inout_state, uint8_t *dev_inout_flags, int32_t *dev_out_wait_ticks_left,
                                 void *stream);

/* The state half of the tick in ONE host-buffer call (fork_join_state_updates, movement.c:4196, as navhip_agent_step is
 * the velocity half): heading gate -> navhip_state_update on the gate's new positions -> navhip_state_update_aux, the
 * snapshot staged once, one wait at the end.  state.new_pos_xz, state.vdes_xz and aux.new_pos_xz are IGNORED (the gate's
 * output and gate.vdes_xz are used); aux.fstate == NULL: no aux pass.  A unit the gate leaves to the host
 * (NAVHIP_GATE_HOST) comes back NAVHIP_SU_HOST with its state and wait counter untouched: the host decides all of it.
 * Units of flocks with an active arrival zone are skipped as before (state.skip) and decided afterwards by
 * navhip_settled_count / navhip_arrival_settle on the returned positions.  Rows of the slab are written. */
typedef struct navhip_state_pass_in {
    navhip_gate_in      gate;
    navhip_state_in     state;
    navhip_state_aux_in aux;
} navhip_state_pass_in;
typedef struct navhip_state_pass_out {
    uint8_t  *state, *flags;          /* [n] next state, NAVHIP_SU_*                                                   */
    uint8_t  *gate;                   /* [n] NAVHIP_GATE_*                                                             */
    float    *new_pos_xz;             /* [n][2] new_pos_for_vel of the gated velocity                                  */
    float    *vel_xz;                 /* [n][2] the gated velocity, or NULL                                            */
    int32_t  *wait_ticks_left;        /* [n] or NULL (required with an aux pass)                                       */
} navhip_state_pass_out;
int  navhip_state_pass(navhip_ctx *ctx, const navhip_world *world, const navhip_state_pass_in *in,
                       const navhip_state_pass_out *out);

/* The same pass ON THE SNAPSHOT THE VELOCITY HALF LEFT ON THE DEVICE: between navhip_agent_step_wait (or a poll that
 * returned 0) and the next submit, the arrays of that step -- positions, velocities, radii, flags, states, flock tables --
 * and its results -- the new velocities, the desired directions -- are still in HBM.  The state half of the same tick
 * (fork_join_state_updates follows the velocity fork-join in navigation_tick_task, movement.c:4263-4280) only uploads
 * what it alone reads: movestate.next_rot, the per-flock query results, the flag / counter / target inputs (24 bytes
 * per unit in the common case instead of 95), packed through pinned memory as one transfer each way.  in->gate.new_vel_xz
 * and .vdes_xz are ignored (the step's own outputs are used: the step must have been asked for vdes_xz unless every
 * desired direction was the caller's, world->vdes_xz without NaN entries); world = that step's, slab included.
 * NAVHIP_ERR_INVALID when no completed host-buffer step is resident: call navhip_state_pass instead. */
int  navhip_state_pass_resident(navhip_ctx *ctx, const navhip_state_pass_in *in, const navhip_state_pass_out *out);

/* adjacent_settled_count (movement.c:982) for nq units of the snapshot: G_Pos_EntsInCircleFrom (r = max(30,
 * 2 radius + 5), at most 128 results, garrisoned entities dropped, position.c:379) and of those the movable
 * ones of the same air / ground kind in STATE_ARRIVED that touch the unit (distance <= both radii +
 * ADJACENCY_SEP_DIST).  out_counts[q] = -1 for a unit with radius > 12.5 (its query is wider than the 30 units
 * the spatial index is asked for here): the host counts.  world: n_ents, pos_xz, radius, flags, state, grid
 * bounds.  Host buffers. */
int  navhip_settled_count(navhip_ctx *ctx, const navhip_world *world, int nq, const int32_t *uids,
                          int32_t *out_counts);
/* The same on the snapshot the velocity half of the tick left on the device (see navhip_state_pass_resident): nothing of
 * the snapshot travels, the index is built over the resident positions, the query ids stay in HBM; only the uids go up
 * and the counts come back.  world: n_ents and the grid bounds.  NAVHIP_ERR_INVALID when no such step is resident. */
int  navhip_settled_count_resident(navhip_ctx *ctx, const navhip_world *world, int nq, const int32_t *uids,
                                   int32_t *out_counts);

/* G_Arrival_ShouldSettle (arrival.c:946) for nq units whose flock has an active arrival zone (G_Arrival_IsActive)
 * for their nav layer -- the arm of entity_compute_update at movement.c:2443-2451 that navhip_state_update leaves
 * to the host (skip[i]).  A zone is one struct arrival_state (arrival.h:66): the slots, their fill ranks and the
 * sorted tile keys of its footprint are given as ranges of three shared arrays.  Per unit: the position the
 * state update tests, the count of settled neighbours (navhip_settled_count), and its struct
 * arrival_unit_state (arrival.h:105) -- which the rule also UPDATES (arming, the progress anchor, the stuck
 * count): the out_* arrays receive the state after the call, as the reference leaves it in movestate.arrival.
 * world: n_ents, vel_xz (movestate.velocity), radius, map_pos.  Needs the BLOCKERS plane of the zones' layers
 * (M_NavPositionBlocked on a slot).  out_settle[q] = 1: UPDATE_SET_STATE, STATE_ARRIVED, next_block. */
typedef struct navhip_arrival_zone {
    float    centre_x, centre_z;      /* arrival_state.centre                                                   */
    float    unit_radius;             /* .unit_radius                                                           */
    float    fill_frac;               /* .fill_frac                                                             */
    int32_t  radius;                  /* .radius (nav tiles)                                                    */
    int32_t  layer;                   /* .layer                                                                 */
    int32_t  active_row, num_rows;    /* .active_row, .num_rows                                                 */
    int32_t  slot_begin, slot_end;    /* .slots / .slot_ring [0, num_slots) as a range of slots_xz / slot_ring  */
    int32_t  key_begin, key_end;      /* .region_keys [0, num_region) as a range of region_keys                 */
} navhip_arrival_zone;
typedef struct navhip_settle_in {
    int32_t  n_zones;
    int32_t  nq;
    const navhip_arrival_zone *zones; /* [n_zones]                                                              */
    const float    *slots_xz;         /* [..][2]                                                                */
    const int32_t  *slot_ring;        /* [..]                                                                   */
    const uint64_t *region_keys;      /* [..] td_key (nav.c:207): chunk_r << 48 | chunk_c << 32 | tile_r << 16 | tile_c,
                                              ascending inside a zone (N_TileKeysForPositions, nav.c:4303)      */
    const int32_t  *uid;              /* [nq] the unit (row of the world's arrays)                              */
    const int32_t  *zone;             /* [nq] its zone                                                          */
    const float    *new_pos_xz;       /* [nq][2] the position entity_compute_update tests (navhip_state_in)     */
    const int32_t  *nsettled;         /* [nq] adjacent_settled_count                                            */
    const uint8_t  *substate;         /* [nq] arrival_unit_state.substate (enum arrival_substate, arrival.h:55) */
    const uint8_t  *sink_valid;       /* [nq] .sink_valid                                                       */
    const float    *sink_xz;          /* [nq][2] .sink                                                          */
    const float    *order_pos_xz;     /* [nq][2] .order_pos                                                     */
    const float    *progress_anchor_xz; /* [nq][2] .progress_anchor                                             */
    const uint8_t  *progress_anchored;  /* [nq] .progress_anchored                                              */
    const int32_t  *stuck;            /* [nq] .stuck                                                            */
} navhip_settle_in;
typedef struct navhip_settle_out {
    uint8_t  *settle;                 /* [nq] the rule's answer                                                 */
    uint8_t  *substate;               /* [nq] arrival_unit_state after the call                                 */
    float    *progress_anchor_xz;     /* [nq][2]                                                                */
    uint8_t  *progress_anchored;      /* [nq]                                                                   */
    int32_t  *stuck;                  /* [nq]                                                                   */
    int32_t  *nsettled;               /* [nq] or NULL: the counts the rule used (navhip_arrival_settle_resident with
                                              in->nsettled == NULL); -1 = the host counts AND decides this unit     */
} navhip_settle_out;
int  navhip_arrival_settle(navhip_ctx *ctx, const navhip_world *world, const navhip_settle_in *in,
                           const navhip_settle_out *out);
/* The same with world->vel_xz / ->radius read from the snapshot the velocity half of the tick left on the device (see
 * navhip_state_pass_resident; world: n_ents, map_pos).  NAVHIP_ERR_INVALID when no such step is resident.
 * in->nsettled == NULL: adjacent_settled_count is taken on the device too (navhip_settled_count_resident's rule on the
 * same snapshot; world: the grid bounds as well) -- the two passes of the arm in ONE call, every per-unit array packed
 * through pinned memory as one transfer each way. */
int  navhip_arrival_settle_resident(navhip_ctx *ctx, const navhip_world *world, const navhip_settle_in *in,
                                    const navhip_settle_out *out);
/* Everything resident on the device (the zones' arrays and the per-unit arrays too), asynchronous on `stream`. */
int  navhip_arrival_settle_dev(navhip_ctx *ctx, const navhip_world *dev_world, const navhip_settle_in *dev_in,
                               const navhip_settle_out *dev_out, void *stream);

/* G_Arrival_DesiredVelocity (arrival.c:862-944) for nq units whose flock's arrival zone is in ARRIVAL_PHASE_FILLING --
 * the rows with bit 1 of navhip_world.arrival_flags, the one producer of move_work_in.ent_des_v that reads nav data and
 * was still the host's (ent_desired_velocity, movement.c:1509-1515).  Statement for statement: arrival_near_region
 * commits the unit (APPROACH -> SEEK, APPROACH_ARMED -> SEEK_ARMED); a committed unit re-targets a blocked sink
 * (arrival_nearest_open_slot: of equal distance the EARLIEST slot wins, a distance that is not < INFINITY never), beelines
 * its sink while N_SegmentWithinRegion holds, else heads for arrival_nearest_slot, else (0, 0); an approaching unit takes
 * N_DesiredGroupArrivalVelocity of the zone's TARGET_ZONE field, else debounces has_dest_los (ARRIVAL_LOS_HYST 12) and
 * beelines the centre or samples the flock's centre-of-mass point-seek field.  The rule UPDATES the unit's struct
 * arrival_unit_state: the out arrays receive the state after the call.
 * Zones as in navhip_settle_in, plus per zone the mapping rows of its two sets of fields: zone_row indexes
 * world->region_field_slot (the TARGET_ZONE chunk fields, navhip_build_region_fields), com_row indexes
 * world->flock_field_slot (the fields of arrival_state.com_dest_id); -1 = none cached.  With world->n_field_slots ==
 * NAVHIP_POOL_RESIDENT both are rows of the resident pool's mapping table.
 * world: n_ents, pos_xz (the unit's position), map_pos, n_flocks (rows of flock_field_slot), n_region_rows, the two tables
 * and field_pool / n_field_slots.  Needs the BLOCKERS plane of the zones' layers. */
#define NAVHIP_AV_COM_MISS  0x01   /* an approaching unit without static LOS whose centre-of-mass field is missing or has
                                      FD_NONE under it (NAVHIP_ST_FIELD_MISS / _NONE of the sample): every state output is
                                      final -- the debounce has counted -- and vdes is (NaN, NaN); the host supplies
                                      M_NavDesiredPointSeekVelocity(com_dest_id, pos, com) for the row and nothing else   */
#define NAVHIP_AV_HOST      0x80   /* not decided: the state outputs repeat the inputs, vdes is (NaN, NaN).  A uid outside
                                      the world, a zone index outside the table, a NaN position or one off the map, a
                                      substate above 3, a layer without a BLOCKERS plane                                  */
typedef struct navhip_arrival_vel_in {
    int32_t  n_zones;
    int32_t  nq;
    int32_t  n_slots;                 /* rows of slots_xz / slot_ring                                           */
    int32_t  n_keys;                  /* rows of region_keys                                                    */
    const navhip_arrival_zone *zones; /* [n_zones]                                                              */
    const float    *slots_xz;         /* [..][2]                                                                */
    const int32_t  *slot_ring;        /* [..]                                                                   */
    const uint64_t *region_keys;      /* [..] ascending inside a zone, as in navhip_settle_in                   */
    const int32_t  *zone_row;         /* [n_zones] mapping row of the zone's TARGET_ZONE fields, -1 = none      */
    const int32_t  *com_row;          /* [n_zones] mapping row of the fields of .com_dest_id, -1 = none         */
    const int32_t  *uid;              /* [nq] the unit (row of the world's arrays)                              */
    const int32_t  *zone;             /* [nq] its zone                                                          */
    const uint8_t  *has_dest_los;     /* [nq] move_work_in.has_dest_los                                         */
    const uint8_t  *substate;         /* [nq] arrival_unit_state.substate                                       */
    const uint8_t  *sink_valid;       /* [nq] .sink_valid                                                       */
    const float    *sink_xz;          /* [nq][2] .sink                                                          */
    const uint8_t  *los_latched;      /* [nq] .los_latched                                                      */
    const int32_t  *los_hyst;         /* [nq] .los_hyst                                                         */
} navhip_arrival_vel_in;
typedef struct navhip_arrival_vel_out {
    float    *vdes_xz;                /* [nq][2] *out_vel; (NaN, NaN) for a COM_MISS or HOST row                */
    uint8_t  *status;                 /* [nq] 0, NAVHIP_AV_COM_MISS or NAVHIP_AV_HOST                           */
    uint8_t  *substate;               /* [nq] arrival_unit_state after the call                                 */
    uint8_t  *sink_valid;             /* [nq]                                                                   */
    float    *sink_xz;                /* [nq][2]                                                                */
    uint8_t  *los_latched;            /* [nq]                                                                   */
    int32_t  *los_hyst;               /* [nq]                                                                   */
    float    *dense_vdes_xz;          /* navhip_arrival_velocity_dev only, or NULL: [n_ents][2], row uid[q] receives
                                              vdes of query q, rows not listed are left alone (vdes_xz may then be NULL).
                                              Pre-filled with NaN it is navhip_agent_step_dev's world.vdes_xz as it
                                              stands: NaN = sample the flock's field on the device                  */
} navhip_arrival_vel_out;
/* Host buffers.  NAVHIP_ERR_ARG with the reason in navhip_last_error, before any launch and with the outputs untouched:
 * a missing array, nq < 0, a zone whose ranges leave the shared arrays (in->n_slots / n_keys rows), keys not ascending
 * inside a zone, a mapping row outside its table, a layer outside the map's, dense_vdes_xz. */
int  navhip_arrival_velocity(navhip_ctx *ctx, const navhip_world *world, const navhip_arrival_vel_in *in,
                             const navhip_arrival_vel_out *out);
/* Everything resident on the device, asynchronous on `stream`, no allocation: one launch.  What the host form checks in
 * the arrays is the caller's promise here; a mapping row outside its table makes the unit a NAVHIP_AV_HOST row. */
int  navhip_arrival_velocity_dev(navhip_ctx *ctx, const navhip_world *dev_world, const navhip_arrival_vel_in *dev_in,
                                 const navhip_arrival_vel_out *dev_out, void *stream);

/* The built-zone branch of G_Arrival_UpdateFlock (arrival.c:767-853, everything but the first build at :796-848) for
 * n_zones zones at once -- what update_flock_arrival_fields (movement.c:900-920) runs serially per flock and nav layer,
 * and the producer of the zone table the two calls above read.  Per zone, in the reference's order: every member settled
 * -> phase DONE and nothing else changes; otherwise layer / unit_radius from the call's arguments, radius =
 * arrival_zone_radius(total_members, unit_radius), ++realloc_counter, and when it reaches ARRIVAL_REALLOC_PERIOD (4)
 * arrival_realloc_slots (:391-516): while fill_frac < 0.25 the rings are recomputed (arrival_compute_geodesic_rings :257
 * over N_RegionGeodesicDist nav.c:4389: the entry is the float sum of the unsettled members' positions in member order
 * times 1.0f / cnt, the source the key whose tile centre is nearest to it, a 4-connected flood through the keys, ring =
 * (maxd - distance) / ring_w) and active_row = 0; then the occupancy (slots under blockers, and the slot nearest to every
 * settled member), fill_frac, the frontier with its stall counter, and for every unsettled member inside the footprint
 * unit_commit and its sink: the nearest slot that is not occupied and lies at or behind the frontier (of equal distance
 * the EARLIEST slot wins, a distance that is not < INFINITY never).
 * A zone is a navhip_arrival_zone (as in navhip_settle_in / navhip_arrival_vel_in) plus a navhip_arrival_flock: what
 * struct arrival_state has and that table lacks, the call's arguments, and the zone's members as a range of the member
 * arrays, in the reference's member order (members[].pos is world->pos_xz[uid]).
 * world: n_ents, pos_xz, map_pos.  Needs the BLOCKERS plane of the layers the flocks name. */
#define NAVHIP_ARRIVAL_PHASE_INACTIVE 0    /* enum arrival_phase, arrival.h:49 */
#define NAVHIP_ARRIVAL_PHASE_FILLING  1
#define NAVHIP_ARRIVAL_PHASE_DONE     2
#define NAVHIP_ARRIVAL_MAX_SLOTS      4096 /* ARRIVAL_MAX_SLOTS, arrival.h:47 */
#define NAVHIP_AF_HOST      0x80   /* not decided: every output of the zone and of its members repeats its input.  A layer
                                      without a BLOCKERS plane (or outside the map's), more than NAVHIP_ARRIVAL_MAX_SLOTS
                                      slots or keys, a uid outside the world, a phase other than FILLING, num_rows above
                                      NAVHIP_ARRIVAL_MAX_SLOTS or active_row outside [0, num_rows)                        */
typedef struct navhip_arrival_flock {
    int32_t  phase;                   /* arrival_state.phase (NAVHIP_ARRIVAL_PHASE_*)                           */
    int32_t  realloc_counter;         /* .realloc_counter                                                       */
    int32_t  stall_counter;           /* .stall_counter                                                         */
    int32_t  prev_occ;                /* .prev_occ                                                              */
    float    row_height;              /* .row_height                                                            */
    float    unit_radius;             /* the call's arguments: unit_radius,                                     */
    int32_t  total_members;           /* ... total_members,                                                     */
    int32_t  layer;                   /* ... layer                                                              */
    int32_t  member_begin, member_end;/* members[0, nmembers) as a range of the member arrays                   */
} navhip_arrival_flock;
typedef struct navhip_arrival_flock_in {
    int32_t  n_zones;
    int32_t  nm;                      /* rows of the member arrays                                              */
    int32_t  n_slots;                 /* rows of slots_xz / slot_ring                                           */
    int32_t  n_keys;                  /* rows of region_keys                                                    */
    const navhip_arrival_zone  *zones;  /* [n_zones]                                                            */
    const navhip_arrival_flock *flocks; /* [n_zones]                                                            */
    const float    *slots_xz;         /* [..][2]                                                                */
    const int32_t  *slot_ring;        /* [..]                                                                   */
    const uint64_t *region_keys;      /* [..] ascending inside a zone, as in navhip_settle_in                   */
    const int32_t  *uid;              /* [nm] the member (row of world->pos_xz)                                 */
    const uint8_t  *settled;          /* [nm] arrival_member.settled                                            */
    const uint8_t  *substate;         /* [nm] arrival_unit_state.substate                                       */
    const uint8_t  *sink_valid;       /* [nm] .sink_valid                                                       */
    const float    *sink_xz;          /* [nm][2] .sink                                                          */
} navhip_arrival_flock_in;
typedef struct navhip_arrival_flock_out {
    navhip_arrival_zone  *zones;      /* [n_zones] the zone table after the call                                */
    navhip_arrival_flock *flocks;     /* [n_zones] the companion after the call                                 */
    int32_t  *slot_ring;              /* [n_slots]                                                              */
    uint8_t  *substate;               /* [nm] arrival_unit_state after the call                                 */
    uint8_t  *sink_valid;             /* [nm]                                                                   */
    float    *sink_xz;                /* [nm][2]                                                                */
    uint8_t  *status;                 /* [n_zones] 0 or NAVHIP_AF_HOST                                          */
} navhip_arrival_flock_out;
/* Host buffers.  NAVHIP_ERR_ARG with the reason in navhip_last_error, before any launch and with the outputs untouched:
 * a missing array, nm < 0, a zone whose slot, key or member range leaves the shared arrays, keys not ascending inside a
 * zone. */
int  navhip_arrival_flock_update(navhip_ctx *ctx, const navhip_world *world, const navhip_arrival_flock_in *in,
                                 const navhip_arrival_flock_out *out);
/* Everything resident on the device, asynchronous on `stream`, no allocation: one launch, a workgroup per zone.  out may
 * alias in array by array (in place); what the host form checks in the arrays is the caller's promise here.  Behind it
 * navhip_arrival_velocity_dev and navhip_arrival_settle_dev on the same device arrays see the new rings, frontier and
 * sinks. */
int  navhip_arrival_flock_update_dev(navhip_ctx *ctx, const navhip_world *dev_world, const navhip_arrival_flock_in *dev_in,
                                     const navhip_arrival_flock_out *dev_out, void *stream);

/* The FIRST build of a zone: the `!built` branch of G_Arrival_UpdateFlock (arrival.c:784-848) for n_zones zones at once,
 * which takes a zone from INACTIVE to FILLING.  Per zone, statement for statement: the gate (:785-788: total_members >=
 * ARRIVAL_MIN_UNITS 4 and arrival_near_goal :377, a member with PFM_Vec2_Len(target - pos) < 150.0f), arrival_zone_radius
 * (:363), centre = N_ClosestPathable(target) ? snapped : target (:801, nav.c:4126), arrival_approach_axis (:236: the float
 * sum of the member positions in member order times 1.0f / n), arrival_build_slots (:181) over
 * N_ClosestConnectedPathableTiles (nav.c:4192: the best-first 8-connected flood whose ties the heap of pqueue.h:109-208
 * decides, replayed operation for operation, budget arrival_region_area :147) and N_TileKeysForPositions (nav.c:4304),
 * arrival_thin_centered_slots (:196), the clear-line filter (:810-817, N_SegmentWithinRegion nav.c:4326), the centre of
 * mass in slot order with its N_ClosestPathable and N_DestIDForPos (:819-830, nav.c:3367), arrival_order_slots_far_near
 * (:231, slot_cmp_far_banded :130), and the tail :839-847: row_height, arrival_compute_geodesic_rings, the counters, and
 * arrival_realloc_slots exactly as navhip_arrival_flock_update runs it for a zone below a quarter full.
 * The two qsort calls (:210, :233) promise nothing for equal elements; glibc's qsort is a stable merge sort for arrays of
 * this size, so the engine's behaviour on its platform is "ties keep their order", and that is the contract here: ties of
 * the near-reference sort keep flood order, ties of the banded sort the order the clear-line filter left.
 *
 * In, per zone: a navhip_arrival_flock with phase INACTIVE and the call's arguments (unit_radius, total_members, layer,
 * the member range), target_xz, and the zone's row of the zone table, of which only the ROOM is read: [slot_begin,
 * slot_end) of slots_xz / slot_ring and [key_begin, key_end) of region_keys.  A zone needs room for
 * area = arrival_region_area keys (min((int)(M_PI * radius * radius + 0.5f), 4096), radius = arrival_zone_radius) and for
 * min(total_members, area) slots; the raw flood lives in the kernel's LDS.  Too little room (or a range that leaves the
 * shared arrays) is NAVHIP_ERR_ARG in the host form and a NAVHIP_AB_HOST row in the resident form.
 * Out (may alias in, array by array): the zone row (centre, unit_radius, radius, layer, fill_frac, active_row, num_rows,
 * slot_end = slot_begin + num_slots, key_end = key_begin + num_region), the companion (phase FILLING, the counters,
 * row_height), slots_xz / slot_ring / region_keys inside the new ranges, axis_xz, com_xz, com_dest_id (what struct
 * arrival_state has and the table lacks: com_row and G_Arrival_RequestField need them), the members' state, status.
 * world: n_ents, pos_xz, map_pos.  Needs the COST_BASE and BLOCKERS planes of the layers the flocks name. */
#define NAVHIP_AB_WAIT      0x01   /* the gate said not yet: every output repeats its input (axis_xz, com_xz and com_dest_id,
                                      which have none, are not written), phase stays INACTIVE                               */
#define NAVHIP_AB_HOST      0x80   /* not decided, never a wrong answer: outputs as for NAVHIP_AB_WAIT.  A layer without cost
                                      or blockers plane; a member uid outside the world; a phase other than INACTIVE; a
                                      unit_radius that is not a positive finite number; too little room; a target or a centre
                                      of mass that is NaN or off the map (the reference asserts; (0, 0) off the map when no
                                      slot survives included); a NAVHIP_DQ_HOST answer of either N_ClosestPathable; a flood
                                      that meets an unvisited on-map neighbour outside the WINDOW of
                                      NAVHIP_AB_WINDOW_R tiles (Chebyshev) around the centre tile; a heap that would hold
                                      more than NAVHIP_AB_HEAP_NODES nodes                                                  */
#define NAVHIP_AB_WINDOW_R   127
#define NAVHIP_AB_HEAP_NODES 4096
typedef struct navhip_arrival_build_in {
    int32_t  n_zones;
    int32_t  nm;                      /* rows of the member arrays                                              */
    int32_t  n_slots;                 /* rows of slots_xz / slot_ring                                           */
    int32_t  n_keys;                  /* rows of region_keys                                                    */
    const navhip_arrival_zone  *zones;  /* [n_zones] slot_begin/slot_end, key_begin/key_end: the zone's room    */
    const navhip_arrival_flock *flocks; /* [n_zones] phase INACTIVE, the call's arguments, the member range     */
    const float    *target_xz;        /* [n_zones][2] the call's target_xz                                      */
    const float    *slots_xz;         /* [n_slots][2] what the rooms hold now: repeated on WAIT / HOST rows     */
    const int32_t  *slot_ring;        /* [n_slots]                                                              */
    const uint64_t *region_keys;      /* [n_keys]                                                               */
    const int32_t  *uid;              /* [nm] the member (row of world->pos_xz), the reference's member order   */
    const uint8_t  *settled;          /* [nm] arrival_member.settled                                            */
    const uint8_t  *substate;         /* [nm] arrival_unit_state.substate                                       */
    const uint8_t  *sink_valid;       /* [nm] .sink_valid                                                       */
    const float    *sink_xz;          /* [nm][2] .sink                                                          */
} navhip_arrival_build_in;
typedef struct navhip_arrival_build_out {
    navhip_arrival_zone  *zones;      /* [n_zones] the zone table after the call                                */
    navhip_arrival_flock *flocks;     /* [n_zones] the companion after the call                                 */
    float    *slots_xz;               /* [n_slots][2] arrival_state.slots, far -> near                          */
    int32_t  *slot_ring;              /* [n_slots]                                                              */
    uint64_t *region_keys;            /* [n_keys] ascending inside a zone                                       */
    float    *axis_xz;                /* [n_zones][2] arrival_state.axis                                        */
    float    *com_xz;                 /* [n_zones][2] .com                                                      */
    uint32_t *com_dest_id;            /* [n_zones] .com_dest_id (N_DestIDForPos, nav.c:3367)                    */
    uint8_t  *substate;               /* [nm] arrival_unit_state after the call                                 */
    uint8_t  *sink_valid;             /* [nm]                                                                   */
    float    *sink_xz;                /* [nm][2]                                                                */
    uint8_t  *status;                 /* [n_zones] 0 = built, NAVHIP_AB_WAIT, NAVHIP_AB_HOST                    */
} navhip_arrival_build_out;
/* Host buffers.  NAVHIP_ERR_ARG with the reason in navhip_last_error, before any launch and with the outputs untouched:
 * a missing array, a negative count, a zone whose slot, key or member range leaves the shared arrays, and -- for a zone
 * the call would go on to build (phase INACTIVE, a layer with its planes, every uid inside the world, the gate passed)
 * -- too little room.  A zone that comes back NAVHIP_AB_WAIT needs no room. */
int  navhip_arrival_zone_build(navhip_ctx *ctx, const navhip_world *world, const navhip_arrival_build_in *in,
                               const navhip_arrival_build_out *out);
/* Everything resident on the device, asynchronous on `stream`, no allocation: two launches, a workgroup per zone each
 * (the build; navhip_arrival_flock_update's kernel for the tail).  out may alias in array by array.  Behind it
 * navhip_arrival_flock_update_dev, navhip_arrival_velocity_dev and navhip_arrival_settle_dev on the same device arrays
 * see a FILLING zone. */
int  navhip_arrival_zone_build_dev(navhip_ctx *ctx, const navhip_world *dev_world, const navhip_arrival_build_in *dev_in,
                                   const navhip_arrival_build_out *dev_out, void *stream);

/* ---- enemy-seek and surround fields from the snapshot (compute_async_fields, movement.c:4149-4164) ---------------- */

/* The whole job of N_RequestAsyncEnemySeekField / N_RequestAsyncSurroundField: the seed tiles come from the snapshot on the
 * device (field_enemies_initial_frontier field.c:1209, field_entity_initial_frontier :1317), the field from
 * navhip_build_region_fields' kernel behind them (out_mode 1, enemies 0, the geometry of field.c:1558-1572, 1596-1597).
 *   kind 0  the rectangle of the chunk widened by half a chunk + SEARCH_BUFFER (16) per side, in bitmap_grid.h's fixed point
 *           (bg_ent_inrange_rect, inclusive bounds, the grid of world.grid_*); garrisoned entities dropped (G_Pos_EntsInRect);
 *           field_enemy_ent :963 + ent_dying; M_Tile_AllUnderCircle + one contour of everything so far per layer step
 *           (layer >= 3X3, >= 5X5, >= 7X7: every water and air layer three); tds[512] replayed in row-major order
 *   kind 1  the circle of entity target_uid, contours for layer == 3X3, >= 5X5, >= 7X7; the tiles inside the region */
#define NAVHIP_SEEK_ENEMIES 0   /* field_update_enemies, field.c:1537 (TARGET_ENEMIES) */
#define NAVHIP_SEEK_ENTITY  1   /* field_update_entity,  field.c:1612 (TARGET_ENTITY)  */
#define NAVHIP_SK_HOST   0x80   /* out_status: not decided here, slot and seed row untouched, never a wrong field.  For: a map
                                   one chunk high or wide (the padded region is not square); a chunk outside the map; a layer
                                   without resident cost_base and blockers planes; more than 4 096 entities in the rectangle,
                                   garrisoned ones included (the reference truncates in its grid's cell order); a source entity
                                   or the kind-1 target with ENTITY_FLAG_BUILDING (its OBB is not here), with ceil(radius / 4)
                                   plus its contours above 31 (the 64 x 64 window), with a NaN radius or with a position that
                                   is not finite or at or beyond 2^22 world units (no fixed-point value); target_uid outside
                                   [0, n_ents); faction_id outside [0, 15] for kind 0; in the resident form, a kind above 1 or
                                   a layer outside [0, NAVHIP_NAV_LAYER_MAX) */

typedef struct navhip_seek_req {      /* one job of N_RequestAsyncEnemySeekField / ...SurroundField.  12 bytes */
    uint8_t  kind, layer;
    int16_t  chunk_r, chunk_c;        /* the chunk of curr_pos (nav.c:3789, :3844) */
    int16_t  faction_id;              /* kind 0: enemies_desc.faction_id */
    int32_t  target_uid;              /* kind 1: entity_desc.target */
} navhip_seek_req;

typedef uint16_t navhip_enemy_masks[16];   /* (a type of its own: a record of this header has no array declarator) */

typedef struct navhip_seek_game {     /* what field.c asks game.c / combat.c / fog_of_war.c per entity */
    const int32_t *faction;           /* [n_ents] G_GetFactionID */
    const uint8_t *exclude;           /* [n_ents] or NULL: nonzero = dying (ent_dying) or not player-visible
                                         (ent_player_visible): fog and death stay the host's, one byte per entity */
    navhip_enemy_masks enemy_mask;    /* bit g of [f]: G_GetDiplomacyState(f, g) is known and DIPLOMACY_STATE_WAR */
} navhip_seek_game;

/* Host buffers.  inout: n chunk fields of one direction per byte, stride >= 4096, read-modify-write exactly as
 * navhip_build_region_fields writes them in out_mode 1 (an unreached tile keeps its byte; a request without any seed
 * returns status 0 with the slot as it was).  out_status [n]: 0 or NAVHIP_SK_HOST.  out_seed_bits, or NULL: n rows of
 * 2 048 bytes, the request's has_enemy bitmap over the 128 x 128 region, row-major, bit r * 128 + c in byte (r * 128 + c) / 8
 * (kind 1: the in-region tiles of the target).  Of `world` the call reads n_ents, pos_xz, radius, flags, map_pos_* and
 * grid_*.  NAVHIP_ERR_INVALID, with the reason in navhip_last_error, before any launch and with the buffers untouched: a
 * missing array (world, game, game->faction, pos_xz, radius, flags, reqs, inout, out_status), n < 0, stride < 4096, a
 * negative n_ents, a kind above 1, a layer outside [0, NAVHIP_NAV_LAYER_MAX). */
int  navhip_build_seek_fields(navhip_ctx *ctx, const navhip_world *world, const navhip_seek_game *game,
                              const navhip_seek_req *reqs, int n, uint8_t *inout, size_t stride,
                              uint8_t *out_status, uint8_t *out_seed_bits);
/* Every buffer resident, two launches on `stream` (seeds; fields), no synchronisation.  dev_world and dev_game are HOST
 * structures that cross by value and whose array pointers are DEVICE pointers, as navhip_world is in
 * navhip_agent_step_dev: the scalars and enemy_mask are read at the call.  The seed lists and the navhip_region_req table
 * between the two kernels live in the context (64 KB per request, grown on demand: a call with more requests than any
 * before it allocates); one such call of a context in flight at a time, or all of them on one stream.  dev_seed_bits may be
 * NULL.  A row the host form refuses comes back NAVHIP_SK_HOST. */
int  navhip_build_seek_fields_dev(navhip_ctx *ctx, const navhip_world *dev_world, const navhip_seek_game *dev_game,
                                  const navhip_seek_req *dev_reqs, int n, uint8_t *dev_inout, size_t stride,
                                  uint8_t *dev_status, uint8_t *dev_seed_bits, void *stream);

/* N_DesiredGroupArrivalVelocity (nav.c:3561) for nq points: the direction under each point in the chunk
 * field of mapping row rows[q] (region_field_slot / field_pool as in navhip_world; resident pool: pass
 * region_field_slot = field_pool = NULL), and whether that tile is a sink inside the zone's disc
 * (out_at_slot; centre_abs = zone centre in absolute nav tiles [nq][2] (row, column), radius[nq] in tiles).
 * out_dir[q]: 0..8 = enum flow_dir, 0xff = no field cached for the point's chunk (the reference returns
 * false).  Host buffers.  The arrival overlay's decisions around it (G_Arrival_DesiredVelocity,
 * arrival.c:862) are navhip_arrival_velocity's, which makes this lookup itself, per unit, on the device. */
int  navhip_region_lookup(navhip_ctx *ctx, int nq, const float *pos_xz, const int32_t *rows,
                          const int32_t *region_field_slot, int n_region_rows, const uint8_t *field_pool,
                          int n_field_slots, const int32_t *centre_abs, const int32_t *radius,
                          float map_pos_x, float map_pos_z, uint8_t *out_dir, uint8_t *out_at_slot);

/* Device spatial index only (bg_ent insert-all + cleanup + inrange_circle, bitmap_grid.h:1376):
 * for each query point the ids within `range`, in the reference's visiting order, capped at
 * maxout.  Host buffers.  Used by the parity tests of the neighbour gather. */
int  navhip_spatial_query(navhip_ctx *ctx, const navhip_world *world, const float *query_xz,
                          int nq, float range, int maxout, int32_t *out_counts, uint32_t *out_ids);

/* G_ClearPath_NewVelocity (clearpath.c:694) for nq independent problems, host buffers.
 * ent: [nq][5] {pos.x,pos.z,vel.x,vel.z,radius}; des_v: [nq][2]; dyn/stat: [nq][32][5] with
 * n_dyn/n_stat counts; out: [nq][2]. */
int  navhip_clearpath(navhip_ctx *ctx, int nq, const float *ent, const float *des_v,
                      const float *dyn, const int32_t *n_dyn, const float *stat,
                      const int32_t *n_stat, float *out);
/* The same problems on one row of 16 lanes each -- the form the agent step uses for agents with at most
 * 16 ClearPath neighbours (n_dyn + n_stat <= 16; navhip_clearpath runs one wave per problem, the
 * form for agents in a crowd). */
int  navhip_clearpath_rows(navhip_ctx *ctx, int nq, const float *ent, const float *des_v,
                           const float *dyn, const int32_t *n_dyn, const float *stat,
                           const int32_t *n_stat, float *out);
/* The same problems, each searched by the waves of one workgroup as a team -- the form the agent step
 * uses for agents with 17..64 ClearPath neighbours. */
int  navhip_clearpath_team(navhip_ctx *ctx, int nq, const float *ent, const float *des_v,
                           const float *dyn, const int32_t *n_dyn, const float *stat,
                           const int32_t *n_stat, float *out);

#ifdef __cplusplus
}
#endif
#endif /* NAVHIP_H */
