"""What the workload of tick.NavTick IS, on the host alone: the region tiling, the obstacle circles and their move stream,
destinations and agents, which destinations' tiles travel, the request stream with its per-rank slices and slot table,
the level order of the planner's LOS chain.  Pure numpy over synth and the record types of navhip: nothing here loads
the library, touches a device or needs PyTorch, so every table a benchmark line rests on can be tested by itself
(tests/test_plan_cpu.py).  tick.NavTick supplies the two planes only the library gives -- the blocker plane behind the
start circles, the local-island plane -- between the calls."""
import collections

import numpy as np

from . import navhip, synth

Layout = collections.namedtuple("Layout", "chunk_w shared_map reg_rows reg_cols Wt H nchunks")
Requests = collections.namedtuple("Requests", "reqs dest_of_req req_bounds xchg_bounds tile_exchange slot_tbl "
                                              "n_requests_served request_source")
LosLayout = collections.namedtuple("LosLayout", "reqs prev_slot chain_prev bounds level slot_tbl")


def region_grid(world):
    """(rows, cols) of the region tiling for `world` ranks: cols = the smallest power of two that is
    >= sqrt(world), rows = ceil(world / cols): 1x1, 1x2, 2x2, 2x4, 4x4."""
    cols = 1
    while cols * cols < world:
        cols *= 2
    return -(-world // cols), cols


def layout(chunk_w, world, shared_map=False):
    """`world` regions of chunk_w x chunk_w chunks tiling one map of Wt x H chunks (a map side is at most 64 chunks, the
    reference's 6-bit chunk ids).  shared_map (BASELINE configs[3], strong scaling): ONE chunk_w x chunk_w map for
    every rank; destinations and agents are split over the ranks, anywhere on the map."""
    reg_rows, reg_cols = (1, 1) if shared_map else region_grid(world)
    Wt, H = chunk_w * reg_cols, chunk_w * reg_rows
    if max(Wt, H) > 64:
        raise ValueError("%d regions of %d chunks do not fit a 64x64-chunk map" % (world, chunk_w))
    return Layout(chunk_w, bool(shared_map), reg_rows, reg_cols, Wt, H, Wt * H)


def region_cells(lay, q):
    """(row0, row1, col0, col1) of region q, in cells."""
    rcols = lay.chunk_w * 64                        # cell rows / columns per region
    if lay.shared_map:
        return 0, rcols, 0, rcols
    qr, qc = divmod(q, lay.reg_cols)
    return qr * rcols, (qr + 1) * rcols, qc * rcols, (qc + 1) * rcols


def obstacle_stream(grid, lay, obstacles, move_frac, obstacle_ticks):
    """configs[4]: dynamic obstacles (circles, radius U(2,6) wu, seed 99) dropped through the device N_BlockersIncref
    path; every tick `move_frac` of them move (decref + incref).  Returns the start circles and the (ticks, 2*nmove)
    move records of CIRCLE_DTYPE: per tick the nmove circles that leave (delta -1), then where they land (delta +1)."""
    rng = np.random.RandomState(99)
    cells = synth.passable_cells(grid)
    pos = synth.cell_centre(lay.Wt, lay.H, *cells[rng.randint(len(cells), size=obstacles)].T)
    circ = np.zeros(obstacles, navhip.CIRCLE_DTYPE)
    circ["x"], circ["z"] = pos[:, 0], pos[:, 1]
    circ["radius"] = rng.uniform(2.0, 6.0, obstacles)
    circ["delta"] = 1
    nmove = max(1, int(round(obstacles * move_frac)))
    moves = np.zeros((obstacle_ticks, 2 * nmove), navhip.CIRCLE_DTYPE)
    cur = circ.copy()
    for t in range(obstacle_ticks):
        who = rng.choice(obstacles, nmove, replace=False)
        moves[t, :nmove] = cur[who]
        moves[t, :nmove]["delta"] = -1
        npos = synth.cell_centre(lay.Wt, lay.H, *cells[rng.randint(len(cells), size=nmove)].T)
        cur["x"][who], cur["z"][who] = npos[:, 0], npos[:, 1]
        moves[t, nmove:] = cur[who]
        moves[t, nmove:]["delta"] = 1
    return circ, moves


def population(grid, lay, world, fields_per_rank, agents_per_rank, hz, blockers=None, crowd_cells=0, straddle=0.0):
    """Destinations (cheap, all regions; global cells) and agents (the replicated snapshot, the columns of
    synth.agents concatenated in rank order): region q's flocks are its own destinations."""
    dests, ag_parts = [], []
    for q in range(world):
        r0, r1, c0, c1 = region_cells(lay, q)
        d = synth.destinations(grid[r0:r1, c0:c1], fields_per_rank, seed=42 + q)
        dests.append(d + np.array([r0, c0]))
        a = synth.agents(grid, agents_per_rank, fields_per_rank, seed=7 + q, hz=hz, blockers=blockers,
                         cols=(c0, c1), rows=(r0, r1), crowd_cells=crowd_cells)
        a["flock"] = a["flock"] + q * fields_per_rank
        ag_parts.append(a)
    if straddle > 0 and world > 1:
        # flocks that straddle ranks: in the last `straddle` of every rank's uid slab sit agents of the
        # NEXT region (position and flock; the lower half of its flocks only) -- stepped here, sampling
        # fields another rank builds
        m = int(round(agents_per_rank * (1.0 - straddle)))
        swapped = []
        for q, a in enumerate(ag_parts):
            nxt = ag_parts[(q + 1) % world]
            take = np.zeros(agents_per_rank, bool)
            take[m:] = (nxt["flock"][m:] % fields_per_rank) < max(1, fields_per_rank // 2)
            swapped.append({k: (v if k == "hz" else
                                np.where(take.reshape((-1,) + (1,) * (np.ndim(v) - 1)), nxt[k], v))
                            for k, v in a.items()})
        ag_parts = swapped
    ag = {k: (np.concatenate([a[k] for a in ag_parts]) if k != "hz" else hz) for k in ag_parts[0]}
    return np.concatenate(dests), ag


def travelling_destinations(flock, agents_per_rank, fields_per_rank, n_dests):
    """tile_exchange="auto": destination d is built by rank d // fields_per_rank; its baked tiles have to
    travel when some agent of its flock sits in another rank's uid slab (uid // agents_per_rank).
    Returns a bool array [n_dests]."""
    flock = np.asarray(flock)
    travels = np.zeros(n_dests, bool)
    ok = flock >= 0
    stepped_by = np.arange(len(flock)) // agents_per_rank
    travels[np.unique(flock[ok & (stepped_by != flock // fields_per_rank)])] = True
    return travels


def travel_first(dest_of_req, travels):
    """Stable order of one rank's requests with those of the travelling destinations first -- one
    contiguous run per rank to exchange -- and the length of that run."""
    first = np.asarray(travels)[np.asarray(dest_of_req)]
    return np.argsort(~first, kind="stable"), int(first.sum())


def request_stream(grid, lay, dests, flock, liid, rank, world, fields_per_rank, agents_per_rank, tile_exchange="auto",
                   solo=False, planner_requests=True, share_fields=False, obstacles=0):
    """The chunk-field requests of the job: region-major, destination-major inside a region; field slot = position in
    the stream.  req_bounds[q] = the slice rank q builds, xchg_bounds[q] = its rows the other ranks need,
    slot_tbl[destination, chunk] = the slot that holds the field (-1: none).
    tile_exchange: "auto" = only the fields some other rank samples travel (none when flocks are rank aligned, the
    default world; `straddle` makes some); "all" = every rank holds every tile, all-gathered every tick (SURVEY
    section 8(e) worst case: any agent may sample any field).  solo (tests): this one process builds every region's
    fields and steps every agent.  Where no tile travels only `rank`'s own region is planned."""
    if share_fields and (world != 1 or obstacles):
        raise ValueError("share_fields: single-process worlds without moving obstacles only")
    K = fields_per_rank * world
    tile_exchange = "all" if ((tile_exchange == "all" or solo) and world > 1) else "none"
    # "auto": destination d (built by rank d // fields_per_rank) travels when some agent of its flock sits in another
    # rank's uid slab
    travels = np.zeros(K, bool)
    if world > 1:
        travels = travelling_destinations(flock, agents_per_rank, fields_per_rank, K)
        if tile_exchange == "none" and travels.any():
            tile_exchange = "auto"
    req_parts, dest_parts, nreq = [], [], 0
    req_bounds, xchg_bounds = [(0, 0)] * world, [(0, 0)] * world
    for q in (range(world) if tile_exchange != "none" else [rank]):
        r0, r1, c0, c1 = region_cells(lay, q)
        d_q = dests[q * fields_per_rank:(q + 1) * fields_per_rank] - np.array([r0, c0])
        # the reference planner's own request stream where a fixture holds it (the single-GPU configs:
        # tests/tools/make_requests.py), else the numpy stand-in
        cols = synth.planner_requests(grid[r0:r1, c0:c1], d_q) if planner_requests else None
        request_source = "reference planner (n_request_path) fixture" if cols is not None else \
            "numpy stand-in (synth.whole_map_requests)"          # (the last region's answer is the one reported)
        if cols is None:
            cols = synth.whole_map_requests(grid[r0:r1, c0:c1], d_q, liid[r0:r1, c0:c1])
        n_q = len(cols["type"])
        if tile_exchange == "auto":
            # the travelling destinations' requests first: one contiguous run per rank to exchange
            order, n_first = travel_first(np.asarray(cols["dest"]) + q * fields_per_rank, travels)
            cols = {k: np.asarray(v)[order] for k, v in cols.items() if k in synth.REQ_FIELDS or k == "dest"}
            xchg_bounds[q] = (nreq, nreq + n_first)
        else:
            xchg_bounds[q] = (nreq, nreq + n_q)
        reqs_q = navhip.make_reqs(n_q)
        for k in synth.REQ_FIELDS:
            reqs_q[k] = cols[k]
        reqs_q["chunk_r"] += r0 // 64
        reqs_q["chunk_c"] += c0 // 64
        portal = reqs_q["type"] == navhip.TARGET_PORTAL
        reqs_q["next_chunk_r"][portal] += r0 // 64
        reqs_q["next_chunk_c"][portal] += c0 // 64
        req_parts.append(reqs_q)
        dest_parts.append(np.asarray(cols["dest"]) + q * fields_per_rank)
        req_bounds[q] = (nreq, nreq + n_q)
        nreq += n_q
    reqs, dest_of_req = np.concatenate(req_parts), np.concatenate(dest_parts)
    if obstacles:
        reqs["flags"] = navhip.REQ_LIVE_IIDS | navhip.REQ_IF_CHANGED
    slot_tbl = -np.ones((K, lay.nchunks), np.int32)
    chunk = reqs["chunk_r"].astype(np.int64) * lay.Wt + reqs["chunk_c"]
    if share_fields:
        # the reference keys its field cache by N_FlowFieldID (field.c:1952) -- chunk + target, NOT the destination --
        # so destinations whose paths leave a chunk through the same portal share ONE field (N_FC_PutDestFFMapping maps
        # both to it, nav.c:2008-2021), and a tick after a wholesale invalidation rebuilds every DISTINCT field once.
        # Identical request records are built once and every (dest, chunk) entry of the slot table points at the
        # shared slot.  (Default off: every request is rebuilt.)
        uniq, first, inv = np.unique(reqs, return_index=True, return_inverse=True)
        order = np.sort(first)                       # (keep the stream's order: first occurrences)
        rank_of = np.empty(len(first), np.int64)
        rank_of[np.argsort(first)] = np.arange(len(first))
        slot_tbl[dest_of_req, chunk] = rank_of[inv.reshape(-1)]
        reqs, dest_of_req = reqs[order], dest_of_req[order]
        req_bounds, xchg_bounds = [(0, len(reqs))], [(0, len(reqs))]
    else:
        slot_tbl[dest_of_req, chunk] = np.arange(nreq)
    return Requests(reqs, dest_of_req, req_bounds, xchg_bounds, tile_exchange, slot_tbl, nreq, request_source)


def los_layout(lc, dests, lay, K):
    """The planner's LOS chain `lc` (synth.planner_los: creation order) laid out for the device: pool slot = position in
    level order (level = hops from the destination chunk along the chain), so that one build per level finds every
    predecessor in the level before.  reqs: the LOS_REQ_DTYPE records in slot order; prev_slot: the predecessor's slot
    (0 where there is none: never read), chain_prev the same with -1 there; bounds: levels + 1 slot offsets; level: of
    every slot; slot_tbl[destination, chunk] = slot (-1: the planner holds no such field)."""
    n = len(lc["dest"])
    key = lc["dest"] * lay.nchunks + lc["chunk_r"] * lay.Wt + lc["chunk_c"]
    pkey = lc["dest"] * lay.nchunks + (lc["chunk_r"] + lc["prev_dr"]) * lay.Wt + (lc["chunk_c"] + lc["prev_dc"])
    has_prev = (lc["prev_dr"] != 0) | (lc["prev_dc"] != 0)
    index_of = {int(k): i for i, k in enumerate(key)}
    level = np.zeros(n, np.int64)
    prev_i = np.full(n, -1, np.int64)
    for i in range(n):                       # (creation order: a predecessor always comes first)
        if has_prev[i]:
            prev_i[i] = index_of[int(pkey[i])]
            level[i] = level[prev_i[i]] + 1
    order = np.argsort(level, kind="stable")
    slot_of = np.empty(n, np.int64)
    slot_of[order] = np.arange(n)
    reqs = np.zeros(n, navhip.LOS_REQ_DTYPE)
    reqs["faction_id"] = navhip.FACTION_ID_NONE
    reqs["chunk_r"], reqs["chunk_c"] = lc["chunk_r"][order], lc["chunk_c"][order]
    d = lc["dest"][order]
    reqs["target_chunk_r"], reqs["target_chunk_c"] = dests[d, 0] // 64, dests[d, 1] // 64
    reqs["target_tile_r"], reqs["target_tile_c"] = dests[d, 0] % 64, dests[d, 1] % 64
    reqs["prev_dr"], reqs["prev_dc"] = lc["prev_dr"][order], lc["prev_dc"][order]
    prev_slot = np.where(prev_i[order] >= 0, slot_of[np.maximum(prev_i[order], 0)], 0)
    chain_prev = np.where(prev_i[order] >= 0, prev_slot, -1).astype(np.int32)
    lv = level[order]
    bounds = np.searchsorted(lv, np.arange(lv.max() + 2))
    tbl = -np.ones((K, lay.nchunks), np.int32)
    tbl[lc["dest"], lc["chunk_r"] * lay.Wt + lc["chunk_c"]] = slot_of
    return LosLayout(reqs, prev_slot, chain_prev, bounds, lv, tbl)
