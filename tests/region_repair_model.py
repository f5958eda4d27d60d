"""A numpy model of N_CellArrivalFieldUpdateToNearestPathable, written from the reference's field.c and from nothing else:
clamped_region :1892, field_passable_frontier :1441 (a literal serial FIFO with the visited index of :1431, stride R while
dc runs to C - 1), the seeds :2663, field_build_integration_nonpass_region :678 (heapq), field_flow_dir :355 and the bake
:2691 with set_flow_cell :790.  `create` is N_CellArrivalFieldCreate :2445 (enemies == 0), the input of the cases.

A world is (cost [H][W] u8, blockers [H][W] u16) over absolute tiles.  `wrong` switches on ONE of the variants of WRONG, the
mistakes a restatement is likely to make; tests/test_region_repair_cpu.py shows that each changes bytes on some case."""
import heapq

import numpy as np

INF = np.inf
FD_NONE, FD_NW, FD_N, FD_NE, FD_W, FD_E, FD_SW, FD_S, FD_SE = range(9)
RR_HOST = 0x80
WRONG = ("injective_visited", "flood_last_row", "flood_overlay", "unit_cost", "enemies_passability", "create_base",
         "seeds_to_none")


def passable(cost, blk):
    """field_tile_passable :117"""
    return (cost != 255) & (blk == 0)


def flow_dirs(integ):
    """field_flow_dir :355 of every cell of a square integration field (float, INF = unreached); cells whose neighbours
    are all INF get FD_SE's slot of the select and must not be used."""
    P = np.full((integ.shape[0] + 2, integ.shape[1] + 2), INF)
    P[1:-1, 1:-1] = integ
    dn, ds, dw, de = P[:-2, 1:-1], P[2:, 1:-1], P[1:-1, :-2], P[1:-1, 2:]
    dnw, dne, dsw, dse = P[:-2, :-2], P[:-2, 2:], P[2:, :-2], P[2:, 2:]
    mc = np.minimum(np.minimum(dn, ds), np.minimum(dw, de))
    mc = np.where((dn < INF) & (dw < INF), np.minimum(mc, dnw), mc)
    mc = np.where((dn < INF) & (de < INF), np.minimum(mc, dne), mc)
    mc = np.where((ds < INF) & (dw < INF), np.minimum(mc, dsw), mc)
    mc = np.where((ds < INF) & (de < INF), np.minimum(mc, dse), mc)
    return np.select([dn == mc, ds == mc, de == mc, dw == mc, dnw == mc, dne == mc, dsw == mc, dse == mc],
                     [FD_N, FD_S, FD_E, FD_W, FD_NW, FD_NE, FD_SW, FD_SE], 0).astype(np.uint8)


def pack(dirs):
    """[dim][dim] directions -> dim * dim / 2 bytes, even column in the high nibble (set_flow_cell :790)"""
    return ((dirs[:, 0::2] << 4) | dirs[:, 1::2]).astype(np.uint8).reshape(-1)


def unpack(field, dim):
    b = np.asarray(field, np.uint8)[:dim * dim // 2].reshape(dim, dim // 2)
    out = np.zeros((dim, dim), np.uint8)
    out[:, 0::2], out[:, 1::2] = b >> 4, b & 15
    return out


def _overlay_mask(overlay, base, dim):
    m = np.zeros((dim, dim), bool)                                      # build_overlay_mask :571
    for r, c in (() if overlay is None else overlay):
        dr, dc = int(r) - base[0], int(c) - base[1]
        if 0 <= dr < dim and 0 <= dc < dim:
            m[dr, dc] = True
    return m


def _dijkstra(integ, heap, base, dim, H, W, may_enter, step_cost):
    """The loop of :599 / :690: 4 neighbours on the map and inside [base, base + dim)^2.  Returns the hops of each tile's
    cheapest path as found."""
    hops = np.zeros((dim, dim), np.int32)
    while heap:
        d, dr, dc = heapq.heappop(heap)
        if d > integ[dr, dc]:
            continue
        for ddr, ddc in ((-1, 0), (0, -1), (0, 1), (1, 0)):
            nr, nc = dr + ddr, dc + ddc
            ar, ac = base[0] + nr, base[1] + nc
            if not (0 <= ar < H and 0 <= ac < W) or not (0 <= nr < dim and 0 <= nc < dim):
                continue
            if not may_enter(nr, nc, ar, ac):
                continue
            t = d + step_cost(ar, ac)
            if t < integ[nr, nc]:
                integ[nr, nc] = t
                hops[nr, nc] = hops[dr, dc] + 1
                heapq.heappush(heap, (t, nr, nc))
    return hops


def create(cost, blk, dim, target, centre, overlay=None):
    """N_CellArrivalFieldCreate :2445 with enemies == 0 -> dim * dim / 2 bytes"""
    H, W = cost.shape
    base = [centre[0] - dim // 2, centre[1] - dim // 2]
    for k in (0, 1):
        if target[k] - base[k] >= dim:                                  # :2483
            base[k] = target[k] - (dim - 1)
    ok = passable(cost, blk)
    mask = _overlay_mask(overlay, base, dim)
    integ = np.full((dim, dim), INF)
    tr, tc = target[0] - base[0], target[1] - base[1]
    assert 0 <= tr < dim and 0 <= tc < dim
    integ[tr, tc] = 0.0
    _dijkstra(integ, [(0.0, tr, tc)], base, dim, H, W, lambda nr, nc, ar, ac: ok[ar, ac] and not mask[nr, nc],
              lambda ar, ac: float(cost[ar, ac]))
    dirs = np.where((integ < INF) & (integ != 0.0), flow_dirs(integ), 0).astype(np.uint8)      # :816-826
    return pack(dirs)


def clamped_region(H, W, dim, centre, last_row=False):
    """:1892 -> (cb_r, cb_c, R, C)"""
    base = (centre[0] - dim // 2, centre[1] - dim // 2)
    cb = (max(base[0], 0), max(base[1], 0))
    far = 0 if last_row else 1
    return cb[0], cb[1], min(base[0] + dim, H - far) - cb[0], min(base[1] + dim, W - far) - cb[1]


def status(cost, blk, dim, start, centre):
    """0, or RR_HOST for the rows on which the reference asserts or leaves its arrays"""
    H, W = cost.shape
    if not (0 <= start[0] < H and 0 <= start[1] < W and 0 <= centre[0] < H and 0 <= centre[1] < W):
        return RR_HOST
    if passable(cost, blk)[start[0], start[1]]:
        return RR_HOST
    cb_r, cb_c, R, C = clamped_region(H, W, dim, centre)
    if not (0 <= start[0] - cb_r < R and 0 <= start[1] - cb_c < C):
        return RR_HOST
    return 0


def repair(cost, blk, dim, start, centre, field, overlay=None, wrong=None, target=None):
    """N_CellArrivalFieldUpdateToNearestPathable :2603 on a copy of `field` -> (bytes, info).  info: R, C, emitted (absolute
    tiles in queue order), alias_hits (pushes a flag set for ANOTHER tile prevented), flood_depth, relax_hops, written."""
    assert wrong is None or wrong in WRONG
    H, W = cost.shape
    ok = passable(cost, blk)
    base = [centre[0] - dim // 2, centre[1] - dim // 2]                  # :2654: no target clamp
    if wrong == "create_base":
        for k in (0, 1):
            if target[k] - base[k] >= dim:
                base[k] = target[k] - (dim - 1)
    mask = _overlay_mask(overlay, base, dim)
    cb_r, cb_c, R, C = clamped_region(H, W, dim, centre, last_row=wrong == "flood_last_row")
    stride = max(R, C) if wrong == "injective_visited" else R

    def flood_passable(ar, ac):
        if wrong == "flood_overlay":
            mr, mc = ar - base[0], ac - base[1]
            if 0 <= mr < dim and 0 <= mc < dim and mask[mr, mc]:
                return False
        return ok[ar, ac]

    # ---- field_passable_frontier :1441
    assert not ok[start[0], start[1]]
    nelems = max(R, C) ** 2
    visited, owner = np.zeros(nelems, bool), {}
    queue, head, emitted, alias_hits = [(start[0] - cb_r, start[1] - cb_c, 0)], 0, [], 0
    visited[queue[0][0] * stride + queue[0][1]] = True
    owner[queue[0][0] * stride + queue[0][1]] = queue[0][:2]
    flood_depth = 0
    while head < len(queue):
        dr, dc, depth = queue[head]
        head += 1
        flood_depth = max(flood_depth, depth)
        if flood_passable(cb_r + dr, cb_c + dc):
            emitted.append((cb_r + dr, cb_c + dc))
            continue
        for ddr, ddc in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            nr, nc = dr + ddr, dc + ddc
            if not (0 <= cb_r + nr < H and 0 <= cb_c + nc < W):          # M_Tile_RelativeDesc
                continue
            if nr < 0 or nr >= R or nc < 0 or nc >= C:                  # tile_outside_region
                continue
            vi = nr * stride + nc
            if visited[vi]:
                alias_hits += owner[vi] != (nr, nc)
                continue
            visited[vi] = True
            owner[vi] = (nr, nc)
            assert len(queue) < nelems
            queue.append((nr, nc, depth + 1))

    # ---- the seeds :2663
    integ = np.full((dim, dim), INF)
    heap = []
    for ar, ac in emitted:
        dr, dc = ar - base[0], ac - base[1]
        if dr < 0 or dr >= dim or dc < 0 or dc >= dim:
            continue
        integ[dr, dc] = 0.0
        heap.append((0.0, dr, dc))
    heapq.heapify(heap)

    # ---- field_build_integration_nonpass_region :678
    relax_ok = (cost != 255) if wrong == "enemies_passability" else ok
    hops = _dijkstra(integ, heap, base, dim, H, W, lambda nr, nc, ar, ac: not (relax_ok[ar, ac] and not mask[nr, nc]),
                     lambda ar, ac: 1.0 if wrong == "unit_cost" else float(cost[ar, ac]))

    # ---- the bake :2691
    rr, cc = np.meshgrid(np.arange(dim) + base[0], np.arange(dim) + base[1], indexing="ij")
    on_map = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
    write = on_map & (integ < INF) & (integ != 0.0)
    dirs = unpack(field, dim)
    dirs[write] = flow_dirs(integ)[write]
    if wrong == "seeds_to_none":
        dirs[on_map & (integ == 0.0)] = FD_NONE
    out = np.array(field, np.uint8)
    out[:dim * dim // 2] = pack(dirs)
    info = dict(R=R, C=C, base=tuple(base), emitted=emitted, alias_hits=int(alias_hits), flood_depth=flood_depth,
                relax_hops=int(hops[write].max()) if write.any() else 0, written=write, integ=integ)
    return out, info
