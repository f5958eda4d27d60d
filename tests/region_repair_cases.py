"""Hand-drawn worlds for the nearest-pathable repair of a region field (N_CellArrivalFieldUpdateToNearestPathable): at most
2 x 2 chunks, dim 96 unless stated.  A case is a dict: cost [H][W] u8, blk [H][W] u16 (absolute tiles), dim, centre, start,
target (of the N_CellArrivalFieldCreate field that is the repair's input), overlay ([k][2] or None) and `premise`, a function
of (case, model output, model info, model module) that asserts what the case is drawn for -- so no test passes on a
world that does not show it.  HOST_CASES are the rows that come back NAVHIP_RR_HOST; the reference asserts on them."""
import numpy as np


def _world(h, w):
    return np.ones((h * 64, w * 64), np.uint8), np.zeros((h * 64, w * 64), np.uint16)


def _case(cost, blk, centre, start, target, dim=96, overlay=None, premise=None):
    return dict(cost=cost, blk=blk, dim=dim, centre=centre, start=start, target=target,
                overlay=None if overlay is None else np.asarray(overlay, np.int16).reshape(-1, 2), premise=premise)


def _dir_at(case, out, M, tile):
    base = (case["centre"][0] - case["dim"] // 2, case["centre"][1] - case["dim"] // 2)
    return int(M.unpack(out, case["dim"])[tile[0] - base[0], tile[1] - base[1]])


def _differs(case, out, M, **kw):
    args = dict(overlay=case["overlay"], target=case["target"])
    args.update(kw)
    other, _ = M.repair(case["cost"], case["blk"], case["dim"], case["start"], case["centre"], case["field"], **args)
    return not np.array_equal(other, out)


def blob():
    cost, blk = _world(2, 2)
    blk[58:63, 68:73] = 1

    def premise(case, out, info, M):
        assert len(info["emitted"]) == 20 and info["written"].sum() == 25
        assert _dir_at(case, out, M, (60, 70)) in (M.FD_N, M.FD_S, M.FD_E, M.FD_W)
    return _case(cost, blk, (60, 70), (60, 70), (40, 50), premise=premise)


def single_tile():
    cost, blk = _world(2, 2)
    blk[60, 70] = 3

    def premise(case, out, info, M):
        assert info["emitted"] == [(60, 69), (60, 71), (59, 70), (61, 70)]          # the queue order W, E, N, S
        assert info["written"].sum() == 1 and _dir_at(case, out, M, (60, 70)) == M.FD_N
    return _case(cost, blk, (62, 66), (60, 70), (80, 90), premise=premise)


def weights():
    """A corridor of blocked cost-1 ground, open at its east end, between walls of cost-255 terrain one tile thick: out
    through a wall is 2 tiles and costs 256, out along the corridor is 8 tiles and costs 8."""
    cost, blk = _world(2, 2)
    cost[49:52, 40:48] = 255
    cost[50, 41:48] = 1
    blk[50, 41:48] = 1

    def premise(case, out, info, M):
        assert _dir_at(case, out, M, (50, 41)) == M.FD_E
        assert _differs(case, out, M, wrong="unit_cost")
    return _case(cost, blk, (60, 60), (50, 41), (70, 70), premise=premise)


def seams():
    cost, blk = _world(2, 2)
    blk[61:67, 61:67] = 1
    cost[62:66, 63] = 255

    def premise(case, out, info, M):
        rows, cols = np.nonzero(info["written"])
        base = info["base"]
        assert {(r + base[0]) >> 6 for r in rows} == {0, 1} and {(c + base[1]) >> 6 for c in cols} == {0, 1}
    return _case(cost, blk, (64, 64), (63, 64), (30, 100), premise=premise)


def far_clamp():
    """1 x 1 chunks, the centre in the middle: both clamps bind on both axes, R == C == 63.  The blob lies in the map's
    corner; arms of it run along the last row and the last column, which are not part of the flood."""
    cost, blk = _world(1, 1)
    blk[58:64, 58:64] = 1
    blk[63, 45:58] = 1
    blk[45:58, 63] = 1

    def premise(case, out, info, M):
        assert (info["R"], info["C"]) == (63, 63)
        assert all(r < 63 and c < 63 for r, c in info["emitted"])
        assert (62, 50) not in info["emitted"] and _dir_at(case, out, M, (63, 50)) != M.FD_N
        assert _differs(case, out, M, wrong="flood_last_row")
    return _case(cost, blk, (32, 32), (60, 60), (10, 12), premise=premise)


def tall():
    """2 chunks high, 1 wide: R == 96 > C == 63, the injective arm on a clamped region that is not square."""
    cost, blk = _world(2, 1)
    blk[60:70, 20:30] = 1
    blk[64, 30:63] = 1

    def premise(case, out, info, M):
        assert (info["R"], info["C"]) == (96, 63) and info["alias_hits"] == 0
        assert not _differs(case, out, M, wrong="injective_visited")
    return _case(cost, blk, (64, 32), (65, 25), (100, 40), premise=premise)


def wide():
    """1 chunk high, 2 wide: R == 63 < C == 96.  Two bars two rows thick, joined, run past column 63 of the clamped region,
    where (dr, dc >= R) shares its visited flag with (dr + 1, dc - R)."""
    cost, blk = _world(1, 2)
    blk[30:32, 36:107] = 1
    blk[32:40, 66] = 1
    blk[40:42, 50:110] = 1

    def premise(case, out, info, M):
        assert (info["R"], info["C"]) == (63, 96) and info["alias_hits"] > 0
        assert _differs(case, out, M, wrong="injective_visited")
    return _case(cost, blk, (32, 64), (30, 56), (10, 20), premise=premise)


def overlay():
    cost, blk = _world(2, 2)
    blk[58:63, 68:73] = 1
    # beside the component: (57, 70), (60, 73); behind them: (56, 70), (55, 70), (60, 74), (60, 75); outside the region: (5, 5)
    ov = [(57, 70), (60, 73), (56, 70), (55, 70), (60, 74), (60, 75), (5, 5)]

    def premise(case, out, info, M):
        assert (57, 70) in info["emitted"] and (60, 73) in info["emitted"]
        for t in ((56, 70), (55, 70), (60, 74), (60, 75)):
            assert t not in info["emitted"] and info["written"][t[0] - info["base"][0], t[1] - info["base"][1]]
        assert _dir_at(case, out, M, (55, 70)) == M.FD_S and _dir_at(case, out, M, (60, 75)) == M.FD_W
        assert _differs(case, out, M, overlay=None)
    return _case(cost, blk, (64, 64), (60, 70), (90, 40), overlay=ov, premise=premise)


def overlay_on_start():
    """The unit stands on a blocked tile that another subformation's occupied cell covers too: the overlay names the start
    tile itself -- several times, at indices 64 and above, behind padding of in-region tiles that nothing reaches -- and the
    rest of the blob.  The flood takes no overlay, so the start is still where it begins."""
    cost, blk = _world(2, 2)
    blk[58:63, 68:73] = 1
    pad = [(100, c) for c in range(20, 96)] + [(102, c) for c in range(20, 96)] + [(104, c) for c in range(20, 96)]
    ov = pad[:76] + [(60, 70)] + pad[76:130] + [(60, 70)] + pad[130:200] + [(60, 70), (60, 70)] + pad[200:]
    ov += [(r, c) for r in range(58, 63) for c in range(68, 73)] + [(57, 70), (56, 70)]

    def premise(case, out, info, M):
        at = [k for k, t in enumerate(case["overlay"].tolist()) if tuple(t) == case["start"]]
        assert len(at) == 5 and min(at) >= 64 and {k // 64 for k in at} >= {1, 2, 3}
        assert len(info["emitted"]) == 20 and info["written"].sum() == 26
        base = info["base"]
        assert info["written"][60 - base[0], 70 - base[1]] and info["written"][56 - base[0], 70 - base[1]]
        assert not info["written"][100 - base[0], 50 - base[1]]
    return _case(cost, blk, (64, 64), (60, 70), (90, 40), overlay=ov, premise=premise)


def _serpentine(runs, r0=22, c0=23, c1=105, wall=5):
    """Two serpentines in one component.  The upper one drives the relaxation: a block of cost-255 terrain with a serpentine
    of blocked cost-1 ground inside, `runs` rows c0 .. c1 - 1 joined at alternating ends, `wall` tiles of terrain around and
    a neck from the first run's west end up through the top wall -- along the serpentine is cheaper than through 255 * wall
    of terrain, so the cheapest way out is as long as it.  The lower one drives the flood: `runs` - 1 rows of blocked ground
    in open ground, hung below the block; every tile of it has a way out beside it, and the flood from its far end has to
    walk all of it.  Returns (cost, blk, tiles of the upper one, tiles of the lower one)."""
    cost, blk = _world(2, 2)
    rows = 2 * runs - 1
    cost[r0 - wall:r0 + rows + wall, c0 - wall:c1 + wall] = 255

    def snake(top, n, left, right):
        out = []
        for k in range(n):
            r = top + 2 * k
            out += [(r, c) for c in (range(left, right) if k % 2 == 0 else range(right - 1, left - 1, -1))]
            if k + 1 < n:
                out.append((r + 1, right - 1 if k % 2 == 0 else left))
        return out
    upper = [(r, c0) for r in range(r0 - wall, r0)] + snake(r0, runs, c0, c1)
    below = r0 + rows + wall
    lower = [(below, 20)] + snake(below + 1, runs - 1, 20, 108)
    for r, c in upper + lower:
        cost[r, c], blk[r, c] = 1, 1
    return cost, blk, upper, lower


def depth():
    cost, blk, upper, lower = _serpentine(13)

    def premise(case, out, info, M):
        assert len(upper) >= 1000 and len(lower) >= 1000 and info["flood_depth"] >= 1000 and info["relax_hops"] >= 1000
    return _case(cost, blk, (64, 64), lower[-1], (100, 100), premise=premise)


def border():
    """The start's component leaves the region on its west side (the region is rows and columns 16 .. 111); the target lies
    on the region's far edge, where N_CellArrivalFieldCreate shifts its base by one tile and the repair does not."""
    cost, blk = _world(2, 2)
    blk[50, 10:60] = 1
    blk[40:50, 16] = 1

    def premise(case, out, info, M):
        assert blk[50, 10:16].all() and all(16 <= r < 112 and 16 <= c < 112 for r, c in info["emitted"])
        assert info["base"] == (16, 16) and _dir_at(case, out, M, (50, 16)) in (M.FD_N, M.FD_S, M.FD_E)
        assert (45, 15) not in info["emitted"] and _dir_at(case, out, M, (45, 16)) == M.FD_E
        assert _differs(case, out, M, wrong="create_base")
    return _case(cost, blk, (64, 64), (50, 30), (112, 70), premise=premise)


def dim8():
    cost, blk = _world(1, 1)
    blk[19:21, 20:22] = 1
    cost[20, 21] = 255

    def premise(case, out, info, M):
        assert info["written"].sum() == 4 and len(info["emitted"]) == 8
    return _case(cost, blk, (20, 20), (19, 20), (17, 23), dim=8, premise=premise)


def dim128():
    """The largest region: 2 x 2 chunks, base (0, 0), R == C == 127."""
    cost, blk = _world(2, 2)
    blk[100:128, 90:95] = 1
    blk[110, 20:90] = 1
    cost[3:9, 3:9] = 255
    blk[0:3, 0:12] = 1

    def premise(case, out, info, M):
        assert (info["R"], info["C"]) == (127, 127) and info["base"] == (0, 0)
        assert info["written"][127, 92] and info["written"][110, 20] and not info["written"][1, 1]
    return _case(cost, blk, (64, 64), (120, 92), (30, 30), dim=128, premise=premise)


CASES = {"blob": blob, "single_tile": single_tile, "weights": weights, "seams": seams, "far_clamp": far_clamp, "tall": tall,
         "wide": wide, "overlay": overlay, "overlay_on_start": overlay_on_start, "depth": depth, "border": border, "dim8": dim8,
         "dim128": dim128}


def host_cases():
    """name -> (case, why): rows that are the host's.  Their slots come back byte for byte as they went in."""
    a = blob()
    a["start"] = (50, 50)                                   # passable
    b = far_clamp()
    b["start"] = (63, 60)                                   # blocked, on the map's last row: outside the clamped region
    c = far_clamp()
    c["start"] = (64, 60)                                   # off the map
    return {"passable_start": a, "start_outside_clamped_region": b, "start_off_map": c}


_built = {}


def get(name, M):
    """The case with its input fields: `field` (the model's N_CellArrivalFieldCreate for the case's target) and `noise`
    (random nibbles: every nibble the repair does not own must survive).  Built once."""
    if name not in _built:
        case = (CASES.get(name) or host_cases().get(name))
        case = case() if callable(case) else case
        case["name"] = name
        case["field"] = M.create(case["cost"], case["blk"], case["dim"], case["target"], case["centre"], case["overlay"])
        case["noise"] = np.random.RandomState(len(name)).randint(0, 256, case["dim"] ** 2 // 2).astype(np.uint8)
        _built[name] = case
    return _built[name]
