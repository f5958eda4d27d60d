"""The worlds of the arrival first-build tests (tests/test_arrival_build_cpu.py, _gpu.py): INACTIVE zones with their rooms
on maps of at most 2 x 2 chunks (one 3 x 1 map for the window row: a 2 x 2 map cannot leave a window of 127 tiles), as the
dicts tests/arrival_build_model.py takes.  A world: w, h, cost / blockers {layer: [h][w][64][64]}, zones, members, targets,
pos [n][2], names {zone name: index}.  Every builder returns plain data; nothing here calls the device or the reference."""
import numpy as np

from tests import arrival_build_model as abm
from tests.arrival_flock_worlds import members, xz

F = np.float32
EXACT_UR = F(6.4864864)          # 1.85f * this == 12.0f: slots three tiles apart lie at exactly spacing * spacing


class World:
    def __init__(self, w, h, layers=(0,)):
        self.w, self.h = w, h
        self.blockers = {l: np.zeros((h, w, 64, 64), np.uint16) for l in layers}
        self.cost = {l: np.ones((h, w, 64, 64), np.uint8) for l in layers}
        self.zones, self.members, self.targets, self.pos, self.names = [], [], [], [], {}

    def block(self, tiles, layer=0, count=1):
        for r, c in tiles:
            self.blockers[layer][r >> 6, c >> 6, r & 63, c & 63] = count

    def wall(self, tiles):
        """COST_IMPASSABLE tiles: one base cost for every layer, as the reference derives its layers"""
        for layer in self.cost:
            for r, c in tiles:
                self.cost[layer][r >> 6, c >> 6, r & 63, c & 63] = 255

    def p(self, r, c, off=(0.0, 0.0)):
        return xz(self.w, self.h, r, c, off)

    def add(self, name, target, member_pos, ur=1.0, total=None, layer=0, phase=abm.INACTIVE, room=None, settled=None):
        """An INACTIVE zone with exactly the room it needs (or `room` = (slots, keys)), filled with recognisable junk."""
        n = len(member_pos)
        total = n if total is None else total
        with np.errstate(all="ignore"):
            ok = np.isfinite(ur) and ur > 0
            slots, keys = abm.room_needed(total, F(ur)) if ok and total > 0 else (4, 4)
        if room is not None:
            slots, keys = room
        k = len(self.zones)
        z = {"layer": 7, "centre_xz": np.array([-1.5, 2.5], F), "radius": 99, "unit_radius": F(0.25), "fill_frac": F(0.5),
             "active_row": 3, "num_rows": 5, "slots_xz": np.full((slots, 2), F(1000 + k), F), "slot_ring": np.full(slots, 40 + k, np.int32),
             "room_keys": np.arange(keys, dtype=np.uint64) + np.uint64(1 << 60), "phase": phase, "realloc_counter": 2,
             "stall_counter": 5, "prev_occ": 6, "row_height": F(9.5), "arg_layer": layer, "arg_unit_radius": F(ur),
             "arg_total_members": total}
        rows = []
        for i, pos in enumerate(member_pos):
            self.pos.append(np.asarray(pos, F))
            rows.append((len(self.pos) - 1, 0 if settled is None else settled[i], i % 2, i % 3 == 0, (F(i), F(-i))))
        self.names[name] = k
        self.zones.append(z)
        self.members.append(members(rows))
        self.targets.append(np.asarray(target, F))
        return k

    def done(self):
        for _ in range(3):
            self.pos.append(np.zeros(2, F))
        self.pos = np.array(self.pos, F).reshape(-1, 2)
        self.targets = np.array(self.targets, F).reshape(-1, 2)
        self.map = abm.BuildMap(self.w, self.h, self.blockers, self.cost)
        return self


def crowd(W, r, c, n, spread=3, seed=1):
    """n member positions around tile (r, c)"""
    rng = np.random.RandomState(seed)
    return [W.p(r + int(rng.randint(-spread, spread + 1)), c + int(rng.randint(-spread, spread + 1)), rng.uniform(-1.9, 1.9, 2)) for _ in range(n)]


def line(r0, c0, r1, c1):
    return [(r, c) for r in range(r0, r1 + 1) for c in range(c0, c1 + 1)]


def open_world():
    """Open ground: the centre on a tile centre (ties everywhere), off it (none), axis (0, 1), a negative-band axis,
    budgets 24 and 25 members (the list ends first / the target is reached first), total_members 4."""
    W = World(2, 2)
    W.add("tile_centre", W.p(40, 40), crowd(W, 60, 40, 12))
    W.add("off_centre", W.p(40, 90, (0.7, -1.3)), crowd(W, 30, 110, 12, seed=2))
    sym = [W.p(90, 38), W.p(90, 42), W.p(88, 40), W.p(92, 40)]                # centroid == target
    W.add("axis_zero", W.p(90, 40), sym)
    W.add("diagonal", W.p(90, 90, (0.3, 0.9)), crowd(W, 70, 75, 60, seed=3), ur=1.0)
    W.add("big_units", W.p(20, 20), crowd(W, 25, 30, 5, seed=4), ur=6.0)       # spacing 11.1: the thinning skips tiles
    W.add("list_ends", W.p(100, 20), crowd(W, 110, 20, 30, seed=5), ur=0.5, total=400)
    W.add("four", W.p(20, 100), crowd(W, 24, 100, 4, seed=6))
    W.add("exact_spacing", W.p(60, 100), crowd(W, 70, 100, 8, seed=7), ur=EXACT_UR)
    return W.done()


def walls_world():
    """A target inside a blocked block (snapped centre), a wall through the disc (a push below the last pop), a thin wall
    the flood wraps (the clear-line filter drops slots), a pocket smaller than the budget, blockers against impassable cost."""
    W = World(2, 2, layers=(0, 1))
    W.block(line(19, 19, 21, 21))
    W.add("blocked_target", W.p(20, 20, (0.4, 0.2)), crowd(W, 30, 20, 8))
    W.wall(line(22, 80, 22, 88))
    W.add("wall_in_disc", W.p(20, 84), crowd(W, 40, 84, 10, seed=2))
    W.block(line(60, 14, 60, 27))                                             # one tile thin, the target right below it
    W.add("thin_wall", W.p(61, 20), crowd(W, 75, 20, 40, seed=3), ur=1.0)
    box = line(98, 98, 106, 106)
    W.wall([t for t in box if t[0] in (98, 106) or t[1] in (98, 106)])
    W.add("pocket", W.p(102, 102), crowd(W, 102, 102, 30, spread=2, seed=4), total=60)
    W.wall(line(60, 90, 60, 96))
    W.block(line(64, 90, 64, 96), layer=1)
    W.block(line(62, 88, 62, 98), layer=0)                                    # (the other layer's blockers must not count)
    W.add("layer_1", W.p(62, 93), crowd(W, 70, 93, 10, seed=5), layer=1)
    return W.done()


def edges_world():
    """Zones in the map's corner, at its edge, across a chunk seam and the four-chunk corner."""
    W = World(2, 2)
    W.add("corner", W.p(1, 1), crowd(W, 8, 8, 10, spread=2))
    W.add("far_corner", W.p(127, 127, (1.9, 1.9)), crowd(W, 120, 120, 10, spread=2, seed=2))
    W.add("edge", W.p(0, 64), crowd(W, 10, 60, 16, seed=3))
    W.add("seam", W.p(30, 63, (-2.0, 0.0)), crowd(W, 30, 80, 12, seed=4))
    W.add("four_chunks", W.p(64, 64, (2.0, -2.0)), crowd(W, 80, 64, 20, seed=5), ur=2.0)
    return W.done()


def cap_world():
    """The 4 096-tile budget with four members: unit_radius 64 gives radius 37 and an area above the cap."""
    W = World(2, 2)
    W.block(line(60, 70, 75, 70))
    W.add("cap", W.p(64, 64), crowd(W, 80, 64, 4), ur=64.0)
    return W.done()


def box(W, r0, c0, side, closed):
    """A walled square of side x side open tiles with its first `closed` interior tiles walled as well; its centre tile."""
    rim = line(r0 - 1, c0 - 1, r0 + side, c0 + side)
    W.wall([t for t in rim if t[0] in (r0 - 1, r0 + side) or t[1] in (c0 - 1, c0 + side)])
    W.wall([(r0, c0 + k) for k in range(closed)])
    return r0 + side // 2, c0 + side // 2


BUDGET = abm.room_needed(6, 1.0)[1]                 # 79 tiles for six members of radius 1


def budget_world():
    """Pockets of area - 1, area and area + 1 open tiles: the heap runs empty one tile short, exactly at the budget, and
    the flood stops at n == area with one tile left in the heap."""
    W = World(2, 2)
    assert BUDGET == 79
    for name, (r0, c0), closed in (("short", (10, 10), 3), ("exact", (10, 60), 2), ("one_over", (60, 10), 1)):
        r, c = box(W, r0, c0, 9, closed)
        W.add(name, W.p(r, c), crowd(W, r, c, 6, spread=2))
    return W.done()


def gate_world():
    """total_members 3 and 4, nobody within 150 wu, one member just inside; the rows the device leaves to the host."""
    W = World(2, 2, layers=(0,))
    t = W.p(64, 64)
    far = [np.array([t[0] + F(150.0), t[1]], F), np.array([t[0], t[1] - F(200.0)], F), W.p(10, 10), W.p(120, 10)]
    W.add("ok_0", t, crowd(W, 70, 64, 6))
    W.add("total_3", t, crowd(W, 70, 64, 6, seed=2), total=3)
    W.add("total_4", t, crowd(W, 70, 64, 6, seed=3), total=4)
    W.add("nobody_near", t, far)
    W.add("one_near", t, far[:3] + [np.array([t[0] + np.nextafter(F(150.0), F(0)), t[1]], F)])
    W.add("no_members", t, [], total=8)
    W.add("host_layer", t, crowd(W, 70, 64, 6, seed=4), layer=2)
    W.add("host_phase", t, crowd(W, 70, 64, 6, seed=5), phase=abm.FILLING)
    W.add("host_uid", t, crowd(W, 70, 64, 6, seed=6))
    W.add("host_room_keys", t, crowd(W, 70, 64, 6, seed=7), room=(6, abm.room_needed(6, 1.0)[1] - 1))
    W.add("host_room_slots", t, crowd(W, 70, 64, 6, seed=8), room=(5, abm.room_needed(6, 1.0)[1]))
    W.add("host_target_off", np.array([W.w * 128.0 + 1.0, 0.0], F), [np.array([W.w * 128.0 - 1.0, 0.0], F)] * 4)
    W.add("nan_target", np.array([np.nan, 0.0], F), crowd(W, 70, 64, 6, seed=9))
    W.add("host_radius", t, crowd(W, 70, 64, 6, seed=10), ur=-1.0)
    W.add("ok_1", W.p(30, 30), crowd(W, 36, 30, 6, seed=11))
    W.done()
    W.members[W.names["host_uid"]]["uid"][1] = len(W.pos)
    return W


def window_world():
    """3 x 1 chunks: a corridor one tile wide leads the flood 130 tiles east of the centre -- beyond the window."""
    W = World(3, 1)
    W.wall(line(9, 0, 9, 140) + line(11, 0, 11, 140) + [(10, 141)])
    W.add("window", W.p(10, 5), crowd(W, 10, 8, 6, spread=0), ur=5.0, total=60)
    W.add("ok", W.p(40, 100), crowd(W, 46, 100, 6))
    return W.done()


def batch_world(count=50):
    """Mixed zones side by side: sizes, layers, WAIT and HOST rows between them."""
    W = World(2, 2)
    rng = np.random.RandomState(9)
    W.block([(int(r), int(c)) for r, c in rng.randint(0, 128, (500, 2))])
    for k in range(count):
        r, c = int(rng.randint(4, 124)), int(rng.randint(4, 124))
        n = int(rng.randint(4, 30))
        kw = {}
        if k % 9 == 4:
            kw["total"] = 3
        if k % 11 == 6:
            kw["phase"] = abm.FILLING
        W.add("z%d" % k, W.p(r, c, rng.uniform(-1.9, 1.9, 2)), crowd(W, min(r + 6, 126), c, n, seed=100 + k),
              ur=float(rng.choice([0.5, 1.0, 2.5, 4.0])), **kw)
    return W.done()


WORLDS = {"open": open_world, "walls": walls_world, "edges": edges_world, "cap": cap_world, "gate": gate_world,
          "window": window_world, "batch_50": batch_world, "budget": budget_world}
_BUILT = {}


def world(name):
    """The world and the model's answer for it, computed once and left unchanged."""
    if name not in _BUILT:
        W = WORLDS[name]()
        _BUILT[name] = (W, abm.build_zones(W.map, W.zones, W.pos, W.members, W.targets))
    return _BUILT[name]


def premises(name, W, want):
    """What every world is there to show, asserted from the model alone."""
    n = W.names
    st = {k: want[i]["status"] for k, i in n.items()}
    part = lambda k: want[n[k]]["parts"]                                    # noqa: E731
    for k, s in st.items():
        expect = abm.AB_HOST if (k.startswith("host_") or k == "window") else abm.AB_WAIT if k in ("total_3", "nobody_near", "no_members", "nan_target") else None
        if expect is not None:
            assert s == expect, (name, k, s)
        elif name != "batch_50":
            assert s == 0, (name, k, s)
    for i, res in enumerate(want):                                          # inside the window and the heap
        if res["status"] == 0:
            # No two slots of a zone tie in slot_cmp_far_banded.  Kept slots lie at least `spacing` apart, and the band
            # width IS the spacing: two slots of equal lateral key differ along the axis alone, by at least one band width,
            # so their bands differ.  The stable tie-break of that sort can therefore decide nothing on a built zone; it
            # is held against libc's qsort on hand-made lists (tests/test_arrival_build_cpu.py).
            z = res["zone"]
            band, lat = abm.band_keys(z["slots_xz"], z["centre_xz"], res["axis"], z["row_height"])
            assert len(set(zip(band.tolist(), lat.tolist()))) == len(band), (name, i)
            stats = {}
            c = res["zone"]["centre_xz"]
            abm.connected_tiles(W.map, W.zones[i]["arg_layer"], c[0], c[1], res["parts"]["area"], stats=stats)
            assert stats["reach"] <= abm.WINDOW_R and stats["peak"] <= abm.HEAP_NODES
    if name == "open":
        def prios(k):                                                       # the flood's priorities
            c = want[n[k]]["zone"]["centre_xz"]
            return abm.near_ref_keys(part(k)["flood"], c)
        assert len(prios("tile_centre")) - len(np.unique(prios("tile_centre"))) > 50
        assert len(np.unique(prios("off_centre"))) == len(prios("off_centre"))
        dd = part("axis_zero")["near_keys"]                                  # ties of the near-reference sort: flood order decides
        assert len(dd) - len(np.unique(dd)) > 20
        assert want[n["axis_zero"]]["axis"].tolist() == [0.0, 1.0]
        band, _ = abm.band_keys(want[n["diagonal"]]["zone"]["slots_xz"], want[n["diagonal"]]["zone"]["centre_xz"], want[n["diagonal"]]["axis"], F(1.85))
        assert band.min() < 0 <= band.max() and (np.diff(band) <= 0).all()
        assert len(part("big_units")["thinned"]) == 5 and len(part("big_units")["flood"]) > 50
        assert len(part("list_ends")["thinned"]) == 400 < len(part("list_ends")["flood"])   # the target is reached first
        assert len(part("four")["thinned"]) == 4
        t = part("exact_spacing")["thinned"]
        assert F(F(1.85) * EXACT_UR) == F(12) and any(F(F(a[0] - b[0]) ** 2 + F(a[1] - b[1]) ** 2) == F(144) for a in t for b in t)
    if name == "walls":
        z = want[n["blocked_target"]]["zone"]
        assert not np.array_equal(z["centre_xz"], W.targets[n["blocked_target"]])
        t = part("wall_in_disc")["tiles"]
        c = want[n["wall_in_disc"]]["zone"]["centre_xz"]
        d = [float((W.map.centre_of(*x)[0] - c[0]) ** 2 + (W.map.centre_of(*x)[1] - c[1]) ** 2) for x in t]
        assert len(t) == part("wall_in_disc")["area"]
        assert not part("thin_wall")["clear"].all() and part("thin_wall")["clear"].any()
        assert len(part("pocket")["thinned"]) == len(part("pocket")["tiles"]) == 49 < 60 < part("pocket")["area"]    # the list ends first
        assert d != sorted(d)                                               # a push below the last pop: around the wall
        r = want[n["thin_wall"]]                                            # the filter empties whole bands
        bt, _ = abm.band_keys(part("thin_wall")["thinned"], r["zone"]["centre_xz"], r["axis"], r["zone"]["row_height"])
        bk, _ = abm.band_keys(part("thin_wall")["kept"], r["zone"]["centre_xz"], r["axis"], r["zone"]["row_height"])
        assert len(set(bt.tolist()) - set(bk.tolist())) >= 2 and len(bk) > 5
        # layer 1: its flood crosses layer 0's blockers and stops at its own blockers and at the cost wall, all inside the disc
        r = want[n["layer_1"]]
        tiles, c = set(part("layer_1")["tiles"]), r["zone"]["centre_xz"]
        dist = lambda t: float((W.map.centre_of(*t)[0] - c[0]) ** 2 + (W.map.centre_of(*t)[1] - c[1]) ** 2)      # noqa: E731
        far = max(dist(t) for t in tiles)
        wall, own, other = line(60, 90, 60, 96), line(64, 90, 64, 96), line(62, 88, 62, 98)
        assert r["zone"]["layer"] == 1 and not tiles & set(wall) and not tiles & set(own) and len(tiles & set(other)) > 5
        assert all(dist(t) < far for t in wall + own) and any(t[0] > 64 for t in tiles) and any(t[0] < 60 for t in tiles)
    if name == "budget":
        for k, count, left in (("short", BUDGET - 1, 0), ("exact", BUDGET, 0), ("one_over", BUDGET, 1)):
            stats = {}
            c = want[n[k]]["zone"]["centre_xz"]
            abm.connected_tiles(W.map, 0, c[0], c[1], BUDGET, stats=stats)
            assert part(k)["area"] == BUDGET and len(part(k)["tiles"]) == count and stats["left"] == left, (k, stats)
    if name == "edges":
        assert len({int(k) >> 32 for k in want[n["four_chunks"]]["keys"]}) == 4 and len({int(k) >> 32 for k in want[n["seam"]]["keys"]}) == 2
    if name == "cap":
        assert len(want[0]["keys"]) == 4096 and want[0]["zone"]["radius"] >= 37 and len(want[0]["zone"]["slots_xz"]) <= 4
    if name == "gate":
        assert st["one_near"] == 0 and st["total_4"] == 0
    if name == "batch_50":
        vals = [r["status"] for r in want]
        assert len(vals) == 50 and vals.count(abm.AB_WAIT) >= 3 and vals.count(abm.AB_HOST) >= 3 and vals.count(0) >= 30
