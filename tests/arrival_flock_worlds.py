"""The worlds of the arrival flock-update tests (tests/test_arrival_flock_cpu.py, _gpu.py): zones on open maps of at most
4 x 4 chunks, as the dicts tests/arrival_flock_model.py takes.  A world: w, h, blockers {layer: [h][w][64][64] u16}, zones,
keys (per zone the sorted u64 td_keys), members (per zone the member rows), pos [n][2].  Every builder returns plain data;
nothing here calls the device or the reference."""
import numpy as np

from tests import arrival_flock_model as afm

F = np.float32
FILLING = afm.FILLING


def xz(w, h, r, c, off=(0.0, 0.0)):
    """A point of the absolute tile (r, c): its centre moved by `off`."""
    return np.array([F(w * 128.0) - F(4 * c + 2) + F(off[0]), F(-h * 128.0) + F(4 * r + 2) + F(off[1])], F)


def rect(r0, c0, nr, nc):
    return [(r0 + i, c0 + j) for i in range(nr) for j in range(nc)]


def keys_of(tiles):
    """td_key (nav.c:207) of absolute tiles, ascending, each once"""
    return np.array(sorted({afm.key_of((r >> 6, c >> 6, r & 63, c & 63)) for r, c in tiles}), np.uint64)


def zone(w, h, tiles, slots_xz, fill=0.0, rings=None, active_row=0, num_rows=1, counter=3, stall=0, prev_occ=0, row_height=4.0,
         layer=0, ur=1.0, total=None, phase=FILLING, centre=None, old_layer=None, old_radius=9, old_ur=0.75):
    slots = np.asarray(slots_xz, F).reshape(-1, 2)
    tiles = list(tiles)
    if centre is None:
        centre = xz(w, h, *tiles[len(tiles) // 2]) if tiles else np.zeros(2, F)
    return {"layer": layer if old_layer is None else old_layer, "centre_xz": np.asarray(centre, F), "radius": old_radius,
            "unit_radius": F(old_ur), "fill_frac": F(fill), "active_row": active_row, "num_rows": num_rows, "slots_xz": slots,
            "slot_ring": np.zeros(len(slots), np.int32) if rings is None else np.asarray(rings, np.int32),
            "phase": phase, "realloc_counter": counter, "stall_counter": stall, "prev_occ": prev_occ, "row_height": F(row_height),
            "arg_layer": layer, "arg_unit_radius": F(ur), "arg_total_members": len(slots) if total is None else total,
            "tiles": tiles}


def members(rows):
    """rows: (uid, settled, substate, sink_valid, sink (x, z))"""
    n = len(rows)
    return {"uid": np.array([r[0] for r in rows], np.int32).reshape(n), "settled": np.array([r[1] for r in rows], np.uint8).reshape(n),
            "substate": np.array([r[2] for r in rows], np.uint8).reshape(n), "sink_valid": np.array([r[3] for r in rows], np.uint8).reshape(n),
            "sink_xz": np.array([r[4] for r in rows], F).reshape(n, 2)}


class World:
    def __init__(self, w, h, layers=(0,)):
        self.w, self.h = w, h
        self.blockers = {l: np.zeros((h, w, 64, 64), np.uint16) for l in layers}
        self.zones, self.members, self.pos = [], [], []

    def block(self, tiles, layer=0, count=1):
        for r, c in tiles:
            self.blockers[layer][r >> 6, c >> 6, r & 63, c & 63] = count

    def unit(self, p):
        self.pos.append(np.asarray(p, F))
        return len(self.pos) - 1

    def add(self, z, rows):
        """rows: (position, settled, substate, sink_valid, sink) -- the units are appended to the world"""
        self.zones.append(z)
        self.members.append(members([(self.unit(r[0]),) + tuple(r[1:]) for r in rows]))
        return len(self.zones) - 1

    def done(self, extra_units=3):
        for _ in range(extra_units):
            self.unit((0.0, 0.0))
        self.pos = np.array(self.pos, F).reshape(-1, 2)
        self.keys = [keys_of(z["tiles"]) for z in self.zones]
        self.map = afm.Map(self.w, self.h, self.blockers)
        return self


def crowd(W, rng, tiles, n, slots, p_settled=0.3, spread=1.9, outside=0.2):
    """n member rows in and around `tiles`: every substate, some settled (on or near a slot), some outside the footprint."""
    rows = []
    lo_r, lo_c = min(t[0] for t in tiles), min(t[1] for t in tiles)
    for i in range(n):
        r, c = tiles[rng.randint(len(tiles))]
        p = xz(W.w, W.h, r, c, rng.uniform(-spread, spread, 2))
        if rng.rand() < outside:
            p = xz(W.w, W.h, max(lo_r - 3, 0), max(lo_c - 2, 0), rng.uniform(-1.9, 1.9, 2))
        settled = rng.rand() < p_settled
        if settled and len(slots):
            p = (slots[rng.randint(len(slots))] + rng.uniform(-1.0, 1.0, 2)).astype(F)
        sink = slots[rng.randint(len(slots))] if len(slots) else np.zeros(2, F)
        rows.append((p, int(settled), i % 4, int(rng.rand() < 0.6), sink))
    return rows


# ---------------------------------------------------------------------------------------------
# slot counts; M == 0, num_rows == 0; blockers on two layers
# ---------------------------------------------------------------------------------------------
SLOT_COUNTS = (1, 63, 64, 65, 257)


def shapes_world():
    """Re-orienting zones of 1, 63, 64, 65 and 257 slots (a lane without a slot, one stride of the wave, one more, several),
    a zone without slots, a zone whose num_rows is 0, and a zone on layer 1 with blockers of its own; every fourth call."""
    W = World(2, 2, layers=(0, 1))
    rng = np.random.RandomState(41)
    spots = [(4, 4), (4, 40), (4, 70), (40, 4), (40, 40), (80, 4), (80, 40), (100, 90)]
    specs = list(SLOT_COUNTS) + [0, 5, 40]
    for k, (n, (r0, c0)) in enumerate(zip(specs, spots)):
        side = int(np.ceil(np.sqrt(max(n, 4)))) + 2
        tiles = rect(r0, c0, side, side)
        slots = np.array([xz(2, 2, r, c, rng.uniform(-1.5, 1.5, 2)) for r, c in tiles[:n]], F).reshape(-1, 2)
        layer = 1 if k == 7 else 0
        z = zone(2, 2, tiles, slots, row_height=F(1.85 * 2.5), ur=2.5, layer=layer, old_layer=0,
                 num_rows=0 if k == 6 else 1, total=n + 3)
        W.block([tiles[i] for i in range(0, n, 7)], layer)
        if k == 7:
            W.block([tiles[i] for i in range(1, n, 5)], 0)                    # (the other layer's blockers must not count)
        W.add(z, crowd(W, rng, tiles, 12 + n // 4, slots))
    return W.done()


def cap_world():
    """One zone at the cap: 4 096 keys (a 64 x 64 square across the corner where the four chunks of the map meet), 4 096
    slots, three members."""
    W = World(2, 2)
    tiles = rect(32, 32, 64, 64)
    rng = np.random.RandomState(5)
    slots = np.array([xz(2, 2, r, c) for r, c in tiles], F) + rng.uniform(-1.0, 1.0, (4096, 2)).astype(F)
    z = zone(2, 2, tiles, slots, row_height=F(8.0), total=4096)
    W.add(z, [(xz(2, 2, 33, 34, (0.5, 0.25)), 0, 0, 0, (0, 0)), (xz(2, 2, 90, 60), 1, 2, 1, slots[7]), (xz(2, 2, 36, 33), 0, 1, 1, slots[9])])
    return W.done()


# ---------------------------------------------------------------------------------------------
# footprints
# ---------------------------------------------------------------------------------------------
def footprints_world():
    """Across a chunk corner, against the map's edge, in its corner, C-shaped around a wall, with a hole, in two
    disconnected parts, with slots off the region and off the map.  4 x 4 chunks."""
    W = World(4, 4)
    rng = np.random.RandomState(77)
    w = h = 4

    def put(tiles, slot_tiles, entry_tile, extra_slots=(), n=10, **kw):
        slots = [xz(w, h, r, c, rng.uniform(-1.2, 1.2, 2)) for r, c in slot_tiles] + [np.asarray(s, F) for s in extra_slots]
        slots = np.array(slots, F).reshape(-1, 2)
        rows = crowd(W, rng, tiles, n, slots, p_settled=0.25, outside=0.1)
        rows.append((xz(w, h, *entry_tile), 0, 0, 0, (0, 0)))                # pulls the entry to its side
        return W.add(zone(w, h, tiles, slots, **kw), rows)

    corner = rect(60, 124, 9, 9)                                             # chunks (0,1) (0,2) (1,1) (1,2)
    W.names = {}
    W.names["chunk_corner"] = put(corner, corner[::2], (60, 124))
    edge = rect(0, 100, 6, 12)                                               # row 0 is the map's edge
    W.names["edge"] = put(edge, edge[::3], (5, 111))
    mcorner = rect(250, 250, 6, 6)                                           # the map's far corner
    W.names["corner"] = put(mcorner, mcorner[::2], (250, 250))
    # a C around a wall: rows 150..156, the wall is row 153 from column 20 to 29; the bend at columns 30..31
    c_tiles = [t for t in rect(150, 20, 7, 12) if not (t[0] == 153 and t[1] < 30)]
    W.names["c_shape"] = put(c_tiles, [t for t in c_tiles if t[1] < 30][::2], (150, 20), row_height=F(4.0))
    holed = [t for t in rect(200, 40, 9, 9) if not (203 <= t[0] <= 205 and 43 <= t[1] <= 45)]
    W.names["hole"] = put(holed, holed[::2], (200, 40), row_height=F(6.0))
    two = rect(100, 200, 5, 5) + rect(100, 210, 5, 5)                        # columns 205..209 are missing
    W.names["two_parts"] = put(two, two[::2], (100, 200))
    off = rect(30, 30, 6, 6)
    W.names["off_region"] = put(off, off[::2], (30, 30), extra_slots=[xz(w, h, 40, 40), (600.0, 0.0), xz(w, h, 29, 30), (0.0, -600.0)])
    return W.done()


# ---------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------
def ties_world():
    """A settled member and an unsettled one on a tile corner equidistant from four slots; an entry equidistant from two
    keys; two coincident slots."""
    W = World(2, 2)
    tiles = rect(20, 20, 4, 4)
    four = np.array([xz(2, 2, 20, 20), xz(2, 2, 20, 21), xz(2, 2, 21, 20), xz(2, 2, 21, 21)], F)
    corner = (four[0] + four[3]) * F(0.5)                                    # the corner the four tiles share
    z = zone(2, 2, tiles, np.concatenate([four, [xz(2, 2, 23, 23)]]), fill=0.5)          # (frozen: one ring, every slot behind the frontier)
    W.names = {"four": W.add(z, [(corner, 1, 2, 1, four[2]), (corner, 0, 0, 0, (0, 0)), (corner, 0, 3, 1, four[1])])}
    # the entry on the border between tiles (40, 40) and (40, 41): both centres 2.0 away
    pair = rect(40, 40, 1, 6)
    mid = (xz(2, 2, 40, 40) + xz(2, 2, 40, 41)) * F(0.5)
    z = zone(2, 2, pair, [xz(2, 2, 40, c) for c in range(40, 46)], row_height=F(4.0))
    W.names["entry"] = W.add(z, [(mid, 0, 0, 0, (0, 0))])
    twin = rect(60, 60, 3, 3)
    s = xz(2, 2, 61, 61, (0.5, 0.5))
    z = zone(2, 2, twin, [xz(2, 2, 60, 60), s, s, xz(2, 2, 62, 62)], fill=0.5)
    W.names["coincident"] = W.add(z, [(s + F(0.25), 1, 2, 1, s), (s - F(0.25), 0, 0, 0, (0, 0)), (s, 1, 3, 1, s)])
    return W.done()


# ---------------------------------------------------------------------------------------------
# frozen zones: the frontier, fill fractions, the realloc period, the all-settled arm
# ---------------------------------------------------------------------------------------------
def row_zone(W, r0, c0, per_row, settled_per_row, unsettled, outside=0, **kw):
    """A frozen zone of len(per_row) rows of slots (row k = ring k, one tile row each) on a footprint three columns wider;
    settled_per_row[k] members sit on the first slots of row k; `unsettled` members stand in the footprint's spare columns."""
    nrow, width = len(per_row), max(per_row) + 3
    tiles = rect(r0, c0, nrow, width)
    slots, rings, rows = [], [], []
    for k, n in enumerate(per_row):
        for j in range(n):
            slots.append(xz(W.w, W.h, r0 + k, c0 + j))
            rings.append(k)
    slots = np.array(slots, F).reshape(-1, 2)
    at = 0
    for k, n in enumerate(per_row):
        for j in range(settled_per_row[k]):
            rows.append((slots[at + j] + F(0.25), 1, 2, 1, slots[at + j]))
        at += n
    for j in range(unsettled):
        rows.append((xz(W.w, W.h, r0 + j % nrow, c0 + width - 1 - (j // nrow) % 2, (0.5, -0.5)), 0, j % 4, j % 2, slots[0]))
    for j in range(outside):                                                 # unsettled, off the footprint
        rows.append((xz(W.w, W.h, r0 + j % nrow, c0 + width + 2), 0, j % 4, 1, slots[0]))
    kw.setdefault("fill", 0.5)
    kw.setdefault("num_rows", nrow)
    return W.add(zone(W.w, W.h, tiles, slots, rings=rings, **kw), rows)


def frontier_world():
    """Frozen zones (fill_frac >= 0.25), every one at its fourth call."""
    W = World(2, 2, layers=(0, 1))
    n = W.names = {}
    n["exact_cap"] = row_zone(W, 4, 4, (4, 4, 4), (4, 1, 0), 3)                      # row 0 exactly full: one step
    n["three_rows"] = row_zone(W, 10, 4, (3, 2, 2, 4), (3, 2, 2, 0), 2)              # three rows advance in one call
    n["stall_18"] = row_zone(W, 16, 4, (4, 4), (2, 0), 2, stall=18, prev_occ=2)      # flat: 18 -> 19
    n["stall_19"] = row_zone(W, 20, 4, (4, 4), (2, 0), 2, stall=19, prev_occ=2)      # ... 19 -> forced advance
    n["last_row"] = row_zone(W, 24, 4, (2, 3), (2, 3), 2, active_row=1, stall=19, prev_occ=3)    # full and stalled: stays
    n["crowd_0"] = row_zone(W, 28, 4, (4, 4), (2, 0), 0, outside=2, stall=7, prev_occ=2)   # nobody unsettled inside: reset
    n["rising"] = row_zone(W, 32, 4, (4, 4), (3, 0), 2, stall=5, prev_occ=2)         # occ 3 > prev_occ 2: reset
    n["not_rising"] = row_zone(W, 36, 4, (4, 4), (3, 0), 2, stall=5, prev_occ=3)     # flat: 5 -> 6
    # fill fractions either side of 0.25 in the INPUT (what decides the re-orientation); the frozen ones keep their rings
    n["fill_above"] = row_zone(W, 44, 4, (4, 4), (3, 0), 2, fill=np.nextafter(F(0.25), F(1)))
    n["fill_exact"] = row_zone(W, 48, 4, (4, 4), (3, 0), 2, fill=0.25)
    # blockers under slots: layer 0 for one zone, layer 1 for another (whose layer-0 blockers must not count)
    n["blocked_l0"] = row_zone(W, 56, 4, (4, 4), (1, 0), 3)
    W.block([(56, 5), (56, 6), (56, 7), (57, 4)], 0, 2)
    n["blocked_l1"] = row_zone(W, 60, 4, (4, 4), (1, 0), 3, layer=1, old_layer=0)
    W.block([(60, 5), (61, 4)], 1)
    W.block([(60, 6), (60, 7)], 0)
    return W.done()


def period_world():
    """realloc_counter 0..3 on copies of one frozen zone (only the fourth call reallocs), and the all-settled arm with
    0, 1 and 300 members of which none, some or all are settled."""
    W = World(2, 2)
    n = W.names = {}
    for c in range(4):
        n["counter_%d" % c] = row_zone(W, 4 + 4 * c, 4, (4, 4), (4, 0), 3, counter=c)
    rng = np.random.RandomState(3)
    tiles = rect(40, 40, 20, 20)
    slots = np.array([xz(2, 2, r, c) for r, c in tiles[::2]], F)
    rings = (np.arange(len(slots)) // 40).astype(np.int32)
    for name, count, p in (("none_of_0", 0, 0.0), ("settled_1", 1, 1.0), ("unsettled_1", 1, 0.0), ("none_of_300", 300, 0.0),
                           ("some_of_300", 300, 0.5), ("all_of_300", 300, 1.0)):
        rows = crowd(W, rng, tiles, count, slots, p_settled=p, outside=0.1)
        n[name] = W.add(zone(2, 2, tiles, slots, fill=0.5, rings=rings, num_rows=int(rings.max()) + 1, active_row=1, ur=1.5), rows)
    return W.done()


def fill_below_world():
    """The row zone of fill_exact with fill_frac one ulp below 0.25: it re-orients (rings recomputed, active_row 0)."""
    W = World(2, 2)
    W.names = {"fill_below": row_zone(W, 44, 4, (4, 4), (3, 0), 2, fill=np.nextafter(F(0.25), F(0)), active_row=1),
               "fill_exact": row_zone(W, 48, 4, (4, 4), (3, 0), 2, fill=0.25, active_row=1)}
    return W.done()


# ---------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------
def batch_world(n_zones, seed=0):
    """n_zones zones in a 4 x 4 map, re-orienting and frozen, at every realloc_counter; zones without members in front, in the
    middle and at the end (they take the all-settled arm)."""
    W = World(4, 4)
    rng = np.random.RandomState(100 + n_zones + seed)
    empty = {0, n_zones // 2, n_zones - 1} if n_zones >= 3 else set()
    for k in range(n_zones):
        r0, c0 = 4 + 24 * (k // 10), 4 + 24 * (k % 10)
        side = 4 + k % 5
        tiles = rect(r0, c0, side, side + 2)
        slots = np.array([xz(4, 4, r, c, rng.uniform(-1, 1, 2)) for r, c in tiles[::2]], F)
        frozen = k % 3 == 1
        nrows = 3
        rings = rng.randint(0, nrows, len(slots)) if frozen else None
        z = zone(4, 4, tiles, slots, fill=0.4 if frozen else 0.1, rings=rings, num_rows=nrows if frozen else 1,
                 active_row=k % 2 if frozen else 0, counter=3 if k % 4 else k % 3, row_height=F(4.0 + k % 3), ur=1.0 + 0.5 * (k % 4))
        W.block([tiles[1]], 0)
        W.add(z, [] if k in empty else crowd(W, rng, tiles, 6 + k % 7, slots))
    return W.done()


# ---------------------------------------------------------------------------------------------
# a chain: members moving and settling by script between calls
# ---------------------------------------------------------------------------------------------
def chain_world():
    """Two zones followed over twelve calls: one starts re-orienting and freezes as it fills, one is frozen."""
    W = World(2, 2)
    rng = np.random.RandomState(9)
    tiles = rect(30, 30, 8, 8)
    slots = np.array([xz(2, 2, r, c) for r, c in tiles[::4]], F)
    rows = [(xz(2, 2, 30 + i % 8, 30 + (i * 3) % 8, rng.uniform(-1.5, 1.5, 2)), 0, i % 2, 0, (0, 0)) for i in range(28)]
    rows += [(xz(2, 2, 24, 30 + i, rng.uniform(-1.5, 1.5, 2)), 0, 0, 0, (0, 0)) for i in range(4)]      # outside, walking in
    W.add(zone(2, 2, tiles, slots, row_height=F(32.0), counter=3, total=32), rows)
    row_zone(W, 60, 60, (4, 4, 4), (4, 0, 0), 8, counter=2)
    return W.done()


def chain_step(W, zones_after, mem_after, call, speed=8.0):
    """The script between two calls of a chain: an unsettled member with a sink walks `speed` towards it and settles within
    1.0 of it; one without walks towards the zone's centre.  Returns the next call's (zones, members); W.pos is moved."""
    zones, mems = [], []
    for zi, (z0, za, m0, ma) in enumerate(zip(W.zones, zones_after, W.members, mem_after)):
        z = dict(z0, **{k: za[k] for k in afm.ZONE_OUT}, slot_ring=np.array(za["slot_ring"], np.int32))
        mem = dict(m0, **{k: np.array(ma[k]) for k in afm.MEMBER_OUT})
        mem["settled"] = np.array(m0["settled"])
        for j, uid in enumerate(m0["uid"]):
            if mem["settled"][j]:
                continue
            goal = mem["sink_xz"][j] if mem["sink_valid"][j] else z0["centre_xz"]
            d = (goal - W.pos[uid]).astype(F)
            dist = F(np.hypot(d[0], d[1]))
            if dist <= F(1.0) and mem["sink_valid"][j]:
                mem["settled"][j] = 1
            elif dist > 0:
                W.pos[uid] = (W.pos[uid] + d * F(min(1.0, speed / float(dist)))).astype(F)
        zones.append(z)
        mems.append(mem)
    W.zones, W.members = zones, mems
    return zones, mems
