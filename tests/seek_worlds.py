"""Small worlds for the enemy-seek / surround seed pass (navhip_build_seek_fields): a map, its planes, a snapshot of entities,
the game-side arrays and a list of requests.  Each world says what it is for; tests/test_seek_fields_cpu.py asserts those
premises from tests/seek_seed_model.py.  Test infrastructure only.

A world is a dict: w, h, layers (mask of the layers with planes), cost ([h*64, w*64] u8, every layer's cost_base), blockers
([h*64, w*64] u16, every layer's), pos [n, 2] f32, radius [n] f32, flags [n] u32, faction [n] i32, exclude [n] u8 or None,
enemy_mask [16] u16, reqs (SEEK_REQ_DTYPE) and, for the hand-placed world, `cases`: name -> what the CPU test looks at."""
import functools

import numpy as np

from permafrost_engine_amd import synth
from tests import seek_seed_model as ssm
from tests import surround_model as sm

F = np.float32
MOVABLE = 1 << 3
SEEK_REQ_DTYPE = np.dtype([("kind", np.uint8), ("layer", np.uint8), ("chunk_r", np.int16), ("chunk_c", np.int16),
                           ("faction_id", np.int16), ("target_uid", np.int32)])
RANDOM = ((4, 4, 0x1, 41), (3, 2, 0xf, 42), (2, 2, 0x3, 43))      # (w, h, layers, seed): the three random worlds


def _req(kind, layer, cr, cc, faction=0, target=0):
    return (kind, layer, cr, cc, faction, target)


@functools.lru_cache(maxsize=None)
def random_world(w, h, layers, seed):
    """About 300 entities of 3 factions with asymmetric enemy masks (0 fights 1 and 2, 1 fights 0, 2 fights 1), radii from
    {1, 2.5, 4, 9, 20}, a tenth not combatable, some garrisoned, some excluded; 120 of them stand on blockers, so seeds are
    mostly not passable; 60 kind-0 and 40 kind-1 requests over every layer of the map, every edge and corner chunk among
    them (base with and without the half-chunk offset), some twice."""
    rng = np.random.RandomState(seed)
    grid = synth.cost_grid(w, h, seed=seed, frac_impassable=0.20)
    n = 300
    inner = np.zeros(grid.shape, bool)
    inner[2:-2, 2:-2] = True
    cells = np.argwhere((grid != 255) & inner)
    pick = cells[rng.choice(len(cells), size=n, replace=False)]
    pos = (synth.cell_centre(w, h, pick[:, 0], pick[:, 1]) + rng.uniform(-1.9, 1.9, (n, 2))).astype(F)
    radius = rng.choice([1.0, 2.5, 4.0, 9.0, 20.0], size=n, p=[0.4, 0.25, 0.2, 0.1, 0.05]).astype(F)
    faction = rng.randint(0, 3, n).astype(np.int32)
    flags = np.full(n, MOVABLE | ssm.COMBATABLE, np.uint32)
    flags[rng.rand(n) < 0.1] &= ~np.uint32(ssm.COMBATABLE)
    flags[rng.rand(n) < 0.05] |= np.uint32(ssm.GARRISONED)
    exclude = (rng.rand(n) < 0.05).astype(np.uint8)
    blockers = np.zeros(grid.shape, np.uint16)
    for i in rng.choice(n, 120, replace=False):
        blockers[pick[i, 0], pick[i, 1]] += 1
    masks = np.zeros(16, np.uint16)
    masks[:3] = (0b110, 0b001, 0b010)
    lay = [l for l in range(12) if (layers >> l) & 1]
    chunks = [(r, c) for r in range(h) for c in range(w)]
    reqs = []
    for k in range(60):
        cr, cc = chunks[k % len(chunks)] if k < 2 * len(chunks) else chunks[rng.randint(len(chunks))]
        reqs.append(_req(0, lay[k % len(lay)], cr, cc, faction=int(rng.randint(3))))
    for k in range(40):
        t = int(rng.randint(n))
        cr, cc = pick[t, 0] // 64, pick[t, 1] // 64
        if k % 3 == 0:      # a neighbour chunk's field of the same target
            cr, cc = min(max(cr + rng.randint(-1, 2), 0), h - 1), min(max(cc + rng.randint(-1, 2), 0), w - 1)
        reqs.append(_req(1, lay[k % len(lay)], cr, cc, target=t))
    reqs += reqs[3:6] + reqs[70:72]                                   # duplicates
    return dict(name="random %dx%d" % (w, h), w=w, h=h, layers=layers, cost=grid, blockers=blockers, pos=pos, radius=radius,
                flags=flags, faction=faction, exclude=exclude, enemy_mask=masks, reqs=np.array(reqs, SEEK_REQ_DTYPE), cases={})


@functools.lru_cache(maxsize=None)
def hand_world():
    """4 x 4 chunks, layers 0xf, open ground.  Seeker faction s fights victim faction 14 - s only (15 is FACTION_ID_NONE in the planes), so every case has the
    requests of its seeker to itself.  `cases` names the entities and requests of each case."""
    w, h = 4, 4
    grid = np.ones((h * 64, w * 64), np.uint8)
    grid[90:94, 40:90] = 255
    mx, mz = sm.map_pos(w, h)
    E, R, cases = [], [], {}

    def ent(x, z, radius, faction, flags=MOVABLE | ssm.COMBATABLE):
        E.append((F(x), F(z), F(radius), faction, flags))
        return len(E) - 1

    def at(r, c):
        return sm.xz(w, h, r, c)

    def req(*a, **k):
        R.append(_req(*a, **k))
        return len(R) - 1

    # seeker 0 / victims 14, chunk (1, 1), layer 0.  Its rectangle ends at x = mx - 112 (column 28), its region at column 32.
    p = at(100, 30); a = ent(p[0], p[1], 9.0, 14)             # between the two edges, reaches into the region
    p = at(140, 27); b = ent(p[0], p[1], 20.0, 14)            # outside the rectangle, would reach in: must not seed
    edge = F(mx - F(112))
    c_on = ent(edge, at(60, 0)[1], 20.0, 14)                  # fixed-point coordinate == the bound
    c_off = ent(F(edge + F(1.0 / 256)), at(80, 0)[1], 20.0, 14)      # one unit beyond it
    c_round = ent(F(edge + F(1.0 / 1024)), at(40, 0)[1], 20.0, 14)    # beyond it in float, on it in fixed point: a member
    cases["rectangle"] = dict(req=req(0, 0, 1, 1, faction=0), a=a, b=b, on=c_on, off=c_off, round=c_round)
    # seeker 1 / victims 13, chunk (0, 0): a centre off the map; a circle the map edge clips, on each layer
    off = ent(F(mx + F(2)), at(30, 0)[1], 9.0, 13)
    p = at(1, 1); clip = ent(p[0], p[1], 9.0, 13)
    cases["map edge"] = dict(reqs=[req(0, l, 0, 0, faction=1) for l in range(4)], off=off, clip=clip)
    # kind 1: the 512 cap in the first call; in a contour; the window rule (layer 3: two contours)
    p = at(100, 100)
    big = [ent(p[0], p[1], r, 9) for r in (52.0, 44.0, 116.0, 120.0, 40.0)]
    cases["cap second contour"] = dict(req=req(1, 3, 1, 1, target=big[4]), ent=big[4])
    cases["cap first"] = dict(req=req(1, 0, 1, 1, target=big[0]), ent=big[0])
    cases["cap contour"] = dict(req=req(1, 1, 1, 1, target=big[1]), ent=big[1])
    cases["window in"] = dict(req=req(1, 3, 1, 1, target=big[2]), ent=big[2])
    cases["window out"] = dict(req=req(1, 3, 1, 1, target=big[3]), ent=big[3])
    # seeker 2 / victims 12: a building source; a building target
    p = at(170, 20); bld = ent(p[0], p[1], 4.0, 12, MOVABLE | ssm.COMBATABLE | ssm.BUILDING)
    cases["building"] = dict(source_req=req(0, 0, 2, 0, faction=2), target_req=req(1, 0, 2, 0, target=bld), ent=bld)
    # seeker 3 / victims 11: 4 096 entities 100 wu inside chunk (3, 3) and one 200 wu inside: both in the rectangle of chunk
    # (3, 3), the 4 096 alone in that of chunk (3, 2).  Three of them can be fought, the rest only count
    pa, pb = at(3 * 64 + 30, 3 * 64 + 25), at(3 * 64 + 30, 3 * 64 + 50)
    first = len(E)
    for i in range(4096):
        ent(pa[0], pa[1], 1.0, 11, MOVABLE | (ssm.COMBATABLE if i < 3 else 0) | (ssm.GARRISONED if i % 64 == 5 else 0))
    ent(pb[0], pb[1], 1.0, 11)
    cases["crowd"] = dict(over=req(0, 0, 3, 3, faction=3), at_limit=req(0, 0, 3, 2, faction=3), first=first)
    # seeker 4 fights nobody
    cases["no enemy"] = dict(req=req(0, 2, 1, 2, faction=4))
    # rows the request alone hands back: a chunk outside the map, a uid outside the snapshot, a faction outside the table, a
    # layer without planes
    cases["refused"] = dict(reqs=[req(0, 0, 4, 0, faction=0), req(0, 0, 0, -1, faction=0), req(1, 0, 1, 1, target=len(E) + 5000),
                                  req(1, 0, 1, 1, target=-1), req(0, 0, 1, 1, faction=16), req(0, 0, 1, 1, faction=-1),
                                  req(0, 5, 1, 1, faction=0)])
    masks = np.zeros(16, np.uint16)
    for s in range(4):
        masks[s] = 1 << (14 - s)
    E = np.array(E, dtype=[("x", F), ("z", F), ("radius", F), ("faction", np.int32), ("flags", np.uint32)])
    return dict(name="hand", w=w, h=h, layers=0xf, cost=grid, blockers=np.zeros(grid.shape, np.uint16),
                pos=np.stack([E["x"], E["z"]], 1).astype(F), radius=E["radius"].copy(), flags=E["flags"].copy(),
                faction=E["faction"].copy(), exclude=None, enemy_mask=masks, reqs=np.array(R, SEEK_REQ_DTYPE), cases=cases)


@functools.lru_cache(maxsize=None)
def strip_world():
    """A 1 x 3 map (one chunk high): the padded region is 64 x 128, not square -- every request is the host's."""
    w, h = 3, 1
    grid = np.ones((h * 64, w * 64), np.uint8)
    pos = np.stack([sm.xz(w, h, 30, 20 + 50 * i) for i in range(3)]).astype(F)
    masks = np.zeros(16, np.uint16)
    masks[0] = 0b10
    reqs = [_req(0, 0, 0, c, faction=0) for c in range(3)] + [_req(1, 0, 0, 1, target=1)]
    return dict(name="strip", w=w, h=h, layers=0x1, cost=grid, blockers=np.zeros(grid.shape, np.uint16), pos=pos,
                radius=np.full(3, 2.5, F), flags=np.full(3, MOVABLE | ssm.COMBATABLE, np.uint32), faction=np.array([0, 1, 1], np.int32),
                exclude=None, enemy_mask=masks, reqs=np.array(reqs, SEEK_REQ_DTYPE), cases={})


def all_worlds():
    return [random_world(*a) for a in RANDOM] + [hand_world(), strip_world()]


NAMES = ["random %dx%d" % (a[0], a[1]) for a in RANDOM] + ["hand", "strip"]


def world(name):
    return all_worlds()[NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(status [n], seed bits [n, 128, 128] bool) of the world's requests by the model: computed once, shared, not to be
    changed."""
    W = world(name)
    out = [ssm.seeds_of(W, r) for r in W["reqs"]]
    st, bits = np.array([o[0] for o in out], np.uint8), np.stack([o[1] for o in out])
    st.setflags(write=False); bits.setflags(write=False)
    return st, bits


def existing_fields(W, seed=5):
    """What the slots hold before the call: random directions (read-modify-write shows)."""
    return np.random.RandomState(seed).randint(0, 9, (len(W["reqs"]), 4096)).astype(np.uint8)


def fields_by_oracle(W, status, bits, inout):
    """The model's seeds through the restatement's region build (oracle/navoracle): the expected slots."""
    from oracle import navoracle
    cost, blk = synth.to_chunks(W["cost"]), synth.to_chunks(W["blockers"])
    nav = None
    for l in range(12):
        if (W["layers"] >> l) & 1:
            if nav is None:
                nav = navoracle.OracleNav(cost, blockers=blk, layer=l)
            else:
                nav.set_layer(l, cost=cost, blockers=blk)
    out = np.array(inout, np.uint8, copy=True)
    rows, reqs, seeds = [], [], []
    for i, r in enumerate(W["reqs"]):
        if status[i] or not bits[i].any():
            continue
        br, bc, _, _ = ssm.base_of(int(r["chunk_r"]), int(r["chunk_c"]))
        sd = np.argwhere(bits[i]) + (br, bc)
        reqs.append(ssm.region_req(r, sum(len(s) for s in seeds), len(sd)))
        seeds.append(sd.astype(np.int16)); rows.append(i)
    if rows:
        from tests import cases
        got = nav.build_region_fields(cases.region_reqs_to(navoracle.REGION_REQ_DTYPE, reqs), np.concatenate(seeds),
                                      inout=out[rows], out_stride=4096)
        out[rows] = got
    return out
