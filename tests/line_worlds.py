"""Agent-step worlds whose units stand where units really stand: on tile lines, tile corners and exact tile centres, on chunk
seams and chunk corners, in formations on a regular lattice.  The shared source of tests/test_line_worlds_cpu.py and
tests/test_line_worlds_gpu.py.  Test infrastructure only.

Every other world of the suite puts its agents at a tile centre + uniform(-1.5, 1.5): never on a line.  Destinations of the
order-time queries are tile corners, arrival slots are tile centres; units that have arrived are stepped from there.
csrc/agent_math.h has arms only such positions reach: tile_for_point at x == base of a tile or chunk, sample_flow with dx == 0
(dc = -1 by the strictness of `dx < 0`, weight 0), with wc == 0.5 (two opposing taps cancel exactly: the base tile's
direction), taps and +-4 wu probes across a chunk seam, into a chunk without a field.

`lines`: cases.make_agents (uniform, 1 600 agents) on the 4 x 4-chunk map cases.ref_nav_for(4, 4, seed=21), positions snapped
by kind = uid % 8:

    0 untouched | 1 tile corner | 2 x on a tile line | 3 z on a tile line | 4 exact tile centre | 5 centre in x only
    6 the nearest inner chunk corner (many agents coincide there: the coincident-neighbour arm through the real neighbour
      walk) | 7 x on the nearest chunk seam

(kinds 1-3: the line on the side of the tile uid picks, so both the tile's own base line and its neighbour's occur); a third
of the velocities rounded to multiples of 0.5.  A flock = the agents of one chunk column, its target a tile centre in column
TARGET_COLUMN[flock]: the fields of a flock cover its own column (and the path of flocks 0 and 1 into each other's), so the
taps across most column seams find NO slot.  Some agents of kind 2 / 3 are then moved onto watersheds of their flock's field
(two adjacent tiles with opposite directions, e.g. behind a rectangle of impassable tiles), centred in the other coordinate:
wc == 0.5 and the two taps cancel.

`formation`: blocks of 5 x 5, 7 x 7 and 9 x 9 units (12-36 ClearPath neighbours) and, for the short work lists, of 1 x 2, 2 x 2,
2 x 3 and 3 x 3 units (1, 3, 5, 8 neighbours) on a 3-wu lattice that starts on a tile corner, one common velocity per block,
all MOVING, on open ground.

The expected values come from the reference build (oracle/_ref) and are computed once per process."""
import numpy as np

f32 = np.float32
W = H = 4
KINDS = 8
KIND_NAMES = ("control", "tile corner", "x on tile line", "z on tile line", "tile centre", "centre in x", "chunk corner", "chunk seam in x")
TARGET_COLUMN = (1, 0, 2, 3)
FD_NONE = 0
# N_FlowDir (field.c:2428), indexed by direction byte
_D = 0.70710678118654757
DIR_VEC = np.array([[0, 0], [_D, -_D], [0, -1], [-_D, -_D], [1, 0], [-1, 0], [_D, _D], [0, 1], [-_D, _D]], f32)


# ---------------------------------------------------------------------------------------------
# numpy models of M_Tile_DescForPoint2D (tile.c:547) and n_interpolated_flow_dir (nav.c:3407): float32, expression by expression
# ---------------------------------------------------------------------------------------------
def tile_of(w, h, x, z):
    """(on map, chunk_r, chunk_c, tile_r, tile_c) of points: the inclusive map test, the chunk clamp, tile 64 -> 63."""
    x, z = np.asarray(x, f32), np.asarray(z, f32)
    map_x, map_z = f32(w * 128), f32(-h * 128)
    on = ~((x > map_x) | (x < map_x - f32(w * 256)) | (z < map_z) | (z > map_z + f32(h * 256)))
    cr = np.clip((np.abs(map_z - z) / f32(256)).astype(np.int64), 0, h - 1)
    cc = np.clip((np.abs(map_x - x) / f32(256)).astype(np.int64), 0, w - 1)
    bx = map_x - (cc * 256).astype(f32)
    bz = map_z + (cr * 256).astype(f32)
    tr = np.clip((np.abs(bz - z) / f32(4)).astype(np.int64), 0, 63)
    tc = np.clip((np.abs(bx - x) / f32(4)).astype(np.int64), 0, 63)
    return on, cr, cc, tr, tc


def flow_taps(w, h, pos, flock, slots, pool):
    """The four taps of every agent's sample: dict of dx, dz, wc, wr, present (own chunk has a slot), base_dir, and per tap
    [n][4]: weight, counted (weight > 0 and on the map), chunk index, slot, direction byte (FD_NONE where not counted or
    without a slot); cancel: the blend of the counted taps has length < 1e-6 while their weights do not."""
    pos = np.asarray(pos, f32)
    n = len(pos)
    on, cr, cc, tr, tc = tile_of(w, h, pos[:, 0], pos[:, 1])
    assert on.all()
    own = slots[flock, cr * w + cc]
    bx = (f32(w * 128) - (cc * 256).astype(f32)) - (tc * 4).astype(f32)
    bz = (f32(-h * 128) + (cr * 256).astype(f32)) + (tr * 4).astype(f32)
    dx, dz = pos[:, 0] - (bx - f32(2)), pos[:, 1] - (bz + f32(2))
    dc = np.where(dx < 0, 1, -1)
    dr = np.where(dz > 0, 1, -1)
    wc = np.minimum(np.abs(dx) / f32(4), f32(1))
    wr = np.minimum(np.abs(dz) / f32(4), f32(1))
    one = f32(1)
    sw = np.stack([(one - wc) * (one - wr), wc * (one - wr), (one - wc) * wr, wc * wr], 1).astype(f32)
    abs_r = (cr * 64 + tr)[:, None] + np.stack([0 * dr, 0 * dr, dr, dr], 1)
    abs_c = (cc * 64 + tc)[:, None] + np.stack([0 * dc, dc, 0 * dc, dc], 1)
    counted = (sw > 0) & ~((abs_r < 0) | (abs_r >= h * 64) | (abs_c < 0) | (abs_c >= w * 64))
    chunk = np.where(counted, (abs_r >> 6) * w + (abs_c >> 6), (cr * w + cc)[:, None])
    tslot = slots[flock[:, None], chunk]
    d = np.zeros((n, 4), np.int64)
    ok = counted & (tslot >= 0) & (own >= 0)[:, None]
    d[ok] = pool[tslot[ok], ((abs_r & 63) * 64 + (abs_c & 63))[ok]] & 0xf
    acc = np.zeros((n, 2), f32)
    wsum = np.zeros(n, f32)
    for i in range(4):
        use = ok[:, i] & (d[:, i] != FD_NONE)
        acc = np.where(use[:, None], acc + DIR_VEC[d[:, i]] * sw[:, i:i + 1], acc).astype(f32)
        wsum = np.where(use, wsum + sw[:, i], wsum).astype(f32)
    alen = np.sqrt(acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1], dtype=f32)
    base_dir = np.zeros(n, np.int64)
    base_dir[own >= 0] = pool[own[own >= 0], (tr * 64 + tc)[own >= 0]] & 0xf
    return {"dx": dx, "dz": dz, "wc": wc, "wr": wr, "present": own >= 0, "base_dir": base_dir, "weight": sw, "counted": counted,
            "chunk": chunk, "own_chunk": cr * w + cc, "slot": tslot, "dir": d,
            "cancel": (own >= 0) & (wsum >= f32(1e-6)) & (alen < f32(1e-6))}


def premises(L):
    """The counters of a world, over its agents: what the positions reach in tile_for_point / sample_flow / probe_tiles_bits."""
    a = L.arrays
    pos, flock = a["pos_xz"], a["flock"]
    T = flow_taps(L.w, L.h, pos, flock, a["flock_field_slot"], a["field_pool"])
    other = T["counted"] & (T["chunk"] != T["own_chunk"][:, None])
    probe_other = np.zeros(len(pos), bool)
    own = T["own_chunk"]
    for ox, oz in ((4, 0), (-4, 0), (0, 4), (0, -4)):
        on, cr, cc, tr, tc = tile_of(L.w, L.h, pos[:, 0] + f32(ox), pos[:, 1] + f32(oz))
        probe_other |= on & (cr * L.w + cc != own)
    return {"dx_zero": int((T["dx"] == 0).sum()), "dz_zero": int((T["dz"] == 0).sum()),
            "weight_half": int(((T["wc"] == 0.5) | (T["wr"] == 0.5)).sum()),
            "taps_cancel": int(T["cancel"].sum()),
            "tap_in_other_chunk": int(other.any(1).sum()),
            "tap_in_chunk_without_slot": int((other & (T["slot"] < 0) & T["present"][:, None]).any(1).sum()),
            "probe_in_other_chunk": int(probe_other.sum())}


# ---------------------------------------------------------------------------------------------
# the worlds
# ---------------------------------------------------------------------------------------------
class LineWorld:
    """name; w, h (chunks); grid; nav (the reference's RefNav, kept alive for its position tests); world (cases.make_agents
    style); kind [n]; arrays (navhip_world members: field table and pool of the reference's cache, vdes_xz = None -- the
    step samples --, the flocks in the reference's member order); ref_vel / ref_vdes (move_velocity_work /
    N_DesiredPointSeekVelocity of the reference build); count / searching (formation: ClearPath neighbours per agent)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._oracle = None

    @property
    def n(self):
        return len(self.kind)

    def oracle(self):
        """The restatement's step of this world (navoracle.OracleNav.agent_step), computed once."""
        if self._oracle is None:
            from tests import cases
            self._oracle = cases.oracle_nav_from_ref(self.nav).agent_step(self.arrays, nthreads=16)
        return self._oracle

    def moving(self):
        return ~np.isin(self.world["state"], (2, 4))

    def point_seek(self):
        return np.isin(self.world["state"], (0, 5, 6))


def _cell_of(pos):
    """(row, col) of the tile the builder considers a position in (positions off the lines)."""
    return np.floor((pos[:, 1] + H * 128.0) / 4.0).astype(int), np.floor((W * 128.0 - pos[:, 0]) / 4.0).astype(int)


def snap(pos, kind, uid):
    """The kind table of the module docstring on float64 positions; returns float32.  Lines and centres are multiples of 2:
    exact.  Every agent keeps 12 wu and more off the map edge (cases.make_agents has the tiles 3 and more inside)."""
    R, Cc = _cell_of(pos)
    cx, cz = W * 128.0 - 4.0 * (Cc + 0.5), -H * 128.0 + 4.0 * (R + 0.5)
    sx = np.where((uid // KINDS) % 2 == 0, 2.0, -2.0)          # +2: the tile's own base line (x == bx); -2: its neighbour's
    sz = np.where((uid // (2 * KINDS)) % 2 == 0, -2.0, 2.0)
    seam_x = np.clip(np.rint(pos[:, 0] / 256.0), -(W // 2 - 1), W // 2 - 1) * 256.0
    seam_z = np.clip(np.rint(pos[:, 1] / 256.0), -(H // 2 - 1), H // 2 - 1) * 256.0
    x, z = pos[:, 0].copy(), pos[:, 1].copy()
    x = np.where(np.isin(kind, (1, 2)), cx + sx, np.where(np.isin(kind, (4, 5)), cx, np.where(np.isin(kind, (6, 7)), seam_x, x)))
    z = np.where(np.isin(kind, (1, 3)), cz + sz, np.where(kind == 4, cz, np.where(kind == 6, seam_z, z)))
    return np.stack([x, z], 1).astype(f32)


def _lines_world(grid, n, seed):
    from tests import cases
    world = cases.make_agents(grid, n, 4, seed=seed, clustered=False)
    uid = np.arange(n)
    kind = uid % KINDS
    world["pos_xz"] = snap(world["pos_xz"].astype(np.float64), kind, uid)
    third = uid % 3 == 0
    world["vel_xz"] = np.where(third[:, None], np.rint(world["vel_xz"] * 2) / 2, world["vel_xz"]).astype(f32)
    # a flock = a chunk column; its target an exact tile centre in column TARGET_COLUMN[flock], away from the map edge
    on, cr, cc, tr, tc = tile_of(W, H, world["pos_xz"][:, 0], world["pos_xz"][:, 1])
    world["flock"] = cc.astype(np.int32)
    rng = np.random.RandomState(seed + 2)
    inner = np.zeros(grid.shape, bool)
    inner[8:-8, 8:-8] = True
    dests = []
    for f in range(W):
        cells = np.argwhere((grid != 255) & inner)
        cells = cells[cells[:, 1] // 64 == TARGET_COLUMN[f]]
        dests.append(cells[rng.randint(len(cells))])
    world["dest_cells"] = np.array(dests)
    world["flock_target_xz"] = cases.synth.cell_centre(W, H, world["dest_cells"][:, 0], world["dest_cells"][:, 1])
    return world, kind


def _reference(nav, world):
    """(ref_vel, ref_vdes, slots, pool, flock orders): two passes of the reference's move_velocity_work (the first one
    populates and merges its field cache, as tests/test_agents_gpu.py::test_device_flow_sampling_matches_reference), then its
    cache as a field table."""
    from oracle import pfref
    from tests import cases
    mv, dest_ids = cases.ref_move_for(nav, world)
    try:
        mv.velocity(None)
        vel = mv.velocity(None)
        vdes = mv.vdes()
        slots, pool = cases.cached_field_table(nav, dest_ids, nav.w, nav.h)
        order = [mv.flock_order(f) for f in range(len(world["flock_target_xz"]))]
    finally:
        pfref.RefMove.unload()
    return vel, vdes, slots, pool, order


def watersheds(w, h, slots, pool, flock):
    """Sites where two adjacent tiles of a flock's field point against each other, in the chunks of the flock's own column:
    [(x, z, 2 | 3)] -- x on the line between the tiles (columns c - 1 | c) and z on the row's centre (for an agent of kind
    2), or z on the line (rows r - 1 | r) and x on the column's centre (kind 3).  Tiles 3 and more from the map edge."""
    out = []
    for cr in range(h):
        s = slots[flock, cr * w + flock]
        if s < 0:
            continue
        d = (pool[s].reshape(64, 64) & 0xf).astype(int)
        v = DIR_VEC[d]
        live = d != FD_NONE
        bx, bz = w * 128.0 - flock * 256.0, -h * 128.0 + cr * 256.0
        opp_c = live[:, 1:] & live[:, :-1] & ((v[:, 1:] + v[:, :-1]) == 0).all(2)      # tiles (r, c - 1) and (r, c), c = 1 ..
        opp_r = live[1:, :] & live[:-1, :] & ((v[1:, :] + v[:-1, :]) == 0).all(2)
        for r, c in np.argwhere(opp_c):
            out.append((bx - 4.0 * (c + 1), bz + 4.0 * r + 2.0, 2, cr * 64 + r, flock * 64 + c + 1))
        for r, c in np.argwhere(opp_r):
            out.append((bx - 4.0 * c - 2.0, bz + 4.0 * (r + 1), 3, cr * 64 + r + 1, flock * 64 + c))
    return [(x, z, k) for x, z, k, ar, ac in out if 3 <= ar < h * 64 - 3 and 3 <= ac < w * 64 - 3]


def plant_on_watersheds(world, kind, slots, pool, per_flock=12):
    """Move up to per_flock agents of kind 2 / 3 of every flock -- never a flock's first member, whose position the path
    request of the flock starts from -- onto watersheds of its field.  Returns how many were moved."""
    moved = 0
    for f in range(W):
        sites = watersheds(W, H, slots, pool, f)
        members = np.flatnonzero(world["flock"] == f)[1:]
        for k in (2, 3):
            cand = [u for u in members if kind[u] == k]
            here = [s for s in sites if s[2] == k]
            for u, s in list(zip(cand, here))[:per_flock // 2]:
                world["pos_xz"][u] = (s[0], s[1])
                moved += 1
    return moved


_WORLDS = {}


def lines():
    """The `lines` world, built once."""
    if "lines" not in _WORLDS:
        from tests import cases
        grid, nav = cases.ref_nav_for(W, H, seed=21)
        world, kind = _lines_world(grid, 1600, seed=77)
        # the fields the reference builds for this world, the watersheds in them, then the world with agents on those
        _, _, slots, pool, _ = _reference(nav, world)
        planted = plant_on_watersheds(world, kind, slots, pool)
        vel, vdes, slots, pool, order = _reference(nav, world)
        arrays = cases.step_arrays(world, None, order)
        arrays["flock_field_slot"], arrays["field_pool"] = slots, pool
        _WORLDS["lines"] = LineWorld(name="lines", w=W, h=H, grid=grid, nav=nav, world=world, kind=kind, arrays=arrays, ref_vel=vel,
                                     ref_vdes=vdes, planted=planted)
    return _WORLDS["lines"]


# blocks of the formation world: (units in x, units in z, how many blocks)
BLOCKS = ((5, 5, 6), (7, 7, 4), (9, 9, 3), (1, 2, 8), (2, 2, 8), (2, 3, 6), (3, 3, 6))
BLOCK_VELS = ((0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (-0.5, 0.25), (0.25, 0.0), (0.0, -0.75))      # ((0.25, 0): below the still speed)
LATTICE = 3.0
SITE = 64.0


def _formation_world():
    shapes = [(a, b) for a, b, k in BLOCKS for _ in range(k)]
    # interleave large and small blocks over the sites
    order = np.random.RandomState(5).permutation(len(shapes))
    per = 14                                                   # sites per row: 64 wu apart, from -416
    pos, vel, block = [], [], []
    for s, k in enumerate(order):
        a, b = shapes[k]
        ox, oz = -416.0 + SITE * (s % per), -416.0 + SITE * (s // per)            # a tile corner (a multiple of 4)
        i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
        p = np.stack([ox + LATTICE * i.ravel(), oz + LATTICE * j.ravel()], 1)
        pos.append(p)
        vel.append(np.tile(BLOCK_VELS[s % len(BLOCK_VELS)], (len(p), 1)))
        block.append(np.full(len(p), s))
    pos, vel, block = np.concatenate(pos), np.concatenate(vel), np.concatenate(block)
    n, nb = len(pos), len(shapes)
    p = np.random.RandomState(6).permutation(n)                # (uids: a fixed permutation of the build order)
    pos, vel, block = pos[p], vel[p], block[p]
    # ClearPath neighbours: everybody within 10 wu (no lattice distance 3 sqrt(a^2 + b^2) is near 10: 9.49 | 10.82), moving
    # ones dynamic, the slow block's static, 32 of each at most
    d = np.linalg.norm(pos[:, None, :] - pos[None, :, :], axis=2)
    near = (d < 10.0) & ~np.eye(n, dtype=bool)
    fast = np.linalg.norm(vel, axis=1) >= 0.3
    count = np.minimum(32, (near & fast[None, :]).sum(1)) + np.minimum(32, (near & ~fast[None, :]).sum(1))
    # a flock per block; its target a tile corner 64 wu further on (what the order-time queries hand out)
    origin = np.stack([pos[block == s].min(0) for s in range(nb)])
    target = np.clip(origin + [64.0, 32.0], -480.0, 480.0)
    rng = np.random.RandomState(7)
    world = {"pos_xz": pos.astype(f32), "vel_xz": vel.astype(f32), "radius": np.ones(n, f32),
             "max_speed": rng.choice([20.0, 15.0, 25.0], nb).astype(f32)[block], "speed": np.full(n, 20.0, f32),
             "flags": np.full(n, 1 << 3, np.uint32), "state": np.zeros(n, np.uint8), "has_dest_los": np.zeros(n, np.uint8),
             "flock": block.astype(np.int32), "flock_target_xz": target.astype(f32)}
    return world, count.astype(np.int32)


def formation():
    """The `formation` world, built once."""
    if "formation" not in _WORLDS:
        from oracle import pfref
        from tests import cases
        nav = pfref.RefNav(np.ones((H, W, 64, 64), np.uint8))
        world, count = _formation_world()
        vel, vdes, slots, pool, order = _reference(nav, world)
        arrays = cases.step_arrays(world, None, order)
        arrays["flock_field_slot"], arrays["field_pool"] = slots, pool
        n = len(count)
        _WORLDS["formation"] = LineWorld(name="formation", w=W, h=H, grid=np.ones((H * 64, W * 64), np.uint8), nav=nav, world=world,
                                         kind=np.zeros(n, int), arrays=arrays, ref_vel=vel, ref_vdes=vdes, count=count,
                                         searching=np.ones(n, bool), irregular=np.zeros(n, bool))
    return _WORLDS["formation"]
