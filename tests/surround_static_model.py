"""The static half of the surround queries -- a target without ENTITY_FLAG_MOVABLE, a building -- for the tests of
navhip_static_targets_set / navhip_surround_queries_ex[_dev]:

  * the reference side through ctypes on oracle/_ref's library (oracle/ is not touched): M_Tile_AllUnderObj (tile.c:594) for
    the lists a test registers, N_ObjAdjacentToStaticWith (nav.c:4932) and N_ClosestReachableAdjacentPosStatic (nav.c:4621)
    for the answers.  vec2_t, vec3_t and struct map_resolution go by value as ctypes structures, struct obb as 39 floats of
    which only the bottom corners 0, 1, 5, 4 are read;
  * a numpy model of the static arm on top of tests/surround_model.py (its floods, its circle tiles): n_objects_adjacent
    (nav.c:1682) and n_closest_adjacent_pos (nav.c:1636) over a tile LIST in list order.  The model rasterises nothing:
    the lists are the reference's.  Per row it exposes what a test asserts its premise from: the winning list entry, the
    answer tiles that tie with it, the depth of every flood;
  * the scenes the tests run on.

TEST INFRASTRUCTURE: never imported by the product."""
import ctypes as C

import numpy as np

from tests import surround_model as sm

F = np.float32
CAP = 2048                # the reference's tds[2048]
MOVABLE, SQ_ADJACENT, SQ_HOST = sm.MOVABLE, sm.SQ_ADJACENT, sm.SQ_HOST


# ---- the reference through ctypes --------------------------------------------------------------------------------------
class Vec2(C.Structure):
    _fields_ = [("x", C.c_float), ("z", C.c_float)]


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class MapRes(C.Structure):
    _fields_ = [("chunk_w", C.c_int), ("chunk_h", C.c_int), ("tile_w", C.c_int), ("tile_h", C.c_int),
                ("field_w", C.c_float), ("field_h", C.c_float)]


class TileDesc(C.Structure):
    _fields_ = [("chunk_r", C.c_int), ("chunk_c", C.c_int), ("tile_r", C.c_int), ("tile_c", C.c_int)]


OBB_FLOATS = 39           # center 3, axes 9, half_lengths 3, corners 8 x 3 (collision.h:63)
_CORNER0 = 15
_bound = None


def _lib():
    global _bound
    if _bound is None:
        from oracle import pfref
        L = pfref.lib()
        L.pfref_nav_private.restype = C.c_void_p
        L.pfref_nav_private.argtypes = [C.c_void_p]
        L.M_Tile_AllUnderObj.restype = C.c_size_t
        L.M_Tile_AllUnderObj.argtypes = [Vec3, MapRes, C.c_void_p, C.c_void_p, C.c_size_t]
        L.N_ObjAdjacentToStaticWith.restype = C.c_bool
        L.N_ObjAdjacentToStaticWith.argtypes = [C.c_void_p, Vec3, Vec2, C.c_float, C.c_void_p]
        L.N_ClosestReachableAdjacentPosStatic.restype = C.c_bool
        L.N_ClosestReachableAdjacentPosStatic.argtypes = [C.c_void_p, C.c_int, Vec3, Vec2, C.c_void_p, C.POINTER(Vec2)]
        L.N_DestIDForPos.restype = C.c_uint32
        L.N_DestIDForPos.argtypes = [C.c_void_p, Vec3, Vec2, C.c_int]
        _bound = L
    return _bound


def map_res(w, h):
    """N_GetResolution (nav.c:4982) of a map of w x h chunks."""
    return MapRes(w, h, 64, 64, 256.0, 256.0)


def map_vec3(w, h):
    mx, mz = sm.map_pos(w, h)
    return Vec3(float(mx), 0.0, float(mz))


def make_obb(w, h, centre_rc, half_tiles, angle_deg=0.0, off=(0.0, 0.0)):
    """A struct obb as 39 floats: the rectangle of half_tiles = (half rows, half columns) tiles around the point `off` away
    from the corner point of tile centre_rc (the corner with the lower row and column), turned by angle_deg.  Only the
    bottom corners are filled: 0, 1, 5, 4 go round the rectangle."""
    o = np.zeros(OBB_FLOATS, F)
    c = sm.corner(w, h, *centre_rc).astype(np.float64) + np.asarray(off, np.float64)
    hz, hx = 4.0 * half_tiles[0], 4.0 * half_tiles[1]
    a = np.deg2rad(angle_deg)
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    for slot, (sx, sz) in zip((0, 1, 5, 4), ((-1, -1), (1, -1), (1, 1), (-1, 1))):
        p = c + rot @ np.array([sx * hx, sz * hz])
        o[_CORNER0 + 3 * slot], o[_CORNER0 + 3 * slot + 2] = p[0], p[1]
    return o


def ref_tiles(w, h, obb):
    """M_Tile_AllUnderObj: the absolute tiles [n][2] int16 in the reference's order, duplicates and all, cut at 2 048."""
    out = (TileDesc * CAP)()
    obb = np.ascontiguousarray(obb, F)
    n = _lib().M_Tile_AllUnderObj(map_vec3(w, h), map_res(w, h), obb.ctypes.data_as(C.c_void_p), out, CAP)
    return np.array([(t.chunk_r * 64 + t.tile_r, t.chunk_c * 64 + t.tile_c) for t in out[:n]], np.int16).reshape(-1, 2)


class Ref:
    """The static queries of one pfref.RefNav."""

    def __init__(self, nav):
        self.nav = nav
        self.priv = _lib().pfref_nav_private(nav._h)
        self.mp = Vec3(*[float(v) for v in nav.map_pos])

    def dest_id(self, xz, layer=0):
        return int(_lib().N_DestIDForPos(self.priv, self.mp, Vec2(float(xz[0]), float(xz[1])), layer))

    def adjacent(self, pos, radius, obb):
        obb = np.ascontiguousarray(obb, F)
        return bool(_lib().N_ObjAdjacentToStaticWith(self.priv, self.mp, Vec2(float(pos[0]), float(pos[1])), float(radius),
                                                     obb.ctypes.data_as(C.c_void_p)))

    def closest(self, layer, src, obb):
        obb = np.ascontiguousarray(obb, F)
        out = Vec2(0.0, 0.0)
        ok = _lib().N_ClosestReachableAdjacentPosStatic(self.priv, layer, self.mp, Vec2(float(src[0]), float(src[1])),
                                                        obb.ctypes.data_as(C.c_void_p), C.byref(out))
        return (True, (out.x, out.z)) if ok else (False, (0.0, 0.0))

    def answers(self, scene, rows=None):
        """(query [n] u8, dest [n][2][2] f32) of the scene's static rows, as movement.c:2509-2567 asks: touching first and
        nothing else then, else the closest position from pos + new_vel and from pos.  Other rows stay 0."""
        w = scene.world
        query, dest = np.zeros(w.n, np.uint8), np.zeros((w.n, 2, 2), F)
        for i in (scene.static_rows() if rows is None else rows):
            obb = scene.obbs[scene.target_set[i]]
            if self.adjacent(w.pos[i], w.radius[i], obb):
                query[i] = SQ_ADJACENT
                continue
            for c, src in enumerate((w.pos[i] + w.vel[i], w.pos[i])):
                ok, p = self.closest(w.layer_of(i), src, obb)
                if ok:
                    query[i] |= sm.SQ_HAS_DEST_0 << c
                    dest[i, c] = p
        return query, dest


# ---- the model ---------------------------------------------------------------------------------------------------------
def first_occurrences(tiles):
    """The list without its later duplicates, order kept: what the library keeps of a registered list."""
    seen, out = set(), []
    for t in map(tuple, np.asarray(tiles).tolist()):
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def touching(world, pos, radius, tiles):
    """n_objects_adjacent: a tile of the unit's circle within one row and one column of a tile of the list."""
    ut = np.array(world.tiles_under(pos, radius), np.int32).reshape(-1, 2)
    tt = np.asarray(tiles, np.int32).reshape(-1, 2)
    if not len(ut) or not len(tt):
        return False
    d = np.abs(tt[:, None, :] - ut[None, :, :])
    return bool(((d[..., 0] <= 1) & (d[..., 1] <= 1)).any())


def closest(world, layer, src, tiles, key="list"):
    """n_closest_adjacent_pos over the list in list order: dict(dest or None, entry: the winning list index, tile: its
    answer tile, tied: the OTHER answer tiles as far as the winner, floods: per entry (answer, depth)).
    key = "tile" is the deliberate mistake of a pick keyed on the answer tile's position: of equal lengths the
    row-major-first answer tile."""
    s = sm.tile_for_point(world.w, world.h, src[0], src[1])
    assert s is not None
    iid = world.islands[s]
    best, entry, floods, lens = np.inf, None, [], []
    for i, t in enumerate(map(tuple, np.asarray(tiles).tolist())):
        ans, depth = world.flood(layer, t, iid)
        floods.append((ans, depth))
        if ans is None:
            continue
        p = sm.corner(world.w, world.h, *ans)
        d = sm._len(F(src[0] - p[0]), F(src[1] - p[1]))
        lens.append((d, ans))
        if d < best:
            best, entry = d, i
    if entry is None:
        return {"dest": None, "entry": None, "tile": None, "tied": [], "floods": floods}
    tile = floods[entry][0]
    tied = sorted({a for d, a in lens if d == best and a != tile})
    if key == "tile" and tied:
        tile = min([tile] + tied)
    return {"dest": sm.corner(world.w, world.h, *tile), "entry": entry, "tile": tile, "tied": tied, "floods": floods}


def answers(scene, key="list", rows=None):
    """(query, dest, info per row) of the scene's static rows: the reference's answers, and NAVHIP_SQ_HOST where the device
    leaves the row to the host (the rules of tests/surround_model.py: radius, NaN, a source off the map, the window)."""
    w = scene.world
    n = w.n
    H, W = w.cost.shape
    query, dest, info = np.zeros(n, np.uint8), np.zeros((n, 2, 2), F), [None] * n
    for i in (scene.static_rows() if rows is None else rows):
        tiles = scene.lists[scene.target_set[i]]
        inf = info[i] = {"adjacent": False, "host": None, "closest": [None, None]}
        if sm.ntiles_of(w.radius[i]) > sm.SQ_NT:
            inf["host"] = "radius"
        elif np.isnan([*w.pos[i], w.radius[i]]).any():
            inf["host"] = "nan"
        if inf["host"]:
            query[i] = SQ_HOST
            continue
        if touching(w, w.pos[i], w.radius[i], tiles):
            inf["adjacent"] = True
            query[i] = SQ_ADJACENT
            continue
        srcs = [w.pos[i] + w.vel[i], w.pos[i]]
        if any(sm.tile_for_point(w.w, w.h, *s) is None for s in srcs):
            inf["host"] = "source"
            query[i] = SQ_HOST
            continue
        for c in range(2):
            got = inf["closest"][c] = closest(w, w.layer_of(i), srcs[c], tiles, key)
            if got["dest"] is not None:
                query[i] |= sm.SQ_HAS_DEST_0 << c
                dest[i, c] = got["dest"]
            for tile, (ans, depth) in zip(map(tuple, np.asarray(tiles).tolist()), got["floods"]):
                far = max(tile[0], H - 1 - tile[0], tile[1], W - 1 - tile[1])
                if (ans is not None and depth > sm.WINDOW + 1) or (ans is None and far > sm.WINDOW):
                    inf["host"] = "window"
        if inf["host"]:
            query[i], dest[i] = SQ_HOST, 0
    return query, dest, info


def max_depth(info):
    """The deepest flood of the rows: the Chebyshev distance of an answer from the entry it belongs to."""
    return max([depth for inf in info if inf for got in inf["closest"] if got for ans, depth in got["floods"]] + [0])


# ---- the scenes --------------------------------------------------------------------------------------------------------
class Scene:
    """A map with buildings and a dense batch: entity rows first the buildings (no MOVABLE flag; row j is set j), then
    whatever add() appends.  The buildings' tiles are blocked on every layer of the scene."""

    def __init__(self, name, w, h, obbs, layers=(0,), cost=None, block_sets=True):
        self.name, self.w, self.h = name, w, h
        self.obbs = [np.ascontiguousarray(o, F) for o in obbs]
        self.lists = [ref_tiles(w, h, o) for o in self.obbs]
        self.cost = np.ones((h * 64, w * 64), np.uint8) if cost is None else cost
        self.blockers = {l: np.zeros((h * 64, w * 64), np.uint16) for l in layers}
        if block_sets:
            for tiles in self.lists:
                for bl in self.blockers.values():
                    bl[tiles[:, 0], tiles[:, 1]] = 1
        self._rows = []
        for j, tiles in enumerate(self.lists):
            centre = tiles[len(tiles) // 2] if len(tiles) else (0, 0)
            self._rows.append((sm.xz(w, h, int(centre[0]), int(centre[1])), 1.0, 0, (0.0, 0.0), -1, -1))
        self._world = None

    def add(self, p, radius, set_index=-1, vel=(0.0, 0.0), flags=MOVABLE, target=None):
        """A row: a unit with the building `set_index` as its target (target: another entity row instead, or -1)."""
        assert self._world is None
        tgt = set_index if target is None else target
        self._rows.append((np.asarray(p, F), radius, flags, vel, tgt, set_index if target is None else -1))
        return len(self._rows) - 1

    def add_at(self, r, c, radius=1.0, set_index=0, vel=(0.0, 0.0), off=(0.0, 0.0)):
        return self.add(sm.xz(self.w, self.h, r, c, off), radius, set_index, vel)

    @property
    def world(self):
        if self._world is None:
            pos, radius, flags, vel, target, tset = zip(*self._rows)
            self._world = sm.SWorld(self.name, self.w, self.h, self.cost, self.blockers, pos, radius, flags, vel, target)
            self.target_set = np.array(tset, np.int32)
        return self._world

    def static_rows(self):
        w = self.world
        return [i for i in range(w.n) if w.target[i] >= 0 and not (w.flags[w.target[i]] & MOVABLE) and self.target_set[i] >= 0]


def _around(scene, set_index, dists, radii=(1.0,), vel=(0.3, -0.2)):
    """Units on every side and on the diagonals of the set's bounding box, `dists` tiles beyond it."""
    t = scene.lists[set_index]
    r0, r1, c0, c1 = int(t[:, 0].min()), int(t[:, 0].max()), int(t[:, 1].min()), int(t[:, 1].max())
    rm, cm = (r0 + r1) // 2, (c0 + c1) // 2
    H, W = scene.h * 64, scene.w * 64
    k = 0
    for d in dists:
        for r, c in ((r0 - d, cm), (r1 + d, cm), (rm, c0 - d), (rm, c1 + d), (r0 - d, c0 - d), (r0 - d, c1 + d), (r1 + d, c0 - d),
                     (r1 + d, c1 + d), (r0 - d, c0 + 1), (r1 + d, c1 - 1)):
            if 0 <= r < H and 0 <= c < W:
                rad = radii[k % len(radii)]
                scene.add_at(r, c, rad, set_index, [(vel[0], vel[1]), (0.0, 0.0), (-vel[1], vel[0])][k % 3], off=(0.4, -0.3))
                k += 1


def axis_aligned():
    """Case 1: boxes of 1 x 1, 5 x 3 and 10 x 10 tiles inside a chunk of a 2 x 2 map; units on every side, touching and
    not, diagonal neighbours, two tiles away, radii 0.5 to 32 (layers 0 to 3)."""
    w = h = 2
    obbs = [make_obb(w, h, (20, 20), (0.49, 0.49), off=(-2.0, 2.0)), make_obb(w, h, (20, 44), (2.49, 1.49), off=(-2.0, 2.0)),
            make_obb(w, h, (45, 25), (4.99, 4.99))]
    sc = Scene("axis_aligned", w, h, obbs, layers=(0, 1, 2, 3))
    for j in range(3):
        _around(sc, j, (1, 2, 3, 5), radii=(0.5, 1.0, 3.9))
        _around(sc, j, (4, 7, 9, 12), radii=(4.9, 9.0, 14.0, 20.0, 32.0))
    return sc


def rotated():
    """Case 2 and 3: boxes of 7 x 4 tiles turned by 30, 45 and 60 degrees, and a square one turned by 45; units on tile
    centres all around, where equal lengths are common."""
    w = h = 2
    obbs = [make_obb(w, h, (24, 24), (3.5, 2.0), 30.0), make_obb(w, h, (24, 90), (3.5, 2.0), 45.0),
            make_obb(w, h, (90, 24), (3.5, 2.0), 60.0), make_obb(w, h, (90, 90), (3.0, 3.0), 45.0)]
    sc = Scene("rotated", w, h, obbs)
    for j in range(4):
        t = sc.lists[j]
        r0, r1, c0, c1 = int(t[:, 0].min()), int(t[:, 0].max()), int(t[:, 1].min()), int(t[:, 1].max())
        for r in range(r0 - 6, r1 + 7, 2):
            for c in range(c0 - 6, c1 + 7, 2):
                if r < r0 - 1 or r > r1 + 1 or c < c0 - 1 or c > c1 + 1:
                    sc.add_at(r, c, 1.0, j, (0.0, 0.0) if (r + c) % 4 else (0.2, 0.1))
    return sc


def chunk_corner_and_edge():
    """Case 4: a box across the meeting point of the four chunks of a 2 x 2 map, and two whose sets touch the map's first
    rows and last columns."""
    w = h = 2
    obbs = [make_obb(w, h, (64, 64), (4.0, 5.0), 20.0), make_obb(w, h, (2, 40), (2.0, 4.0)),
            make_obb(w, h, (100, 125), (4.0, 2.5), 10.0)]
    sc = Scene("chunk_corner_and_edge", w, h, obbs)
    for j in range(3):
        _around(sc, j, (2, 4, 8), radii=(1.0, 2.5))
    return sc


def two_islands():
    """Case 5: a one-tile wall of impassable cost; pos and pos + new_vel lie across it."""
    w = h = 2
    cost = np.ones((128, 128), np.uint8)
    cost[:, 60] = 255
    sc = Scene("two_islands", w, h, [make_obb(w, h, (40, 40), (3.0, 4.0), 15.0)], cost=cost)
    for r in (20, 40, 70):
        sc.add_at(r, 59, 1.0, 0, (-5.0, 0.0), off=(-1.5, 0.0))        # from the left island onto the right one
        sc.add_at(r, 61, 1.0, 0, (5.0, 0.0), off=(1.5, 0.0))       # ... and back
        sc.add_at(r, 80, 1.0, 0, (0.3, 0.0))                        # both on the right island
    return sc


def nothing_reachable():
    """Case 6: the units' island is blocked wall to wall.  A 1 x 1 map: a flood that finds nothing has to visit the whole map,
    and only a map that fits the window lets it (the rule of NAVHIP_DQ_HOST)."""
    cost = np.ones((64, 64), np.uint8)
    cost[:, 40:42] = 255
    sc = Scene("nothing_reachable", 1, 1, [make_obb(1, 1, (30, 20), (1.5, 1.5))], cost=cost)
    sc.blockers[0][:, 42:] = 1
    sc.add_at(30, 50, 1.0, 0, (0.2, 0.0))
    sc.add_at(10, 60, 1.0, 0)
    sc.add_at(30, 10, 1.0, 0, (0.2, 0.0))                           # (the left island: answered)
    return sc


def cap(side=45):
    """Case 7: a box of about side x side tiles; at 45 the reference's list is cut at 2 048 entries.  Two rows."""
    w = h = 2
    sc = Scene("cap_%d" % side, w, h, [make_obb(w, h, (64, 60), (side / 2.0, side / 2.0), 0.0, off=(-1.0, 1.0))])
    sc.add_at(64, 100, 1.0, 0, (0.3, 0.1))
    sc.add_at(20, 20, 1.0, 0, (0.0, 0.0))
    return sc


def window(free_col):
    """Case 8: a 3 x 2 map blocked everywhere but column free_col; the set is the two tiles (64, 90) and (64, 91).  With
    free_col = 154 the nearest free tile is 63 tiles from the entry (64, 91) and 64 from (64, 90): answered.  With 155 it
    is 64 tiles from the nearer entry and 65 from the other, whose flood has to leave the window."""
    w, h = 3, 2
    sc = Scene("window_%d" % free_col, w, h, [make_obb(w, h, (64, 91), (0.25, 0.75), off=(0.0, 2.0))])
    sc.blockers[0][:] = 1
    sc.blockers[0][:, free_col] = 0
    sc.add_at(64, 170, 1.0, 0, (0.2, 0.0))
    sc.add_at(30, 180, 1.0, 0)
    return sc


def mixed(nq):
    """Case 9: nq rows of no-target, movable-target and static rows on layers 0 and 2, in the sparse form over one world."""
    w = h = 2
    obbs = [make_obb(w, h, (30, 30), (2.5, 1.5), 30.0), make_obb(w, h, (80, 70), (5.0, 5.0))]
    sc = Scene("mixed", w, h, obbs, layers=(0, 2))
    movers = [sc.add(sm.xz(w, h, r, c, (0.6, -0.3)), rad, target=-1) for (r, c), rad in (((50, 50), 6.5), ((100, 30), 4.0))]
    for bl in sc.blockers.values():
        sm._disc(bl, 50, 50, 2, 1)
    rng = np.random.RandomState(17)
    for i in range(300):
        kind, rad = i % 4, (1.0, 10.5)[(i // 4) % 2]
        r, c = int(rng.randint(4, 124)), int(rng.randint(4, 124))
        vel = rng.normal(0, 0.4, 2).astype(F)
        if kind == 0:
            sc.add(sm.xz(w, h, r, c), rad, vel=vel, target=(-1, -2)[i % 8 == 0])
        elif kind == 1:
            sc.add(sm.xz(w, h, r, c), rad, vel=vel, target=movers[i % 2])
        else:
            sc.add(sm.xz(w, h, r, c, (0.3, 0.2)), rad, i % 2, vel)
    return sc


_cache = {}


def scene(name, *args):
    """The scene `name`, built once (its world caches its floods: leave it unchanged)."""
    key = (name,) + args
    if key not in _cache:
        _cache[key] = globals()[name](*args)
        _cache[key].world
    return _cache[key]
