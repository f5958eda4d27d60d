"""A numpy model of the two unit queries of STATE_SURROUND_ENTITY for circle (movable) targets, written from the reference's
nav.c / tile.c / collision.c -- n_objects_adjacent (nav.c:1682), n_closest_adjacent_pos (nav.c:1636), the flood of
n_closest_island_tiles (nav.c:1226) with maxout = 1, M_Tile_AllUnderCircle (tile.c:687), M_Tile_DescForPoint2D (tile.c:547),
C_CircleRectIntersection (collision.c:997), n_update_island_field (nav.c:1731) -- and the worlds the surround-query tests
run on.  Floats are np.float32 operation by operation (double where the reference is).  Per target tile the model exposes
the flood's answer and its depth, so that a test can assert the premise of its case.

`variant` names ONE deliberate mistake (tests/test_surround_queries_cpu.py shows that each changes an answer):
    "le"  "colmajor"  "centres"  "start_unvisited"  "four"  "ignore_blockers"  "dest_island"  "vel_both"
"""
import collections

import numpy as np

F = np.float32
MOVABLE = 1 << 3
SQ_ADJACENT, SQ_HAS_DEST_0, SQ_HAS_DEST_1, SQ_HOST = 1, 2, 4, 0x80
SQ_NT = 8                 # ceil(radius / 4) the device answers up to
WINDOW = 63               # Chebyshev radius of the device's flood window
DELTAS8 = [(0, 0), (0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)]      # (dr, dc), nav.c:1257
DELTAS4 = DELTAS8[:5]
EPS = F(1.0 / 1024)


def map_pos(w, h):
    return F(w * 128.0), F(-h * 128.0)


def xz(w, h, r, c, off=(0.0, 0.0)):
    """A point of tile (r, c): its centre moved by `off`."""
    mx, mz = map_pos(w, h)
    return np.array([mx - F(4 * c + 2) + F(off[0]), mz + F(4 * r + 2) + F(off[1])], F)


def corner(w, h, r, c):
    """The corner n_closest_adjacent_pos answers with (nav.c:1662)."""
    mx, mz = map_pos(w, h)
    return np.array([mx - F(c) * F(4.0), mz + F(r) * F(4.0)], F)


def tile_for_point(w, h, x, z):
    """M_Tile_DescForPoint2D as an absolute tile, None outside the map."""
    x, z = F(x), F(z)
    mx, mz = map_pos(w, h)
    if not (x <= mx) or not (x >= mx - F(w * 256)) or not (z >= mz) or not (z <= mz + F(h * 256)):
        return None
    chunk_r = min(max(int(abs(mz - z) / F(256.0)), 0), h - 1)
    chunk_c = min(max(int(abs(mx - x) / F(256.0)), 0), w - 1)
    base_x, base_z = mx - F(chunk_c * 256), mz + F(chunk_r * 256)
    tile_r = min(max(int(abs(base_z - z) / F(4.0)), 0), 63)
    tile_c = min(max(int(abs(base_x - x) / F(4.0)), 0), 63)
    return chunk_r * 64 + tile_r, chunk_c * 64 + tile_c


def _len(x, z):
    return np.sqrt(F(x * x + z * z))


def _line_circle(ax, az, bx, bz, cx, cz, radius):
    dx, dz = F(bx - ax), F(bz - az)
    A = F(float(dx) * float(dx) + float(dz) * float(dz))
    B = F(F(2) * F(F(dx * F(ax - cx)) + F(dz * F(az - cz))))
    fx, fz = F(ax - cx), F(az - cz)
    Cc = F(float(fx) * float(fx) + float(fz) * float(fz) - float(radius) * float(radius))
    det = F(float(B) * float(B) - float(F(F(F(4) * A) * Cc)))
    if det < 0 or A < EPS:
        return False
    if det == 0:
        t = F(-B) / F(F(2) * A)
    else:
        sq = np.sqrt(float(det))
        t1 = F((float(-B) + sq) / float(F(F(2) * A)))
        t2 = F((float(-B) - sq) / float(F(F(2) * A)))
        t = min(t1, t2)
    return not (t < 0 or t > 1)


def circle_hits_tile(w, h, cx, cz, radius, r, c):
    """C_CircleRectIntersection against M_Tile_Bounds of the nav tile (r, c)."""
    mx, mz = map_pos(w, h)
    cx, cz, radius = F(cx), F(cz), F(radius)
    x = F(F(mx - F((c >> 6) * 256)) - F((c & 63) * 4))
    z = F(F(mz + F((r >> 6) * 256)) + F((r & 63) * 4))
    qx = [F(x - F(4)), x, x, F(x - F(4))]
    qz = [z, z, F(z + F(4)), F(z + F(4))]
    apx, apz = F(cx - qx[0]), F(cz - qz[0])
    abx, abz, adx, adz = F(qx[1] - qx[0]), F(qz[1] - qz[0]), F(qx[3] - qx[0]), F(qz[3] - qz[0])
    ap_ab, ap_ad = F(F(apx * abx) + F(apz * abz)), F(F(apx * adx) + F(apz * adz))
    if 0 <= ap_ab <= F(F(abx * abx) + F(abz * abz)) and 0 <= ap_ad <= F(F(adx * adx) + F(adz * adz)):
        return True
    for i in range(4):
        if _len(F(qx[i] - cx), F(qz[i] - cz)) <= radius:
            return True
    return any(_line_circle(qx[i], qz[i], qx[(i + 1) & 3], qz[(i + 1) & 3], cx, cz, radius) for i in range(4))


def ntiles_of(radius):
    return int(np.ceil(float(F(radius) / F(4))))


def islands_of(cost):
    """n_update_island_field: 4-connected components of cost != 255, numbered in chunk-major, then row-major order of
    their first tile; 0xffff elsewhere."""
    H, W = cost.shape
    isl = np.full((H, W), 0xffff, np.uint16)
    nid = 0
    for cr in range(H // 64):
        for cc in range(W // 64):
            for r in range(cr * 64, cr * 64 + 64):
                for c in np.flatnonzero((isl[r, cc * 64:cc * 64 + 64] == 0xffff) & (cost[r, cc * 64:cc * 64 + 64] != 255)) + cc * 64:
                    if isl[r, c] != 0xffff:
                        continue
                    isl[r, c] = nid
                    todo = [(r, int(c))]
                    while todo:
                        a, b = todo.pop()
                        for dr, dc in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                            rr, cc2 = a + dr, b + dc
                            if 0 <= rr < H and 0 <= cc2 < W and isl[rr, cc2] == 0xffff and cost[rr, cc2] != 255:
                                isl[rr, cc2] = nid
                                todo.append((rr, cc2))
                    nid += 1
    return isl


class SWorld:
    """One map and one batch: cost [h*64][w*64] u8, blockers {layer: [h*64][w*64] u16}, the snapshot (pos, radius, flags),
    the step's velocity and the target row per entity (dense form: one row per entity)."""

    def __init__(self, name, w, h, cost, blockers, pos, radius, flags, vel, target):
        self.name, self.w, self.h = name, w, h
        self.cost = np.ascontiguousarray(cost, np.uint8)
        self.blockers = {l: np.ascontiguousarray(b, np.uint16) for l, b in blockers.items()}
        self.pos = np.ascontiguousarray(pos, F).reshape(-1, 2)
        n = len(self.pos)
        self.radius = np.ascontiguousarray(radius, F).reshape(n)
        self.flags = np.ascontiguousarray(flags, np.uint32).reshape(n)
        self.vel = np.ascontiguousarray(vel, F).reshape(n, 2)
        self.target = np.ascontiguousarray(target, np.int32).reshape(n)
        for i in range(n):                       # every entity is a row of the dense form: its layer has planes
            self.blockers.setdefault(self.layer_of(i), np.zeros(self.cost.shape, np.uint16))
        self.islands = islands_of(self.cost)
        self._tiles, self._floods = {}, {}

    @property
    def n(self):
        return len(self.pos)

    def layer_of(self, i):
        """Entity_NavLayerWithRadius"""
        f, r = int(self.flags[i]), self.radius[i]
        base = 4 if f & (1 << 14) else (8 if f & (1 << 15) else 0)
        return base + (3 if r >= 15 else 2 if r >= 10 else 1 if r >= 5 else 0)

    def tiles_under(self, p, radius, colmajor=False):
        """M_Tile_AllUnderCircle: the tiles in the reference's order."""
        key = (float(p[0]), float(p[1]), float(radius), colmajor)
        if key not in self._tiles:
            out = []
            t = tile_for_point(self.w, self.h, p[0], p[1])
            if t is not None:
                nt = ntiles_of(radius)
                for a in range(-nt, nt + 1):
                    for b in range(-nt, nt + 1):
                        dr, dc = (b, a) if colmajor else (a, b)
                        r, c = t[0] + dr, t[1] + dc
                        if 0 <= r < self.h * 64 and 0 <= c < self.w * 64 and circle_hits_tile(self.w, self.h, p[0], p[1], radius, r, c):
                            out.append((r, c))
            self._tiles[key] = out
        return self._tiles[key]

    def flood(self, layer, start, giid, variant=None):
        """n_closest_island_tiles(start, giid, ignore_blockers = false, maxout = 1): (tile or None, depth: the Chebyshev
        distance of the answer from the start -- of the furthest tile visited when there is none)."""
        key = (layer, start, int(giid), variant if variant in ("start_unvisited", "four", "ignore_blockers") else None)
        if key in self._floods:
            return self._floods[key]
        H, W = self.cost.shape
        bl = self.blockers[layer]
        visited = np.zeros((H, W), bool)
        if variant != "start_unvisited":
            visited[start] = True
        q = collections.deque([start])
        deltas = DELTAS4 if variant == "four" else DELTAS8
        ans, depth = None, 0
        while q and ans is None:
            r0, c0 = q.popleft()
            for dr, dc in deltas:
                r, c = r0 + dr, c0 + dc
                if not (0 <= r < H and 0 <= c < W) or visited[r, c]:
                    continue
                depth = max(depth, abs(r - start[0]), abs(c - start[1]))
                if self.islands[r, c] == giid and (variant == "ignore_blockers" or bl[r, c] == 0):
                    ans, depth = (r, c), max(abs(r - start[0]), abs(c - start[1]))
                    break
                visited[r, c] = True
                q.append((r, c))
        self._floods[key] = (ans, depth)
        return self._floods[key]

    def closest_adjacent(self, layer, src, tiles, variant=None):
        """n_closest_adjacent_pos: (dest or None, per tile (answer, depth), how many answers with another corner are as
        close as the winner)."""
        s = tile_for_point(self.w, self.h, src[0], src[1])
        assert s is not None
        iid = self.islands[s]
        best, best_pos, per_tile, lens = np.inf, None, [], []
        for t in tiles:
            ans, depth = self.flood(layer, t, self.islands[t] if variant == "dest_island" else iid, variant)
            per_tile.append((ans, depth))
            if ans is None:
                continue
            p = corner(self.w, self.h, *ans)
            if variant == "centres":
                p = p + np.array([-2.0, 2.0], F)
            d = _len(F(src[0] - p[0]), F(src[1] - p[1]))
            lens.append((d, tuple(p)))
            if d < best or (variant == "le" and d <= best):
                best, best_pos = d, p
        ties = len({p for d, p in lens if d == best}) - 1 if best_pos is not None else 0
        return best_pos, per_tile, ties

    def answers(self, variant=None, rows=None):
        """(query [n] u8, dest [n][2][2] f32, info per row) for every entity as a unit: what
        pfref_move_surround_queries gives, and NAVHIP_SQ_HOST where the device leaves the row to the host."""
        n = self.n
        query, dest, info = np.zeros(n, np.uint8), np.zeros((n, 2, 2), F), [None] * n
        for i in (range(n) if rows is None else rows):
            t = int(self.target[i])
            if t < 0:
                continue
            inf = info[i] = {"adjacent": False, "host": None, "tiles": [], "floods": [[], []], "ties": [0, 0]}
            if t >= n or not (self.flags[t] & MOVABLE):
                inf["host"] = "target"
            elif ntiles_of(self.radius[i]) > SQ_NT or ntiles_of(self.radius[t]) > SQ_NT:
                inf["host"] = "radius"
            elif np.isnan([*self.pos[i], *self.pos[t], self.radius[i], self.radius[t]]).any():
                inf["host"] = "nan"
            if inf["host"]:
                query[i] = SQ_HOST
                continue
            tt = self.tiles_under(self.pos[t], self.radius[t], colmajor=(variant == "colmajor"))
            ut = self.tiles_under(self.pos[i], self.radius[i])
            inf["tiles"] = tt
            if any(abs(a[0] - b[0]) <= 1 and abs(a[1] - b[1]) <= 1 for a in tt for b in ut):
                inf["adjacent"] = True
                query[i] = SQ_ADJACENT
                continue
            moved = self.pos[i] + self.vel[i]
            srcs = [moved, moved if variant == "vel_both" else self.pos[i]]
            if any(tile_for_point(self.w, self.h, *s) is None for s in srcs):
                inf["host"] = "source"
                query[i] = SQ_HOST
                continue
            layer = self.layer_of(i)
            H, W = self.cost.shape
            for c in range(2):
                p, per_tile, ties = self.closest_adjacent(layer, srcs[c], tt, variant)
                inf["floods"][c], inf["ties"][c] = per_tile, ties
                if p is not None:
                    query[i] |= SQ_HAS_DEST_0 << c
                    dest[i, c] = p
                # the device's window: a level beyond 64 needs a tile outside it pushed first
                for tile, (ans, depth) in zip(tt, per_tile):
                    far = max(tile[0], H - 1 - tile[0], tile[1], W - 1 - tile[1])
                    if (ans is not None and depth > WINDOW + 1) or (ans is None and far > WINDOW):
                        inf["host"] = "window"
            if inf["host"]:
                query[i], dest[i] = SQ_HOST, 0
        return query, dest, info

    def duplicate_flood_share(self):
        """Of the floods the device runs (one per row, target tile and distinct source island), the share that repeats
        another row's (target, layer, island)."""
        q, d, info = self.answers()
        total, seen = 0, set()
        for i, inf in enumerate(info):
            if not inf or inf["adjacent"] or inf["host"] in ("target", "radius", "nan", "source"):
                continue
            moved = self.pos[i] + self.vel[i]
            iids = {int(self.islands[tile_for_point(self.w, self.h, *s)]) for s in (moved, self.pos[i])}
            for iid in iids:
                total += len(inf["tiles"])
                seen.add((int(self.target[i]), self.layer_of(i), iid))
        distinct = sum(len(self.tiles_under(self.pos[t], self.radius[t])) for t, l, iid in seen)
        return 0.0 if not total else 1.0 - distinct / total


# ---- the worlds ------------------------------------------------------------------------------------------------------
def _disc(grid, r, c, rad, value):
    rr, cc = np.ogrid[:grid.shape[0], :grid.shape[1]]
    grid[(rr - r) ** 2 + (cc - c) ** 2 <= rad * rad] = value


class _Batch:
    """Entities collected row by row."""

    def __init__(self):
        self.pos, self.radius, self.flags, self.vel, self.target = [], [], [], [], []

    def add(self, p, radius, target=-1, vel=(0.0, 0.0), flags=MOVABLE):
        self.pos.append(np.asarray(p, F)); self.radius.append(radius); self.flags.append(flags)
        self.vel.append(vel); self.target.append(target)
        return len(self.pos) - 1

    def world(self, name, w, h, cost, blockers):
        return SWorld(name, w, h, cost, blockers, self.pos, self.radius, self.flags, self.vel, self.target)


DIRS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]


def _ring(b, t, centre, trad, dists, urad=1.0, vel_scale=0.5):
    """Units around target row t on the axes and diagonals of the target, `dists` beyond its rim."""
    for k, (dx, dz) in enumerate(DIRS):
        nrm = F(np.hypot(dx, dz))
        for j, d in enumerate(dists):
            p = centre + np.array([dx, dz], F) / nrm * F(trad + urad + d)
            # the step: along the axis, across it, or none
            v = [(dx * vel_scale, dz * vel_scale), (-dz * vel_scale, dx * vel_scale), (0.0, 0.0)][(k + j) % 3]
            b.add(p, urad, t, v)


def open_ground():
    """1 x 1 map, no blockers: targets of radius 1.0, 4.0, 6.5 and 12.0 (ceil(radius / 4) at and beside a multiple of 4), on
    a tile centre and on a tile corner; units in rings on both sides of touching."""
    b = _Batch()
    cost = np.ones((64, 64), np.uint8)
    spots = [((12, 12), 1.0, (0, 0)), ((12, 40), 4.0, (0, 0)), ((40, 12), 6.5, (0, 0)), ((42, 42), 12.0, (0, 0)),
             ((12, 26), 1.0, (2, -2)), ((26, 12), 4.0, (2, -2)), ((26, 26), 6.5, (2, 2))]
    for (r, c), rad, off in spots:
        centre = xz(1, 1, r, c, off)
        t = b.add(centre, rad)
        _ring(b, t, centre, rad, (-0.5, 1.0, 2.5, 4.5, 7.0, 11.0))
        if (r, c) == (40, 12):
            # on the bisector of the answers of tiles (r + 1, c + 2) and (r + 2, c + 1): row-major and column-major
            # order disagree on which of the two comes first
            for k in (5, 7):
                b.add(xz(1, 1, r + 1 + k, c + k), 1.0, t)
    return b.world("open_ground", 1, 1, cost, {0: np.zeros((64, 64), np.uint16)})


def on_own_blockers():
    """Targets that stand on their own blocker disc, as a stopped unit does, with blocked neighbours around them: the
    floods of the inner tiles run several levels."""
    b = _Batch()
    cost = np.ones((64, 64), np.uint8)
    bl = np.zeros((64, 64), np.uint16)
    for (r, c), rad, brad in (((20, 20), 6.5, 3), ((20, 44), 6.5, 5), ((44, 20), 12.0, 6), ((46, 46), 1.0, 2)):
        centre = xz(1, 1, r, c, (0.7, -0.4))
        _disc(bl, r, c, brad, 1)
        t = b.add(centre, rad)
        _ring(b, t, centre, rad, (3.0, 9.0, 16.0))
    for r, c in ((20, 27), (14, 44), (44, 29), (52, 20), (26, 50)):            # stopped neighbours
        _disc(bl, r, c, 2, 2)
    return b.world("on_own_blockers", 1, 1, cost, {0: bl})


def map_corner_and_edge():
    """Targets on tiles (0,0), (63,63) and (0,30) of a 1 x 1 map: the circle is cut by the map."""
    b = _Batch()
    cost = np.ones((64, 64), np.uint8)
    bl = np.zeros((64, 64), np.uint16)
    for (r, c), rad in (((0, 0), 6.5), ((63, 63), 6.5), ((0, 30), 9.0)):
        centre = xz(1, 1, r, c, (0.5, 0.5))
        _disc(bl, r, c, 2, 1)
        t = b.add(centre, rad)
        for ur, uc in ((r + 6, c), (r - 6, c), (r, c + 7), (r, c - 7), (r + 5, c + 5), (r - 5, c - 5), (r + 9, c - 3), (r - 9, c + 3)):
            if 0 <= ur < 64 and 0 <= uc < 64:
                b.add(xz(1, 1, ur, uc, (0.3, -0.2)), 1.5, t, (0.4, -0.3))
    return b.world("map_corner_and_edge", 1, 1, cost, {0: bl})


def chunk_corner():
    """A target at the meeting point of the four chunks of a 2 x 2 map, on its own blockers."""
    b = _Batch()
    cost = np.ones((128, 128), np.uint8)
    bl = np.zeros((128, 128), np.uint16)
    centre = xz(2, 2, 64, 64, (2.0, -2.0))               # the corner point itself
    _disc(bl, 64, 64, 3, 1)
    bl[60:68, 60:68] = 1
    t = b.add(centre, 12.0)
    _ring(b, t, centre, 12.0, (8.0, 20.0), urad=1.0)
    return b.world("chunk_corner", 2, 2, cost, {0: bl})


def two_islands():
    """A wall of impassable cost splits a 1 x 1 map; targets near the wall on the left, units on the right (the far side)
    and on the wall itself, some stepping across an island boundary."""
    b = _Batch()
    cost = np.ones((64, 64), np.uint8)
    cost[:, 30:33] = 255                                  # the wall: columns 30..32
    cost[40:50, 50:60] = 255                              # a block of impassable ground on the right
    bl = np.zeros((64, 64), np.uint16)
    t0 = b.add(xz(1, 1, 20, 27), 6.5)
    t1 = b.add(xz(1, 1, 44, 28, (1.0, 1.0)), 4.0)
    _disc(bl, 20, 27, 2, 1)
    for r in (10, 20, 30):
        b.add(xz(1, 1, r, 40), 1.0, t0, (0.3, 0.1))                   # the far side: another island
        b.add(xz(1, 1, r, 20), 1.0, t0, (0.3, 0.1))                   # the near side
    # on the edge of the wall: pos on the right island, pos + vel on the wall (island 0xffff), and the other way round
    b.add(xz(1, 1, 22, 33, (1.9, 0.0)), 1.0, t0, (0.3, 0.0))
    b.add(xz(1, 1, 24, 32, (-1.9, 0.0)), 1.0, t0, (-0.3, 0.0))
    b.add(xz(1, 1, 18, 29, (-1.9, 0.0)), 1.0, t1, (-0.3, 0.0))         # left island -> wall
    b.add(xz(1, 1, 44, 31), 1.0, t0, (0.0, 0.2))                      # on the wall with both sources
    b.add(xz(1, 1, 45, 55), 1.0, t1, (0.1, 0.1))                      # on the impassable block
    b.add(xz(1, 1, 50, 40), 1.0, t1, (0.2, 0.2))
    return b.world("two_islands", 1, 1, cost, {0: bl})


def nothing_reachable():
    """1 x 1 map (it fits the window): the units' island is blocked everywhere, so no flood finds a tile."""
    b = _Batch()
    cost = np.ones((64, 64), np.uint8)
    cost[:, 40:42] = 255
    bl = np.zeros((64, 64), np.uint16)
    bl[:, 42:] = 1                                        # the right island: blocked wall to wall
    t = b.add(xz(1, 1, 30, 20), 4.0)
    b.add(xz(1, 1, 30, 50), 1.0, t, (0.2, 0.0))
    b.add(xz(1, 1, 10, 60), 1.0, t, (0.0, 0.0))
    b.add(xz(1, 1, 30, 10), 1.0, t, (0.2, 0.0))           # (the left island: answered)
    return b.world("nothing_reachable", 1, 1, cost, {0: bl})


def beyond_the_window():
    """3 x 2 map: a band of blockers 141 columns wide around the target; the units' island has no free tile within 63
    tiles of the target -- those rows are the host's -- while a second target near the band's edge is answered."""
    b = _Batch()
    cost = np.ones((128, 192), np.uint8)
    bl = np.zeros((128, 192), np.uint16)
    bl[:, 26:167] = 1
    far = b.add(xz(3, 2, 64, 96), 1.0)
    near = b.add(xz(3, 2, 64, 30), 4.0)
    b.add(xz(3, 2, 64, 10), 1.0, far, (0.2, 0.0))
    b.add(xz(3, 2, 64, 180), 1.0, far, (0.0, 0.1))
    b.add(xz(3, 2, 60, 10), 1.0, near, (0.2, 0.0))
    b.add(xz(3, 2, 100, 20), 1.0, near, (0.0, 0.0))
    return b.world("beyond_the_window", 3, 2, cost, {0: bl}), (2, 3)


def two_layers():
    """Unit radii on both sides of the 1x1 / 3x3 threshold of Entity_NavLayerWithRadius (5.0), with different blocker
    planes per layer."""
    b = _Batch()
    cost = np.ones((64, 64), np.uint8)
    b0, b1 = np.zeros((64, 64), np.uint16), np.zeros((64, 64), np.uint16)
    _disc(b0, 32, 32, 3, 1)
    _disc(b1, 32, 32, 5, 1)
    b1[20:30, 40:44] = 1
    centre = xz(1, 1, 32, 32, (0.5, 0.5))
    t = b.add(centre, 6.5)
    for k, (dx, dz) in enumerate(DIRS):
        nrm = F(np.hypot(dx, dz))
        for urad in (4.9, 5.0, 1.0, 5.5):
            b.add(centre + np.array([dx, dz], F) / nrm * F(6.5 + urad + 14.0), urad, t, (0.1 * dx, -0.2 * dz))
    return b.world("two_layers", 1, 1, cost, {0: b0, 1: b1})


def bench_like(n_units, n_targets, w=4, h=4, seed=3):
    """The benchmark-like batch: n_units surround units around n_targets targets of radius 6.5 that stand on their
    blockers, on a map of w x h chunks."""
    rng = np.random.RandomState(seed)
    b = _Batch()
    cost = np.ones((h * 64, w * 64), np.uint8)
    bl = np.zeros((h * 64, w * 64), np.uint16)
    side = int(np.ceil(np.sqrt(n_targets)))
    cells = [(int((i // side + 0.5) * h * 64 / side), int((i % side + 0.5) * w * 64 / side)) for i in range(n_targets)]
    for r, c in cells:
        _disc(bl, r, c, 2, 1)
        b.add(xz(w, h, r, c, (0.6, -0.3)), 6.5)
    for i in range(n_units):
        t = i % n_targets
        ang, d = rng.uniform(0, 2 * np.pi), rng.uniform(14.0, 40.0)
        p = b.pos[t] + np.array([np.cos(ang), np.sin(ang)], F) * F(d)
        r, c = tile_for_point(w, h, *p)
        bl[r, c] += 1
        b.add(p, 1.0, t, rng.normal(0, 0.4, 2).astype(F))
    return b.world("bench_like_%d_%d" % (n_units, n_targets), w, h, cost, {0: bl})


WORLDS = {"open_ground": open_ground, "on_own_blockers": on_own_blockers, "map_corner_and_edge": map_corner_and_edge,
          "chunk_corner": chunk_corner, "two_islands": two_islands, "nothing_reachable": nothing_reachable,
          "beyond_the_window": lambda: beyond_the_window()[0], "two_layers": two_layers}
_cache = {}


def world(name):
    """The world `name`, built once (its floods are cached in it: leave it unchanged)."""
    if name not in _cache:
        _cache[name] = WORLDS[name]()
    return _cache[name]


# ---- the reference's answers for a world (needs oracle/_ref) ----------------------------------------------------------
def to_chunks(grid):
    H, W = grid.shape
    return np.ascontiguousarray(grid.reshape(H // 64, 64, W // 64, 64).transpose(0, 2, 1, 3))


def ref_nav(world):
    """The world's map in the reference: pfref.RefNav with its blockers planes."""
    from oracle import pfref
    nav = pfref.RefNav(to_chunks(world.cost), layer_mask=sum(1 << l for l in world.blockers))
    for l, b in world.blockers.items():
        nav.set_blockers(to_chunks(b), l)
    return nav


def ref_answers(world, nav=None, target=None):
    """RefMove.surround_queries for the world's batch: (query, dest [n][2][2]).  Rows whose target the reference build
    cannot take (a static target aborts there; a row >= n) are asked with no target and come back 0."""
    from oracle import pfref
    own = nav is None
    nav = ref_nav(world) if own else nav
    n = world.n
    tgt = (world.target if target is None else np.asarray(target, np.int32)).copy()
    ok = (tgt >= 0) & (tgt < n)
    ok[ok] &= (world.flags[tgt[ok]] & MOVABLE) != 0
    tgt[~ok] = -1
    state = np.where(tgt >= 0, 5, 0).astype(np.int32)
    z2 = np.zeros((n, 2), F)
    mv = pfref.RefMove(nav, world.pos, z2, world.radius, np.full(n, 20.0, F), np.full(n, 20.0, F), world.flags, state,
                       np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((1, 2), F), np.zeros(1, np.uint32))
    try:
        mv.set_surround(tgt, z2, z2)
        query, dest = mv.surround_queries(world.vel)
    finally:
        pfref.RefMove.unload()
        if own:
            nav.close()
    return query, np.asarray(dest, F).reshape(n, 2, 2)
