"""A plain numpy / Python restatement of the five nav functions behind navhip_order_queries, written from the reference's
nav.c / tile.c: N_ClosestReachableInRange (nav.c:5067) over M_Tile_AllUnderCircle (tile.c:687) -- a literal double loop --,
N_ClosestReachableDest (nav.c:4085) over n_closest_island_tiles (nav.c:1226) with maxout = 1 -- a literal FIFO queue and a
visited array --, N_LocationsReachable (nav.c:4593), N_DestIDForPos / N_DestIDForPosAttacking (nav.c:3367, :3376, :839).
Floats are np.float32 operation by operation.  The geometry every query model shares (the tile of a point, the circle test)
is tests/surround_model.py's.  tests/test_order_queries_cpu.py pins every function to the reference's own.

`wrong` names ONE deliberate mistake (the CPU test shows that each changes bits on some row):
    "blockers"  "euclid"  "nocap"  "le"  "centre_in_range"  "corner_reachable"  "floor"  "dest_island"
"""
import collections
import math

import numpy as np

from tests import surround_model as sm

F = np.float32
OQ_IN_RANGE, OQ_REACHABLE = 1, 2
OQ_SAME_ISLAND, OQ_NO_TILE, OQ_HOST = 1, 2, 0x80
FACTION_NONE = 15
CAP = 2048                # the reference's tds[2048], nav.c:5090
NT_MAX = 32               # ceil(range / 4) the entry points take
WINDOW = 63               # Chebyshev radius of the device's flood window
WRONG = ("blockers", "euclid", "nocap", "le", "centre_in_range", "corner_reachable", "floor", "dest_island")
QUERY_DTYPE = np.dtype([("src_x", F), ("src_z", F), ("dst_x", F), ("dst_z", F), ("range", F), ("layer", np.int32),
                        ("faction", np.int32), ("flags", np.uint32)])


def ntiles_of(rng, wrong=None):
    v = float(F(rng) / F(4))
    return int(math.floor(v) if wrong == "floor" else math.ceil(v))


class Model:
    """islands: {layer: [rows][cols] uint16 global island ids}; blockers: {layer: grid} (read by the wrong model only)."""

    def __init__(self, w, h, islands, blockers=None, wrong=None):
        assert wrong is None or wrong in WRONG
        self.w, self.h, self.islands, self.blockers, self.wrong = w, h, islands, blockers or {}, wrong
        self.rows, self.cols = h * 64, w * 64
        self.mx, self.mz = sm.map_pos(w, h)

    def tile(self, p):
        return sm.tile_for_point(self.w, self.h, p[0], p[1])

    # -- M_Tile_AllUnderCircle ------------------------------------------------------------------------------------------
    def under_circle(self, centre, rng, cap=CAP):
        """The tiles in the reference's order, at most `cap`; ([], 0) for a centre off the map."""
        t = self.tile(centre)
        if t is None:
            return []
        nt = ntiles_of(rng, self.wrong)
        out = []
        for dr in range(-nt, nt + 1):
            for dc in range(-nt, nt + 1):
                r, c = t[0] + dr, t[1] + dc
                if not (0 <= r < self.rows and 0 <= c < self.cols):
                    continue
                if not sm.circle_hits_tile(self.w, self.h, centre[0], centre[1], rng, r, c):
                    continue
                out.append((r, c))
                if len(out) == cap:
                    return out
        return out

    # -- N_ClosestReachableInRange --------------------------------------------------------------------------------------
    def in_range(self, layer, src, target, rng):
        """(xz, info): info["no_tile"], ["n_tiles"] the circle's tiles in front of the cap, ["winner"] the tile, ["ties"] how
        many tiles of the source's island share the winning length."""
        isl = self.islands[layer]
        s = self.tile(src)
        iid = isl[self.tile(target)] if self.wrong == "dest_island" else isl[s]
        tiles = self.under_circle(target, rng, cap=1 << 30 if self.wrong == "nocap" else CAP)
        best, pos, winner, lens = F(np.inf), None, None, []
        for r, c in tiles:
            if isl[r, c] != iid:
                continue
            if self.wrong == "centre_in_range":
                p = np.array([self.mx - F(F(c) + F(0.5)) * F(4), self.mz + F(F(r) + F(0.5)) * F(4)], F)
            else:
                p = np.array([self.mx - F(c) * F(4), self.mz + F(r) * F(4)], F)
            d = sm._len(F(src[0]) - p[0], F(src[1]) - p[1])
            lens.append(d)
            if (d <= best) if self.wrong == "le" else (d < best):
                best, pos, winner = d, p, (r, c)
        info = {"no_tile": pos is None, "n_tiles": len(tiles), "winner": winner,
                "ties": sum(1 for d in lens if d == best)}
        if pos is None:
            return np.array([F(target[0]), F(target[1])], F), info
        return pos, info

    # -- n_closest_island_tiles(start, iid, ignore_blockers = true, maxout = 1) ------------------------------------------
    def flood_first(self, layer, start, iid):
        """The first hit in queue order, or None: a literal FIFO queue over a visited array of the whole map."""
        isl = self.islands[layer]
        blk = self.blockers.get(layer)
        if self.wrong == "euclid":
            rr, cc = np.nonzero(isl == iid)
            if len(rr) == 0:
                return None
            k = np.lexsort((cc, rr, (rr - start[0]) ** 2 + (cc - start[1]) ** 2))[0]
            return int(rr[k]), int(cc[k])
        visited = np.zeros((self.rows, self.cols), bool)
        visited[start] = True
        queue = collections.deque([start])
        while queue:
            cr, cc = queue.popleft()
            for dr, dc in sm.DELTAS8:
                r, c = cr + dr, cc + dc
                if not (0 <= r < self.rows and 0 <= c < self.cols) or visited[r, c]:
                    continue
                skip = isl[r, c] != iid
                if self.wrong == "blockers" and blk is not None and blk[r, c] > 0:
                    skip = True
                if not skip:
                    return r, c
                visited[r, c] = True
                queue.append((r, c))
        return None

    # -- N_ClosestReachableDest -----------------------------------------------------------------------------------------
    def reachable(self, layer, src, dst):
        """(xz, info): info["tile"] the flood's answer (None: no flood, or no hit), ["depth"] its Chebyshev distance from
        the start, ["host"] the device leaves the row to the host (the answer lies outside its window)."""
        isl = self.islands[layer]
        s, t = self.tile(src), self.tile(dst)
        info = {"tile": None, "depth": 0, "host": False, "start": t}
        if isl[s] == isl[t]:
            return np.array([F(dst[0]), F(dst[1])], F), info
        a = self.flood_first(layer, t, isl[s])
        if a is None:
            return np.array([F(src[0]), F(src[1])], F), info
        info["tile"], info["depth"] = a, max(abs(a[0] - t[0]), abs(a[1] - t[1]))
        info["host"] = info["depth"] > WINDOW
        if self.wrong == "corner_reachable":
            return np.array([self.mx - F(a[1]) * F(4), self.mz + F(a[0]) * F(4)], F), info
        return np.array([self.mx - F(F(a[1]) + F(0.5)) * F(4), self.mz + F(F(a[0]) + F(0.5)) * F(4)], F), info

    def locations_reachable(self, layer, a, b):
        isl = self.islands[layer]
        return bool(isl[self.tile(a)] == isl[self.tile(b)])

    def dest_id(self, p, layer, faction=FACTION_NONE):
        r, c = self.tile(p)
        return ((r >> 6) << 26) | ((c >> 6) << 20) | ((r & 63) << 14) | ((c & 63) << 8) | ((layer & 15) << 4) | (faction & 15)

    # -- one row of navhip_order_queries --------------------------------------------------------------------------------
    def row(self, q):
        """(dest [2] float32, dest id, status, info) of one QUERY_DTYPE record."""
        layer, flags = int(q["layer"]), int(q["flags"])
        src, dst = (F(q["src_x"]), F(q["src_z"])), (F(q["dst_x"]), F(q["dst_z"]))
        status = OQ_SAME_ISLAND if self.locations_reachable(layer, src, dst) else 0
        info = {"in_range": None, "reachable": None}
        t = np.array(dst, F)
        if flags & OQ_IN_RANGE:
            t, info["in_range"] = self.in_range(layer, src, dst, F(q["range"]))
            if info["in_range"]["no_tile"]:
                status |= OQ_NO_TILE
        d = t
        if flags & OQ_REACHABLE:
            d, info["reachable"] = self.reachable(layer, src, t)
            if info["reachable"]["host"]:
                return np.array([np.nan, 0.0], F), 0, OQ_HOST, info
        return d, self.dest_id(d, layer, int(q["faction"])), status, info


def make_queries(rows):
    """rows: (src xz, dst xz, range, layer, faction, flags) -> QUERY_DTYPE records."""
    q = np.zeros(len(rows), QUERY_DTYPE)
    for i, (src, dst, rng, layer, faction, flags) in enumerate(rows):
        q[i] = (src[0], src[1], dst[0], dst[1], rng, layer, faction, flags)
    return q
