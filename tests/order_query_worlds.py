"""The worlds and the rows of the order-query tests (tests/test_order_queries_cpu.py, tests/test_order_queries_gpu.py):
cost grids per layer -- islands made by impassable walls, impassable blobs, a lake wider than the device's window -- and,
per case, the rows asked.  Data only: the islands come from the reference's own plane, the premises from the model.

A row is (src xz, dst xz, range, layer, faction, flags), made into records by order_query_model.make_queries."""
import numpy as np

from tests import order_query_model as om
from tests import surround_model as sm

IR, RE = om.OQ_IN_RANGE, om.OQ_REACHABLE
NONE = om.FACTION_NONE


def _disc(grid, r, c, rad, value):
    rr, cc = np.ogrid[:grid.shape[0], :grid.shape[1]]
    grid[(rr - r) ** 2 + (cc - c) ** 2 <= rad * rad] = value


class OWorld:
    def __init__(self, name, w, h, costs, blockers=None):
        self.name, self.w, self.h, self.costs, self.blockers = name, w, h, costs, blockers or {}
        self.cases = {}           # case name -> rows

    def xz(self, r, c, off=(0.0, 0.0)):
        return sm.xz(self.w, self.h, r, c, off)

    def corner(self, r, c):
        return sm.corner(self.w, self.h, r, c)

    def rows(self):
        return [row for rows in self.cases.values() for row in rows]


# ---- 2 x 2 chunks (128 x 128 tiles) ---------------------------------------------------------------------------------------
# layer 0: a wall along columns 60-61 (islands WEST and EAST), a walled ROOM in the east, a round blob in the west, an
#          L-shaped block in the east (its short arm keeps the flood of a click inside it from the nearest edge)
# layer 2: a wall along rows 70-71 (islands NORTH and SOUTH) and a round blob on the chunk border below it
# blockers of layer 0: the WEST tiles along the wall between rows 35 and 45
ROOM = (88, 112)
BLOB_A, BLOB_L2 = ((30, 30), 6), ((100, 64), 5)
LBLOCK_CLICK = (36, 93)
TARGET = (64, 30)                 # the in-range target of the plain cases, WEST


def small():
    c0 = np.ones((128, 128), np.uint8)
    c0[:, 60:62] = 255
    a, b = ROOM
    c0[a:b + 1, a] = c0[a:b + 1, b] = 255
    c0[a, a:b + 1] = c0[b, a:b + 1] = 255
    _disc(c0, *BLOB_A[0], BLOB_A[1], 255)
    c0[20:41, 90:111] = 255
    c0[24:41, 86:90] = 255
    c2 = np.ones((128, 128), np.uint8)
    c2[70:72, :] = 255
    _disc(c2, *BLOB_L2[0], BLOB_L2[1], 255)
    b0 = np.zeros((128, 128), np.uint16)
    b0[35:46, 59] = 2
    W = OWorld("small", 2, 2, {0: c0, 2: c2}, {0: b0})
    xz = W.xz
    west, east, room = xz(10, 10, (0.7, -1.1)), xz(10, 100, (-0.3, 0.9)), xz(100, 100, (1.0, 1.0))
    north, south = xz(10, 10, (0.7, -1.1)), xz(100, 20, (0.2, 0.4))

    # 1. same island: the destination comes back bit for bit
    rows = []
    for faction in (0, 7, 14, NONE):
        for flags, rng in ((0, 0.0), (RE, 0.0), (IR | RE, 10.0)):
            rows.append((west, xz(50, 40, (1.3, -0.7)), rng, 0, faction, flags))
            rows.append((north, xz(50, 100, (1.3, -0.7)), rng, 2, faction, flags))
    W.cases["same_island"] = rows
    # 2. a click on a blob and on another island; a source on an impassable tile (island 0xffff)
    W.cases["blob_and_other_island"] = [
        (west, xz(*BLOB_A[0]), 0.0, 0, NONE, RE), (west, xz(32, 28, (0.5, 0.5)), 0.0, 0, 3, RE),
        (west, xz(40, 70), 0.0, 0, NONE, RE), (west, xz(64, 66, (-1.0, 1.0)), 0.0, 0, NONE, RE),
        (room, xz(100, 50), 0.0, 0, NONE, RE), (room, xz(80, 100), 0.0, 0, 5, RE),
        (xz(*BLOB_A[0]), xz(50, 40), 0.0, 0, NONE, RE), (xz(*BLOB_A[0]), xz(29, 31), 0.0, 0, NONE, RE),
        (east, xz(*LBLOCK_CLICK), 0.0, 0, NONE, RE), (east, xz(38, 96), 0.0, 0, NONE, RE), (west, xz(100, 100), 0.0, 0, NONE, RE),
    ]
    # ... clicks whose first hit in queue order is not the Euclidean-nearest tile of the source's island
    W.cases["queue_order"] = [(west, xz(28, 30), 0.0, 0, NONE, RE), (east, xz(27, 97), 0.0, 0, NONE, RE), (west, xz(26, 28), 0.0, 0, NONE, RE)]
    # ... sources on grid points from which two tiles of the circle are equally far
    W.cases["ties"] = [(W.corner(35, 2), xz(*TARGET), 17.0, 0, NONE, IR), (W.corner(36, 57), xz(*TARGET), 17.0, 0, NONE, IR | RE),
                       (W.corner(30, 18), xz(*TARGET), 60.0, 0, NONE, IR), (W.corner(37, 2), xz(*TARGET), 17.0, 0, 6, IR)]
    # 3. the nearest tile of the source's island holds a blocker
    W.cases["blocker"] = [(xz(40, 10), xz(40, 66), 0.0, 0, NONE, RE), (xz(40, 10), xz(38, 64, (1.0, 0.0)), 0.0, 0, 1, RE)]
    # 4. chunk corners, map edges and corners, floods across a chunk border
    W.cases["borders"] = [
        (south, xz(63, 63), 0.0, 2, NONE, RE), (south, xz(64, 64), 0.0, 2, NONE, RE), (south, xz(63, 64), 0.0, 2, NONE, RE),
        (south, xz(60, 0), 0.0, 2, NONE, RE), (south, xz(60, 127), 0.0, 2, NONE, RE), (north, xz(127, 0), 0.0, 2, NONE, RE),
        (east, xz(0, 0), 0.0, 0, NONE, RE), (east, xz(127, 0), 0.0, 0, NONE, RE), (south, xz(0, 64, (2.0, -2.0)), 0.0, 2, NONE, 0),
        (xz(120, 10), xz(*BLOB_L2[0]), 0.0, 2, NONE, RE), (north, xz(101, 63), 0.0, 2, NONE, RE),
    ]
    # 6. in range, plain: sources on all sides; a source on a grid point (ties); a target two tiles from the map's edge
    sources = [xz(20, 30, (0.7, -1.1)), xz(110, 30, (0.3, 0.3)), xz(64, 50, (-0.9, 0.1)), xz(64, 5, (1.9, 1.9)), xz(30, 8), W.corner(40, 30)]
    rows = []
    for rng in (0.5, 4.0, 4.01, 17.0, 60.0):
        for i, s in enumerate(sources):
            rows.append((s, xz(*TARGET, (0.4, -0.9)), rng, 0, NONE, IR if i % 2 else IR | RE))
    rows += [(xz(40, 30, (0.7, 0.2)), xz(2, 30), 17.0, 0, NONE, IR), (xz(40, 100), xz(125, 100, (0.5, 0.5)), 17.0, 0, 2, IR | RE),
             (W.corner(64, 10), xz(*TARGET), 17.0, 0, NONE, IR), (W.corner(40, 30), xz(*TARGET), 17.0, 0, NONE, IR),
             (W.corner(47, 13), xz(*TARGET), 17.0, 0, NONE, IR), (W.corner(64, 30), xz(*TARGET), 60.0, 0, NONE, IR),
             # (a target half a unit from its tile's edge: the circle reaches the outermost ring of the box)
             (xz(20, 30, (0.7, -1.1)), xz(*TARGET, (0.0, -1.5)), 17.0, 0, NONE, IR)]
    W.cases["in_range"] = rows
    # 8. negative and zero ranges
    rows = []
    for rng in (-0.0, -2.0, -3.99, -4.0, -50.0):
        rows.append((xz(20, 30, (0.7, -1.1)), xz(*TARGET, (0.4, -0.9)), rng, 0, NONE, IR))
        rows.append((xz(20, 30, (0.7, -1.1)), xz(40, 100), rng, 0, NONE, IR | RE))
    W.cases["small_ranges"] = rows
    # 9. no tile of the source's island within range: the target, then (REACHABLE) onto the source's island
    W.cases["no_tile"] = [(xz(40, 10), xz(40, 100), 20.0, 0, NONE, IR), (xz(40, 10), xz(40, 100), 20.0, 0, 4, IR | RE),
                          (room, xz(100, 40), 33.0, 0, NONE, IR | RE), (south, xz(20, 64), 60.0, 2, NONE, IR | RE)]
    return W


# ---- 3 x 3 chunks (192 x 192 tiles) ---------------------------------------------------------------------------------------
# layer 0: a lake of 131 x 131 impassable tiles (wider than the window of 127), a walled-off CORNER
# layer 1: a wall along rows 96-97 (NORTH and SOUTH)
LAKE = (30, 160)
CAP_TARGET = (90, 96)


def big():
    c0 = np.ones((192, 192), np.uint8)
    c0[LAKE[0]:LAKE[1] + 1, LAKE[0]:LAKE[1] + 1] = 255
    c0[0:26, 170:172] = 255
    c0[25:27, 170:192] = 255
    c1 = np.ones((192, 192), np.uint8)
    c1[96:98, :] = 255
    _disc(c1, 60, 96, 4, 255)
    W = OWorld("big", 3, 3, {0: c0, 1: c1})
    xz = W.xz
    land = xz(10, 10, (0.7, -1.1))
    # 5. the lake: the nearest land 63 tiles away is answered, 64 tiles away is the host's
    W.cases["lake"] = [(land, xz(92, 92), 0.0, 0, NONE, RE), (land, xz(93, 93), 0.0, 0, NONE, RE), (land, xz(95, 97), 0.0, 0, NONE, RE),
                       (land, xz(40, 150), 0.0, 0, 2, RE), (xz(10, 180), xz(50, 185), 0.0, 0, NONE, RE), (land, xz(93, 92), 0.0, 0, NONE, RE)]
    # 7. in range at the cap of 2048 tiles: sources north and south of the target
    rows = []
    for rng in (120.0, 126.0, 128.0):
        rows.append((xz(20, 96, (0.7, -1.1)), xz(*CAP_TARGET, (0.4, -0.9)), rng, 1, NONE, IR))
        rows.append((xz(170, 96, (0.7, -1.1)), xz(*CAP_TARGET, (0.4, -0.9)), rng, 1, NONE, IR | RE))
    W.cases["cap"] = rows
    return W


def small_walled():
    """small() with one more wall on layer 0: the WEST island cut in two along rows 80-81."""
    W = small()
    W.name = "small_walled"
    W.costs[0] = W.costs[0].copy()
    W.costs[0][80:82, 0:60] = 255
    W.cases = {"after_upload": [(W.xz(10, 10), W.xz(100, 30), 0.0, 0, NONE, RE), (W.xz(10, 10), W.xz(50, 40), 0.0, 0, NONE, RE),
                                (W.xz(100, 10), W.xz(64, 30), 30.0, 0, NONE, IR | RE), (W.xz(10, 10), W.xz(86, 30), 30.0, 0, NONE, IR)]}
    return W


WORLDS = {"small": small, "big": big, "small_walled": small_walled}
