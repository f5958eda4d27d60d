"""tests/arrival_build_model.py held against the reference (oracle/_ref) through ctypes on its library, on the worlds of
tests/test_arrival_build_gpu.py.  The harness links M_NavRegionGeodesicDist as an abort stub, so G_Arrival_UpdateFlock is
NEVER called with an INACTIVE zone; the pieces pin the model instead: N_ClosestPathable, N_ClosestConnectedPathableTiles
(order and count), N_TileKeysForPositions, N_SegmentWithinRegion per slot and N_DestIDForPos, exported by the reference; the
two sorts through libc's own qsort with the comparators restated; the tail is tests/arrival_flock_model.py, pinned by
tests/test_arrival_flock_cpu.py.  The last test shows that each wrong model of abm.WRONG changes bits.  No GPU."""
import ctypes as C
import ctypes.util
import time

import numpy as np
import pytest

from oracle import pfref
from tests import arrival_build_model as abm
from tests import arrival_build_worlds as bw
from tests.test_arrival_flock_cpu import Vec2, Vec3

pytestmark = pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")

F = np.float32
_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = pfref.lib()
        L.pfref_nav_private.restype = C.c_void_p
        L.pfref_nav_private.argtypes = [C.c_void_p]
        L.N_ClosestPathable.restype = C.c_bool
        L.N_ClosestPathable.argtypes = [C.c_void_p, C.c_int, Vec3, Vec2, C.POINTER(Vec2)]
        L.N_ClosestConnectedPathableTiles.restype = C.c_int
        L.N_ClosestConnectedPathableTiles.argtypes = [C.c_void_p, C.c_int, Vec3, Vec2, C.c_void_p, C.c_int, C.c_float]
        L.N_TileKeysForPositions.restype = C.c_size_t
        L.N_TileKeysForPositions.argtypes = [C.c_void_p, Vec3, C.c_void_p, C.c_size_t, C.c_void_p]
        L.N_SegmentWithinRegion.restype = C.c_bool
        L.N_SegmentWithinRegion.argtypes = [C.c_void_p, Vec3, Vec2, Vec2, C.c_void_p, C.c_size_t]
        L.N_DestIDForPos.restype = C.c_uint32
        L.N_DestIDForPos.argtypes = [C.c_void_p, Vec3, Vec2, C.c_int]
        _bound = L
    return _bound


def v2(p):
    return Vec2(float(p[0]), float(p[1]))


class Ref:
    """The reference's nav state of a world: its base cost, its blockers per layer."""

    def __init__(self, W):
        self.nav = pfref.RefNav(W.cost[min(W.cost)], layer_mask=sum(1 << l for l in W.blockers))
        for layer, b in W.blockers.items():
            self.nav.set_blockers(b, layer)
        self.priv = _lib().pfref_nav_private(self.nav._h)
        self.mp = Vec3(*[float(v) for v in self.nav.map_pos])
        self.seconds_in_the_reference = 0.0                                  # (scripts/bench_arrival_build.py reads it)

    def close(self):
        self.nav.close()

    def timed(self, fn, *args):
        t0 = time.perf_counter()
        r = fn(*args)
        self.seconds_in_the_reference += time.perf_counter() - t0
        return r

    def closest_pathable(self, layer, p):
        out = Vec2(0, 0)
        ok = self.timed(_lib().N_ClosestPathable, self.priv, layer, self.mp, v2(p), C.byref(out))
        return (F(out.x), F(out.z)) if ok else (F(p[0]), F(p[1]))

    def connected(self, layer, centre, maxout):
        out = np.zeros((maxout + 1, 2), F)
        n = self.timed(_lib().N_ClosestConnectedPathableTiles, self.priv, layer, self.mp, v2(centre), out.ctypes.data_as(C.c_void_p), maxout, 0.0)
        return out[:n]

    def keys(self, positions):
        q = np.ascontiguousarray(positions, F).reshape(-1, 2)
        out = np.zeros(len(q) + 1, np.uint64)
        n = self.timed(_lib().N_TileKeysForPositions, self.priv, self.mp, q.ctypes.data_as(C.c_void_p), len(q), out.ctypes.data_as(C.c_void_p))
        return out[:n]

    def segment(self, a, b, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        return bool(self.timed(_lib().N_SegmentWithinRegion, self.priv, self.mp, v2(a), v2(b), keys.ctypes.data_as(C.c_void_p), len(keys)))

    def dest_id(self, p, layer):
        return int(self.timed(_lib().N_DestIDForPos, self.priv, self.mp, v2(p), layer))


def built(name):
    W, want = bw.world(name)
    return W, [(i, r) for i, r in enumerate(want) if r["status"] == 0]


@pytest.mark.parametrize("name", sorted(bw.WORLDS))
def test_premises_of_every_world(name):
    W, want = bw.world(name)
    bw.premises(name, W, want)


@pytest.mark.parametrize("name", sorted(bw.WORLDS))
def test_exported_nav_functions(name):
    """Centre, flood order and count, keys, the clear-line test of every thinned slot, com and its dest id."""
    W, zones = built(name)
    R = Ref(W)
    assert tuple(R.nav.map_pos[[0, 2]]) == (W.map.mx, W.map.mz)
    for i, r in zones:
        layer, p = W.zones[i]["arg_layer"], r["parts"]
        centre = R.closest_pathable(layer, W.targets[i])
        assert np.array_equal(F(centre).view(np.uint32), r["zone"]["centre_xz"].view(np.uint32)), (name, i)
        flood = R.connected(layer, centre, p["area"])
        assert flood.shape == p["flood"].shape and np.array_equal(flood.view(np.uint32), p["flood"].view(np.uint32)), (name, i)
        assert np.array_equal(R.keys(flood), r["keys"]), (name, i)
        clear = [R.segment(centre, s, r["keys"]) for s in p["thinned"]]
        assert clear == p["clear"].tolist(), (name, i)
        com = abm.centre_of_mass(p["kept"])
        snapped = R.closest_pathable(layer, com)
        assert np.array_equal(F(snapped).view(np.uint32), r["com"].view(np.uint32)), (name, i)
        assert R.dest_id(snapped, layer) == r["com_dest_id"], (name, i)
    R.close()


class Sorter:
    """libc's qsort on vec2 records with the two comparators of arrival.c restated (:118, :130)"""

    def __init__(self):
        self.libc = C.CDLL(ctypes.util.find_library("c"))
        self.CMP = C.CFUNCTYPE(C.c_int, C.POINTER(Vec2), C.POINTER(Vec2))

    def sort(self, slots, cmp):
        arr = (Vec2 * len(slots))(*[Vec2(float(s[0]), float(s[1])) for s in slots])
        self.libc.qsort(arr, len(slots), C.sizeof(Vec2), self.CMP(cmp))
        return np.array([(a.x, a.z) for a in arr], F).reshape(-1, 2)

    def near_ref(self, slots, ref):
        def key(p):
            dx, dz = F(F(p[0].x) - ref[0]), F(F(p[0].z) - ref[1])
            return F(F(dx * dx) + F(dz * dz))
        return self.sort(slots, lambda a, b: int(key(a) > key(b)) - int(key(a) < key(b)))

    def far_banded(self, slots, centre, axis, band_w):
        def keys(p):
            b, l = abm.band_keys(np.array([[p[0].x, p[0].z]], F), centre, axis, band_w)
            return int(b[0]), l[0]

        def cmp(a, b):
            (ba, la), (bb, lb) = keys(a), keys(b)
            if ba != bb:
                return int(ba < bb) - int(ba > bb)
            return int(la > lb) - int(la < lb)
        return self.sort(slots, cmp)


@pytest.mark.parametrize("name", ["open", "walls", "edges", "gate", "window"])
def test_libc_qsort_gives_the_models_stable_orders(name):
    W, zones = built(name)
    S = Sorter()
    for i, r in zones:
        p, z = r["parts"], r["zone"]
        if len(p["flood"]) == 0:
            continue
        fwd = F(8)
        ref = (F(z["centre_xz"][0] + F(r["axis"][0] * fwd)), F(z["centre_xz"][1] + F(r["axis"][1] * fwd)))
        got = S.near_ref(p["flood"], ref)
        assert np.array_equal(got.view(np.uint32), p["flood"][p["near_order"]].view(np.uint32)), (name, i)
        got = S.far_banded(p["kept"], z["centre_xz"], r["axis"], z["row_height"])
        assert np.array_equal(got.view(np.uint32), z["slots_xz"].view(np.uint32)), (name, i)


def test_flood_from_a_blocked_centre_tile():
    """N_ClosestPathable never leaves the centre on a blocked tile next to open ones, so no zone shows that the centre
    tile is pushed even when blocked (nav.c:4221); the flood itself does, started on the blocked target."""
    W, want = bw.world("walls")
    i = W.names["blocked_target"]
    R = Ref(W)
    t = W.p(19, 20, (0.5, 0.5))                                          # a rim tile of the blocked block
    assert i >= 0 and W.map.tile_blocked(0, *W.map.abs_tile(*t))
    tiles = abm.connected_tiles(W.map, 0, t[0], t[1], 60)
    flood = np.array([W.map.centre_of(r, c) for r, c in tiles], F).reshape(-1, 2)
    assert len(tiles) == 60 and np.array_equal(R.connected(0, t, 60).view(np.uint32), flood.view(np.uint32))
    assert abm.connected_tiles(W.map, 0, t[0], t[1], 60, wrong="centre_not_pushed") == []
    R.close()


def test_ordered_sum_against_a_tree_on_positions_off_the_tile_grid():
    """The slots are tile centres, integers on these maps: their float sums are exact in any order, so no zone tells the
    ordered sum of arrival.c:819-823 from a tree.  The variant itself differs as soon as the addends are not integers."""
    rng = np.random.RandomState(3)
    p = (rng.uniform(-250, 250, (300, 2))).astype(F)
    a, b = abm.centre_of_mass(p), abm.centre_of_mass(p, "pairwise_com")
    assert F(a[0]).view(np.uint32) != F(b[0]).view(np.uint32) or F(a[1]).view(np.uint32) != F(b[1]).view(np.uint32)


def test_libc_qsort_keeps_ties_of_the_banded_comparator_in_order():
    """No built zone has two slots that tie in slot_cmp_far_banded (arrival_build_worlds.premises says why), so the contract
    "ties keep the order the filter left" is held on hand-made lists: duplicates and slots that differ along the axis by
    less than a band, 5 to 300 records, libc's qsort against the model's stable order."""
    S = Sorter()
    rng = np.random.RandomState(11)
    centre, axis, band_w = np.array([10.0, -6.0], F), (F(0), F(1)), F(4.625)
    for n in (5, 64, 300):
        base = (rng.randint(-6, 7, (n // 3 + 1, 2)) * 2).astype(F)
        slots = base[rng.randint(0, len(base), n)] + centre
        slots[:, 1] += (np.arange(n) % 2).astype(F)                           # same band, same lateral key, another record
        band, lat = abm.band_keys(slots, centre, axis, band_w)
        assert len(set(zip(band.tolist(), lat.tolist()))) < n                 # ties
        want = abm.far_near(slots, centre, axis, band_w)
        assert np.array_equal(S.far_banded(slots, centre, axis, band_w).view(np.uint32), want.view(np.uint32)), n
        wrong = abm.far_near(slots, centre, axis, band_w, "unstable_sort")
        assert n < 64 or not np.array_equal(wrong.view(np.uint32), want.view(np.uint32))


def test_the_heap_of_the_kernel_at_a_small_capacity():
    """csrc/pq_heap.h itself, compiled for the host, against the model's heap on random scripts with heavy ties, and the
    refusal of the push that would exceed the capacity -- the path behind NAVHIP_AB_HOST "a heap that outgrows its LDS",
    which no world reaches: every node in the heap is an open tile next to a popped one and not nearer than the pop in
    progress (a nearer push is popped before anything else), i.e. a tile of a ring about two tiles deep around the
    popped region, and inside the window of 255 x 255 tiles such a ring holds some 2 * pi * 180 * 2 < 2 300 tiles at the
    very most against 4 096 nodes; the worlds' peaks are asserted in arrival_build_worlds.premises (32 to a few hundred)."""
    import os
    import subprocess
    from tests import hostsim
    lib_path = os.path.join(hostsim.HERE, "_pq_heap_sim.so")
    src = os.path.join(hostsim.HERE, "pq_heap_sim.cpp")
    hdr = os.path.join(hostsim.CSRC, "pq_heap.h")
    if not os.path.exists(lib_path) or os.path.getmtime(lib_path) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + hostsim.CSRC, src, "-o", lib_path])
    L = C.CDLL(lib_path)
    rng = np.random.RandomState(4)
    cap = 16
    for trial in range(20):
        n = 400
        ops = np.where(rng.rand(n) < 0.58, np.arange(n), -1).astype(np.int32)
        prio = rng.randint(0, 6, n).astype(F)                                 # ties everywhere
        out = np.zeros(n, np.int32)
        node_prio, node_data = np.zeros(cap + 2, F), np.zeros(cap + 2, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
        size = L.pq_heap_script(cap, n, p(ops), p(prio), p(out), p(node_prio), p(node_data))
        H, want, refused = abm.Heap(), [], 0
        for i in range(n):
            if ops[i] >= 0:
                fits = H.size + 1 <= cap
                refused += not fits
                if fits:
                    H.push(prio[i], int(ops[i]))
                want.append(int(fits))
            else:
                want.append(H.pop() if H.size > 0 else -1)
        assert out.tolist() == want and size == H.size, trial
        assert refused > 0 and H.peak == cap


# "centre_not_pushed" and "pairwise_com" cannot change the bits of a built zone: N_ClosestPathable never leaves the centre on
# a blocked tile while an open one exists, and the slots are tile centres -- integers on these maps -- whose float sums are
# exact in any order.  test_flood_from_a_blocked_centre_tile and
# test_ordered_sum_against_a_tree_on_positions_off_the_tile_grid show them on the functions instead.
@pytest.mark.parametrize("wrong", [w for w in abm.WRONG if w not in ("centre_not_pushed", "pairwise_com")])
def test_wrong_models_change_bits(wrong):
    changed = 0
    for name in ("open", "walls", "edges"):
        W, want = bw.world(name)
        for i, r in enumerate(want):
            if r["status"] != 0:
                continue
            bad = abm.build_zone(W.map, W.zones[i], W.pos, W.members[i], W.targets[i], wrong=wrong)
            same = (bad["status"] == 0 and np.array_equal(bad["zone"]["slots_xz"].view(np.uint32), r["zone"]["slots_xz"].view(np.uint32))
                    and np.array_equal(bad["keys"], r["keys"]) and np.array_equal(bad["com"].view(np.uint32), r["com"].view(np.uint32))
                    and np.array_equal(bad["zone"]["slot_ring"], r["zone"]["slot_ring"]))
            changed += not same
    assert changed > 0, wrong
