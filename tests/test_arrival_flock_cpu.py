"""tests/arrival_flock_model.py held against the reference (oracle/_ref) through ctypes on its library, on the worlds of
tests/test_arrival_flock_gpu.py.  arrival_realloc_slots is static and the harness links M_NavRegionGeodesicDist as an abort
stub, so the reference cannot run the rule for a zone that re-orients; three pieces pin the model instead:
  * N_RegionGeodesicDist (nav.c:4389, exported) for the flood, the source key and the slot distances of every world;
  * N_PositionBlocked and N_TileKeysForPositions for the blocked test and the keys;
  * G_Arrival_UpdateFlock ITSELF, with a hand-filled struct arrival_state and the pfref_nav* as its map, for zones whose
    fill_frac >= 0.25 and whose phase is FILLING -- the path that calls only M_NavPositionBlocked, M_NavSegmentWithinRegion
    and M_NavGetResolution -- bit for bit over at least 8 consecutive calls per zone.  It is NEVER called with fill_frac <
    0.25 or phase INACTIVE (ref_update asserts both).
The last test shows that each wrong model of afm.WRONG changes bits on these worlds.  No GPU."""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import pfref
from tests import arrival_flock_model as afm
from tests import arrival_flock_worlds as aw
from tests import test_arrival_flock_gpu as worlds

pytestmark = pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")

F = np.float32
CAP = afm.MAX_SLOTS


class Vec2(C.Structure):
    _fields_ = [("x", C.c_float), ("z", C.c_float)]


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class ArrivalState(C.Structure):
    """struct arrival_state, arrival.h:66"""
    _fields_ = [("phase", C.c_int), ("layer", C.c_int), ("centre", Vec2), ("axis", Vec2), ("com", Vec2), ("com_dest_id", C.c_uint32),
                ("radius", C.c_uint16), ("unit_radius", C.c_float), ("num_slots", C.c_int), ("active_row", C.c_int),
                ("realloc_counter", C.c_int), ("stall_counter", C.c_int), ("prev_occ", C.c_int), ("fill_frac", C.c_float),
                ("num_rows", C.c_int), ("row_height", C.c_float), ("slots", Vec2 * CAP), ("slot_ring", C.c_int * CAP),
                ("num_region", C.c_int), ("region_keys", C.c_uint64 * CAP)]


class UnitState(C.Structure):
    """struct arrival_unit_state, arrival.h:105"""
    _fields_ = [("substate", C.c_int), ("sink_valid", C.c_bool), ("sink", Vec2), ("stuck", C.c_int), ("progress_anchor", Vec2),
                ("progress_anchored", C.c_bool), ("los_latched", C.c_bool), ("los_hyst", C.c_int), ("order_pos", Vec2)]


class Member(C.Structure):
    """struct arrival_member, arrival.h:130"""
    _fields_ = [("pos", Vec2), ("settled", C.c_bool), ("layer", C.c_int), ("radius", C.c_float), ("us", C.POINTER(UnitState))]


def check_layouts():
    """The offsets arrival.h gives by the C rules (4-byte ints, enums and floats, 8-byte vec2_t of 4-byte alignment, a
    uint16_t padded to the float behind it, uint64_t keys on 8): derived by hand, held against the mirror."""
    scalars = 4 + 4 + 8 + 8 + 8 + 4 + 2 + 2 + 4 + 4 * 5 + 4 + 4 + 4                  # phase .. row_height (radius + 2 of padding)
    assert scalars == 76 == ArrivalState.slots.offset
    assert ArrivalState.slot_ring.offset == 76 + 8 * CAP and ArrivalState.num_region.offset == 76 + 12 * CAP
    assert ArrivalState.region_keys.offset == 76 + 12 * CAP + 4 and ArrivalState.region_keys.offset % 8 == 0    # (no padding needed)
    assert C.sizeof(ArrivalState) == 76 + 12 * CAP + 4 + 8 * CAP == 82000
    assert (ArrivalState.radius.offset, ArrivalState.unit_radius.offset, ArrivalState.fill_frac.offset) == (36, 40, 64)
    assert C.sizeof(UnitState) == 44 and (UnitState.sink.offset, UnitState.stuck.offset, UnitState.los_hyst.offset) == (8, 16, 32)
    assert C.sizeof(Member) == 32 and (Member.settled.offset, Member.layer.offset, Member.us.offset) == (8, 12, 24)


_bound = None


def _lib():
    global _bound
    if _bound is None:
        check_layouts()
        L = pfref.lib()
        L.pfref_nav_private.restype = C.c_void_p
        L.pfref_nav_private.argtypes = [C.c_void_p]
        L.N_RegionGeodesicDist.restype = C.c_int
        L.N_RegionGeodesicDist.argtypes = [C.c_void_p, Vec3, C.c_void_p, C.c_size_t, Vec2, C.c_void_p, C.c_size_t, C.c_void_p]
        L.N_PositionBlocked.restype = C.c_bool
        L.N_PositionBlocked.argtypes = [Vec2, C.c_int, C.c_void_p, Vec3]
        L.N_TileKeysForPositions.restype = C.c_size_t
        L.N_TileKeysForPositions.argtypes = [C.c_void_p, Vec3, C.c_void_p, C.c_size_t, C.c_void_p]
        L.G_Arrival_UpdateFlock.restype = None
        L.G_Arrival_UpdateFlock.argtypes = [C.POINTER(ArrivalState), C.c_void_p, Vec2, C.c_int, C.c_float, C.c_int, C.POINTER(Member), C.c_int]
        _bound = L
    return _bound


class Ref:
    """The reference's nav state of a world: an open map, the world's blockers."""

    def __init__(self, W):
        self.nav = pfref.RefNav(np.ones((W.h, W.w, 64, 64), np.uint8), layer_mask=sum(1 << l for l in W.blockers))
        for layer, b in W.blockers.items():
            self.nav.set_blockers(b, layer)
        self.priv = _lib().pfref_nav_private(self.nav._h)
        self.mp = Vec3(*[float(v) for v in self.nav.map_pos])
        self.seconds_in_the_reference = 0.0

    def close(self):
        self.nav.close()

    def geodesic(self, keys, entry, queries):
        keys = np.ascontiguousarray(keys, np.uint64)
        q = np.ascontiguousarray(queries, F).reshape(-1, 2)
        out = np.full(max(len(q), 1), 77, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
        res = _lib().N_RegionGeodesicDist(self.priv, self.mp, p(keys), len(keys), Vec2(float(entry[0]), float(entry[1])), p(q), len(q), p(out))
        return out[:len(q)], res

    def blocked(self, layer, xz):
        return bool(_lib().N_PositionBlocked(Vec2(float(xz[0]), float(xz[1])), layer, self.priv, self.mp))

    def keys(self, positions):
        q = np.ascontiguousarray(positions, F).reshape(-1, 2)
        out = np.zeros(len(q) + 1, np.uint64)
        n = _lib().N_TileKeysForPositions(self.priv, self.mp, q.ctypes.data_as(C.c_void_p), len(q), out.ctypes.data_as(C.c_void_p))
        return out[:n]

    def update(self, zone, keys, pos, mem):
        """G_Arrival_UpdateFlock on a hand-filled struct arrival_state: (the zone's outputs, the members' outputs)."""
        assert F(zone["fill_frac"]) >= F(0.25) and zone["phase"] == afm.FILLING          # never the stubbed path, never the first build
        st = ArrivalState()
        st.phase, st.layer, st.radius, st.unit_radius = zone["phase"], zone["layer"], zone["radius"], float(zone["unit_radius"])
        st.centre = Vec2(*[float(v) for v in zone["centre_xz"]])
        st.axis, st.com, st.com_dest_id = Vec2(0.0, 1.0), st.centre, 0
        slots = np.asarray(zone["slots_xz"], F).reshape(-1, 2)
        st.num_slots, st.active_row, st.num_rows = len(slots), zone["active_row"], zone["num_rows"]
        st.realloc_counter, st.stall_counter, st.prev_occ = zone["realloc_counter"], zone["stall_counter"], zone["prev_occ"]
        st.fill_frac, st.row_height = float(zone["fill_frac"]), float(zone["row_height"])
        C.memmove(st.slots, slots.ctypes.data, slots.nbytes)
        ring = np.ascontiguousarray(zone["slot_ring"], np.int32)
        C.memmove(st.slot_ring, ring.ctypes.data, ring.nbytes)
        kk = np.ascontiguousarray(keys, np.uint64)
        st.num_region = len(kk)
        C.memmove(st.region_keys, kk.ctypes.data, kk.nbytes)
        n = len(mem["uid"])
        us = (UnitState * max(n, 1))()
        ms = (Member * max(n, 1))()
        for j in range(n):
            us[j].substate, us[j].sink_valid = int(mem["substate"][j]), bool(mem["sink_valid"][j])
            us[j].sink = Vec2(float(mem["sink_xz"][j][0]), float(mem["sink_xz"][j][1]))
            p = pos[mem["uid"][j]]
            ms[j].pos, ms[j].settled, ms[j].layer, ms[j].radius = Vec2(float(p[0]), float(p[1])), bool(mem["settled"][j]), zone["arg_layer"], 1.0
            ms[j].us = C.pointer(us[j])
        t0 = time.perf_counter()
        _lib().G_Arrival_UpdateFlock(C.byref(st), self.nav._h, st.centre, zone["arg_layer"], float(zone["arg_unit_radius"]),
                                     int(zone["arg_total_members"]), ms, n)
        self.seconds_in_the_reference += time.perf_counter() - t0            # (scripts/bench_arrival_flock.py reads it)
        z = {f: getattr(st, f) for f in afm.ZONE_OUT}
        z["slot_ring"] = np.array(st.slot_ring[:len(slots)], np.int32)
        out = {"substate": np.array([us[j].substate for j in range(n)], np.uint8), "sink_valid": np.array([us[j].sink_valid for j in range(n)], np.uint8),
               "sink_xz": np.array([(us[j].sink.x, us[j].sink.z) for j in range(n)], F).reshape(n, 2)}
        return z, out


REORIENTING = ("shapes", "cap", "footprints", "ties", "batch_50", "fill_below")


@pytest.mark.parametrize("name", sorted(worlds.WORLDS))
def test_premises_of_every_world(name):
    W, want = worlds.world(name)
    worlds.premises(name, W, want)


def test_premises_of_the_chain():
    worlds.chain_premises(worlds.chain()[1])


@pytest.mark.parametrize("name", REORIENTING)
def test_flood_source_key_and_slot_distances(name):
    """N_RegionGeodesicDist with the model's entry: the slots' distances and the maximum; with every KEY's tile centre as
    the queries: the flood itself, whose one zero is the source key."""
    W, _ = worlds.world(name)
    R = Ref(W)
    n_floods = 0
    for z, keys, mem in zip(W.zones, W.keys, W.members):
        if len(z["slots_xz"]) == 0 or len(keys) == 0:
            continue
        entry = afm.entry_point(z, W.pos, mem)
        mine, mx, kd = afm.geodesic_dist(W.map, keys, entry, z["slots_xz"])
        ref, rmx = R.geodesic(keys, entry, z["slots_xz"])
        assert np.array_equal(mine, ref) and mx == rmx
        centres = np.array([afm.tile_centre(W.map, int(k)) for k in keys], F)
        ref_k, _ = R.geodesic(keys, entry, centres)
        assert np.array_equal(np.array(kd, np.int32), ref_k) and int(np.flatnonzero(ref_k == 0)[0]) == afm.source_key(W.map, keys, entry)
        n_floods += 1
    R.close()
    assert n_floods >= (1 if name == "cap" else 2)


@pytest.mark.parametrize("name", ("shapes", "footprints", "frontier"))
def test_blocked_test_and_keys(name):
    W, _ = worlds.world(name)
    R = Ref(W)
    n_blocked = 0
    for z, keys in zip(W.zones, W.keys):
        on_map = np.array([W.map.tile(x, zz) is not None for x, zz in z["slots_xz"]], bool)
        for layer in W.blockers:
            mine = [W.map.blocked(layer, *s) for s in z["slots_xz"][on_map]]
            ref = [R.blocked(layer, s) for s in z["slots_xz"][on_map]]
            assert mine == ref
            n_blocked += sum(ref)
        centres = np.array([aw.xz(W.w, W.h, r, c) for r, c in z["tiles"]], F)
        assert np.array_equal(R.keys(centres), keys)
        assert len(R.keys(np.array([(1e6, 0.0), (0.0, -1e6)], F))) == 0        # off the map: dropped
    R.close()
    assert n_blocked > 4 or name == "footprints"                            # (the footprints world has no blockers)


def follow(R, W, zi, calls, speed=1.5):
    """`calls` consecutive calls of one zone, model and reference side by side, each fed its own outputs, members moved by
    the chain's script; returns the reallocs seen.  Stops short of a call the reference must not get."""
    Wz = aw.World(W.w, W.h, layers=tuple(W.blockers))
    Wz.blockers, Wz.map = W.blockers, W.map
    Wz.zones, Wz.members, Wz.keys, Wz.pos = [W.zones[zi]], [W.members[zi]], [W.keys[zi]], W.pos.copy()
    reallocs = 0
    for call in range(calls):
        z, mem = Wz.zones[0], Wz.members[0]
        if z["phase"] != afm.FILLING or F(z["fill_frac"]) < F(0.25):
            return reallocs, call
        want = afm.update_flock(W.map, z, Wz.keys[0], Wz.pos, mem, decide_host=False)
        rz, rm = R.update(z, Wz.keys[0], Wz.pos, mem)
        worlds.same(([rz], [rm], np.zeros(1, np.uint8)), ([want[0]], [want[1]], np.zeros(1, np.uint8)), "zone %d, call %d" % (zi, call))
        reallocs += int(want[0]["realloc_counter"] == 0 and want[0]["phase"] == afm.FILLING)
        aw.chain_step(Wz, [want[0]], [want[1]], call, speed)
    return reallocs, calls


@pytest.mark.parametrize("name", ("frontier", "period"))
def test_frozen_zones_against_G_Arrival_UpdateFlock_over_consecutive_calls(name):
    """Occupancy, frontier, stall counter, sinks, commit, radius, the realloc period and the all-settled arm."""
    W, _ = worlds.world(name)
    R = Ref(W)
    followed = 0
    for zi in range(len(W.zones)):
        reallocs, calls = follow(R, W, zi, 9)
        assert calls >= 1, zi                                                # (a zone whose members are all settled ends its chain: DONE)
        if calls >= 8:
            followed += 1
            assert reallocs >= 2
    R.close()
    # (period: three zones are DONE at once, two empty out below fill_frac 0.25, where the reference must not be called)
    assert followed >= (10 if name == "frontier" else 5), followed


def test_frozen_chain_zone_and_batch_zones_against_the_reference():
    W = aw.chain_world()
    R = Ref(W)
    assert follow(R, W, 1, 12, speed=0.7) == (3, 12)
    R.close()
    W, _ = worlds.world("batch_50")
    R = Ref(W)
    n = sum(follow(R, W, zi, 8)[1] >= 1 for zi in range(len(W.zones)) if zi % 3 == 1)
    R.close()
    assert n >= 10


WRONG_SHOWS = {"centroid_all": ("shapes", "footprints"), "maxd_keys": ("shapes", "footprints"), "unreached_ring0": ("footprints",),
               "le_settled": ("ties",), "le_sink": ("ties",), "freeze_le": ("frontier", "fill_below"), "settled_neighbour": ("ties", "shapes")}


@pytest.mark.parametrize("wrong", afm.WRONG)
def test_wrong_models_change_bits(wrong):
    changed = 0
    for name in WRONG_SHOWS[wrong]:
        W, want = worlds.world(name)
        other = afm.update_flocks(W.map, W.zones, W.keys, W.pos, W.members, wrong=wrong)
        try:
            worlds.same(other, want, wrong)
        except AssertionError:
            changed += 1
    assert changed >= 1, wrong
