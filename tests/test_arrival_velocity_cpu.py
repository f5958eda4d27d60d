"""tests/arrival_velocity_model.py held against the reference (oracle/_ref), ingredient by ingredient, on the zone worlds of
tests/test_arrival_velocity_gpu.py: the reference build has no entry point for G_Arrival_DesiredVelocity itself, so the model
is arrival.c:862-944 as plain control flow and everything it calls in the nav module is pinned here -- the blocked test, the
zone-field lookup with at_slot, the centre-of-mass sample, the footprint keys, N_SegmentWithinRegion and arrival_near_region
(the last two read out of G_Arrival_ShouldSettle with arguments under which its answer IS that predicate).  No GPU."""
import numpy as np
import pytest

from oracle import pfref
from tests import arrival_velocity_model as avm
from tests import cases
from tests import test_arrival_velocity_gpu as worlds

pytestmark = pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")

F = np.float32
SEEDS = (9, 23)


def ref_nav(W):
    """The reference's nav state of a zone world: the same map, the same blockers."""
    grid, nav = cases.ref_nav_for(4, 4, seed=21, layer_mask=0x3)
    nav.set_blockers(W["planes"][0], 0)
    return nav


def unit_pos(W):
    return W["pos"][W["units"]["uid"]]


@pytest.mark.parametrize("seed", SEEDS)
def test_every_arm_of_the_rule_is_taken(seed):
    W = worlds.zone_world(seed)
    want = W["want"]
    for arm in ("beeline", "nearest", "zone", "centre", "com", "com_miss"):
        assert (want["arm"] == arm).sum() > 30, (arm, (want["arm"] == arm).sum())
    assert (want["sink_xz"] != W["units"]["sink_xz"]).any(1).sum() > 30          # the re-target arm
    assert (want["status"] == avm.AV_HOST).sum() == 0
    for sub in range(4):
        assert (W["units"]["substate"] == sub).sum() > 300


@pytest.mark.parametrize("seed", SEEDS)
def test_blocked_tiles_and_footprint_keys(seed):
    W = worlds.zone_world(seed)
    m, nav = W["m"], ref_nav(W)
    pts = np.concatenate([unit_pos(W), W["units"]["sink_xz"]] + [z["slots_xz"] for z in W["zones"]])
    mine = np.array([m.blocked(0, x, z) for x, z in pts])
    ref = np.array([nav.position_blocked(p) for p in pts])
    assert np.array_equal(mine, ref) and 100 < ref.sum() < len(ref) - 100
    for z, keys in zip(W["zones"], W["keys"]):
        units = {"new_pos_xz": z["slots_xz"][:1], "vel_xz": np.zeros((1, 2), F), "radius": np.ones(1, F), "nsettled": np.zeros(1, np.int32),
                 "substate": np.zeros(1, np.uint8), "sink_valid": np.zeros(1, np.uint8), "sink_xz": np.zeros((1, 2), F),
                 "order_pos_xz": z["slots_xz"][:1], "progress_anchor_xz": np.zeros((1, 2), F), "progress_anchored": np.zeros(1, np.uint8),
                 "stuck": np.zeros(1, np.int32)}
        _, ref_keys, _ = pfref.arrival_should_settle(nav, z, units)
        assert np.array_equal(ref_keys, keys) and len(keys) == len(z["tiles"])
    nav.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_segment_within_region_and_near_region_through_the_settle_rule(seed):
    """G_Arrival_ShouldSettle (arrival.c:946) with every unit armed, no slot at or behind the frontier (at_sink false), the
    frontier short of the last row (fill_done false) and a fresh progress anchor (stuck counts to 1):
      nsettled 3, zero velocity, fill_frac 0:         settle == in_region && sink_valid && N_SegmentWithinRegion(pos, sink)
      sink_valid 0, nsettled 1, fill_frac 0.95:       settle == arrival_near_region(pos)"""
    W = worlds.zone_world(seed)
    m, nav = W["m"], ref_nav(W)
    pos_all, U = unit_pos(W), W["units"]
    n_seg = n_near = 0
    for zi, (z, keys) in enumerate(zip(W["zones"], W["keys"])):
        sel = U["zone"] == zi
        pos, sink = pos_all[sel], U["sink_xz"][sel]
        nq = len(pos)
        ks = set(int(k) for k in keys)
        zone = dict(z, active_row=-1, fill_frac=0.0)
        # the premises
        assert zone["active_row"] < z["slot_ring"].min() and zone["active_row"] < z["num_rows"] - 1
        base = {"new_pos_xz": pos, "vel_xz": np.zeros((nq, 2), F), "radius": np.ones(nq, F), "substate": np.full(nq, 3, np.uint8),
                "sink_xz": sink, "order_pos_xz": pos, "progress_anchor_xz": np.zeros((nq, 2), F),
                "progress_anchored": np.zeros(nq, np.uint8), "stuck": np.zeros(nq, np.int32)}
        ref, _, after = pfref.arrival_should_settle(nav, zone, dict(base, nsettled=np.full(nq, 3, np.int32), sink_valid=np.ones(nq, np.uint8)))
        assert (after["stuck"] <= 1).all() and (after["substate"] == 3).all()
        inreg = np.array([avm.in_region(m, ks, x, zz) for x, zz in pos])
        mine = np.array([bool(i) and avm.segment_within(m, ks, p[0], p[1], s[0], s[1]) for i, p, s in zip(inreg, pos, sink)])
        assert np.array_equal(mine, ref.astype(bool)), (zi, np.flatnonzero(mine != ref.astype(bool))[:8])
        assert 15 < mine.sum() and 15 < (inreg & ~mine).sum()                # reachable and walled-off slots, both
        n_seg += int(inreg.sum())
        ref, _, _ = pfref.arrival_should_settle(nav, dict(zone, fill_frac=0.95),
                                                dict(base, nsettled=np.ones(nq, np.int32), sink_valid=np.zeros(nq, np.uint8)))
        near = np.array([avm.near_region(m, ks, z["unit_radius"], x, zz) for x, zz in pos])
        assert np.array_equal(near, ref.astype(bool)), (zi, np.flatnonzero(near != ref.astype(bool))[:8])
        assert 20 < (near & ~inreg).sum() and 30 < (~near).sum()             # the pad ring decides, both ways
        n_near += int((near & ~inreg).sum())
    assert n_seg > 400 and n_near > 100
    nav.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_zone_field_lookup_and_at_slot(seed):
    """N_DesiredGroupArrivalVelocity (pfref_desired_region_velocities, kind 2) on the TARGET_ZONE fields the reference's
    own async batch builds for the three zones: returned-true, the velocity and at_slot."""
    W = worlds.zone_world(seed)
    nav = ref_nav(W)
    zones = W["zones"]
    reqs = np.array([(pfref.ASYNC_GROUP_ARRIVAL, 0, 0, z["centre_xz"][0], z["centre_xz"][1], 0, z["radius"]) for z in zones],
                    dtype=pfref.ASYNC_REQ_DTYPE)
    fields = nav.async_batch(reqs)
    ids = sorted(fields)
    pool = np.stack([fields[k].reshape(4096) for k in ids])
    table = -np.ones((len(zones), 16), np.int32)
    for zi, z in enumerate(zones):
        for cr in range(4):
            for cc in range(4):
                # (5: the TARGET_ZONE kind of N_FlowFieldID, field.c:1976)
                fid = pfref.RefNav.region_field_id(5, 0, cr, cc, z["cell"][0], z["cell"][1], z["radius"])
                table[zi, cr * 4 + cc] = ids.index(fid) if fid in fields else -1
    assert (table >= 0).sum() >= 3 and (table < 0).sum() > 3
    m = avm.Map(4, 4, W["planes"], table, None, pool)
    pos_all, U = unit_pos(W), W["units"]
    q = np.array([(pfref.ASYNC_GROUP_ARRIVAL, 0, int(F(zones[z]["centre_xz"][1]).view(np.int32)), p[0], p[1],
                   int(F(zones[z]["centre_xz"][0]).view(np.uint32)), zones[z]["radius"]) for p, z in zip(pos_all, U["zone"])],
                 dtype=pfref.ASYNC_REQ_DTYPE)
    rv, rf = nav.desired_region_velocities(q)
    mine = [avm.zone_lookup(m, zones[z], int(z), p[0], p[1]) for p, z in zip(pos_all, U["zone"])]
    ok = np.array([a[0] for a in mine])
    assert np.array_equal(ok, (rf & 1).astype(bool)) and 300 < ok.sum() < len(ok) - 100
    vel = np.array([a[1] for a in mine], F)
    assert np.array_equal(vel[ok].view(np.uint32), rv[ok].view(np.uint32))
    at = np.array([a[2] for a in mine])
    assert np.array_equal(at[ok], (rf[ok] & 2).astype(bool)) and at.sum() > 30
    none = ok & ~vel.any(1)
    assert (none & ~at).sum() > 0 or at.sum() == none.sum()                   # (FD_NONE outside the disc, where the map has it)
    nav.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_centre_of_mass_sample(seed):
    """The cache-hit path of N_DesiredPointSeekVelocity (pfref_desired_point_seek_velocity) on the fields pfref_request_path
    leaves in the reference's cache: wherever the model reports no miss, the same velocity."""
    W = worlds.zone_world(seed)
    nav = ref_nav(W)
    pos_all, U = unit_pos(W), W["units"]
    rng = np.random.RandomState(seed)
    total = 0
    for zi, z in enumerate(W["zones"]):
        com = z["centre_xz"]
        did = None
        pos = pos_all[U["zone"] == zi]
        for src in pos[rng.choice(len(pos), 12, replace=False)]:
            if nav.position_pathable(src):
                ok, d = nav.request_path(src, com)
                did = d if ok else did
        assert did is not None
        slots, pool = cases.cached_field_table(nav, [did], 4, 4)
        m = avm.Map(4, 4, W["planes"], None, slots, pool)
        mine = [avm.sample_flow(m, 0, p[0], p[1]) for p in pos]
        hit = np.array([s == 0 for _, s in mine])
        assert hit.sum() > 100 and (~hit).sum() > 0
        ref = np.array([nav.desired_velocity(did, p, com) for p in pos[hit]], F)
        got = np.array([v for (v, s) in mine if s == 0], F)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), np.flatnonzero((got != ref).any(1))[:8]
        total += int(hit.sum())
    assert total > 600
    nav.close()
