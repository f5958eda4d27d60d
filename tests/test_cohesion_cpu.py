"""The worlds of tests/cohesion_worlds.py hold what they promise, checked without a GPU: the numpy model of cohesion_force
equals the restatement bit for bit on every member, the restatement equals the reference build where that is present, the
probes are isolated and in the window, the far clusters produce the survivor counts and self positions the kernel's tile
walk can get wrong, every launch-plan shape is there, and every deliberately wrong model changes a probe's bits."""
import numpy as np
import pytest

from oracle import navoracle, pfref
from tests import cohesion_worlds as cw

_CACHE = {}


def _oracle(W, hz):
    """(agent_step outputs, cohesion of every flock member, isolated[uid]) of the restatement, once per (world, hz)."""
    key = (W.name, hz)
    if key not in _CACHE:
        onav = navoracle.OracleNav(W.cost())
        out = onav.agent_step(W.arrays, hz=hz, nthreads=16)
        n = W.n
        coh, isolated = np.zeros((n, 2), np.float32), np.zeros(n, bool)
        for uid in W.arrays["flock_members"]:
            a, c, s = onav.forces(W.arrays, int(uid), W.arrays["vdes_xz"][uid], hz=hz)
            coh[uid] = c
            isolated[uid] = (a == 0).all() and (s == 0).all()
        _CACHE[key] = out, coh, isolated
    return _CACHE[key]


def _model(W, hz, variant=None):
    key = (W.name, hz, variant, "model")
    if key not in _CACHE:
        _CACHE[key] = cw.cohesion_model(W.arrays, hz, variant)
    return _CACHE[key]


def _probes_in_window(W, hz):
    """The probes the restatement confirms: arrive and separation force exactly 0, active, vpref = fl(0.15f * cohesion) --
    the final clamp did not bind --, and smf / 15 < |com - me| < smf."""
    out, coh, isolated = _oracle(W, hz)
    raw = _model(W, hz)[1]
    p = W.probes
    ok = isolated[p] & cw.active_mask(W.arrays)[p] & cw.in_window(raw[p], hz)
    ok &= (out["vpref_xz"][p].view(np.uint32) == cw.vpref_of(coh[p]).view(np.uint32)).all(1)
    return p[ok]


WORLD_HZ = [(name, hz) for name in cw.NAMES for hz in cw.get(name).hz]


@pytest.mark.parametrize("name,hz", WORLD_HZ)
def test_model_equals_the_restatement_bit_for_bit(name, hz):
    W = cw.get(name)
    coh = _oracle(W, hz)[1]
    got = _model(W, hz)[0]
    m = W.arrays["flock_members"]
    bad = m[(got[m].view(np.uint32) != coh[m].view(np.uint32)).any(1)]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:4]], coh[bad[:4]])


@pytest.mark.skipif(not pfref.available(), reason="needs the reference build (oracle/_ref)")
@pytest.mark.parametrize("name", ["window20", "window1", "far_clusters", "arith", "plan_65", "plan_513"])
def test_restatement_equals_the_reference_build(name):
    """The reference keeps a flock's members in its own hash order: the restatement is given that order (as
    tests/test_oracle_cpu.py does), so this pins the restatement on these POSITIONS; the model test above pins it on the
    member order the worlds are built with.  Every probe and every other active member: the three forces and vpref."""
    from tests import cases
    W = cw.get(name)
    hz = W.hz[0]
    a = W.arrays
    nav = pfref.RefNav(W.cost())
    world = {k: a[k] for k in ("pos_xz", "vel_xz", "radius", "max_speed", "speed", "flags", "state", "has_dest_los", "flock",
                               "flock_target_xz")}
    mv, _ = cases.ref_move_for(nav, world, hz=hz)
    k = len(a["flock_target_xz"])
    try:
        orders = [mv.flock_order(f) for f in range(k)]
    except BaseException:
        pfref.RefMove.unload()
        raise
    arrays = cases.step_arrays(world, a["vdes_xz"], orders)
    assert np.array_equal(np.sort(arrays["flock_members"]), np.sort(a["flock_members"]))
    onav = navoracle.OracleNav(W.cost())
    out = onav.agent_step(arrays, hz=hz, nthreads=16)
    try:
        pick = np.flatnonzero(cw.active_mask(a) & (a["flock"] >= 0))
        assert np.isin(W.probes, pick).all()
        for uid in pick:
            ea, ec, es = mv.forces(int(uid), a["vdes_xz"][uid])
            ga, gc, gs = onav.forces(arrays, int(uid), a["vdes_xz"][uid], hz=hz)
            assert np.array_equal(ec.view(np.uint32), gc.view(np.uint32)), (uid, ec, gc)
            assert np.array_equal(ea, ga) and np.array_equal(es, gs), uid
            assert np.array_equal(mv.vpref(int(uid), a["vdes_xz"][uid]).view(np.uint32), out["vpref_xz"][uid].view(np.uint32)), uid
    finally:
        pfref.RefMove.unload()


@pytest.mark.parametrize("hz", [20, 1])
def test_window_world_has_its_probes(hz):
    W = cw.get("window%d" % hz)
    good = _probes_in_window(W, hz)
    assert len(good) == len(W.probes) >= 256, (len(good), len(W.probes))          # every probe isolated and in the window
    for tag in ["size%d" % F for F in cw.WINDOW_SIZES] + ["origin", "tuned", "far_mates"]:
        assert len(np.intersect1d(good, W.tags[tag])) >= 8, (tag, len(np.intersect1d(good, W.tags[tag])))
    sizes = np.diff(W.arrays["flock_offsets"])
    assert set(sizes) == set(cw.WINDOW_SIZES) | set(cw.WINDOW_FAR)
    # the flocks with mates out of range: a weighted mate of the probe waits in a carried tail of the probe's wave
    a = W.arrays
    tails = 0
    for f, wv, sl, act, keep in cw._waves(a):
        own = a["flock_members"][a["flock_offsets"][f] + sl[act[sl]]]
        if np.isin(own, W.tags["far_mates"]).any():
            counts, carried = cw._queue_walk(keep, len(keep))
            assert not keep.all()
            tails += int(carried.sum() > 0)
    assert tails >= 8


def test_arith_world_has_its_lengths_edges_and_batches():
    W = cw.get("arith")
    a = W.arrays
    good = _probes_in_window(W, 20)
    assert len(good) == len(W.probes) >= 256, (len(good), len(W.probes))          # every probe in the window
    for tag in cw.ARITH_EDGES:
        assert len(np.intersect1d(good, W.tags[tag])) >= 8, tag
    # the probe/mate lengths, as the kernel sees them
    lens, sss = [], []
    for uid in W.probes:
        f = a["flock"][uid]
        m = a["flock_members"][a["flock_offsets"][f]:a["flock_offsets"][f + 1]]
        m = m[m != uid]
        d = a["pos_xz"][m] - a["pos_xz"][uid]
        ss = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        lens.append(np.sqrt(ss))
        sss.append(ss)
        if uid in W.tags["len16"]:
            assert {np.float32(16), np.nextafter(np.float32(16), np.float32(0)), np.nextafter(np.float32(16), np.float32(32))} <= set(lens[-1])
        if uid in W.tags["coincident"]:
            assert (lens[-1] == 0).sum() == 1 and len(np.unique(a["pos_xz"][m], axis=0)) <= len(m) - 1
        if uid in W.tags["tiny_ss"]:
            assert ((ss > 0) & (ss < np.float32(2.0 ** -90))).any()
    lens, sss = np.concatenate(lens), np.concatenate(sss)
    assert len(lens) >= 4096 + 4096 // cw.ARITH_SATS
    hist = np.histogram(lens[lens > 0], np.concatenate([10.0 ** np.arange(-20, 1), [16, 100, 200, 300.5]]))[0]
    assert (hist[:20] >= 60).all() and (hist[20:] >= 100).all(), hist             # every decade, then the linear part
    assert ((sss > 0) & (sss < np.float32(2.0 ** -90))).sum() >= 400 and ((sss > 0) & (sss < np.float32(1.2e-38))).sum() >= 100
    close_n, odd_n = cw.batch_lanes(W)
    for arr in (close_n, odd_n):
        assert (arr == 0).sum() >= 8 and (arr == 1).sum() >= 8 and (arr > 1).sum() >= 8, np.bincount(arr)


def test_far_clusters_reach_every_survivor_count_and_self_position():
    W = cw.get("far_clusters")
    a = W.arrays
    assert (W.w, W.h) == (8, 1) and np.diff(a["flock_offsets"]).max() <= 700
    S = cw.tile_survivors(W)
    seen = {c for _, _, counts in S["counts"] for c in counts}
    assert set(cw.SURVIVOR_COUNTS) <= seen, sorted(seen)
    assert S["zero_between"] and S["self_tail"] and S["self_tile"] >= {0, 1, 2}
    # waves that mix active and inactive quads, some 15 % of the members idle or combat-held
    act = cw.active_mask(a)
    assert 0.10 <= 1 - act.mean() <= 0.20
    held = (a["flags"] & cw.FLAG_COMBAT_HELD) != 0
    assert held.sum() >= 50 and (a["state"] == cw.STATE_ARRIVED).sum() >= 50
    mixed = 0
    for f in range(len(a["flock_offsets"]) - 1):
        m = a["flock_members"][a["flock_offsets"][f]:a["flock_offsets"][f + 1]]
        am = act[m][:len(m) // 16 * 16].reshape(-1, 16).sum(1)
        mixed += int(((am > 0) & (am < 16)).sum())
    assert mixed >= 50
    # a box over all 16 quads changes who is dropped: the geometry tells the two rules apart
    wrong = cw.tile_survivors(W, box="all")
    assert sum(c != d for c, d in zip(S["counts"], wrong["counts"])) >= 5
    # the fourth tick: two clusters' positions swapped.  The grouping carried from the old positions is not the one a
    # fresh regrouping would give: its waves hold members of both ends of the map, and their survivor counts differ from
    # the fresh ones and from those the same grouping had before the swap
    sw = W.swapped()
    assert np.array_equal(np.sort(sw["pos_xz"], 0), np.sort(a["pos_xz"], 0)) and (sw["pos_xz"] != a["pos_xz"]).any(1).mean() > 0.3
    carried_perm, fresh_perm = cw.grouping(a, W.w, W.h), cw.grouping(sw, W.w, W.h)
    lists = lambda arrays, perm: sorted(tuple(c) for _, _, c in cw.tile_survivors(W, arrays=arrays, perm=perm)["counts"])    # noqa: E731
    before, stale, fresh = lists(a, carried_perm), lists(sw, carried_perm), lists(sw, fresh_perm)
    assert stale != fresh and stale != before
    assert sum(x != y for x, y in zip(stale, fresh)) >= len(fresh) // 4
    # members of one flock lie in two or three clusters more than 906 wu apart, in interleaved order
    for f in range(len(a["flock_offsets"]) - 1):
        x = a["pos_xz"][a["flock_members"][a["flock_offsets"][f]:a["flock_offsets"][f + 1]], 0]
        side = np.digitize(x, [-500, 500])
        assert len(set(side)) >= 2 and (np.diff(side) != 0).sum() >= 8


@pytest.mark.parametrize("nf", cw.PLAN_SHAPES)
def test_plan_shapes_are_present(nf):
    W = cw.get("plan_%d" % nf)
    a = W.arrays
    sizes = np.diff(a["flock_offsets"])
    assert len(sizes) == nf and sizes.max() <= 20
    b, e, epoch = W.slab
    assert 0 < b < e < W.n and epoch
    if nf == 1:
        return
    assert sizes[0] == 0 and sizes[1] == 0 and sizes[-1] == 0 and (sizes[nf // 2:nf // 2 + 3] == 0).all()
    assert (sizes == 1).sum() >= 3 and (sizes == 20).any()
    act = cw.active_mask(a)
    all_idle = [f for f in range(nf) if sizes[f] and not act[a["flock_members"][a["flock_offsets"][f]:a["flock_offsets"][f + 1]]].any()]
    assert len(all_idle) >= 3
    inside = [((a["flock_members"][a["flock_offsets"][f]:a["flock_offsets"][f + 1]] >= b)
               & (a["flock_members"][a["flock_offsets"][f]:a["flock_offsets"][f + 1]] < e)).sum() for f in range(nf)]
    assert sum(1 for f in range(nf) if sizes[f] and inside[f] == 0) >= 3 and sum(1 for x in inside if x) >= 3


def _caught(variant):
    """(world, hz) -> probes in the window whose fl(0.15f * cohesion) bits the wrong model changes."""
    hits = {}
    for name, hz in WORLD_HZ:
        W = cw.get(name)
        p = _probes_in_window(W, hz) if len(W.probes) else np.flatnonzero(cw.active_mask(W.arrays))
        if name.startswith("plan_"):
            continue
        right, wrong = cw.vpref_of(_model(W, hz)[0][p]), cw.vpref_of(_model(W, hz, variant)[0][p])
        hits[(name, hz)] = int((right.view(np.uint32) != wrong.view(np.uint32)).any(1).sum())
    return hits


@pytest.mark.parametrize("variant", [v for v in cw.WRONG_MODELS if v != "box_all"])
def test_every_wrong_model_is_caught(variant):
    """Each wrong model changes the bits of fl(0.15f * cohesion) of at least one probe in the window (in far_clusters,
    which has no probes: of an active member) in at least one world."""
    hits = _caught(variant)
    print(variant, hits)
    assert sum(hits.values()) > 0, hits
    if variant == "tail_twice":
        # (only the box rule leaves a tail behind a full tile: the far clusters, and the window flocks of 300 whose probes
        # show the sum at full precision)
        assert hits[("far_clusters", 20)] > 0 and hits[("window20", 20)] >= 8 and hits[("window1", 1)] >= 8
    if variant == "box_first":
        assert hits[("far_clusters", 20)] > 0


def test_a_box_over_all_quads_cannot_change_a_force():
    """The ninth wrong model -- the box taken over all 16 quads of a wave instead of the active ones -- changes who is
    dropped in far_clusters (test_far_clusters_reach_...: the survivor counts differ) and NOT ONE BIT of any force, in any
    world: a box over more quads is a larger box, a larger box only keeps more members, and a kept member farther than
    904 wu from a lane weighs exactly +0 there.  No test of the forces can tell the two rules apart; a box that is too
    SMALL is another matter: `box_first` (the box of one quad) is a wrong model of its own in test_every_wrong_model_is_caught."""
    W = cw.get("far_clusters")
    right = _model(W, 20)[0]
    assert np.array_equal(cw.cohesion_model(W.arrays, 20, "box_all")[0].view(np.uint32), right.view(np.uint32))


def test_the_reach_of_a_mate():
    """The largest probe/mate distance whose omission still changes a bit of fl(0.15f * cohesion), measured on the model
    over the probes in the window of the flocks of at most 40 members of every world: 236.2 wu (window20, a flock of 17).  Contributions below half an ulp of the running
    sum are invisible to any test; beyond this distance that is all there is in these worlds.  Reported, and bounded only
    by what float32 allows: a weight is exactly 0 beyond 904 wu."""
    reach, where = 0.0, None
    for name, hz in WORLD_HZ:
        W = cw.get(name)
        if not len(W.probes):
            continue
        a = W.arrays
        base = cw.vpref_of(_model(W, hz)[0])
        for uid in _probes_in_window(W, hz):
            f = a["flock"][uid]
            b, e = a["flock_offsets"][f], a["flock_offsets"][f + 1]
            if e - b > 40:
                continue                                         # (one model run per mate: the small flocks)
            m = a["flock_members"][b:e]
            d = np.hypot(*(a["pos_xz"][m].astype(np.float64) - a["pos_xz"][uid]).T)
            for j in np.argsort(-d):
                if m[j] == uid or d[j] <= reach:
                    continue
                # omission = a weight of 0: move the mate out of range (the count F - 1 stays)
                sub = {"pos_xz": a["pos_xz"][m].copy(), "flock_offsets": np.array([0, e - b], np.int32),
                       "flock_members": np.arange(e - b, dtype=np.int32)}
                sub["pos_xz"][j] = sub["pos_xz"][j] + np.float32(5000.0)
                i = int(np.flatnonzero(m == uid)[0])
                got = cw.vpref_of(cw.cohesion_model(sub, hz)[0][i:i + 1])
                if (got.view(np.uint32) != base[uid:uid + 1].view(np.uint32)).any():
                    reach, where = float(d[j]), (name, hz, int(uid))
                    break                                        # (the nearer mates of this probe are nearer than the reach)
    print("reach of a mate: %.1f wu" % reach, where)
    assert 37.5 < reach <= 904.0, reach
