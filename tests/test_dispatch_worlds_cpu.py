"""The worlds of tests/dispatch_worlds.py hold what they promise -- checked without a GPU, and without the builder's
own bookkeeping: every agent's ClearPath neighbours are counted again from positions, states and flags by the rule of
find_neighbours (movement.c:2768: the r = 10 query on x256 fixed-point coordinates, inclusive; garrisoned entities filtered;
self, immovable, zero-radius and other-medium entities skipped; still or slower than 0.3 = static; 32 of each kind), the
histograms meet the conditions the GPU tests rely on, and the restatement oracle alone is well defined on every world."""
import numpy as np
import pytest

from oracle import navoracle
from tests import cases
from tests import dispatch_worlds as dw


def _pairs(pos_xz, r):
    """(i, j, i != j) with |p_i - p_j| <= r by BG_SCALE_F fixed point (bitmap_grid.h:196, :1376), from a cell list."""
    ix = cases.sp_scale(pos_xz[:, 0])
    iy = cases.sp_scale(pos_xz[:, 1])
    ir = int(cases.sp_scale(r))
    cx, cy = (ix - ix.min()) // ir + 1, (iy - iy.min()) // ir + 1
    m = int(cy.max()) + 2
    key = cx * m + cy
    order = np.argsort(key, kind="stable")
    skey = key[order]
    n = len(ix)
    out_i, out_j = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            k2 = key + dx * m + dy
            lo, hi = np.searchsorted(skey, k2, "left"), np.searchsorted(skey, k2, "right")
            cnt = hi - lo
            i = np.repeat(np.arange(n), cnt)
            within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            j = order[np.repeat(lo, cnt) + within]
            keep = ((ix[i] - ix[j]) ** 2 + (iy[i] - iy[j]) ** 2 <= ir * ir) & (i != j)
            out_i.append(i[keep]); out_j.append(j[keep])
    return np.concatenate(out_i), np.concatenate(out_j)


def recount(W):
    """(n_dyn, n_stat, searching, irregular) of every agent, from the world arrays alone."""
    wd = W.world
    n = W.n
    flags, state, vel = wd["flags"], wd["state"], wd["vel_xz"]
    garr = (flags & dw.FLAG_GARRISONED) != 0
    still = np.isin(state, (2, 4))                                             # ent_still, movement.c:652
    static = still | (np.sqrt(vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1], dtype=np.float32) < np.float32(0.3))
    i, j = _pairs(wd["pos_xz"], 10.0)
    ok = ~garr[j] & ((flags[j] & dw.FLAG_MOVABLE) != 0) & (wd["radius"][j] != 0) & (((flags[i] ^ flags[j]) & (1 << 15)) == 0)
    n_dyn = np.minimum(32, np.bincount(i[ok & ~static[j]], minlength=n))
    n_stat = np.minimum(32, np.bincount(i[ok & static[j]], minlength=n))
    searching = ~still & ((flags & dw.FLAG_COMBAT_HELD) == 0)
    i, j = _pairs(wd["pos_xz"], 30.0)
    irregular = garr | (np.bincount(i[garr[j]], minlength=n) > 0)
    return n_dyn, n_stat, searching, irregular


@pytest.mark.parametrize("name", dw.NAMES)
def test_counts_are_what_the_builder_intends(name):
    W = dw.get(name)
    n_dyn, n_stat, searching, irregular = recount(W)
    assert np.array_equal(n_dyn, W.n_dyn) and np.array_equal(n_stat, W.n_stat)
    assert np.array_equal(searching, W.searching) and np.array_equal(irregular, W.irregular)
    assert dw.list_histogram(n_dyn + n_stat, searching, irregular) == W.lists()
    wd = W.world
    # the geometry the counts rest on: a cluster inside a disc of diameter < 10, clusters 70 wu apart (60 between any two
    # members of different clusters), 12 wu to the map edge, speeds away from CLEARPATH_STILL_SPEED
    pos = wd["pos_xz"].astype(np.float64)
    ncl = int(W.cluster.max()) + 1
    centre = np.stack([np.bincount(W.cluster, pos[:, k], ncl) for k in (0, 1)], 1) / np.bincount(W.cluster, minlength=ncl)[:, None]
    assert np.linalg.norm(pos - centre[W.cluster], axis=1).max() < 4.9
    i, j = _pairs(wd["pos_xz"], 60.0)
    assert (W.cluster[i] == W.cluster[j]).all()
    assert np.abs(pos[:, 0]).max() <= W.w * 128.0 - 12.0 and np.abs(pos[:, 1]).max() <= W.h * 128.0 - 12.0
    speed = np.linalg.norm(wd["vel_xz"], axis=1)
    assert not ((speed > 0.25) & (speed < 0.35)).any()
    # the members of a cluster lie in many k_agent_mid waves (64 consecutive uids)
    big = np.flatnonzero(np.bincount(W.cluster) >= 17)
    if len(big) and W.n >= 640:
        c = big[0]
        assert len(np.unique(np.flatnonzero(W.cluster == c) // 64)) >= 8


def _moving_at(W, count, dyn=None, stat=None):
    sel = W.searching & ~W.irregular & (W.count == count)
    if dyn is not None:
        sel &= (W.n_dyn == dyn) & (W.n_stat == stat)
    return int(sel.sum())


@pytest.mark.parametrize("name", ["ladder", "ladder_garrisoned", "ladder_wide"])
def test_ladder_has_twelve_agents_at_every_edge(name):
    W = dw.get(name)
    for c in dw.LADDER_COUNTS:
        assert _moving_at(W, c) >= 12, (c, _moving_at(W, c))
    # where a cap binds: 64 dynamic + 10 static -> 32 + 10; 40 + 40 -> 32 + 32
    assert _moving_at(W, 42, 32, 10) >= 12 and _moving_at(W, 64, 32, 32) >= 12
    assert (W.n_dyn == 32).sum() > 100 and (W.n_stat == 32).sum() > 100
    lists = W.lists()
    assert all(x > 0 for x in lists[:5])
    garr = (W.world["flags"] & dw.FLAG_GARRISONED) != 0
    if name == "ladder_garrisoned":
        assert 0.015 * W.n <= garr.sum() <= 0.025 * W.n and lists[5] >= 20
        plain = dw.get("ladder")
        assert np.array_equal(W.world["pos_xz"], plain.world["pos_xz"])
    else:
        assert not garr.any() and lists[5] == 0
    assert W.w == (4 if name != "ladder_wide" else dw.get("solo_heavy").w)


def test_sparse_lists_hold_exactly_what_they_say():
    exp = {"one_on_row2": [0, 0, 1, 0, 0, 0], "four_on_row0": [4, 0, 0, 0, 0, 0], "five_on_row1": [0, 5, 0, 0, 0, 0],
           "one_wave_no_heavy": [0, 0, 0, 0, 1, 0], "one_heavy_no_wave": [0, 0, 0, 0, 1, 0]}
    for name in dw.SPARSE:
        W = dw.get(name)
        assert W.lists() == exp[name], name
        assert (W.w, W.h) == (2, 2)
    wave, heavy = dw.get("one_wave_no_heavy"), dw.get("one_heavy_no_wave")
    on = lambda W: W.count[W.searching & (W.count > 0)]                      # noqa: E731
    assert list(on(wave)) == [17] and list(on(heavy)) == [34]
    assert list(on(dw.get("one_on_row2"))) == [6]
    assert dw.get("no_neighbours").lists() == [0] * 6 and dw.get("no_neighbours").searching.all()


def test_large_worlds_cross_their_thresholds():
    full, solo, flood = dw.get("one_list_full"), dw.get("solo_heavy"), dw.get("retry_flood")
    # 9 216 units of four on ROW2 alone: with 4 x 1 024 waves in the main k_cp_rows launch, total / nw - 1 = 1 static round
    assert full.n == 36864 and full.searching.all() and (full.count == 5).all() and full.lists() == [0, 0, 36864, 0, 0, 0]
    assert full.n // 4 == 9216 and 9216 // 4096 - 1 == 1
    # 8 192 problems and more on the wave list, none on the heavy list (CP_SOLO_MIN = 8 192)
    assert solo.searching.all() and (solo.count == 17).all() and solo.n >= 8192 and solo.lists() == [0, 0, 0, 0, solo.n, 0]
    # nwork = 8 192 exactly, everybody with 3 neighbours
    assert flood.n == 8192 and flood.searching.all() and (flood.count == 3).all() and flood.lists() == [0, 8192, 0, 0, 0, 0]


@pytest.mark.parametrize("name", dw.NAMES)
def test_oracle_is_well_defined_on_the_world(name):
    W = dw.get(name)
    out = navoracle.OracleNav(W.cost()).agent_step(cases.step_arrays(W.world, W.vdes), nthreads=16)
    for k in ("vel_xz", "vpref_xz", "new_pos_xz"):
        assert np.isfinite(out[k]).all(), k
    assert (out["vel_xz"][~W.searching] == 0).all()
    if W.searching.any():
        assert np.abs(out["vel_xz"][W.searching]).max() > 0
    assert (out["status"] & ~np.uint8(1) == 0).all()               # nothing but NAVHIP_ST_MOVED


def _first_attempt_fails(W, vpref):
    """Per searching agent: the model of ONE attempt of clearpath_new_velocity (tests/tools/cp_model.py) finds no
    candidate.  The neighbours are the other members of the cluster (test_counts_are_what_the_builder_intends)."""
    from tests.tools import cp_model
    wd = W.world
    order = np.argsort(W.cluster, kind="stable")
    start = np.searchsorted(W.cluster[order], np.arange(W.cluster.max() + 2))
    static = (wd["state"] == 2) | (np.linalg.norm(wd["vel_xz"], axis=1) < 0.3)
    fails = np.zeros(W.n, bool)
    for uid in np.flatnonzero(W.searching):
        c = W.cluster[uid]
        mem = order[start[c]:start[c + 1]]
        mem = mem[mem != uid]
        ent = np.array([*wd["pos_xz"][uid], *wd["vel_xz"][uid], wd["radius"][uid]], np.float32)
        nbs = np.zeros((len(mem), 5), np.float32)
        nbs[:, 0:2], nbs[:, 4] = wd["pos_xz"][mem], wd["radius"][mem]
        nbs[:, 2:4] = np.where(static[mem][:, None], 0, wd["vel_xz"][mem])
        fails[uid] = not cp_model.attempt(ent, vpref[uid], cp_model.make_cones(ent, nbs, ~static[mem]))[0]
    return fails


def test_retry_flood_fails_its_first_attempt():
    """At least RETRY_ESTABLISHED = 2 048 agents of retry_flood have no admissible candidate in their first attempt: 2 x
    256 waves x 4 agents, a non-zero static round for the 64 workgroups of the retry launch.  It is the agent in the
    middle of every quad and, with this seed, one agent of a ring: 2 049 -- a quarter of the world is what this geometry
    gives, some 32 entries per sub-list of the retry list, so the list's capacity (nh_worklist_cap) stays untested.  (Measured while
    choosing it: triads and quads of radius 1 at 1.5-2.2 wu spacing, laid out at random -- 0 of 8 192; random clusters of
    four and five within 0.3-1.0 wu, moving inwards -- 4-12 %.)  With neighbours of one kind a failed attempt ends the
    reference's loop: the oracle's velocity of exactly these agents is 0."""
    W = dw.get("retry_flood")
    out = navoracle.OracleNav(W.cost()).agent_step(cases.step_arrays(W.world, W.vdes), nthreads=16)
    fails = _first_attempt_fails(W, out["vpref_xz"])
    assert fails.sum() >= dw.RETRY_ESTABLISHED, int(fails.sum())
    assert (W.n_stat == 0).all()
    assert np.array_equal(fails, (out["vel_xz"] == 0).all(1))
    # who fails: the first member of every cluster is the one in the middle (dispatch_worlds.build, ring=)
    ring = np.linalg.norm(W.world["pos_xz"] - np.stack([np.bincount(W.cluster, W.world["pos_xz"][:, k]) for k in (0, 1)], 1)[W.cluster] / 4.0,
                          axis=1) > 0.25
    assert fails[~ring].all() and (~ring).sum() == 2048 and fails[ring].sum() == fails.sum() - 2048
