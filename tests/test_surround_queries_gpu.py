"""navhip_surround_queries[_dev] (csrc/surround_query_kernels.hip) against the reference build: the touching test
(M_NavObjAdjacentFrom) and the closest reachable adjacent tile (M_NavClosestReachableAdjacentPosFrom) from pos + new_vel
and from pos, through oracle.pfref's RefMove.surround_queries on the same planes.  Everything is compared bit for bit:
the query bytes, the floats as uint32.

The worlds and the numpy model of the two queries are tests/surround_model.py; every case asserts its premise from the
model or the reference alone.  NAVHIP_SQ_HOST may come back for the rows a case names only: static targets, radii above
the kernel's window, and the "beyond the window" rows.

Host buffers wherever the API allows; the file also runs on the host emulator
(tests/test_surround_queries_emulated_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pfref
from tests import cases
from tests import surround_model as sm

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]


def _dev():
    import torch
    from permafrost_engine_amd import tick
    return torch.device("cpu") if tick.EMULATED else torch.device("cuda", 0)


def _sync():
    import torch
    if _dev().type == "cuda":
        torch.cuda.synchronize()


class Dev:
    """A world of surround_model in the reference and on the device."""

    def __init__(self, navlib, world, islands=True):
        self.navlib, self.world = navlib, world
        self.nav = sm.ref_nav(world)
        self.ctx = navlib.NavContext(world.w, world.h)
        for l in world.blockers:
            self.ctx.upload_plane(l, navlib.PLANE_COST_BASE, self.nav.plane(pfref.PLANE_COST, l))
            self.ctx.upload_plane(l, navlib.PLANE_BLOCKERS, self.nav.plane(pfref.PLANE_BLOCKERS, l))
            if islands:
                self.ctx.upload_plane(l, navlib.PLANE_ISLANDS, self.nav.plane(pfref.PLANE_ISLANDS, l))

    def arrays(self):
        w = self.world
        return {"pos_xz": w.pos, "radius": w.radius, "flags": w.flags}

    def check(self, host_rows=(), target=None, units=None):
        """The device's rows equal the reference's, bit for bit; exactly the rows in host_rows come back NAVHIP_SQ_HOST
        with nothing.  Returns (query, dest) of the reference."""
        w = self.world
        tgt = w.target if target is None else np.asarray(target, np.int32)
        exp_q, exp_d = sm.ref_answers(w, self.nav, tgt)
        for i in host_rows:
            exp_q[i], exp_d[i] = self.navlib.SQ_HOST, 0
        if units is not None:
            exp_q, exp_d, tgt = exp_q[units], exp_d[units], tgt[units]
        q, d = self.ctx.surround_queries(self.arrays(), w.vel, tgt, units)
        assert q.dtype == np.uint8 and d.shape == (len(tgt), 2, 2)
        bad = np.flatnonzero((q != exp_q) | (d.view(np.uint32) != exp_d.view(np.uint32)).any((1, 2)))
        assert len(bad) == 0, [(int(i), int(q[i]), int(exp_q[i]), d[i].tolist(), exp_d[i].tolist()) for i in bad[:6]]
        return exp_q, exp_d

    def close(self):
        self.ctx.close()
        self.nav.close()


def _run(navlib, name, host_rows=()):
    dev = Dev(navlib, sm.world(name))
    try:
        q, d = dev.check(host_rows)
    finally:
        dev.close()
    mq, md, info = sm.world(name).answers()
    assert np.array_equal(mq == sm.SQ_HOST, np.isin(np.arange(len(mq)), list(host_rows)))      # the HOST rows are the named ones
    return q, d, info


def _answers(info, c=None):
    """The answer tiles of every flood of the rows (source c, or both)."""
    return [a for inf in info if inf for s in ((0, 1) if c is None else (c,)) for a, depth in inf["floods"][s] if a is not None]


# ---- the cases ---------------------------------------------------------------------------------------------------------
def test_open_ground(navlib):
    q, d, info = _run(navlib, "open_ground")
    # the premise: at least 10 rows in which two answers with different corners are equally far, touching and not
    assert sum(1 for inf in info if inf and max(inf["ties"]) > 0) >= 10
    assert (q == sm.SQ_ADJACENT).sum() > 50 and (q == 6).sum() > 50
    w = sm.world("open_ground")
    assert sorted({sm.ntiles_of(w.radius[t]) for t in set(w.target[w.target >= 0].tolist())}) == [1, 2, 3]


def test_target_on_its_own_blockers(navlib):
    q, d, info = _run(navlib, "on_own_blockers")
    depths = {depth for inf in info if inf for a, depth in inf["floods"][0] if a is not None}
    assert min(depths) == 1 and max(depths) >= 4
    # distinct target tiles give distinct answers
    assert any(len({a for a, depth in inf["floods"][0]}) >= 4 for inf in info if inf and inf["floods"][0])
    assert (q == 6).sum() > 30


def test_map_corner_and_edge(navlib):
    q, d, info = _run(navlib, "map_corner_and_edge")
    w = sm.world("map_corner_and_edge")
    cells = {sm.tile_for_point(1, 1, *w.pos[t]) for t in set(w.target[w.target >= 0].tolist())}
    assert cells == {(0, 0), (63, 63), (0, 30)}
    for i, inf in enumerate(info):           # the circle is cut: fewer tiles than at the same spot of a tile in mid-map
        if inf:
            assert len(inf["tiles"]) < len(w.tiles_under(sm.xz(1, 1, 32, 32, (0.5, 0.5)), w.radius[w.target[i]]))
    assert (q == 6).sum() >= 8


def test_chunk_corner(navlib):
    q, d, info = _run(navlib, "chunk_corner")
    assert {(r // 64, c // 64) for r, c in _answers(info)} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_two_islands(navlib):
    q, d, info = _run(navlib, "two_islands")
    w = sm.world("two_islands")
    assert (q == 6).sum() >= 8
    far = [i for i, inf in enumerate(info) if inf and w.islands[sm.tile_for_point(1, 1, *w.pos[i])] == w.islands[0, 63]]
    assert len(far) >= 3 and all(c >= 33 for i in far for r, c in [a for a, dep in info[i]["floods"][1] if a])   # beyond the wall
    assert max(dep for i in far for a, dep in info[i]["floods"][1]) >= 6                     # ... past the near free tiles
    # pos and pos + new_vel on different islands, and the two dests differ
    split = [i for i, inf in enumerate(info) if inf and w.islands[sm.tile_for_point(1, 1, *w.pos[i])]
             != w.islands[sm.tile_for_point(1, 1, *(w.pos[i] + w.vel[i]))]]
    assert len(split) >= 2 and all((d[i, 0] != d[i, 1]).any() for i in split)
    # a source on impassable ground: island 0xffff, the answers are unblocked impassable tiles
    wall = [i for i, inf in enumerate(info) if inf and w.islands[sm.tile_for_point(1, 1, *w.pos[i])] == 0xffff]
    assert wall and all(w.cost[a] == 255 for i in wall for a, dep in info[i]["floods"][1] if a)
    assert any(q[i] & 4 for i in wall)


def test_nothing_reachable_on_a_map_that_fits_the_window(navlib):
    q, d, info = _run(navlib, "nothing_reachable")
    assert q.tolist() == [0, 0, 0, 6] and not d[:3].any()
    assert all(a is None for i in (1, 2) for s in (0, 1) for a, dep in info[i]["floods"][s]) and info[1]["tiles"]


def test_beyond_the_window(navlib):
    """Rows 2 and 3: the units' island has no free tile within 63 tiles of the target's tiles."""
    world, host_rows = sm.beyond_the_window()
    assert host_rows == (2, 3)
    q, d, info = _run(navlib, "beyond_the_window", host_rows)
    for i in host_rows:
        assert info[i]["host"] == "window" and min(dep for s in (0, 1) for a, dep in info[i]["floods"][s]) > 64
    assert q[4] == 6 and q[5] == 6


def test_two_layers_in_one_batch(navlib):
    q, d, info = _run(navlib, "two_layers")
    w = sm.world("two_layers")
    layers = np.array([w.layer_of(i) for i in range(w.n)])
    assert set(layers[1:].tolist()) == {0, 1} and set(w.radius[1:].tolist()) >= {np.float32(4.9), np.float32(5.0)}
    a0 = set(_answers([info[i] for i in np.flatnonzero(layers == 0) if info[i]]))
    a1 = set(_answers([info[i] for i in np.flatnonzero(layers == 1) if info[i]]))
    assert a0 - a1 and a1 - a0                          # the planes differ, and so do the answers


@pytest.fixture(scope="module")
def forms(navlib):
    """One world for the batch shapes: the open ground's rows and the blocked targets', with a static target, an oversized
    unit and an oversized target among them."""
    a, b = sm.world("open_ground"), sm.world("on_own_blockers")
    bl = b.blockers[0].copy()
    n = a.n
    pos = np.concatenate([a.pos, b.pos, [sm.xz(1, 1, 50, 8), sm.xz(1, 1, 58, 30), sm.xz(1, 1, 34, 34), sm.xz(1, 1, 30, 56)]])
    radius = np.concatenate([a.radius, b.radius, [2.0, 33.0, 32.5, 1.0]]).astype(np.float32)
    flags = np.concatenate([a.flags, b.flags, [0, sm.MOVABLE, sm.MOVABLE, sm.MOVABLE]]).astype(np.uint32)
    vel = np.concatenate([a.vel, b.vel, np.zeros((4, 2), np.float32)])
    target = np.concatenate([a.target, np.where(b.target >= 0, b.target + n, -1), [-1, 0, -1, -2]]).astype(np.int32)
    m = len(pos)
    static, big_unit, big_target = m - 4, m - 3, m - 2
    target[5], target[9], target[13] = static, big_target, -2
    w = sm.SWorld("forms", 1, 1, a.cost, {0: bl}, pos, radius, flags, vel, target)
    dev = Dev(navlib, w)
    yield dev, (5, 9, big_unit)
    dev.close()


@pytest.mark.parametrize("nq", [1, 64, 65, 1000])
def test_rows_and_forms(navlib, forms, nq):
    """nq rows in the sparse form equal the same units' rows of the dense form; targets -1, -2, a static target and
    ceil(radius / 4) above the window among them."""
    dev, host_rows = forms
    w = dev.world
    assert sm.ntiles_of(w.radius[host_rows[2]]) == 9 and sm.ntiles_of(32.0) == 8
    dense_q, dense_d = dev.check(host_rows)
    assert (dense_q == sm.SQ_HOST).sum() == 3 and set(w.target[w.target < 0].tolist()) == {-1, -2}
    units = np.array([(7 * i + 5) % w.n for i in range(nq)], np.int32) if nq > 1 else np.array([5], np.int32)
    q, d = dev.check(host_rows, units=units)
    assert np.array_equal(q, dense_q[units]) and np.array_equal(d.view(np.uint32), dense_d[units].view(np.uint32))
    if nq >= 64:
        assert {1, 6, sm.SQ_HOST} <= set(q.tolist())


def test_answers_follow_a_blocker_batch(navlib):
    """navhip_blockers_circles, then the queries again without an upload, then the reverse batch."""
    dev = Dev(navlib, sm.world("on_own_blockers"))
    w = dev.world
    before_q, before_d = dev.check()
    circles = np.zeros(3, navlib.CIRCLE_DTYPE)
    for i, ((r, c), rad) in enumerate((((20, 20), 14.0), ((46, 46), 9.0), ((40, 28), 6.0))):
        x, z = sm.xz(1, 1, r, c)
        circles[i] = (x, z, rad, 1, 0, 1)
        dev.nav.blockers_circle(x, z, rad, faction_id=1, flags=0, incref=True)
    dev.ctx.N_BlockersUpdate(circles)
    assert np.array_equal(dev.ctx.download_plane(0, navlib.PLANE_BLOCKERS), dev.nav.plane(pfref.PLANE_BLOCKERS, 0))
    after_q, after_d = dev.check()
    assert (before_d.view(np.uint32) != after_d.view(np.uint32)).any((1, 2)).sum() > 10
    circles["delta"] = -1
    for c in circles:
        dev.nav.blockers_circle(c["x"], c["z"], c["radius"], faction_id=1, flags=0, incref=False)
    dev.ctx.N_BlockersUpdate(circles)
    again_q, again_d = dev.check()
    assert np.array_equal(again_q, before_q) and np.array_equal(again_d.view(np.uint32), before_d.view(np.uint32))
    dev.close()


def test_resident_chain_into_the_state_update(navlib):
    """navhip_surround_queries_dev -> navhip_state_update_aux_dev without a host round trip, on the world of
    test_surround_arm_matches_entity_compute_update: states, flags and out_surround_dest_xz equal the run that is fed
    RefMove.surround_queries' arrays, and so do the queried arrays themselves."""
    import torch
    grid, nav, world, new_vel, vdes = cases.state_world(seed=9)
    n, k = len(world["state"]), len(world["flock_target_xz"])
    rng = np.random.RandomState(31)
    world["state"], world["vel_xz"] = world["state"].copy(), world["vel_xz"].copy()
    su = np.flatnonzero((rng.rand(n) < 0.3) & (world["radius"] < 5.0) & (world["flags"] & (1 << 18) == 0))
    world["state"][su] = 5
    world["vel_xz"][su[rng.rand(len(su)) < 0.4]] = 0
    tgt = np.full(n, -1, np.int32)
    for i in su:
        r = rng.rand()
        if r < 0.08:
            continue
        dist = np.linalg.norm(world["pos_xz"] - world["pos_xz"][i], axis=1)
        dist[i] = np.inf
        order = np.argsort(dist)
        tgt[i] = order[0] if r < 0.25 else order[rng.randint(3, 200)]
    t_prev = world["pos_xz"][np.maximum(tgt, 0)].copy()
    moved = rng.rand(n) < 0.5
    t_prev[moved] += rng.normal(0, 3.0, (moved.sum(), 2)).astype(np.float32)
    n_prev = (world["pos_xz"] + rng.normal(0, 6.0, (n, 2))).astype(np.float32)
    mv, _ = cases.ref_move_for(nav, world)
    try:
        mv.set_surround(tgt, t_prev, n_prev)
        query, dest = mv.surround_queries(new_vel)
    finally:
        pfref.RefMove.unload()
    dest = np.asarray(dest, np.float32).reshape(n, 2, 2)
    assert (query == 1).sum() > 20 and (query == 6).sum() > 200
    ctx = navlib.NavContext(4, 4)
    for layer in (0, 1):
        for plane, which in ((navlib.PLANE_COST_BASE, pfref.PLANE_COST), (navlib.PLANE_BLOCKERS, pfref.PLANE_BLOCKERS),
                             (navlib.PLANE_ISLANDS, pfref.PLANE_ISLANDS)):
            ctx.upload_plane(layer, plane, nav.plane(which, layer))
    arrays = cases.step_arrays(world, None)
    new_pos = (world["pos_xz"] + new_vel).astype(np.float32)
    st0, fl0 = world["state"].astype(np.uint8), np.full(n, navlib.SU_HOST, np.uint8)
    aux = {"fstate": np.zeros(n, np.uint8), "wait_ticks_left": np.full(n, 40, np.int32), "wait_prev": np.zeros(n, np.uint8)}
    surround = {"target": tgt, "query": query, "target_prev_xz": t_prev, "nearest_prev_xz": n_prev, "dest_xz": dest}
    want_st, want_fl, _, want_dest = ctx.state_update_aux(arrays, aux["fstate"], aux["wait_ticks_left"], aux["wait_prev"], new_pos,
                                                          st0, fl0, surround=surround, vdes_xz=vdes)
    is_su = (world["state"] == 5) & (world["flags"] & (1 << 18) == 0)
    assert not (want_fl[is_su] & navlib.SU_HOST).any() and (want_fl[is_su] & navlib.SU_SURROUND_DEST).any()

    dev = _dev()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    dt_of = dict(navlib._WORLD_ARRAYS)
    d_arrays = {name: t(a, dt_of[name]) for name, a in arrays.items() if a is not None}
    d_vel, d_tgt = t(new_vel, np.float32), t(tgt, np.int32)
    d_query = torch.full((n,), 0x55, dtype=torch.uint8, device=dev)
    d_dest = torch.full((n, 2, 2), 7.0, dtype=torch.float32, device=dev)
    d_in = {"fstate": t(aux["fstate"], np.uint8), "wait_ticks_left": t(aux["wait_ticks_left"], np.int32), "wait_prev": t(aux["wait_prev"], np.uint8),
            "new_pos_xz": t(new_pos, np.float32), "vdes_xz": t(vdes, np.float32), "surround_target": d_tgt, "surround_query": d_query,
            "surround_target_prev_xz": t(t_prev, np.float32), "surround_nearest_prev_xz": t(n_prev, np.float32),
            "surround_dest_xz": d_dest, "out_surround_dest_xz": torch.zeros((n, 2), dtype=torch.float32, device=dev)}
    d_state, d_flags, d_ticks = t(st0, np.uint8), t(fl0, np.uint8), torch.zeros(n, dtype=torch.int32, device=dev)
    _sync()
    w, keep = navlib.make_world(4, 4, d_arrays)
    ai = navlib.StateAuxIn()
    for name, a in d_in.items():
        setattr(ai, name, a.data_ptr())
    ctx.surround_queries_dev(w, d_vel, None, d_tgt, n, d_query, d_dest)
    rc = navlib.lib().navhip_state_update_aux_dev(ctx._h, C.byref(w), C.byref(ai), C.c_void_p(d_state.data_ptr()),
                                                  C.c_void_p(d_flags.data_ptr()), C.c_void_p(d_ticks.data_ptr()), None)
    assert rc == 0, ctx.last_error()
    ctx.sync()
    assert np.array_equal(d_query.cpu().numpy(), query)
    assert np.array_equal(d_dest.cpu().numpy().view(np.uint32), dest.view(np.uint32))
    assert np.array_equal(d_state.cpu().numpy(), want_st) and np.array_equal(d_flags.cpu().numpy(), want_fl)
    prev = (want_fl & navlib.SU_SURROUND_PREV) != 0          # (out_surround_dest_xz is written for these rows only)
    assert prev.sum() > 100
    assert np.array_equal(d_in["out_surround_dest_xz"].cpu().numpy()[prev].view(np.uint32), want_dest[prev].view(np.uint32))
    ctx.close()
    nav.close()


def test_argument_errors(navlib):
    """Each is refused with NAVHIP_ERR_ARG and its word in the message, and leaves the outputs untouched."""
    w = sm.world("two_layers")
    dev = Dev(navlib, w)
    L = navlib.lib()
    n = w.n
    base = {"pos_xz": w.pos, "radius": w.radius, "flags": w.flags}

    def call(arrays, vel, units, target, nq):
        world, keep = navlib.make_world(1, 1, dict(base, **arrays))
        for name in base:
            if name not in arrays:
                setattr(world, name, None)
        out = [np.full(max(nq, 1) + 2, 7, np.uint8), np.full((max(nq, 1) + 2, 2, 2), 7.0, np.float32)]
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
        rc = L.navhip_surround_queries(dev.ctx._h, C.byref(world), p(vel), p(units), p(target), nq, p(out[0]), p(out[1]))
        return rc, out

    def refused(word, arrays=base, vel=w.vel, units=None, target=w.target, nq=n):
        rc, out = call(arrays, vel, units, target, nq)
        assert rc == navlib.ERR_ARG and word in dev.ctx.last_error(), (rc, dev.ctx.last_error())
        assert all((a == 7).all() for a in out)

    rc, out = call(base, w.vel, None, w.target, n)
    assert rc == 0 and (out[0][:n] != 7).all() and (out[0][n:] == 7).all()
    for name in base:
        refused("missing", arrays={k: v for k, v in base.items() if k != name})
    refused("missing", vel=None)
    refused("missing", target=None)
    refused("negative", nq=-1)
    refused("dense", nq=n - 1)
    some = np.arange(4, dtype=np.int32)
    refused("outside the world", units=np.array([0, 1, n, 2], np.int32), target=w.target[:4].copy(), nq=4)
    refused("outside the world", units=np.array([0, -1, 1, 2], np.int32), target=w.target[:4].copy(), nq=4)
    big = w.radius.copy()
    big[3] = 10.0                                                       # layer 2 was never uploaded
    refused("planes", arrays=dict(base, radius=big), units=some, target=w.target[:4].copy(), nq=4)
    dev.close()
    # ... and a layer whose islands plane is missing
    dev = Dev(navlib, w, islands=False)
    refused("planes")
    dev.close()
