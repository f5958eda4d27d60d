"""navhip_static_targets_set + navhip_surround_queries_ex[_dev] (csrc/surround_query_kernels.hip) against the reference
build: the surround queries of a unit whose target is a building.  The lists a test registers are M_Tile_AllUnderObj's, the
expected answers N_ObjAdjacentToStaticWith's and N_ClosestReachableAdjacentPosStatic's, all through ctypes on oracle/_ref's
library (tests/surround_static_model.py; tests/test_surround_static_cpu.py pins the calling convention and the model).
Everything is compared bit for bit: the query bytes, the floats as uint32.  Every case asserts its premise from the model or
the reference alone.  NAVHIP_SQ_HOST may come back in the window case and in the table-handling case only.

Two readings of the specification, both the existing rules of this unit:
  * a flood that finds nothing has to visit the whole map, and stays inside the window only on a map of one chunk: the
    "nothing reachable" case runs on a 1 x 1 map, every other case on 2 x 2 or 3 x 2;
  * the host form refuses a static row whose set is outside the table (NAVHIP_ERR_ARG, case 12); the device form, which
    cannot read the rows, returns NAVHIP_SQ_HOST for it (case 10).

Host buffers wherever the API allows; the file also runs on the host emulator (tests/test_surround_static_emulated_cpu.py),
where NAVHIP_STATIC_SMALL_CAP=1 shrinks the box of the cap case."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pfref
from tests import surround_model as sm
from tests import surround_static_model as ssm

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]


def _dev():
    import torch
    from permafrost_engine_amd import tick
    return torch.device("cpu") if tick.EMULATED else torch.device("cuda", 0)


class Dev:
    """A scene in the reference and on the device, its lists registered."""

    def __init__(self, navlib, sc, register=True):
        self.navlib, self.sc, self.world = navlib, sc, sc.world
        self.nav = sm.ref_nav(self.world)
        self.ref = ssm.Ref(self.nav)
        self.ctx = navlib.NavContext(sc.w, sc.h)
        for l in self.world.blockers:
            self.ctx.upload_plane(l, navlib.PLANE_COST_BASE, self.nav.plane(pfref.PLANE_COST, l))
            self.ctx.upload_plane(l, navlib.PLANE_BLOCKERS, self.nav.plane(pfref.PLANE_BLOCKERS, l))
            self.ctx.upload_plane(l, navlib.PLANE_ISLANDS, self.nav.plane(pfref.PLANE_ISLANDS, l))
        if register:
            self.ctx.static_targets_set(sc.lists)

    def arrays(self):
        w = self.world
        return {"pos_xz": w.pos, "radius": w.radius, "flags": w.flags}

    def query(self, units=None, target_set="scene"):
        w = self.world
        ts = self.sc.target_set if isinstance(target_set, str) else target_set
        tgt = w.target
        if units is not None:
            tgt, ts = tgt[units], None if ts is None else ts[units]
        return self.ctx.surround_queries(self.arrays(), w.vel, tgt, units, target_set=ts)

    def check(self, host_rows=(), units=None):
        """The static rows equal the reference's, bit for bit; exactly host_rows come back NAVHIP_SQ_HOST with nothing.
        Returns (query, dest) of the device, dense."""
        rows = self.sc.static_rows()
        exp_q, exp_d = self.ref.answers(self.sc)
        for i in host_rows:
            exp_q[i], exp_d[i] = self.navlib.SQ_HOST, 0
        q, d = self.query(units)
        idx = np.arange(self.world.n) if units is None else np.asarray(units)
        assert q.dtype == np.uint8 and d.shape == (len(idx), 2, 2)
        st = np.isin(idx, rows)
        bad = np.flatnonzero(st & ((q != exp_q[idx]) | (d.view(np.uint32) != exp_d[idx].view(np.uint32)).any((1, 2))))
        assert len(bad) == 0, [(int(idx[i]), int(q[i]), int(exp_q[idx[i]]), d[i].tolist(), exp_d[idx[i]].tolist()) for i in bad[:6]]
        assert st.sum() > 0
        return q, d

    def close(self):
        self.ctx.close()
        self.nav.close()


def _run(navlib, *name, host_rows=()):
    sc = ssm.scene(*name)
    dev = Dev(navlib, sc)
    try:
        q, d = dev.check(host_rows)
    finally:
        dev.close()
    mq, md, info = ssm.answers(sc)
    assert sorted(np.flatnonzero(mq == sm.SQ_HOST).tolist()) == sorted(host_rows)       # the HOST rows are the named ones
    if not host_rows and name[0] != "window":
        assert ssm.max_depth(info) <= sm.WINDOW                                          # every flood ends within 63 tiles
    return sc, q, d, info


# ---- the cases ---------------------------------------------------------------------------------------------------------
def test_axis_aligned_boxes(navlib):
    sc, q, d, info = _run(navlib, "axis_aligned")
    w = sc.world
    sizes = [(int(np.ptp(t[:, 0])) + 1, int(np.ptp(t[:, 1])) + 1) for t in sc.lists]
    assert sizes == [(1, 1), (5, 3), (10, 10)], sizes
    rows = sc.static_rows()
    assert (q[rows] == sm.SQ_ADJACENT).sum() > 40 and (q[rows] == 6).sum() > 100
    assert min(w.radius[rows]) == np.float32(0.5) and max(w.radius[rows]) == np.float32(32.0)
    assert {w.layer_of(i) for i in rows} == {0, 1, 2, 3}
    # a diagonal neighbour touches (|d row| = |d col| = 1), a unit two tiles away with a circle inside its tile does not
    diag = two = 0
    for i in rows:
        if w.radius[i] > 1.0:
            continue
        ut = sm.tile_for_point(sc.w, sc.h, *w.pos[i])
        t = sc.lists[sc.target_set[i]].astype(int)
        dr, dc = np.abs(t[:, 0] - ut[0]), np.abs(t[:, 1] - ut[1])
        cheb = np.maximum(dr, dc).min()
        if cheb == 1 and not ((dr + dc) == 1).any():
            assert q[i] == sm.SQ_ADJACENT
            diag += 1
        if cheb == 2:
            assert q[i] != sm.SQ_ADJACENT
            two += 1
    assert diag >= 3 and two >= 6


def test_rotated_boxes_and_the_tie(navlib):
    sc, q, d, info = _run(navlib, "rotated")
    for t in sc.lists:                                   # duplicates exist; the order is not row-major
        first = ssm.first_occurrences(t)
        assert len(t) > len(first) and first != sorted(first)
    # the tie: two different answer tiles equally far, the winner is the earlier list entry and NOT the row-major-first
    ties = [(i, c) for i, inf in enumerate(info) if inf for c in (0, 1)
            if inf["closest"][c] and inf["closest"][c]["tied"] and min(inf["closest"][c]["tied"]) < inf["closest"][c]["tile"]]
    assert len(ties) >= 10
    vq, vd, _ = ssm.answers(sc, key="tile")               # a pick keyed on the tile's position gives other floats there
    for i, c in ties:
        got = info[i]["closest"][c]
        assert np.array_equal(d[i, c], sm.corner(sc.w, sc.h, *got["tile"]))
        assert not np.array_equal(d[i, c].view(np.uint32), vd[i, c].view(np.uint32))


def test_chunk_corner_and_map_edge(navlib):
    sc, q, d, info = _run(navlib, "chunk_corner_and_edge")
    assert {(r // 64, c // 64) for r, c in sc.lists[0].tolist()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert sc.lists[1][:, 0].min() == 0 and sc.lists[2][:, 1].max() == 127        # the rings of their floods are clipped
    assert (q[sc.static_rows()] == 6).sum() > 40


def test_sources_on_two_islands(navlib):
    sc, q, d, info = _run(navlib, "two_islands")
    w = sc.world
    isl = lambda p: w.islands[sm.tile_for_point(sc.w, sc.h, *p)]      # noqa: E731
    split = [i for i in sc.static_rows() if isl(w.pos[i]) != isl(w.pos[i] + w.vel[i])]
    assert len(split) >= 6 and all(0xffff not in (isl(w.pos[i]), isl(w.pos[i] + w.vel[i])) for i in split)
    assert all(q[i] == 6 and (d[i, 0] != d[i, 1]).any() for i in split)


def test_nothing_reachable(navlib):
    sc, q, d, info = _run(navlib, "nothing_reachable")
    rows = sc.static_rows()
    assert q[rows].tolist() == [0, 0, 6] and not d[rows[:2]].any()
    assert all(a is None for i in rows[:2] for got in info[i]["closest"] for a, dep in got["floods"])


def test_the_cap(navlib):
    """A box of about 45 x 45 tiles: the reference's list is cut at 2 048 entries.  Two rows, the reference alone."""
    small = bool(os.environ.get("NAVHIP_STATIC_SMALL_CAP"))
    sc = ssm.scene("cap", 12 if small else 45)
    if not small:
        assert len(sc.lists[0]) == ssm.CAP == 2048
    assert len(sc.static_rows()) == 2
    dev = Dev(navlib, sc)
    try:
        q, d = dev.check()
    finally:
        dev.close()
    assert q[sc.static_rows()].tolist() == [6, 6]


def test_the_window(navlib):
    """The set is the tiles (64, 91) and (64, 90) in ground that is blocked but for one column.  Column 154: 63 tiles from
    the first entry and 64 from the second, whose flood still tests the ring it stops on -- answered.  Column 155: 64 from
    the first and 65 from the second, whose flood would have to push tiles outside the window -- the host's."""
    for col, host in ((154, False), (155, True)):
        sc = ssm.scene("window", col)
        assert ssm.first_occurrences(sc.lists[0]) == [(64, 91), (64, 90)]
        rows = sc.static_rows()
        sc2, q, d, info = _run(navlib, "window", col, host_rows=rows if host else ())
        depths = sorted({dep for i in rows for got in info[i]["closest"] for a, dep in got["floods"]})
        assert depths == ([64, 65] if host else [63, 64])
        assert (q[rows] == (sm.SQ_HOST if host else 6)).all()


@pytest.fixture(scope="module")
def mixed(navlib):
    sc = ssm.scene("mixed", 257)
    dev = Dev(navlib, sc)
    yield dev
    dev.close()


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257])
def test_mixed_batches(navlib, mixed, nq):
    """No-target, movable and static rows on layers 0 and 2 in one sparse batch: the first two kinds equal
    navhip_surround_queries on the same inputs, the static rows the reference."""
    dev, sc, w = mixed, mixed.sc, mixed.world
    units = np.array([(7 * i + 2) % w.n for i in range(nq)], np.int32) if nq > 1 else np.array([sc.static_rows()[0]], np.int32)
    q, d = dev.check(units=units)
    pq, pd = dev.query(units, target_set=None)
    st = np.isin(units, sc.static_rows())
    assert (pq[st] == sm.SQ_HOST).all() and not (q == sm.SQ_HOST).any()
    assert np.array_equal(q[~st], pq[~st]) and np.array_equal(d[~st].view(np.uint32), pd[~st].view(np.uint32))
    if nq >= 63:
        kinds = w.target[units]
        assert (kinds < 0).any() and st.any() and ((kinds >= 0) & ~st).any() and (pq[~st] == 6).any()
        assert {w.layer_of(i) for i in units[st]} == {0, 2}


def test_table_handling(navlib):
    import torch
    sc = ssm.scene("axis_aligned")
    w, rows = sc.world, sc.static_rows()
    dev = Dev(navlib, sc, register=False)
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())      # noqa: E731
        d_arrays = {k: t(v) for k, v in dev.arrays().items()}
        world, keep = navlib.make_world(sc.w, sc.h, d_arrays)
        d_vel, d_tgt = t(w.vel), t(w.target)

        def dev_form(target_set):
            d_q = torch.full((w.n,), 0x55, dtype=torch.uint8, device=_dev())
            d_d = torch.full((w.n, 2, 2), 7.0, dtype=torch.float32, device=_dev())
            dev.ctx.surround_queries_dev(world, d_vel, None, d_tgt, w.n, d_q, d_d, d_target_set=None if target_set is None else t(target_set))
            dev.ctx.sync()
            return d_q.cpu().numpy(), d_d.cpu().numpy()

        def all_host(q, d):
            return (q[rows] == sm.SQ_HOST).all() and not d[rows].any()

        assert all_host(*dev_form(sc.target_set))                                 # no table yet
        dev.ctx.static_targets_set(sc.lists)
        q1, d1 = dev.check()
        assert not (q1 == sm.SQ_HOST).any()
        dq, dd = dev_form(sc.target_set)
        assert np.array_equal(dq, q1) and np.array_equal(dd.view(np.uint32), d1.view(np.uint32))
        assert all_host(*dev.query(target_set=None)) and all_host(*dev_form(None))        # NULL: as before
        assert all_host(*dev_form(np.full(w.n, -1, np.int32)))                    # -1
        assert all_host(*dev_form(np.full(w.n, len(sc.lists), np.int32)))         # beyond the table
        dev.ctx.static_targets_set([])                                            # cleared
        assert all_host(*dev_form(sc.target_set))
        # other lists under the same numbers: the answers follow the new table
        other = [sc.lists[2], sc.lists[0], sc.lists[1]]
        dev.ctx.static_targets_set(other)
        q2, d2 = dev.query()
        exp_q, exp_d = np.zeros(w.n, np.uint8), np.zeros((w.n, 2, 2), np.float32)
        perm = {0: 2, 1: 0, 2: 1}
        for i in rows:
            obb = sc.obbs[perm[int(sc.target_set[i])]]
            if dev.ref.adjacent(w.pos[i], w.radius[i], obb):
                exp_q[i] = sm.SQ_ADJACENT
                continue
            for c, src in enumerate((w.pos[i] + w.vel[i], w.pos[i])):
                ok, p = dev.ref.closest(w.layer_of(i), src, obb)
                if ok:
                    exp_q[i] |= sm.SQ_HAS_DEST_0 << c
                    exp_d[i, c] = p
        assert np.array_equal(q2[rows], exp_q[rows]) and np.array_equal(d2[rows].view(np.uint32), exp_d[rows].view(np.uint32))
        assert (q2[rows] != q1[rows]).any() or (d2[rows] != d1[rows]).any()
    finally:
        dev.close()


def test_resident_chain_with_a_blocker_batch(navlib):
    """query -> navhip_blockers_circles_dev (a unit stops beside the building) -> query, on one stream without a sync."""
    import torch
    sc = ssm.scene("chunk_corner_and_edge")
    assert sorted(sc.world.blockers) == [0]
    w, rows = sc.world, sc.static_rows()
    dev = Dev(navlib, sc)
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())      # noqa: E731
        d_arrays = {k: t(v) for k, v in dev.arrays().items()}
        world, keep = navlib.make_world(sc.w, sc.h, d_arrays)
        d_vel, d_tgt, d_set = t(w.vel), t(w.target), t(sc.target_set)
        out = [(torch.full((w.n,), 0x55, dtype=torch.uint8, device=_dev()), torch.full((w.n, 2, 2), 7.0, dtype=torch.float32, device=_dev()))
               for _ in range(2)]
        # the unit stops on the tiles above the box across the chunk corner: its disc blocks what were answers
        top = int(sc.lists[0][:, 0].min())
        x, z = sm.xz(sc.w, sc.h, top - 2, 64)
        circles = np.zeros(1, navlib.CIRCLE_DTYPE)
        circles[0] = (x, z, 6.0, 1, 0, 1)
        d_circles = torch.from_numpy(circles.view(np.uint8)).to(_dev())
        before = dev.ref.answers(sc)
        dev.nav.blockers_circle(x, z, 6.0, faction_id=1, flags=0, incref=True)
        after = dev.ref.answers(sc)
        dev.ctx.sync()
        dev.ctx.surround_queries_dev(world, d_vel, None, d_tgt, w.n, out[0][0], out[0][1], d_target_set=d_set)
        dev.ctx.blockers_circles_dev(d_circles, 1)
        dev.ctx.surround_queries_dev(world, d_vel, None, d_tgt, w.n, out[1][0], out[1][1], d_target_set=d_set)
        dev.ctx.sync()
        for (dq, dd), (rq, rd) in zip(out, (before, after)):
            q, d = dq.cpu().numpy(), dd.cpu().numpy()
            assert np.array_equal(q[rows], rq[rows]) and np.array_equal(d[rows].view(np.uint32), rd[rows].view(np.uint32))
        assert (before[1][rows].view(np.uint32) != after[1][rows].view(np.uint32)).any()
        for l in w.blockers:
            assert np.array_equal(dev.ctx.download_plane(l, navlib.PLANE_BLOCKERS), dev.nav.plane(pfref.PLANE_BLOCKERS, l))
    finally:
        dev.close()


def test_argument_errors(navlib):
    """Each is refused with NAVHIP_ERR_ARG and its word in the message; a refused query leaves the outputs untouched, a
    refused registration the table."""
    sc = ssm.scene("chunk_corner_and_edge")
    w, rows = sc.world, sc.static_rows()
    dev = Dev(navlib, sc)
    L = navlib.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    try:
        good_q, good_d = dev.check()

        def set_refused(word, n_sets, off, tiles):
            off, tiles = np.asarray(off, np.int32), np.asarray(tiles, np.int16).reshape(-1, 2)
            rc = L.navhip_static_targets_set(dev.ctx._h, n_sets, p(off), p(tiles))
            assert rc == navlib.ERR_ARG and word in dev.ctx.last_error(), (rc, dev.ctx.last_error())
            q, d = dev.query()                                         # the table is as it was
            assert np.array_equal(q, good_q) and np.array_equal(d.view(np.uint32), good_d.view(np.uint32))

        one = [(3, 3), (3, 4)]
        set_refused("non-monotonic", 2, [0, 2, 1], one)
        set_refused("non-monotonic", 1, [-1, 1], one)
        set_refused("longer than 2048", 1, [0, 2049], [(5, 5)] * 2049)
        set_refused("off the map", 1, [0, 2], [(3, 3), (128, 4)])
        set_refused("off the map", 1, [0, 2], [(3, 3), (4, -1)])
        rc = L.navhip_static_targets_set(dev.ctx._h, 1, None, p(np.zeros((2, 2), np.int16)))
        assert rc == navlib.ERR_ARG and "missing" in dev.ctx.last_error()
        rc = L.navhip_static_targets_set(dev.ctx._h, -1, None, None)
        assert rc == navlib.ERR_ARG and "negative" in dev.ctx.last_error()
        # a list of exactly 2 048 entries is taken
        full = np.array([(r, c) for r in range(32) for c in range(64)], np.int16)
        dev.ctx.static_targets_set([full])
        dev.ctx.static_targets_set(sc.lists)

        base = dev.arrays()

        def refused(word, arrays=base, vel=w.vel, units=None, target=w.target, target_set=sc.target_set, nq=w.n):
            world, keep = navlib.make_world(sc.w, sc.h, dict(base, **arrays))
            for name in base:
                if name not in arrays:
                    setattr(world, name, None)
            out = [np.full(max(nq, 1) + 2, 7, np.uint8), np.full((max(nq, 1) + 2, 2, 2), 7.0, np.float32)]
            rc = L.navhip_surround_queries_ex(dev.ctx._h, C.byref(world), p(vel), p(units), p(target), p(target_set), nq, p(out[0]), p(out[1]))
            assert rc == navlib.ERR_ARG and word in dev.ctx.last_error(), (rc, dev.ctx.last_error())
            assert all((a == 7).all() for a in out)

        ts = sc.target_set.copy()
        ts[rows[3]] = len(sc.lists)
        refused("outside the table", target_set=ts)
        ts[rows[3]] = -1
        refused("outside the table", target_set=ts)
        for name in base:
            refused("missing", arrays={k: v for k, v in base.items() if k != name})
        refused("missing", vel=None)
        refused("missing", target=None)
        refused("negative", nq=-1)
        refused("dense", nq=w.n - 1)
        some = np.array(rows[:4], np.int32)
        bad_units = some.copy()
        bad_units[2] = w.n
        refused("outside the world", units=bad_units, target=w.target[some].copy(), target_set=sc.target_set[some].copy(), nq=4)
        big = w.radius.copy()
        big[some[1]] = 20.0                                                  # layer 3 was never uploaded
        refused("planes", arrays=dict(base, radius=big), units=some, target=w.target[some].copy(),
                target_set=sc.target_set[some].copy(), nq=4)
        dev.ctx.static_targets_set([])
        refused("outside the table")                                         # an empty table
    finally:
        dev.close()
