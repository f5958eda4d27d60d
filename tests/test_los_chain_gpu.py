"""Resident LOS chains (navhip_los_chain_*, csrc/los_chain_api.hip) against the reference build.

The reference drops the LOS fields of a dirty chunk with its flow fields (fieldcache.c:213-227, 526-535) and rebuilds a
missing one from the cached field of the chunk before it (nav.c:2026-2039, 4042-4047).  A chain does that on the device
behind a blocker batch: `refresh` marks the slots the changed chunks make stale and rebuilds them level by level.  Every
pool here is held bit for bit against N_LOSFieldCreate of the reference on the reference's own final planes
(tests/los_chain_cases.py), and the counters against a numpy model of which slots are stale."""
import ctypes as C

import numpy as np
import pytest

from oracle import pfref
from tests import los_chain_cases as lc

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


def _pool(n):
    """A zeroed pool, its memset (torch's stream) finished before the library's streams write into it."""
    import torch
    pool = torch.zeros((n, 4096), dtype=torch.uint8, device=_dev())
    _sync()
    return pool


def _host(pool):
    return pool.cpu().numpy().reshape(-1, 64, 64).copy()


def _world(navlib, name):
    """A context holding the map of `name` (no blockers yet) and a built chain over a fresh pool."""
    ch = lc.chain(name)
    ctx = navlib.NavContext(ch["w"], ch["h"])
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, lc.synth.to_chunks(ch["grid"]))
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, np.zeros((ch["h"], ch["w"], 64, 64), np.uint16))
    pool = _pool(len(ch["reqs"]))
    chain = ctx.los_chain_create(ch["reqs"], ch["prev_slot"], pool)
    chain.build()
    ctx.sync()                                                  # (the context's stream: the pool is read through torch's)
    return ch, ctx, pool, chain


def _apply(navlib, ctx, name, which):
    """The batch on the device; the chunks the device flags changed ([h][w] bool), held against the reference's dirty set
    and against the chunks the batch was made to hit."""
    circles, hit = lc.batch(name, which)
    ctx.N_BlockersUpdate(circles)
    changed = ctx.changed_chunks(0).astype(bool)
    assert not (changed & ~lc.reference(name, which)["dirty"]).any()
    assert np.array_equal(changed, hit), (changed, hit)
    for plane in (navlib.PLANE_BLOCKERS,):                      # (both sides work on the same final planes)
        assert np.array_equal(ctx.download_plane(0, plane), lc.reference(name, which)["nav"].plane(pfref.PLANE_BLOCKERS))
    return changed


@pytest.mark.parametrize("name", sorted(lc.MAPS))
def test_build_equals_the_reference_and_the_per_level_path(navlib, name):
    """`build` from an empty pool: N_LOSFieldCreate of the reference along the chain, and byte for byte what one
    navhip_build_los_dev per level gives from a gathered copy of the predecessors."""
    import torch
    ch, ctx, pool, chain = _world(navlib, name)
    got = _host(pool)
    st = chain.stats()
    assert (st.slots, st.levels) == (len(ch["reqs"]), int(ch["level"].max()) + 1)
    assert (st.stale, st.rebuilt) == (0, 0) and 0 <= st.redone <= st.slots
    assert np.array_equal(got, lc.reference(name, "dest_chunk")["before"])
    old = _pool(len(ch["reqs"]))
    d_reqs = torch.from_numpy(ch["reqs"].copy().view(np.uint8).reshape(-1, 16)).to(_dev())
    bounds = np.searchsorted(ch["level"], np.arange(st.levels + 1))
    for L in range(st.levels):
        b, e = int(bounds[L]), int(bounds[L + 1])
        prev = old.index_select(0, torch.from_numpy(ch["prev_slot"][b:e].astype(np.int64)).to(_dev())) if L else None
        _sync()                                                 # (index_select ran on torch's stream)
        ctx.build_los_dev(d_reqs[b:e], e - b, prev, old[b:e])
        ctx.sync()
    assert np.array_equal(got, _host(old))
    chain.close()
    ctx.close()


@pytest.mark.parametrize("mode", sorted(lc.MODES))
@pytest.mark.parametrize("which", [b for b in lc.BATCHES if b != "twice"])
@pytest.mark.parametrize("name", sorted(lc.MAPS))
def test_refresh_after_a_blocker_batch(navlib, name, which, mode):
    """Batches (a)-(e) of tests/los_chain_cases.py: the pool behind one refresh equals the reference's fields on ITS final
    planes (downstream: the whole chain from scratch; reference: the pool before the batch with exactly the slots on
    changed chunks rebuilt in slot order), the counters equal the numpy model of which slots are stale -- fewer than the
    chain has where something changed, none where the batch changed no passability -- and no other slot is written."""
    ch, ctx, pool, chain = _world(navlib, name)
    before = _host(pool)
    changed = _apply(navlib, ctx, name, which)
    chain.refresh(lc.MODES[mode])
    st = chain.stats()
    got = _host(pool)
    own, stale = lc.stale_model(ch, changed, mode == "downstream")
    print("%s %s %s: stale %d rebuilt %d of %d slots" % (name, which, mode, st.stale, st.rebuilt, st.slots))
    assert (st.stale, st.rebuilt) == (int(own.sum()), int(stale.sum()))
    if which in ("impassable", "in_and_out"):
        assert st.stale == st.rebuilt == 0 and np.array_equal(got, before)
    else:
        assert 0 < st.stale <= st.rebuilt < st.slots           # (not a full rebuild)
    want = lc.reference(name, which)["after"] if mode == "downstream" else lc.reference_mode(name, which, changed)
    bad = [i for i in range(len(got)) if not np.array_equal(got[i], want[i])]
    assert not bad, "LOS slots differ from the reference: %s (stale: %s)" % (bad, np.flatnonzero(stale).tolist())
    assert np.array_equal(got[~stale], before[~stale])          # (nothing else was touched)
    assert np.array_equal(ctx.changed_chunks(0).astype(bool), changed)   # (a refresh clears nothing)
    chain.close()
    ctx.close()


@pytest.mark.parametrize("mode", sorted(lc.MODES))
@pytest.mark.parametrize("name", sorted(lc.MAPS))
def test_refresh_twice_then_after_the_flags_are_cleared(navlib, name, mode):
    """(f): two refreshes without navhip_clear_changed between them rebuild the same set to the same bytes; a third one
    behind the clear rebuilds nothing."""
    ch, ctx, pool, chain = _world(navlib, name)
    changed = _apply(navlib, ctx, name, "twice")
    own, stale = lc.stale_model(ch, changed, mode == "downstream")
    want = lc.reference(name, "twice")["after"] if mode == "downstream" else lc.reference_mode(name, "twice", changed)
    for k in (1, 2):
        chain.refresh(lc.MODES[mode])
        st = chain.stats()
        assert (st.stale, st.rebuilt) == (k * int(own.sum()), k * int(stale.sum()))
        assert np.array_equal(_host(pool), want), k
    ctx.clear_changed()
    ctx.sync()
    chain.refresh(lc.MODES[mode])
    st = chain.stats()
    assert (st.stale, st.rebuilt) == (2 * int(own.sum()), 2 * int(stale.sum()))
    assert np.array_equal(_host(pool), want)
    chain.close()
    ctx.close()


def test_create_rejects_what_is_not_a_chain(navlib):
    ch = lc.chain("3x3")
    ctx = navlib.NavContext(ch["w"], ch["h"])
    for layer in (0, 1):                                            # (two resident layers: a slot may name the wrong one)
        ctx.upload_plane(layer, navlib.PLANE_COST_BASE, lc.synth.to_chunks(ch["grid"]))
    pool = _pool(len(ch["reqs"]))
    n = len(ch["reqs"])
    first = int(np.flatnonzero(ch["prev_slot"] >= 0)[0])            # the first slot with a predecessor (level 1)
    deep = int(np.flatnonzero(ch["level"] == 2)[0])
    other = int(np.flatnonzero((ch["dest"] != ch["dest"][first]) & (ch["prev_slot"] < 0))[0])

    def bad(what):
        reqs, prev = ch["reqs"].copy(), ch["prev_slot"].copy()
        if what == "no predecessor named":
            prev[first] = -1
        elif what == "predecessor named for a destination chunk":
            prev[1] = 0
        elif what == "predecessor is a later slot":
            prev[first] = first + 1
        elif what == "predecessor out of range":
            prev[first] = -2
        elif what == "predecessor on another chunk":
            reqs["prev_dr"][first], reqs["prev_dc"][first] = -reqs["prev_dr"][first], -reqs["prev_dc"][first]
        elif what == "predecessor with another target":
            same_chunk = [i for i in range(first) if (reqs["chunk_r"][i], reqs["chunk_c"][i]) ==
                          (reqs["chunk_r"][prev[first]], reqs["chunk_c"][prev[first]]) and i != prev[first]]
            if same_chunk:
                prev[first] = same_chunk[0]
            else:                                                   # (no such slot in front: move this one's target instead)
                reqs["target_tile_r"][first] ^= 1
        elif what == "predecessor on another layer":
            reqs["layer"][first] = 1
        elif what == "levels decrease":
            # a level-2 slot in front of a level-1 slot of another destination: both predecessors still come first
            j = deep - 1
            assert ch["level"][j] == 1 and ch["prev_slot"][deep] != j
            reqs[[j, deep]] = reqs[[deep, j]]
            prev[[j, deep]] = prev[[deep, j]]
            prev[prev == j] = -3
            prev[prev == deep] = j
            prev[prev == -3] = deep
        elif what == "layer not resident":
            reqs["layer"] = 2
        elif what == "faction":
            reqs["faction_id"][other] = 0
        else:
            raise KeyError(what)
        return reqs, prev

    for what in ("no predecessor named", "predecessor named for a destination chunk", "predecessor is a later slot",
                 "predecessor out of range", "predecessor on another chunk", "predecessor with another target",
                 "predecessor on another layer", "levels decrease", "layer not resident", "faction"):
        reqs, prev = bad(what)
        h = C.c_void_p()
        mx, mz = ctx.map_pos()
        # (a context's error text stays until the next failure: a marker shows that THIS call wrote one)
        rc = navlib.lib().navhip_los_chain_create(ctx._h, reqs.ctypes.data_as(C.c_void_p), prev.ctypes.data_as(C.c_void_p), n,
                                                  C.c_void_p(pool.data_ptr()), mx, mz, C.byref(h))
        assert rc == navlib.ERR_INVALID and not h.value, what
        text = ctx.last_error()
        assert text.startswith("navhip_los_chain_create: slot ") and len(text) > 40, (what, text)
        print("%-45s %s" % (what, text))
    with pytest.raises(navlib.NavHipError):
        ctx.los_chain_create(ch["reqs"][:0], ch["prev_slot"][:0], pool)
    chain = ctx.los_chain_create(ch["reqs"], ch["prev_slot"], pool)     # (the unmodified chain is one)
    with pytest.raises(navlib.NavHipError):
        chain.refresh(2)
    chain.close()
    ctx.close()


# ---- the tick ---------------------------------------------------------------------------------------------------------
TICK_KW = dict(chunk_w=4, fields_per_rank=1, agents_per_rank=600, flow_velocities=True, obstacles=60, obstacle_ticks=8,
               los=True)        # configs[0]'s 4 x 4-chunk world (its LOS fixture: data/los_cfg0.npz) with moving obstacles
TICKS = 8


def _run_tick(driver, los_repair, full_build=False, serial=False):
    from permafrost_engine_amd import tick
    T = tick.NavTick(driver=driver, serial=serial, los_repair=los_repair, **TICK_KW)
    assert T.n_los > 0 and (T.los_chain is not None) == (los_repair is not None)
    if full_build:
        T._los_refresh = lambda stream: T.los_chain.build(stream=stream)
    vel, status = [], []
    for _ in range(TICKS):
        T.step()
        T.sync()
        vel.append(T.t["vel_xz"].cpu().numpy().copy())
        status.append(T.status.cpu().numpy().copy())
    out = dict(vel=np.stack(vel), status=np.stack(status), pool=T.los_pool.cpu().numpy().copy(), driver=T.tick_driver,
               source=T.los_source, stats=T.los_chain.stats() if T.los_chain is not None else None)
    fresh = _pool(T.n_los)
    T._build_los_pool(fresh)
    out["fresh"] = fresh.cpu().numpy().copy()
    T.close()
    return out


@pytest.fixture(scope="module")
def tick_runs(navlib):
    return {"full": _run_tick("python", "downstream", full_build=True),
            "py": _run_tick("python", "downstream"), "c": _run_tick("c", "downstream"),
            "c_serial": _run_tick("c", "downstream", serial=True),
            "none_py": _run_tick("python", None), "none_c": _run_tick("c", None)}


def _same_ticks(a, b):
    assert np.array_equal(a["vel"].view(np.uint32), b["vel"].view(np.uint32))
    assert np.array_equal(a["status"], b["status"])


def test_tick_keeps_the_los_pool_current(tick_runs):
    """los_repair="downstream": after 8 ticks of moving obstacles the pool is the one a fresh build on the final planes
    gives, every tick's velocities and status bytes are those of a run that rebuilt the whole chain every tick, and the C
    tick enqueues what the Python schedule enqueues."""
    full, py, c = tick_runs["full"], tick_runs["py"], tick_runs["c"]
    assert py["driver"].startswith("python") and c["driver"].startswith("c (navhip_tick_run")
    for run in (full, py, c, tick_runs["c_serial"]):
        assert np.array_equal(run["pool"], run["fresh"])
        assert "navhip_los_chain_refresh" in run["source"]
    assert np.array_equal(full["fresh"], py["fresh"])
    assert 0 < py["stats"].stale <= py["stats"].rebuilt < TICKS * py["stats"].slots
    assert (c["stats"].stale, c["stats"].rebuilt) == (py["stats"].stale, py["stats"].rebuilt)
    _same_ticks(full, py)
    _same_ticks(py, c)
    _same_ticks(py, tick_runs["c_serial"])
    assert (py["status"] & 1).any()                                  # (somebody moved)
    # ... and it matters in this world: the fields of the start-up planes are no longer the current ones
    assert not np.array_equal(tick_runs["none_py"]["pool"], tick_runs["none_py"]["fresh"])


def test_tick_without_los_repair_is_unchanged(tick_runs):
    """los_repair=None is the default and today's tick: no chain object exists, the pool keeps the fields of the start-up
    planes for the whole run, and both drivers give what a NavTick made without the argument gives."""
    from permafrost_engine_amd import tick
    a, b = tick_runs["none_py"], tick_runs["none_c"]
    assert a["stats"] is None and "never rebuilt" in a["source"]
    T = tick.NavTick(driver="c", **TICK_KW)
    assert T.los_chain is None and T.los_repair is None
    start = T.los_pool.cpu().numpy().copy()
    vel, status = [], []
    for _ in range(TICKS):
        T.step()
        T.sync()
        vel.append(T.t["vel_xz"].cpu().numpy().copy())
        status.append(T.status.cpu().numpy().copy())
    plain = dict(vel=np.stack(vel), status=np.stack(status))
    assert np.array_equal(T.los_pool.cpu().numpy(), start)
    T.close()
    _same_ticks(plain, a)
    _same_ticks(plain, b)
    assert np.array_equal(a["pool"], start) and np.array_equal(b["pool"], start)
