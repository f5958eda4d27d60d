"""The per-faction changed flags (navhip_faction_changed_chunks) and what follows them -- LOS chains whose slots carry a
faction, NAVHIP_REQ_IF_CHANGED for attacking paths -- against the reference build.

`changed` says "passability WITHOUT a faction differs".  An ally that steps onto tiles an enemy holds already changes no
such passability, but it changes what an attacking path of faction 0 (at war with faction 1) may cross: bit f of
fac_changed[chunk] says that the tiles faction f holds in the chunk differ.  The worlds, the batches and the numpy models
are tests/faction_chain_cases.py; every case asserts its premise from the reference alone.

Host buffers wherever the API allows (a chain's pool is the test's own tensor: host memory on the emulator): the file
also runs on the host emulator (tests/test_faction_changed_emulated_cpu.py), all but the wide level."""
import ctypes as C

import numpy as np
import pytest

from oracle import pfref
from tests import cases
from tests import faction_chain_cases as fc

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]

MODES = {"reference": 0, "downstream": 1}           # navhip_los_chain_refresh flags (NAVHIP_LOS_REFRESH_DOWNSTREAM)


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


def _ctx(navlib, name, factions=True):
    """A context with layers 0 and 1 of the world resident: the map and its standing units."""
    wd, planes = fc.world(name), fc.reference(name)["planes"][0]
    ctx = navlib.NavContext(wd["w"], wd["h"])
    for l in fc.LAYERS:
        ctx.upload_plane(l, navlib.PLANE_COST_BASE, planes[l]["cost"])
        ctx.upload_plane(l, navlib.PLANE_BLOCKERS, planes[l]["blockers"])
        ctx.upload_plane(l, navlib.PLANE_LOCAL_ISLANDS, planes[l]["local_islands"])
        if factions:
            ctx.upload_plane(l, navlib.PLANE_FACTIONS, planes[l]["factions"])
    return ctx


def _apply(navlib, ctx, name, steps):
    """The last batch of `steps` on the device (the earlier ones were applied before); both kinds of flags of both
    layers against the model of ALL of `steps`, the planes against the reference's.  Returns the flags of layer 0."""
    ctx.N_BlockersUpdate(fc.batch(name, steps[-1]))
    after = fc.reference(name, steps)["planes"][-1]
    for l in fc.LAYERS:
        fac, chg = fc.flag_model(name, steps, l)
        got_fac, got_chg = ctx.faction_changed_chunks(l), ctx.changed_chunks(l).astype(bool)
        print("%s %s layer %d: fac_changed %s changed %s" % (name, steps, l, got_fac.ravel().tolist(), got_chg.ravel().astype(int).tolist()))
        assert got_fac.dtype == np.uint16 and np.array_equal(got_fac, fac), (l, got_fac, fac)
        assert np.array_equal(got_chg, chg), (l, got_chg, chg)
        assert np.array_equal(ctx.download_plane(l, navlib.PLANE_FACTIONS), after[l]["factions"])
        assert np.array_equal(ctx.download_plane(l, navlib.PLANE_BLOCKERS), after[l]["blockers"])
    return ctx.changed_chunks(0).astype(bool), ctx.faction_changed_chunks(0)


# ---- 1. the flags ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["allies", "in_and_out", "second_unit", "corner"])
def test_flags_equal_the_model_of_the_reference_planes(navlib, which):
    """After one batch fac_changed is, on both layers, what the reference's factions plane before and after says; then
    navhip_clear_changed zeroes it."""
    fac, chg = fc.flag_model("3x3", (which,), 0)
    if which == "allies":           # (the world of the issue: allies onto enemy-held tiles, no chunk is flagged changed)
        assert not chg.any() and (fac == 1 << 2).any() and not (fac.astype(int) & ~(1 << 2)).any() and not (fac != 0).all()
    elif which in ("in_and_out", "second_unit"):
        planes = fc.reference("3x3", (which,))["planes"]
        assert not fac.any() and not chg.any()
        if which == "second_unit":  # (the counters moved, the masks did not)
            assert not np.array_equal(planes[0][0]["factions"], planes[1][0]["factions"])
    else:
        assert (fac != 0).sum() == 4 and (fac != 0)[:2, :2].all()
    ctx = _ctx(navlib, "3x3")
    for l in fc.LAYERS:             # (uploads raise neither kind of flag)
        assert not ctx.faction_changed_chunks(l).any() and not ctx.changed_chunks(l).any()
    _apply(navlib, ctx, "3x3", (which,))
    ctx.clear_changed()
    ctx.sync()
    for l in fc.LAYERS:
        assert not ctx.faction_changed_chunks(l).any() and not ctx.changed_chunks(l).any()
    ctx.close()


def test_flags_are_sticky_and_each_read_back_clears_its_own(navlib):
    """Two batches without a clear: the flags of the first stay.  navhip_changed_chunks(clear) leaves fac_changed alone,
    navhip_faction_changed_chunks(clear) clears it and nothing else."""
    steps = ("enemies", "corner")
    first, _ = fc.flag_model("3x3", steps[:1], 0)
    both, chg = fc.flag_model("3x3", steps, 0)
    # (the second batch raises bit 2 in four chunks; bit 1 of the first is still there in all nine)
    assert (first == 1 << 1).all() and (both & 1 << 1).all() and ((both & ~first) == 1 << 2).sum() == 4 and chg.sum() == 4
    ctx = _ctx(navlib, "3x3")
    _apply(navlib, ctx, "3x3", steps[:1])
    _apply(navlib, ctx, "3x3", steps)
    assert np.array_equal(ctx.changed_chunks(0, clear=True).astype(bool), chg)
    assert not ctx.changed_chunks(0).any() and np.array_equal(ctx.faction_changed_chunks(0), both)
    assert ctx.changed_chunks(1).any()                                  # (layer 1 was not cleared)
    assert np.array_equal(ctx.faction_changed_chunks(0, clear=True), both)
    assert not ctx.faction_changed_chunks(0).any()
    assert ctx.faction_changed_chunks(1).any() and ctx.changed_chunks(1).any()
    ctx.close()


def test_a_context_without_a_factions_plane_reads_zeros(navlib):
    ctx = _ctx(navlib, "3x3", factions=False)
    ctx.N_BlockersUpdate(fc.batch("3x3", "corner"))
    assert ctx.changed_chunks(0).any()
    out = ctx.faction_changed_chunks(0, clear=True)
    assert out.shape == (3, 3) and out.dtype == np.uint16 and not out.any()
    ctx.close()


# ---- 2. a chain with faction slots -------------------------------------------------------------------------------------
def _chain(navlib, name, kind):
    ctx = _ctx(navlib, name)
    reqs = fc.chain_reqs(name, kind)
    pool = _pool(len(reqs))
    chain = ctx.los_chain_create(reqs, fc.world(name)["prev_slot"], pool)
    chain.build()
    ctx.sync()                                                  # (the context's stream: the pool is read through torch's)
    return ctx, pool, chain


def test_faction_chain_builds_the_reference_fields(navlib):
    """Every slot carries faction 0: the pool equals N_LOSFieldCreate(faction 0) of the reference along the chain, and
    the faction bites -- the same chain without one gives other fields."""
    want, mixed = fc.ref_pool("3x3", "faction"), fc.ref_pool("3x3", "mixed")
    plain = fc.slot_fmask(fc.chain_reqs("3x3", "mixed")) == 0
    assert np.array_equal(want[~plain], mixed[~plain]) and not np.array_equal(want[plain], mixed[plain])
    ctx, pool, chain = _chain(navlib, "3x3", "faction")
    st = chain.stats()
    assert (st.slots, st.stale, st.rebuilt) == (len(want), 0, 0)
    got = _host(pool)
    bad = [i for i in range(len(got)) if not np.array_equal(got[i], want[i])]
    assert not bad, "LOS slots differ from the reference: %s" % bad
    chain.close()
    ctx.close()


def _refresh_case(navlib, name, kind, which, mode):
    steps = (which,)
    ctx, pool, chain = _chain(navlib, name, kind)
    before = _host(pool)
    assert np.array_equal(before, fc.ref_pool(name, kind))
    changed, fac_changed = _apply(navlib, ctx, name, steps)
    chain.refresh(MODES[mode])
    st = chain.stats()
    got = _host(pool)
    own, stale = fc.stale_model(name, kind, changed, fac_changed, mode == "downstream")
    print("%s %s %s %s: stale %d rebuilt %d of %d slots" % (name, kind, which, mode, st.stale, st.rebuilt, st.slots))
    assert (st.stale, st.rebuilt) == (int(own.sum()), int(stale.sum()))
    want = fc.ref_pool(name, kind, steps) if mode == "downstream" else fc.reference_mode(name, kind, steps, own)
    bad = [i for i in range(len(got)) if not np.array_equal(got[i], want[i])]
    assert not bad, "LOS slots differ from the reference: %s (stale: %s)" % (bad, np.flatnonzero(stale).tolist())
    assert np.array_equal(got[~stale], before[~stale])          # (nothing else was touched)
    # (a refresh clears nothing)
    assert np.array_equal(ctx.faction_changed_chunks(0), fac_changed) and np.array_equal(ctx.changed_chunks(0).astype(bool), changed)
    chain.close()
    ctx.close()
    return st, own, stale, before, got


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("which", ["allies", "enemies", "ordinary"])
def test_mixed_chain_refresh_after_a_blocker_batch(navlib, which, mode):
    """Destinations 0 and 1 carry faction 0, destinations 2 and 3 none.  downstream: the pool equals the reference's chain
    from scratch on the final planes; flags = 0: the pool before with exactly the slots stale by either flag rebuilt."""
    name, kind = "3x3", "mixed"
    with_faction = fc.slot_fmask(fc.chain_reqs(name, kind)) != 0
    at = (fc.chain_reqs(name, kind)["chunk_r"], fc.chain_reqs(name, kind)["chunk_c"])
    differs = (fc.ref_pool(name, kind) != fc.ref_pool(name, kind, (which,))).reshape(len(with_faction), -1).any(1)
    fac, chg = fc.flag_model(name, (which,), 0)
    # the premises, from the reference alone
    if which == "allies":           # a faction slot's field differs in a chunk that `changed` does not flag
        assert (differs & with_faction & ~chg[at]).any() and not differs[~with_faction].any()
    elif which == "enemies":        # flags are raised, but of an enemy: no faction slot's field differs
        assert not differs.any() and (fac == 1 << 1).all() and not chg.any()
    else:
        assert chg.any() and differs.any()
    st, own, stale, before, got = _refresh_case(navlib, name, kind, which, mode)
    if which == "allies":
        assert 0 < st.rebuilt < with_faction.sum() and not stale[~with_faction].any()
    elif which == "enemies":
        assert st.stale == st.rebuilt == 0 and np.array_equal(got, before)
    else:
        assert stale[with_faction].any() and stale[~with_faction].any() and st.rebuilt < st.slots


# ---- 3. a level wider than one step of k_los_mark ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_wide_level_takes_two_steps_of_the_mark_kernel(navlib, mode):
    """1 100 faction slots on level 0 (one per target tile of chunk (0, 0)) and their successors: k_los_mark walks each
    level in two steps of 1 024, with both parities of its counters.  The allies step into chunk (0, 0) only."""
    name, kind = "wide", "faction"
    level = fc.world(name)["level"]
    assert (level == 0).sum() == (level == 1).sum() == fc.WIDE_SLOTS > 1024
    fac, chg = fc.flag_model(name, ("allies",), 0)
    assert not chg.any() and fac.ravel().tolist() == [1 << 2, 0]
    differs = (fc.ref_pool(name, kind) != fc.ref_pool(name, kind, ("allies",))).reshape(len(level), -1).any(1)
    assert differs[level == 0].sum() > 100 and differs[level == 1].any() and not differs.all()
    st, own, stale, before, got = _refresh_case(navlib, name, kind, "allies", mode)
    assert st.stale == fc.WIDE_SLOTS and st.rebuilt == (2 if mode == "downstream" else 1) * fc.WIDE_SLOTS


# ---- 4. rejections and IF_CHANGED --------------------------------------------------------------------------------------
def test_create_rejects_faction_slots_it_cannot_follow(navlib):
    wd = fc.world("3x3")
    n = len(wd["reqs"])
    pool = _pool(n)
    first = int(np.flatnonzero(wd["prev_slot"] >= 0)[0])

    def create(ctx, reqs):
        h = C.c_void_p()
        mx, mz = ctx.map_pos()
        rc = navlib.lib().navhip_los_chain_create(ctx._h, reqs.ctypes.data_as(C.c_void_p),
                                                  wd["prev_slot"].ctypes.data_as(C.c_void_p), n,
                                                  C.c_void_p(pool.data_ptr()), mx, mz, C.byref(h))
        return rc, h, ctx.last_error()

    bare = _ctx(navlib, "3x3", factions=False)
    rc, h, text = create(bare, fc.chain_reqs("3x3", "mixed").copy())
    assert rc == navlib.ERR_INVALID and not h.value and text.startswith("navhip_los_chain_create: slot 0: "), text
    assert "factions plane" in text
    bare.close()

    ctx = _ctx(navlib, "3x3")
    for what in ("another faction_id", "faction_id 15 (none) behind a predecessor with a faction", "other enemies", "faction_id 16"):
        reqs = fc.chain_reqs("3x3", "faction").copy()
        slot = first
        if what == "another faction_id":
            reqs["faction_id"][first] = 2
        elif what.startswith("faction_id 15"):
            reqs["faction_id"][first], reqs["enemies"][first] = navlib.FACTION_ID_NONE, 0
        elif what == "other enemies":
            reqs["enemies"][first] = fc.ENEMIES | 0b100
        else:
            reqs["faction_id"][:] = 16
            slot = 0
        rc, h, text = create(ctx, reqs)
        assert rc == navlib.ERR_INVALID and not h.value, what
        assert text.startswith("navhip_los_chain_create: slot %d: " % slot) and len(text) > 40, (what, text)
        print("%-45s %s" % (what, text))
    chain = ctx.los_chain_create(fc.chain_reqs("3x3", "mixed"), wd["prev_slot"], pool)     # (the mixed chain is one)
    chain.close()
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_if_changed_rebuilds_the_attacking_fields_the_flags_name(navlib, mode):
    """After the allies' batch no chunk is flagged changed.  Tile requests with NAVHIP_REQ_IF_CHANGED, three per chunk --
    two of faction 0, one without a faction -- over sentinel-filled slots: exactly the faction requests on chunks whose
    fac_changed names a non-enemy are rebuilt, and equal the reference; every other slot keeps its sentinel."""
    name, steps = "3x3", ("allies",)
    wd = fc.world(name)
    ref = cases.tile_requests(wd["grid"], 27, seed=8)
    ref["chunk_r"], ref["chunk_c"] = np.arange(27) // 9, np.arange(27) // 3 % 3
    ref["faction_id"][np.arange(27) % 3 != 2] = 0
    with_faction = ref["faction_id"] == 0
    fac, chg = fc.flag_model(name, steps, 0)
    stale = with_faction & ((fac[ref["chunk_r"], ref["chunk_c"]] & fc.FMASK) != 0)
    nav0, nav1 = fc.reference(name)["nav"], fc.reference(name, steps)["nav"]
    fc.war()
    old, _ = cases.ref_fields(nav0, ref, None, want_integ=False)
    new, _ = cases.ref_fields(nav1, ref, None, want_integ=False)
    moved = (old != new).reshape(27, -1).any(1)
    assert not chg.any() and 0 < stale.sum() < with_faction.sum() and (moved & stale).any() and not (moved & ~stale).any()
    h = cases.reqs_from_ref(navlib, ref)
    h["enemies"] = np.where(with_faction, fc.ENEMIES, 0)
    h["flags"] = navlib.REQ_IF_CHANGED
    sentinel = np.full((27, 64, 64), 0xEE, np.uint8)
    ctx = _ctx(navlib, name)
    ctx.set_field_kernel(mode)
    got, _ = ctx.N_FlowFieldUpdate(h, inout=sentinel)
    assert np.array_equal(got, sentinel)                        # (nothing has changed yet: nothing is built)
    _apply(navlib, ctx, name, steps)
    got, _ = ctx.N_FlowFieldUpdate(h, inout=sentinel)
    rebuilt = (got != sentinel).reshape(27, -1).any(1)
    assert np.array_equal(rebuilt, stale), (np.flatnonzero(rebuilt).tolist(), np.flatnonzero(stale).tolist())
    assert np.array_equal(got[stale], new[stale])
    assert ctx.last_fields_split() == ((27, 0) if mode == 0 else (0, 27))
    ctx.clear_changed()
    ctx.sync()
    got, _ = ctx.N_FlowFieldUpdate(h, inout=sentinel)
    assert np.array_equal(got, sentinel)
    ctx.close()
