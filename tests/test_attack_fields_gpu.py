"""Attacking-path chunk fields (faction_id != NONE: tiles blocked by enemy factions only are passable,
field_tile_passable_no_enemies field.c:179-201) on the bit-parallel wave kernel: parity of both kernels with the
reference's own N_FlowFieldUpdate (oracle/_ref), bit for bit, WHICH kernel built what (navhip_last_fields_split), and
every writer of the factions plane -- uploads, the device-side blocker updates -- seen by the next build.

Host buffers only: the file also runs on the host emulator (tests/test_attack_fields_emulated_cpu.py)."""
import numpy as np
import pytest

from oracle import pfref
from tests import cases

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]

synth = cases.synth
ENEMIES = 0b010             # faction 0 is at war with faction 1 (cases.faction_cases)


def _war():
    for f in range(16):
        pfref.set_enemy_factions(f, ENEMIES if f == 0 else 0)


def _ctx_for(navlib, nav, factions=True):
    ctx = navlib.NavContext(nav.w, nav.h)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, nav.plane(pfref.PLANE_COST))
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, nav.plane(pfref.PLANE_BLOCKERS))
    ctx.upload_plane(0, navlib.PLANE_LOCAL_ISLANDS, nav.plane(pfref.PLANE_LOCAL_ISLANDS))
    if factions:
        ctx.upload_plane(0, navlib.PLANE_FACTIONS, nav.plane(pfref.PLANE_FACTIONS))
    return ctx


def _hip_reqs(navlib, reqs):
    h = cases.reqs_from_ref(navlib, reqs)
    h["enemies"] = np.where(h["faction_id"] != navlib.FACTION_ID_NONE, ENEMIES, 0)
    return h


def _assert_fields(ctx, h, exp_dirs, exp_integ, before=None):
    """Both template instances of the BFS kernel (with / without the integration output) against the reference."""
    dirs, integ = ctx.N_FlowFieldUpdate(h, inout=before, want_integ=True)
    bad = np.argwhere((dirs != exp_dirs).reshape(len(h), -1).any(1)).ravel()
    assert bad.size == 0, "flow dirs differ for requests %s (first: %s)" % (bad[:8], h[bad[0]])
    assert np.array_equal(integ, exp_integ), "integration field differs"
    dirs2, _ = ctx.N_FlowFieldUpdate(h, inout=before, want_integ=False)
    assert np.array_equal(dirs2, exp_dirs)


def _case_circles(navlib, seed, n_circles=60):
    """The circles cases.faction_cases(seed) laid (the same draws from the same generator), as navhip_circle records."""
    rng = np.random.RandomState(seed)
    grid = synth.cost_grid(3, 3, seed=90 + seed, frac_impassable=0.15)
    cells = synth.passable_cells(grid)
    pos = synth.cell_centre(3, 3, *cells[rng.randint(len(cells), size=n_circles)].T)
    c = np.zeros(n_circles, navlib.CIRCLE_DTYPE)
    c["x"], c["z"], c["delta"] = pos[:, 0], pos[:, 1], 1
    for i in range(n_circles):
        c["radius"][i] = rng.uniform(3, 10)
        c["faction_id"][i] = rng.randint(0, 3)
    return grid, c


def _ref_apply(nav, circles):
    for c in circles:
        nav.blockers_circle(float(c["x"]), float(c["z"]), float(c["radius"]), faction_id=int(c["faction_id"]),
                            incref=bool(c["delta"] > 0))
    nav.flush_dirty()


def _ref_with(grid, circles):
    nav = pfref.RefNav(synth.to_chunks(grid))
    _ref_apply(nav, circles)
    return nav


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_attacking_fields_match_reference_on_both_kernels(navlib, seed, mode):
    """Tile and portal requests of faction 0 on a map held by three factions: directions and integration values of
    either kernel equal the reference's; mode 0 keeps every request on the BFS kernel, mode 1 on the generic one."""
    grid, nav, reqs, enemies, exp_dirs, exp_integ = cases.faction_cases(seed)
    assert enemies == ENEMIES
    ctx = _ctx_for(navlib, nav)
    with pytest.raises(navlib.NavHipError):
        ctx.last_fields_split()                      # nothing built yet
    ctx.set_field_kernel(mode)
    h = _hip_reqs(navlib, reqs)
    _assert_fields(ctx, h, exp_dirs, exp_integ)
    n = len(h)
    assert ctx.last_fields_split() == ((n, 0) if mode == 0 else (0, n))
    # the faction bites: the same requests without one give other fields somewhere
    plain = reqs.copy()
    plain["faction_id"] = pfref.FACTION_ID_NONE
    assert not np.array_equal(cases.ref_fields(nav, plain, None, want_integ=False)[0], exp_dirs)
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_attacking_inplace_requests_match_reference(navlib, seed, mode):
    """The planner's request stream stamped with a faction, a dozen of them updating an EXISTING field in place
    (unreached cells keep their bytes, field.c:737-751)."""
    grid, nav, _r, _e, _d, _i = cases.faction_cases(seed)
    reqs, before, _after = cases.planner_requests(nav, grid, pairs=12, seed=20 + seed)
    reqs["faction_id"] = 0
    reqs, before = cases.with_inplace(reqs, before, seed=seed, count=12)
    assert (reqs["type"] == 0).sum() > 8 and (reqs["inout"] != 0).sum() >= 12
    exp_dirs, exp_integ = cases.ref_fields(nav, reqs, before)
    ctx = _ctx_for(navlib, nav)
    ctx.set_field_kernel(mode)
    h = _hip_reqs(navlib, reqs)
    _assert_fields(ctx, h, exp_dirs, exp_integ, before)
    assert ctx.last_fields_split() == ((len(h), 0) if mode == 0 else (0, len(h)))
    ctx.close()


def test_split_follows_costs_and_repair_builds(navlib):
    """One chunk of the map has costs 1..4: exactly its requests go to the generic kernel (and still equal the
    reference), every other faction request stays on the BFS kernel; a NEAREST_PATHABLE repair with a faction goes
    to the generic kernel as well."""
    rng = np.random.RandomState(7)
    grid = synth.cost_grid(3, 3, seed=95, frac_impassable=0.15)
    sub = grid[64:128, 64:128]
    sub[sub != 255] = rng.randint(1, 5, size=int((sub != 255).sum())).astype(np.uint8)
    assert (sub[sub != 255] > 1).any() and set(np.unique(grid)) - {1, 2, 3, 4, 255} == set()
    c = synth.faction_circles(grid, 60, seed=3)
    circles = np.zeros(60, navlib.CIRCLE_DTYPE)
    for k in ("x", "z", "radius", "faction_id"):
        circles[k] = c[k]
    circles["delta"] = 1
    nav = _ref_with(grid, circles)
    _war()
    reqs = cases.tile_requests(grid, 40, seed=4)
    reqs["faction_id"] = 0
    reqs["chunk_r"][:6] = reqs["chunk_c"][:6] = 1                # some for sure in the chunk with real costs
    costly = (reqs["chunk_r"] == 1) & (reqs["chunk_c"] == 1)
    exp_dirs, exp_integ = cases.ref_fields(nav, reqs, None)
    ctx = _ctx_for(navlib, nav)
    h = _hip_reqs(navlib, reqs)
    _assert_fields(ctx, h, exp_dirs, exp_integ)
    assert ctx.last_fields_split() == (int((~costly).sum()), int(costly.sum())) and 6 <= costly.sum() < len(h)
    # ... and a repair build with a faction on a unit-cost chunk
    blocked = np.argwhere(nav.plane(pfref.PLANE_BLOCKERS)[0, 0] > 0)
    assert len(blocked)
    rep = navlib.make_reqs(1)
    rep["type"], rep["faction_id"], rep["enemies"] = navlib.TARGET_NEAREST_PATHABLE, 0, ENEMIES
    rep["tile_r"], rep["tile_c"] = blocked[0]
    both = np.concatenate([h, rep])
    got, _ = ctx.N_FlowFieldUpdate(both, inout=np.zeros((len(both), 64, 64), np.uint8))
    assert np.array_equal(got[:len(h)], exp_dirs)
    assert ctx.last_fields_split() == (int((~costly).sum()), int(costly.sum()) + 1)
    ctx.close()


@pytest.mark.parametrize("seed", [1, 3])
def test_device_blocker_updates_reach_the_faction_rows(navlib, seed):
    """Units of faction 2 (no enemy) step exactly onto the tiles units of faction 1 (an enemy) hold already, then
    leave again: the passability WITHOUT a faction never changes -- no chunk is flagged changed -- but what an
    attacking path of faction 0 may cross does, and the BFS kernel's fields follow the reference's both times."""
    grid, nav, reqs, _e, exp0, exp0_integ = cases.faction_cases(seed)
    _g, circ = _case_circles(navlib, seed)
    twin = _ref_with(grid, circ)                     # (the replayed circles are the case's own)
    for plane in (pfref.PLANE_BLOCKERS, pfref.PLANE_FACTIONS, pfref.PLANE_LOCAL_ISLANDS):
        assert np.array_equal(twin.plane(plane), nav.plane(plane))
    over = circ[circ["faction_id"] == 1].copy()
    over["faction_id"] = 2
    ctx = _ctx_for(navlib, nav)
    h = _hip_reqs(navlib, reqs)
    _assert_fields(ctx, h, exp0, exp0_integ)
    ctx.changed_chunks(0, clear=True)
    occupied0 = nav.plane(pfref.PLANE_BLOCKERS) > 0
    stages, flags = [], []
    for delta in (1, -1):
        over["delta"] = delta
        _ref_apply(nav, over)
        ctx.N_BlockersUpdate(over)
        exp_dirs, exp_integ = cases.ref_fields(nav, reqs, None)
        _assert_fields(ctx, h, exp_dirs, exp_integ)
        assert ctx.last_fields_split() == (len(h), 0)
        assert np.array_equal(ctx.download_plane(0, navlib.PLANE_FACTIONS), nav.plane(pfref.PLANE_FACTIONS))
        stages.append(exp_dirs)
        flags.append(ctx.changed_chunks(0, clear=True).astype(bool))
        assert np.array_equal(nav.plane(pfref.PLANE_BLOCKERS) > 0, occupied0)
    # the input bites, from the reference alone: fields change with the second faction and come back without it ...
    moved = (stages[0] != exp0).reshape(len(reqs), -1).any(1)
    assert moved.any() and np.array_equal(stages[1], exp0)
    # ... in chunks that were never flagged changed
    assert not flags[0][reqs["chunk_r"][moved], reqs["chunk_c"][moved]].all()
    assert not flags[0].any() and not flags[1].any()
    ctx.close()


def test_uploads_of_the_factions_plane_are_seen(navlib):
    """navhip_upload_chunk(PLANE_FACTIONS) between two builds: the second build reads the new counters in that chunk
    (and the old ones everywhere else).  A context that never got a factions plane cannot tell anybody from an enemy:
    no blocker stops its faction requests, like a reference map whose blockers carry no faction counters."""
    seed = 2
    grid, nav_a, reqs, _e, exp_a, exp_a_integ = cases.faction_cases(seed)
    _g, circ = _case_circles(navlib, seed)
    allied = circ.copy()
    allied["faction_id"][allied["faction_id"] == 1] = 2          # the same units, the enemy's now wear faction 2
    nav_b = _ref_with(grid, allied)
    assert np.array_equal(nav_b.plane(pfref.PLANE_BLOCKERS), nav_a.plane(pfref.PLANE_BLOCKERS))
    exp_b, exp_b_integ = cases.ref_fields(nav_b, reqs, None)
    differs = (exp_a != exp_b).reshape(len(reqs), -1).any(1)
    chunk_of = reqs["chunk_r"] * 3 + reqs["chunk_c"]
    pick = int(np.bincount(chunk_of[differs], minlength=9).argmax())
    assert differs[chunk_of == pick].any()
    ctx = _ctx_for(navlib, nav_a)
    h = _hip_reqs(navlib, reqs)
    _assert_fields(ctx, h, exp_a, exp_a_integ)
    ctx.upload_chunk(0, navlib.PLANE_FACTIONS, pick // 3, pick % 3, nav_b.plane(pfref.PLANE_FACTIONS)[pick // 3, pick % 3])
    exp_mix = np.where((chunk_of == pick)[:, None, None], exp_b, exp_a)
    exp_mix_integ = np.where((chunk_of == pick)[:, None, None], exp_b_integ, exp_a_integ)
    _assert_fields(ctx, h, exp_mix, exp_mix_integ)
    assert ctx.last_fields_split() == (len(h), 0)
    ctx.close()

    # no factions plane at all
    bare = pfref.RefNav(synth.to_chunks(grid))
    bare.set_blockers(nav_a.plane(pfref.PLANE_BLOCKERS))
    assert not bare.plane(pfref.PLANE_FACTIONS).any()
    assert np.array_equal(bare.plane(pfref.PLANE_LOCAL_ISLANDS), nav_a.plane(pfref.PLANE_LOCAL_ISLANDS))
    exp_dirs, exp_integ = cases.ref_fields(bare, reqs, None)
    assert not np.array_equal(exp_dirs, exp_a)
    for mode in (0, 1):
        ctx = _ctx_for(navlib, bare, factions=False)
        ctx.set_field_kernel(mode)
        _assert_fields(ctx, h, exp_dirs, exp_integ)
        assert ctx.last_fields_split() == ((len(h), 0) if mode == 0 else (0, len(h)))
        ctx.close()


def test_attacking_fields_at_benchmark_size(navlib):
    """The 1024 x 1024 map of the benchmark, 4 000 units of three factions placed by the device's own blocker update,
    the benchmark's 16 384 requests stamped with faction 0: all of them stay on the BFS kernel, both kernels give the
    same bytes, and a seeded sample of 256 equals the reference."""
    W, K = 16, 64
    grid = synth.cost_grid(W, W, seed=1234)
    dests = synth.destinations(grid, K, seed=42)
    cols = synth.planner_requests(grid, dests)
    if cols is None:
        cols = synth.whole_map_requests(grid, dests)
    h = cases.cols_to_reqs(cols, navlib.FIELD_REQ_DTYPE)
    assert len(h) == 16384
    h["faction_id"], h["enemies"] = 0, ENEMIES
    nav = pfref.RefNav(synth.to_chunks(grid))
    ctx = navlib.NavContext(W, W)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, nav.plane(pfref.PLANE_COST))
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, np.zeros((W, W, 64, 64), np.uint16))
    ctx.upload_plane(0, navlib.PLANE_FACTIONS, np.zeros((W, W, 15, 64, 64), np.uint8))
    ctx.upload_plane(0, navlib.PLANE_LOCAL_ISLANDS, nav.plane(pfref.PLANE_LOCAL_ISLANDS))
    c = synth.faction_circles(grid, 4000, seed=11)
    circles = np.zeros(4000, navlib.CIRCLE_DTYPE)
    for k in ("x", "z", "radius", "faction_id"):
        circles[k] = c[k]
    circles["delta"] = 1
    ctx.N_BlockersUpdate(circles)
    _ref_apply(nav, circles)
    _war()
    assert np.array_equal(ctx.download_plane(0, navlib.PLANE_BLOCKERS), nav.plane(pfref.PLANE_BLOCKERS))
    assert np.array_equal(ctx.download_plane(0, navlib.PLANE_LOCAL_ISLANDS), nav.plane(pfref.PLANE_LOCAL_ISLANDS))
    fast, _ = ctx.N_FlowFieldUpdate(h)
    assert ctx.last_fields_split() == (16384, 0)
    ctx.set_field_kernel(1)
    slow, _ = ctx.N_FlowFieldUpdate(h)
    assert ctx.last_fields_split() == (0, 16384)
    assert np.array_equal(fast, slow)
    sample = np.random.RandomState(5).choice(len(h), 256, replace=False)
    ref_reqs = np.zeros(len(sample), pfref.FIELD_REQ_DTYPE)
    for name in ref_reqs.dtype.names:
        if name in h.dtype.names:
            ref_reqs[name] = h[name][sample]
    exp, _ = cases.ref_fields(nav, ref_reqs, None, want_integ=False)
    bad = np.flatnonzero((exp != fast[sample]).reshape(len(sample), -1).any(1))
    assert bad.size == 0, "requests %s differ from the reference" % sample[bad][:8]
    assert (exp != 0).sum() > 256 * 1000
    ctx.close()
