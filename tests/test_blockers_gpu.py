"""GPU parity of the dynamic-obstacle path: N_BlockersIncref / N_BlockersDecref tile sets and
refcounts on all size layers, the changed-chunk flags, the local-island relabel, and incremental
field repair; the 8-bit faction counters through 255 | 256; the island labels of hand-drawn chunks
(tests/field_shapes.py) and which chunks a batch relabels -- against the oracle restatement (itself pinned to the reference build in
tests/test_oracle_cpu.py) and, when present, the reference build directly."""
import numpy as np
import pytest

from oracle import navoracle, pfref
from tests import cases
from tests.test_oracle_cpu import _random_circles

pytestmark = pytest.mark.gpu


def _setup(navlib, grid, layers):
    h, w = grid.shape[0] // 64, grid.shape[1] // 64
    chunks = cases.synth.to_chunks(grid)
    onav = navoracle.OracleNav(chunks)
    ctx = navlib.NavContext(w, h)
    for layer in layers:
        onav.set_layer(layer, cost=chunks, blockers=np.zeros((h, w, 64, 64), np.uint16),
                       factions=np.zeros((h, w, 15, 64, 64), np.uint8))
        onav.set_layer(layer, local_islands=onav.local_islands(layer))
        ctx.upload_plane(layer, navlib.PLANE_COST_BASE, chunks)
        ctx.upload_plane(layer, navlib.PLANE_BLOCKERS, onav.plane(layer, "blockers"))
        ctx.upload_plane(layer, navlib.PLANE_FACTIONS, onav.plane(layer, "factions"))
        ctx.upload_plane(layer, navlib.PLANE_LOCAL_ISLANDS, onav.plane(layer, "local_islands"))
    return ctx, onav


def test_blockers_circles_all_layers_match(navlib):
    grid = cases.synth.cost_grid(2, 2, seed=13)
    layers = list(range(12))
    ctx, onav = _setup(navlib, grid, layers)
    circles = _random_circles(grid, 120, seed=2, air_frac=0.2, max_radius=22.0)
    circles["radius"][5], circles["radius"][6], circles["radius"][7] = 100.0, 75.0, 112.0
    undo = circles[::3].copy()
    undo["delta"] = -1
    ref = None
    if pfref.available():
        ref = pfref.RefNav(cases.synth.to_chunks(grid), layer_mask=0xff)
    for batch in (circles, undo):
        before = {l: onav.plane(l, "blockers").copy() for l in layers}
        dirty = onav.blockers_circles(batch)
        ctx.N_BlockersUpdate(batch.view(navlib.CIRCLE_DTYPE))
        for l in layers:
            assert np.array_equal(ctx.download_plane(l, navlib.PLANE_BLOCKERS), onav.plane(l, "blockers")), l
            assert np.array_equal(ctx.download_plane(l, navlib.PLANE_FACTIONS), onav.plane(l, "factions")), l
            # changed == final occupancy differs; a subset of the reference's toggle-based dirty set
            changed = ctx.changed_chunks(l, clear=True).astype(bool)
            occ_b = (before[l] > 0).reshape(2, 2, -1)
            occ_a = (onav.plane(l, "blockers") > 0).reshape(2, 2, -1)
            assert np.array_equal(changed, (occ_b != occ_a).any(-1)), l
            assert not (changed & ~dirty[l].astype(bool)).any(), l
            # local islands relabelled on the device for the changed chunks
            assert np.array_equal(ctx.download_plane(l, navlib.PLANE_LOCAL_ISLANDS), onav.local_islands(l)), l
        if ref is not None:
            for c in batch:
                if not (int(c["flags"]) & (1 << 15)):
                    ref.blockers_circle(float(c["x"]), float(c["z"]), float(c["radius"]),
                                        int(c["faction_id"]), int(c["flags"]), incref=(c["delta"] > 0))
            for l in range(8):
                # air circles never touch ground / water layers, so the reference agrees there
                assert np.array_equal(ctx.download_plane(l, navlib.PLANE_BLOCKERS),
                                      ref.plane(pfref.PLANE_BLOCKERS, l)), l
    assert onav.plane(11, "blockers").sum() > 0 and onav.plane(3, "blockers").sum() > onav.plane(0, "blockers").sum()
    # invalid circles are rejected, not silently clamped
    bad = circles[:1].copy()
    bad["radius"] = 113.0
    with pytest.raises(navlib.NavHipError):
        ctx.N_BlockersUpdate(bad.view(navlib.CIRCLE_DTYPE))
    ctx.close()


@pytest.mark.parametrize("seed,frac", [(5, 0.2), (9, 0.45)])
def test_device_local_island_relabel_matches_reference_labels(navlib, seed, frac):
    grid = cases.synth.cost_grid(3, 3, seed=seed, frac_impassable=frac)
    blk = cases.random_blockers(grid, seed=seed + 1, frac=0.05)
    chunks = cases.synth.to_chunks(grid)
    ctx = navlib.NavContext(3, 3)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, chunks)
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, blk)
    ctx.relabel_local_islands(0)
    got = ctx.download_plane(0, navlib.PLANE_LOCAL_ISLANDS)
    onav = navoracle.OracleNav(chunks, blk)
    assert np.array_equal(got, onav.local_islands(0))
    if pfref.available():
        nav = pfref.RefNav(chunks)
        nav.set_blockers(blk)
        assert np.array_equal(got, nav.plane(pfref.PLANE_LOCAL_ISLANDS))
    assert got[got != 0xFFFF].max() >= 2          # several components somewhere
    ctx.close()


def test_incremental_field_repair_equals_full_rebuild(navlib):
    synth = cases.synth
    W, K = 4, 6
    grid = synth.cost_grid(W, W, seed=1234)
    ctx, onav = _setup(navlib, grid, [0])
    liid = synth.from_chunks(onav.plane(0, "local_islands"))
    dests = synth.destinations(grid, K, seed=42)
    cols = synth.whole_map_requests(grid, dests, liid)
    reqs = cases.cols_to_reqs(cols, navlib.FIELD_REQ_DTYPE)
    reqs["flags"] = navlib.REQ_LIVE_IIDS
    pool, _ = ctx.N_FlowFieldUpdate(reqs)
    exp0, _ = onav.build_fields(reqs.view(navoracle.FIELD_REQ_DTYPE))
    assert np.array_equal(pool, exp0)
    ctx.changed_chunks(0, clear=True)
    # drop obstacles on passable ground (not on a destination), then repair only what changed
    rng = np.random.RandomState(3)
    cells = synth.passable_cells(grid)
    pick = cells[rng.choice(len(cells), 40, replace=False)]
    xz = synth.cell_centre(W, W, pick[:, 0], pick[:, 1])
    circles = np.zeros(len(pick), navlib.CIRCLE_DTYPE)
    circles["x"], circles["z"] = xz[:, 0], xz[:, 1]
    circles["radius"] = rng.uniform(2, 6, len(pick))
    circles["delta"] = 1
    onav.blockers_circles(circles.view(navoracle.CIRCLE_DTYPE))
    onav.set_layer(0, local_islands=onav.local_islands(0))
    ctx.N_BlockersUpdate(circles)
    changed = ctx.changed_chunks(0).astype(bool)
    assert 0 < changed.sum() < W * W
    r2 = reqs.copy()
    r2["flags"] = navlib.REQ_LIVE_IIDS | navlib.REQ_IF_CHANGED
    repaired, _ = ctx.N_FlowFieldUpdate(r2, inout=pool)           # slots start from the old pool
    need = changed[reqs["chunk_r"], reqs["chunk_c"]] | \
        ((reqs["type"] == 0) & changed[reqs["next_chunk_r"], reqs["next_chunk_c"]])
    exp_new, _ = onav.build_fields(r2.view(navoracle.FIELD_REQ_DTYPE))   # full rebuild, new planes
    assert np.array_equal(repaired[need], exp_new[need])
    assert np.array_equal(repaired[~need], pool[~need])           # untouched slots
    assert need.sum() < len(reqs)
    ctx.close()


def test_live_island_ids_come_from_a_labelled_portal_tile(navlib):
    """NAVHIP_REQ_LIVE_IIDS with a blocker on the FIRST tile of a portal: the ids must come from a tile
    that still has a label (the planner only ever hands out ids of reachable tiles), i.e. the fields
    equal those of requests that carry the right ids explicitly; a portal blocked end to end is
    skipped (slot untouched)."""
    synth = cases.synth
    W, K = 4, 6
    grid = synth.cost_grid(W, W, seed=1234)
    ctx, onav = _setup(navlib, grid, [0])
    liid = synth.from_chunks(onav.plane(0, "local_islands"))
    cols = synth.whole_map_requests(grid, synth.destinations(grid, K, seed=42), liid)
    reqs = cases.cols_to_reqs(cols, navlib.FIELD_REQ_DTYPE)
    portal = np.flatnonzero(reqs["type"] == navlib.TARGET_PORTAL)
    rng = np.random.RandomState(4)
    hit = rng.choice(portal, 24, replace=False)
    # a small obstacle on the first tile of the port / next portal of the chosen requests
    rows = np.where(np.arange(len(hit)) % 2 == 0, reqs["chunk_r"][hit] * 64 + reqs["port_r0"][hit],
                    reqs["next_chunk_r"][hit] * 64 + reqs["next_r0"][hit])
    colsx = np.where(np.arange(len(hit)) % 2 == 0, reqs["chunk_c"][hit] * 64 + reqs["port_c0"][hit],
                     reqs["next_chunk_c"][hit] * 64 + reqs["next_c0"][hit])
    xz = synth.cell_centre(W, W, rows, colsx)
    circles = np.zeros(len(hit), navlib.CIRCLE_DTYPE)
    circles["x"], circles["z"], circles["radius"], circles["delta"] = xz[:, 0], xz[:, 1], 3.0, 1
    onav.blockers_circles(circles.view(navoracle.CIRCLE_DTYPE))
    onav.set_layer(0, local_islands=onav.local_islands(0))
    ctx.N_BlockersUpdate(circles)
    li = synth.from_chunks(onav.plane(0, "local_islands"))
    first_port = li[reqs["chunk_r"] * 64 + reqs["port_r0"], reqs["chunk_c"] * 64 + reqs["port_c0"]]
    first_next = li[reqs["next_chunk_r"] * 64 + reqs["next_r0"], reqs["next_chunk_c"] * 64 + reqs["next_c0"]]
    affected = np.zeros(len(reqs), bool)
    affected[portal] = (first_port[portal] == 0xFFFF) | (first_next[portal] == 0xFFFF)
    assert affected.sum() >= 12                                # the case is there

    def first_label(cr, cc, r0, c0, r1, c1):
        blk = li[cr * 64 + r0:cr * 64 + r1 + 1, cc * 64 + c0:cc * 64 + c1 + 1].ravel()
        ok = blk[blk != 0xFFFF]
        return int(ok[0]) if len(ok) else 0xFFFF

    explicit = reqs.copy()
    dead = np.zeros(len(reqs), bool)
    for i in portal:
        q = reqs[i]
        explicit["port_iid"][i] = first_label(q["chunk_r"], q["chunk_c"], q["port_r0"], q["port_c0"], q["port_r1"], q["port_c1"])
        explicit["next_iid"][i] = first_label(q["next_chunk_r"], q["next_chunk_c"], q["next_r0"], q["next_c0"], q["next_r1"], q["next_c1"])
        dead[i] = explicit["port_iid"][i] == 0xFFFF or explicit["next_iid"][i] == 0xFFFF
    live = reqs.copy()
    live["flags"] = navlib.REQ_LIVE_IIDS
    marker = np.full((len(reqs), 64, 64), 7, np.uint8)        # (what a skipped slot keeps)
    live_in = live.copy()
    live_in["flags"] |= navlib.REQ_INOUT
    got, _ = ctx.N_FlowFieldUpdate(live)
    exp, _ = ctx.N_FlowFieldUpdate(explicit)
    assert np.array_equal(got[~dead], exp[~dead])
    ora, _ = onav.build_fields(live.view(navoracle.FIELD_REQ_DTYPE))
    assert np.array_equal(got[~dead], ora[~dead])
    ctx.close()


@pytest.mark.skipif(not pfref.available(), reason="needs the reference build (oracle/_ref)")
@pytest.mark.parametrize("w,h", [(3, 2), (2, 3)])
def test_blockers_on_non_square_maps_match_reference(navlib, w, h):
    """N_BlockersIncref / Decref on 3x2 and 2x3 chunks: refcount planes of the ground and water
    layers against the reference itself, local islands against the restatement."""
    grid = cases.synth.cost_grid(w, h, seed=40 + w)
    layers = list(range(8))
    ctx, onav = _setup(navlib, grid, layers)
    ref = pfref.RefNav(cases.synth.to_chunks(grid), layer_mask=0xff)
    circles = _random_circles(grid, 150, seed=6, air_frac=0.0, max_radius=30.0)
    undo = circles[::4].copy()
    undo["delta"] = -1
    for batch in (circles, undo):
        onav.blockers_circles(batch)
        ctx.N_BlockersUpdate(batch.view(navlib.CIRCLE_DTYPE))
        for c in batch:
            ref.blockers_circle(float(c["x"]), float(c["z"]), float(c["radius"]), int(c["faction_id"]),
                                int(c["flags"]), incref=(c["delta"] > 0))
        for l in layers:
            got = ctx.download_plane(l, navlib.PLANE_BLOCKERS)
            assert np.array_equal(got, ref.plane(pfref.PLANE_BLOCKERS, l)), l
            assert np.array_equal(ctx.download_plane(l, navlib.PLANE_LOCAL_ISLANDS), onav.local_islands(l)), l
    assert ctx.download_plane(0, navlib.PLANE_BLOCKERS).sum() > 0
    ctx.close()


# ---------------------------------------------------------------------------------------------
# faction counters across 255 | 256: a byte per tile and faction in the reference (nav_data.h:141), which wraps
# ---------------------------------------------------------------------------------------------
CROWD_STEPS = ((255, 1), (1, 1), (44, 1), (45, -1), (255, -1))       # (circles per site, delta) of each batch
CROWD_COUNTS = (255, 256, 300, 255, 0)                               # units on every site after each batch


def _open_map(navlib, w, h, layers):
    return _setup(navlib, np.ones((h * 64, w * 64), np.uint8), layers)


def _faction_flags(before, after):
    """[h][w] u16, bit f: the tiles faction f holds in the chunk -- counter != 0 -- differ between two factions planes."""
    h, w = before.shape[:2]
    differs = ((before != 0) != (after != 0)).reshape(h, w, 15, -1).any(-1)
    return (differs << np.arange(15)).sum(-1).astype(np.uint16)


def _reference_applies(ref, batch):
    for c in batch:
        if not (int(c["flags"]) & (1 << 15)):
            ref.blockers_circle(float(c["x"]), float(c["z"]), float(c["radius"]), int(c["faction_id"]), int(c["flags"]),
                                incref=(c["delta"] > 0))


def _planes_equal_oracle_and_reference(navlib, ctx, onav, ref, layers, what):
    for l in layers:
        got_b, got_f = ctx.download_plane(l, navlib.PLANE_BLOCKERS), ctx.download_plane(l, navlib.PLANE_FACTIONS)
        assert np.array_equal(got_b, onav.plane(l, "blockers")), (what, l)
        exp_f = onav.plane(l, "factions")
        if not np.array_equal(got_f, exp_f):
            bad = np.argwhere(got_f != exp_f)                        # (chunk_r, chunk_c, faction, row, col)
            pytest.fail("%s, layer %d: PLANE_FACTIONS differs in %d bytes, byte lanes (column & 3) %s, first %s: got %d, expected %d"
                        % (what, l, len(bad), sorted(set((bad[:, 4] & 3).tolist())), bad[0].tolist(),
                           got_f[tuple(bad[0])], exp_f[tuple(bad[0])]))
        if ref is not None and l < 8:                                # (air circles never reach the reference's 8 layers)
            assert np.array_equal(got_b, ref.plane(pfref.PLANE_BLOCKERS, l)), (what, l)
            assert np.array_equal(got_f, ref.plane(pfref.PLANE_FACTIONS, l)), (what, l)


def test_faction_counters_wrap_in_their_own_byte_like_the_reference(navlib):
    """Crowds of 255, 256, 300, 255 and 0 units of one faction on one tile, on seven sites at once (cases.CROWD_SITES):
    n_update_blockers (nav.c:1032) adds to a uint8_t, so at 256 units the faction's byte reads 0 -- the tile stays
    blocked, the faction's mask bit drops -- and at 300 it reads 44.  The tile's neighbours in the same 32-bit word see
    nothing of it.  After every batch, on all 12 layers: refcounts and faction counters, both kinds of changed flags and
    the island labels against the restatement; the planes of layers 0-7 against the reference build too."""
    w, h, layers = 2, 1, list(range(12))
    ctx, onav = _open_map(navlib, w, h, layers)
    ref = pfref.RefNav(onav.plane(0, "cost"), layer_mask=0xff) if pfref.available() else None
    sites = cases.CROWD_SITES
    ground = [s for s in sites if not s[3]]
    assert sorted({s[1] & 3 for s in ground}) == [0, 1, 2, 3] and any(s[1] == 63 for s in sites) and any(s[3] for s in sites)
    assert any(s[2] == 14 for s in sites) and sum(s[2] >= 4 for s in sites) >= 3
    raised = []
    for step, ((count, delta), units) in enumerate(zip(CROWD_STEPS, CROWD_COUNTS)):
        batch = cases.crowd_circles(w, h, sites, count, delta)
        before_b = {l: onav.plane(l, "blockers").copy() for l in layers}
        before_f = {l: onav.plane(l, "factions").copy() for l in layers}
        onav.blockers_circles(batch)
        ctx.N_BlockersUpdate(batch.view(navlib.CIRCLE_DTYPE))
        if ref is not None:
            _reference_applies(ref, batch)
        # the premise, from the restatement: the site's tile holds `units`, its faction byte units mod 256; no footprints
        # overlap.  (On the 5x5 and 7x7 layers a contour is taken of the previous contour alone, so it comes back over
        # the tiles inside: those count every unit twice and pass 256 in the middle of a batch.)
        for r, c, f, flags in sites:
            for l in ((8, 9) if flags else (0, 1, 4, 5)):
                assert onav.plane(l, "blockers")[0, 0, r, c] == units and onav.plane(l, "factions")[0, 0, f, r, c] == units & 0xFF
        assert all(int(onav.plane(l, "blockers").max()) == (units if l % 4 < 2 else 2 * units) for l in layers)
        assert (onav.plane(0, "blockers") > 0).sum() == (len(ground) if units else 0)
        _planes_equal_oracle_and_reference(navlib, ctx, onav, ref, layers, "step %d (%d units)" % (step, units))
        any_fac = False
        for l in layers:
            changed = ctx.changed_chunks(l, clear=True).astype(bool)
            occ_b, occ_a = (before_b[l] > 0).reshape(h, w, -1), (onav.plane(l, "blockers") > 0).reshape(h, w, -1)
            assert np.array_equal(changed, (occ_b != occ_a).any(-1)), (step, l)
            want_fac = _faction_flags(before_f[l], onav.plane(l, "factions"))
            got_fac = ctx.faction_changed_chunks(l, clear=True)
            assert np.array_equal(got_fac, want_fac), (step, l, got_fac, want_fac)
            any_fac |= bool(got_fac.any())
            assert np.array_equal(ctx.download_plane(l, navlib.PLANE_LOCAL_ISLANDS), onav.local_islands(l)), (step, l)
        raised.append(any_fac)
    # 255 -> 256 drops the mask bit, 256 -> 300 raises it again, 300 -> 255 changes no mask
    assert raised == [True, True, True, False, True], raised
    ctx.close()


def test_increfs_and_decrefs_of_one_batch_leave_the_reference_counters(navlib):
    """300 increfs and then 60 decrefs of every site in ONE batch: the reference applies them in order, the device in
    any order -- a counter may pass 256 and come back, or go below zero first -- and the planes at the end are the same:
    240 units on every site."""
    w, h, layers = 2, 1, list(range(12))
    ctx, onav = _open_map(navlib, w, h, layers)
    ref = pfref.RefNav(onav.plane(0, "cost"), layer_mask=0xff) if pfref.available() else None
    sites = cases.CROWD_SITES
    batch = np.concatenate([cases.crowd_circles(w, h, sites, 300, 1), cases.crowd_circles(w, h, sites, 60, -1)])
    onav.blockers_circles(batch)
    ctx.N_BlockersUpdate(batch.view(navlib.CIRCLE_DTYPE))
    if ref is not None:
        _reference_applies(ref, batch)
    for r, c, f, flags in sites:
        l = 9 if flags else 5
        assert onav.plane(l, "blockers")[0, 0, r, c] == 240 and onav.plane(l, "factions")[0, 0, f, r, c] == 240
    # (the 5x5 and 7x7 layers count the inner tiles twice: 480 units, the byte reads 224)
    assert all(int(onav.plane(l, "blockers").max()) == (240 if l % 4 < 2 else 480) for l in layers)
    _planes_equal_oracle_and_reference(navlib, ctx, onav, ref, layers, "300 up, 60 down")
    ctx.close()


# ---------------------------------------------------------------------------------------------
# k_local_islands on structured chunks
# ---------------------------------------------------------------------------------------------
def _expected_islands(chunks, blk=None):
    """The labels of layer 0 from the restatement, from scipy (synth.local_islands: the same components in the same
    row-major order of their first cells, numbered from 0 where the reference numbers from 1) and, when present, from the
    reference itself -- all three the same."""
    synth = cases.synth
    h, w = chunks.shape[:2]
    want = navoracle.OracleNav(chunks, np.zeros((h, w, 64, 64), np.uint16) if blk is None else blk).local_islands(0)
    sc = synth.to_chunks(synth.local_islands(synth.from_chunks(chunks), None if blk is None else synth.from_chunks(blk)))
    assert np.array_equal(np.where(sc == 0xFFFF, 0xFFFF, sc.astype(np.int64) + 1), want)
    if pfref.available():
        nav = pfref.RefNav(chunks)
        if blk is not None:
            nav.set_blockers(blk)
        assert np.array_equal(nav.plane(pfref.PLANE_LOCAL_ISLANDS), want)
    return want


def _device_islands(navlib, chunks, blk=None):
    h, w = chunks.shape[:2]
    ctx = navlib.NavContext(w, h)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, chunks)
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, np.zeros((h, w, 64, 64), np.uint16) if blk is None else blk)
    ctx.relabel_local_islands(0)
    got = ctx.download_plane(0, navlib.PLANE_LOCAL_ISLANDS)
    ctx.close()
    return got


def _check_components(labels, n):
    """One chunk's labels: exactly the ids 1..n (none: every cell ISLAND_NONE)."""
    ids = np.unique(labels[labels != 0xFFFF])
    assert ids.tolist() == list(range(1, n + 1)), (len(ids), n)


ISLAND_SHAPE_NAMES = ("checkerboard", "checkerboard_less_one", "serpentine", "spiral", "rim", "column_seam", "row_seams",
                      "staircase", "anti_diagonal", "open", "closed", "last_cell")


@pytest.mark.parametrize("name", ISLAND_SHAPE_NAMES)
def test_device_labels_structured_chunks(navlib, name):
    """k_local_islands on a shape of tests/field_shapes.py in one chunk of a 2x2 map, the next three shapes of the list in
    the other chunks (the four waves of the workgroup do different work): 2 048 one-cell components (every label plane,
    the largest id 2048), corridors of thousands of cells, halves joined in one cell, corner contacts that do NOT join,
    no component at all."""
    from tests import field_shapes
    shapes = field_shapes.island_shapes()
    assert tuple(s[0] for s in shapes) == ISLAND_SHAPE_NAMES
    i = ISLAND_SHAPE_NAMES.index(name)
    at = [(i % 4 + k) % 4 for k in range(4)]                          # shape i + k sits in chunk at[k]
    chunks = np.zeros((2, 2, 64, 64), np.uint8)
    for k in range(4):
        chunks[at[k] // 2, at[k] % 2] = shapes[(i + k) % len(shapes)][1]
    want = _expected_islands(chunks)
    got = _device_islands(navlib, chunks)
    assert np.array_equal(got, want)
    for k in range(4):
        _check_components(got[at[k] // 2, at[k] % 2], shapes[(i + k) % len(shapes)][2])
    mine = got[at[0] // 2, at[0] % 2]
    if name == "checkerboard":
        assert int(mine[mine != 0xFFFF].max()) == 2048
    if name == "closed":
        assert (mine == 0xFFFF).all()
    if name == "last_cell":
        assert mine[63, 63] == 1 and (mine != 0xFFFF).sum() == 1


def test_device_labels_a_map_whose_last_wave_has_no_chunk(navlib):
    """3 x 1 chunks: one workgroup of four waves, the fourth without a chunk; the checkerboard in the last chunk."""
    from tests import field_shapes
    shapes = dict((s[0], s[1:]) for s in field_shapes.island_shapes())
    order = ("serpentine", "spiral", "checkerboard")
    chunks = np.stack([shapes[n][0] for n in order])[None]
    assert chunks.shape == (1, 3, 64, 64)
    want = _expected_islands(chunks)
    got = _device_islands(navlib, chunks)
    assert np.array_equal(got, want)
    for k, n in enumerate(order):
        _check_components(got[0, k], shapes[n][1])
    assert int(got[0, 2][got[0, 2] != 0xFFFF].max()) == 2048


def test_device_labels_shapes_carried_by_the_blockers_plane(navlib):
    """An open cost plane, the checkerboard and the serpentine drawn by blockers (refcounts 1-3 where the shape is
    closed): the labels come through the passability masks derived from PLANE_BLOCKERS."""
    from tests import field_shapes
    shapes = dict((s[0], s[1:]) for s in field_shapes.island_shapes())
    order = ("checkerboard", "serpentine", "open", "serpentine")
    chunks = np.ones((2, 2, 64, 64), np.uint8)
    blk = np.zeros((2, 2, 64, 64), np.uint16)
    rng = np.random.RandomState(7)
    for k, n in enumerate(order):
        plane = shapes[n][0] if k < 3 else shapes[n][0].T
        blk[k // 2, k % 2] = np.where(plane == 255, rng.randint(1, 4, (64, 64)), 0)
    want = _expected_islands(chunks, blk)
    got = _device_islands(navlib, chunks, blk)
    assert np.array_equal(got, want)
    for k, n in enumerate(order):
        _check_components(got[k // 2, k % 2], shapes[n][1])
    assert int(got[0, 0][got[0, 0] != 0xFFFF].max()) == 2048


# ---------------------------------------------------------------------------------------------
# the relabel after a blocker batch touches the chunks that changed, of that layer, and no other
# ---------------------------------------------------------------------------------------------
def test_relabel_after_a_batch_leaves_unchanged_chunks_alone(navlib):
    """Layers 0 and 3 of a 2x2 map hold correct labels but for sentinels no labelling produces: 0x7777 on the passable
    cells of chunk (1, 1) of both layers, 0x5555 on those of chunk (0, 1) of layer 0.  A circle of one tile inside chunk
    (0, 0) relabels that chunk on both layers; one in column 62 reaches chunk (0, 1) with its contours on layer 3 only.
    A relabel of a chunk that did not change -- or of a chunk another layer's flags name -- overwrites a sentinel."""
    synth = cases.synth
    grid = synth.cost_grid(2, 2, seed=13)
    grid[12:52, 40:90] = 1                                            # open ground under both circles, across the border
    layers = (0, 3)
    ctx, onav = _setup(navlib, grid, list(layers))
    ok = synth.to_chunks(grid) != 255
    held = {}
    for l in layers:
        li = onav.plane(l, "local_islands").copy()
        li[1, 1][ok[1, 1]] = 0x7777
        if l == 0:
            li[0, 1][ok[0, 1]] = 0x5555
        ctx.upload_plane(l, navlib.PLANE_LOCAL_ISLANDS, li)
        held[l] = li
        assert not ctx.changed_chunks(l).any()
    expect_changed = [{0: [(0, 0)], 3: [(0, 0)]}, {0: [(0, 0)], 3: [(0, 0), (0, 1)]}]
    for step, (r, c) in enumerate(((30, 45), (30, 62))):
        circle = cases.crowd_circles(2, 2, [(r, c, 0, 0)], 1, 1)
        before = {l: onav.plane(l, "blockers").copy() for l in layers}
        onav.blockers_circles(circle)
        ctx.N_BlockersUpdate(circle.view(navlib.CIRCLE_DTYPE))
        for l in layers:
            occ = ((before[l] > 0) != (onav.plane(l, "blockers") > 0)) & ok
            want_changed = occ.reshape(2, 2, -1).any(-1)
            assert [tuple(x) for x in np.argwhere(want_changed).tolist()] == expect_changed[step][l], (step, l)   # the premise
            assert np.array_equal(ctx.changed_chunks(l, clear=True).astype(bool), want_changed), (step, l)
            want, got = onav.local_islands(l), ctx.download_plane(l, navlib.PLANE_LOCAL_ISLANDS)
            assert not np.array_equal(want[0, 0], held[l][0, 0])      # (the circle splits off or closes cells: labels move)
            for cr in range(2):
                for cc in range(2):
                    if want_changed[cr, cc]:
                        assert np.array_equal(got[cr, cc], want[cr, cc]), (step, l, cr, cc)
                        held[l][cr, cc] = want[cr, cc]
                    else:
                        assert np.array_equal(got[cr, cc], held[l][cr, cc]), (step, l, cr, cc)
            assert (got[1, 1][ok[1, 1]] == 0x7777).all(), (step, l)
        assert (ctx.download_plane(0, navlib.PLANE_LOCAL_ISLANDS)[0, 1][ok[0, 1]] == 0x5555).all(), step
    ctx.close()
