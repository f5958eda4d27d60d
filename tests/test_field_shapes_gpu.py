"""GPU parity of the field builders on deep, structured chunks (tests/field_shapes.py).  The maps of the other field tests
are random rectangles: their deepest field has 163 levels, so distance planes 8..11 of k_field_bfs, the level-256 .. 2048
carries of its counter, its bake over 9..12 live planes and the distances >= 256 of its integration output never ran; nor
did the cases of the diagonal rule that need a drawn shape.  Here every case is compared bit for bit with the C restatement
AND with the numpy model of field_shapes.py, both pinned to the reference itself in tests/test_oracle_cpu.py; directions
are bytes and distances integers below 2^24 held in floats, so there is no tolerance anywhere.  Needs no oracle/_ref."""
import numpy as np
import pytest

from oracle import navoracle
from tests import cases, field_shapes as fs

pytestmark = pytest.mark.gpu


def _ctx_for(navlib, case, islands=None):
    ctx = navlib.NavContext(case.w, case.h)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, case.cost)
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, case.blockers_plane())
    ctx.upload_plane(0, navlib.PLANE_LOCAL_ISLANDS, case.li)
    if islands is not None:
        ctx.upload_plane(0, navlib.PLANE_ISLANDS, islands)
    return ctx


def _differ(got, exp):
    return np.flatnonzero((got != exp).reshape(len(got), -1).any(1))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", cases.FIELD_SHAPE_NAMES)
def test_shape_fields_equal_restatement_and_model(navlib, name, mode):
    """mode 0: k_field_bfs builds the unit-cost chunks, k_field_generic the rest; mode 1: k_field_generic builds all."""
    case = cases.field_shape_cases()[name]
    fs.check_premises(case)
    o_dirs, o_integ = cases.shape_oracle(case)
    m_dirs, m_integ, _ = case.model()
    assert np.array_equal(o_dirs, m_dirs) and np.array_equal(o_integ, m_integ), "restatement and model disagree"
    ctx = _ctx_for(navlib, case)
    ctx.set_field_kernel(mode)
    reqs = case.records(navlib.FIELD_REQ_DTYPE, inout_flag=navlib.REQ_INOUT)
    dirs, integ = ctx.N_FlowFieldUpdate(reqs, inout=case.before, want_integ=True)
    bad = _differ(dirs, m_dirs)
    assert bad.size == 0, "flow dirs differ for requests %s (first: %s)" % (bad[:8], case.reqs[bad[0]])
    bad = _differ(integ.view(np.uint32), m_integ.view(np.uint32))
    assert bad.size == 0, "integration fields differ for requests %s (first: %s)" % (bad[:8], case.reqs[bad[0]])
    # and without the integration output (the other template instance of the BFS kernel)
    dirs2, _ = ctx.N_FlowFieldUpdate(reqs, inout=case.before, want_integ=False)
    bad = _differ(dirs2, m_dirs)
    assert bad.size == 0, "flow dirs (no integration output) differ for requests %s" % bad[:8]
    if mode == 0:
        nonunit = ((case.cost != 1) & (case.cost != fs.IMP)).any(axis=(2, 3))
        n_gen = sum(bool(nonunit[q["chunk_r"], q["chunk_c"]]) for q in case.reqs)
        assert ctx.last_fields_split() == (len(reqs) - n_gen, n_gen)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# batch shapes
# ---------------------------------------------------------------------------------------------
def _open_case(name, reqs, h=2, w=2, chunks=None):
    return fs.ShapeCase(name, h, w, chunks or {}, reqs, inplace=False)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 7])
def test_batches_that_part_fill_the_last_workgroup(navlib, n):
    """k_field_bfs puts BFS_WAVES = 4 requests into a workgroup: batches of 1, 3, 4, 5 and 7 leave its last one part-filled
    (or exactly full).  All-open chunks."""
    cells = [(0, 0), (63, 63), (31, 32), (0, 63), (63, 0), (17, 40), (40, 17)]
    case = _open_case("batch%d" % n, [fs.tile(((i + 1) % 4 // 2, (i + 1) % 2), cells[i]) for i in range(n)])
    m_dirs, m_integ, _ = case.model()
    o_dirs, o_integ = cases.shape_oracle(case)
    ctx = _ctx_for(navlib, case)
    dirs, integ = ctx.N_FlowFieldUpdate(case.records(navlib.FIELD_REQ_DTYPE), want_integ=True)
    for exp_d, exp_i in ((m_dirs, m_integ), (o_dirs, o_integ)):
        assert np.array_equal(dirs, exp_d) and np.array_equal(integ, exp_i)
    assert ctx.last_fields_split() == (n, 0)
    ctx.close()


def _small_costed_chunk(seed):
    """Impassable but for a 6 x 6 block with costs 1..9: the relaxation of k_field_generic settles in a few sweeps."""
    rng = np.random.RandomState(seed)
    g = np.full((64, 64), fs.IMP, np.uint8)
    g[29:35, 30:36] = rng.randint(1, 10, (6, 6))
    return g


def test_generic_grid_stride_runs_a_second_time(navlib):
    """2 049 requests on a map with non-unit costs: every one goes to k_field_generic, whose grid is capped at 2 048
    there, so the `w += gridDim.x` stride of one workgroup reaches a second request.  36 distinct (chunk, target) pairs
    cycle through the batch; every output slot is compared."""
    chunks = {(0, 1): _small_costed_chunk(1), (1, 0): _small_costed_chunk(2), (1, 1): _small_costed_chunk(3)}
    distinct = [fs.tile(pos, (29 + k // 3, 30 + 2 * (k % 3) + (k // 3) % 2)) for pos in chunks for k in range(12)]
    case = _open_case("stride", distinct, chunks=chunks)
    assert ((case.cost != 1) & (case.cost != fs.IMP)).any()
    m_dirs = case.model()[0]
    assert np.array_equal(cases.shape_oracle(case)[0], m_dirs)
    n = 2049
    pick = np.arange(n) % len(distinct)
    reqs = case.records(navlib.FIELD_REQ_DTYPE)[pick]
    ctx = _ctx_for(navlib, case)
    dirs, _ = ctx.N_FlowFieldUpdate(reqs)
    assert ctx.last_fields_split() == (0, n)
    bad = _differ(dirs, m_dirs[pick])
    assert bad.size == 0, "requests %s differ" % bad[:8]
    assert (dirs[n - 1] != 0).sum() == 35
    ctx.close()


def _repair_world():
    """A 2 x 2 all-unit-cost map for the two repair builds: chunk (0, 1) is cut into two local islands by a wall with a
    blocked door (one global island while the door's terrain counts), chunk (1, 1) carries a block of blockers."""
    wall = fs.open_chunk()
    wall[30:33, :] = fs.IMP
    wall[30:33, 20] = 1
    door = np.zeros((64, 64), np.uint16)
    door[30:33, 20] = 1
    crowd = np.zeros((64, 64), np.uint16)
    crowd[10:20, 40:52] = 2
    case = fs.ShapeCase("repairs", 2, 2, {(0, 1): wall}, [], blockers={(0, 1): door, (1, 1): crowd}, inplace=False)
    from scipy import ndimage
    lab, _ = ndimage.label(cases.synth.from_chunks(case.cost) != fs.IMP)
    islands = cases.synth.to_chunks(np.where(lab > 0, lab - 1, 0xFFFF).astype(np.uint16))
    return case, islands


def test_repair_batch_past_the_small_generic_grid(navlib):
    """513 repair requests on an all-unit-cost map, where k_field_generic's grid is capped at 512: NEAREST_PATHABLE
    (start tiles inside the wall, under the door's and the crowd's blockers) mixed with ISLAND_NEAREST (a tile target
    moved onto either local island of its chunk), each on an existing field; expected values from the restatement."""
    case, islands = _repair_world()
    assert not ((case.cost != 1) & (case.cost != fs.IMP)).any()
    li = case.li
    base = []
    for k, (r, c) in enumerate([(31, 5), (30, 20), (32, 20), (31, 63), (30, 0), (31, 40)]):
        base.append((dict(type=navlib.TARGET_NEAREST_PATHABLE, chunk_r=0, chunk_c=1, tile_r=r, tile_c=c), 0, 0))
    for k, (r, c) in enumerate([(10, 40), (19, 51), (15, 45)]):
        base.append((dict(type=navlib.TARGET_NEAREST_PATHABLE, chunk_r=1, chunk_c=1, tile_r=r, tile_c=c), 0, 0))
    for (r, c) in [(5, 5), (60, 60), (31, 20), (29, 20), (40, 3)]:
        for iid_cell in ((0, 0), (63, 63)):
            base.append((dict(type=navlib.TARGET_TILE, chunk_r=0, chunk_c=1, tile_r=r, tile_c=c), navlib.REQ_ISLAND_NEAREST,
                         int(li[0, 1][iid_cell])))
    for (r, c) in [(15, 45), (0, 0)]:
        base.append((dict(type=navlib.TARGET_TILE, chunk_r=1, chunk_c=1, tile_r=r, tile_c=c), navlib.REQ_ISLAND_NEAREST,
                     int(li[1, 1][0, 0])))
    n = 513
    pick = np.arange(n) % len(base)
    reqs = navlib.make_reqs(n)
    for i, k in enumerate(pick):
        q, flags, iid = base[k]
        for name, v in q.items():
            reqs[name][i] = v
        reqs["flags"][i], reqs["aux_iid"][i] = flags, iid
    assert int(li[0, 1][0, 0]) != int(li[0, 1][63, 63])
    exist = np.random.RandomState(5).randint(0, 9, (n, 64, 64)).astype(np.uint8)
    onav = navoracle.OracleNav(case.cost, case.blockers_plane(), case.li)
    onav.set_layer(0, islands=islands)
    exp, _ = onav.build_fields(reqs.view(navoracle.FIELD_REQ_DTYPE), inout=exist)
    assert all((exp[i] != exist[i]).any() for i in range(len(base)))       # every kind of repair rewrote something
    ctx = _ctx_for(navlib, case, islands=islands)
    got, _ = ctx.N_FlowFieldUpdate(reqs, inout=exist)
    assert ctx.last_fields_split() == (0, n)
    bad = _differ(got, exp)
    assert bad.size == 0, "repair requests %s differ (first: %s)" % (bad[:8], base[pick[bad[0]]])
    ctx.close()


def test_three_launches_alternate_the_generic_list(navlib):
    """40, 0 and 5 requests for k_field_generic in three launches on one context (beside 8, 6 and 3 for k_field_bfs): the
    two counters of gen_list alternate between launches and each launch zeroes the other one; every launch is compared
    on its own."""
    costed = fs._costed(fs.open_chunk(), 31)
    costed[20:40, 31] = fs.IMP
    rng = np.random.RandomState(3)

    def batch(n_gen, n_bfs):
        cells = rng.randint(0, 64, (n_gen + n_bfs, 2))
        cells[:, 1] = np.where(cells[:, 1] == 31, 30, cells[:, 1])
        reqs = [fs.tile((0, 1), cells[i]) for i in range(n_gen)] + [fs.tile((1, i % 2), cells[n_gen + i]) for i in range(n_bfs)]
        return [reqs[i] for i in rng.permutation(len(reqs))]

    batches = [(40, 8), (0, 6), (5, 3)]
    case = _open_case("three", sum((batch(g, b) for g, b in batches), []), chunks={(0, 1): costed})
    m_dirs, m_integ, _ = case.model()
    o_dirs, o_integ = cases.shape_oracle(case)
    assert np.array_equal(m_dirs, o_dirs) and np.array_equal(m_integ, o_integ)
    recs = case.records(navlib.FIELD_REQ_DTYPE)
    ctx = _ctx_for(navlib, case)
    at = 0
    for g, b in batches:
        sl = slice(at, at + g + b)
        dirs, integ = ctx.N_FlowFieldUpdate(recs[sl], want_integ=True)
        assert ctx.last_fields_split() == (b, g)
        assert np.array_equal(dirs, m_dirs[sl]) and np.array_equal(integ, m_integ[sl]), (g, b)
        at += g + b
    ctx.close()


# ---------------------------------------------------------------------------------------------
# the other two field builders on the same shapes
# ---------------------------------------------------------------------------------------------
def _region_world():
    """2 x 2 chunks: spiral | serpentine over transposed serpentine | rotated spiral.  The serpentine chunk (0, 1) is
    sealed off (column 63 of its W neighbour and row 0 of its S neighbour are closed), so a region field over it is as
    deep as the chunk field."""
    serp, spir = fs.serpentine_path(), fs.spiral_path()
    S, SP = fs.from_path(serp), fs.from_path(spir)
    cost = np.stack([np.stack([SP, S]), np.stack([S.T, np.rot90(SP, 2)])]).astype(np.uint8)
    cost[0, 0][:, 63] = fs.IMP
    cost[1, 1][0, :] = fs.IMP
    return cost, serp


def region_shape_requests():
    """(cost planes, requests, seeds, overlay, existing fields): a 96 x 96 cell-arrival field and a 128 x 128 -> 64 x 64
    window field.  Both regions straddle the chunk corner (64, 64) and hang off the map (rows < 0, columns >= 128); their
    seeds: the far end of the serpentine (2 079 steps of relaxation), a cell of the spiral under an overlay tile, an
    impassable tile, a tile outside the region."""
    cost, serp = _region_world()
    tail = (serp[-1][0], 64 + serp[-1][1])
    seeds = np.array([tail, (70, 50), (1, 64 + 5), (120, 3)], np.int16)
    assert cost[1, 0][70 - 64, 50] == 1 and cost[0, 1][1, 5] == fs.IMP
    overlay = np.array([(70, 50), (1, 64 + 9), (200, 200)], np.int16)
    reqs = [dict(out_mode=0, base_abs_r=-8, base_abs_c=40, rdim=96, cdim=96, seed_begin=0, seed_count=4, overlay_begin=0, overlay_count=3),
            dict(out_mode=1, base_abs_r=-32, base_abs_c=32, rdim=128, cdim=128, roff=32, coff=32, seed_begin=0, seed_count=4,
                 overlay_begin=0, overlay_count=3)]
    inout = np.zeros((2, 8192), np.uint8)
    inout[1, :4096] = np.random.RandomState(8).randint(0, 9, 4096)
    return cost, reqs, seeds, overlay, inout


def test_region_fields_over_serpentine_and_spiral(navlib):
    cost, reqs, seeds, overlay, inout = region_shape_requests()
    onav = navoracle.OracleNav(cost, np.zeros(cost.shape, np.uint16))
    exp = onav.build_region_fields(cases.region_reqs_to(navoracle.REGION_REQ_DTYPE, reqs), seeds, overlay, inout=inout)
    # the whole serpentine got a direction in both (2 080 cells but the seed: packed two to a byte | one byte each) ...
    assert (exp[0, :96 * 96 // 2] != 0).sum() > 1000 and (exp[1, :4096] != inout[1, :4096]).sum() > 1500
    # ... and the window kept the bytes of its unreached cells
    assert (exp[1, :4096] == inout[1, :4096]).sum() > 1500
    ctx = navlib.NavContext(2, 2)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, cost)
    got = ctx.build_region_fields(cases.region_reqs_to(navlib.REGION_REQ_DTYPE, reqs), seeds, overlay, inout=inout)
    assert np.array_equal(got[0, :96 * 96 // 2], exp[0, :96 * 96 // 2])
    assert np.array_equal(got[1, :4096], exp[1, :4096])
    ctx.close()


def test_window_fields_of_regions_smaller_than_a_chunk(navlib):
    """out_mode 1 (the window written in place into a 64 x 64 field) over regions of 2 x 2 and 6 x 6 tiles: the window is
    the whole region then, its rows 64 bytes apart, and every border test of the relaxation and the bake is most of the
    region.  The reference builds such fields over 64- and 128-wide regions only (field_update_zone, field.c:1835), so
    the expected bytes are the restatement's, which tests/test_oracle_cpu.py pins to the reference."""
    cost = cases.synth.to_chunks(cases.small_region_world())
    # (side, base tile, seed tile): round the chunk corner, off the map at both ends, one row of two on the map
    regions = [(2, (63, 63), (64, 63)), (6, (61, 61), (66, 61)), (6, (-2, -2), (0, 2)), (6, (123, 123), (127, 127)),
               (2, (-1, 4), (0, 4))]
    reqs = [dict(out_mode=1, base_abs_r=b[0], base_abs_c=b[1], rdim=d, cdim=d, roff=0, coff=0, seed_begin=k, seed_count=1)
            for k, (d, b, _s) in enumerate(regions)]
    seeds = np.array([s for _d, _b, s in regions], np.int16)
    inout = np.zeros((len(reqs), 8192), np.uint8)
    inout[:, :4096] = np.random.RandomState(5).randint(0, 9, (len(reqs), 4096))
    onav = navoracle.OracleNav(cost, np.zeros(cost.shape, np.uint16))
    exp = onav.build_region_fields(cases.region_reqs_to(navoracle.REGION_REQ_DTYPE, reqs), seeds, None, inout=inout)
    for k, (d, _b, _s) in enumerate(regions):
        win = np.zeros((64, 64), bool)
        win[:d, :d] = True
        changed = exp[k, :4096].reshape(64, 64) != inout[k, :4096].reshape(64, 64)
        assert changed[win].any() and not changed[~win].any(), regions[k]
    ctx = navlib.NavContext(2, 2)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, cost)
    got = ctx.build_region_fields(cases.region_reqs_to(navlib.REGION_REQ_DTYPE, reqs), seeds, None, inout=inout)
    assert np.array_equal(got, exp)
    ctx.close()


def los_shape_requests():
    """(cost planes, LOS requests) on a 2 x 2 map with the serpentine at (0, 1) and the checkerboard at (1, 1): pairs of a
    destination chunk's field and one chained neighbour -- targets inside the shapes (walls on every side: LOS corners
    and blocked lines, next to nothing visible) and in the open chunks beside them, chained INTO the shapes."""
    serp = fs.serpentine_path()
    cost = np.ones((2, 2, 64, 64), np.uint8)
    cost[0, 1], cost[1, 1] = fs.from_path(serp), fs.checkerboard()
    mid = serp[len(serp) // 2]
    reqs = []
    assert serp[-1] == (63, 0)
    for chunk, t, nb in (((0, 1), (20, 0), (0, 0)), ((0, 1), serp[-1], (1, 1)), ((1, 1), (30, 0), (1, 0)), ((1, 1), (0, 32), (0, 1)),
                         ((0, 1), mid, (0, 0)), ((0, 0), (20, 60), (0, 1)), ((1, 0), (30, 60), (1, 1)), ((1, 0), (3, 30), (0, 0))):
        first = dict(chunk_r=chunk[0], chunk_c=chunk[1], target_chunk_r=chunk[0], target_chunk_c=chunk[1], target_tile_r=t[0],
                     target_tile_c=t[1], prev_dr=0, prev_dc=0)
        reqs += [first, dict(first, chunk_r=nb[0], chunk_c=nb[1], prev_dr=chunk[0] - nb[0], prev_dc=chunk[1] - nb[1])]
    return cost, reqs


def los_shape_expected():
    """(cost, requests, previous fields, expected fields, peak heap occupancy per request) from the restatement."""
    cost, reqs = los_shape_requests()
    onav = navoracle.OracleNav(cost, np.zeros(cost.shape, np.uint16))
    prevs, exps, peaks = [], [], []
    for k, r in enumerate(reqs):
        prev = np.zeros((64, 64), np.uint8) if k % 2 == 0 else exps[k - 1]
        onav.los_heap_peak()
        exps.append(onav.build_los(cases.los_reqs_to(navoracle.LOS_REQ_DTYPE, [r]), prev[None])[0])
        peaks.append(onav.los_heap_peak())
        prevs.append(prev)
    return cost, reqs, np.stack(prevs), np.stack(exps), peaks


def test_los_fields_on_serpentine_and_checkerboard(navlib):
    """Largest peak heap occupancy of these fields, measured on the restatement's heap: 88 nodes (an all-open destination
    chunk; 64 for a field chained into a shape, 2 inside the serpentine).  None comes near the 1 022 nodes of the first
    launch, so none takes the second (REDO) launch."""
    cost, reqs, prevs, exps, peaks = los_shape_expected()
    assert 0 < max(peaks) < 1022, peaks
    assert (exps & 1).any() and (exps & 2).sum() > 500                     # something visible, many blocked lines
    ctx = navlib.NavContext(2, 2)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, cost)
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, np.zeros(cost.shape, np.uint16))
    got = ctx.N_LOSFieldCreate(cases.los_reqs_to(navlib.LOS_REQ_DTYPE, reqs), prevs)
    bad = [i for i in range(len(reqs)) if not np.array_equal(got[i], exps[i])]
    assert not bad, "LOS fields differ: %s" % bad
    ctx.close()
