"""The device spatial index -- k_sp_count .. k_sp_place, k_sp_build_small, sp_query_wave -- on its own, through
navhip_spatial_query and host buffers, over the worlds of cases.spatial_cases(): grid shapes (1 x 1 .. 32 x 32 chunks,
8 192 cells exactly, bounds that are no multiple of a cell), both build paths on either side of their thresholds, and
radii that take every segment-pass shape of the query (1, 2, 4, 8 block columns per pass, more than 8 block columns,
the wide scan and the radii around its threshold, the 32-bit and the 64-bit distance arm).

Three things are compared with the device, lists in ORDER and with their caps:
  * the restatement (oracle/navoracle.c), always;
  * the reference's own bg_ent_inrange_circle (oracle/_ref), where it is built;
  * a model written here in numpy from bitmap_grid.h alone: the SET of hits by brute force (x256 fixed point, int64,
    inclusive), and -- for the queries whose cap binds and a sample of the others -- the visiting order rebuilt from a
    sort by (cell, descending uid).
The model functions are plain numpy and need no device: tests/test_oracle_cpu.py runs the same checks on the restatement."""
import functools

import numpy as np
import pytest

from oracle import navoracle, pfref
from tests import cases

pytestmark = pytest.mark.gpu

CASES = list(cases.spatial_cases())
# (one context, alternating build paths and grid sizes; the two 8 192-cell grids and the two ragged builds side by side)
LEAK_ORDER = ["many_blocks", "small_full", "large_by_cells", "one", "blobs", "small_cells_max_8x4", "small_cells_max_4x8",
              "ragged", "ragged_small", "many_blocks"]


# ---------------------------------------------------------------------------------------------
# the model: bitmap_grid.h in numpy
# ---------------------------------------------------------------------------------------------
class Model:
    """One world: fixed-point coordinates, the clean pool (cells row-major, descending uid inside a cell:
    bg_ent_insert pushes at the head of the cell's chain, bg_ent_cleanup copies head first) and the squared distances
    of every (query, entity) pair."""

    def __init__(self, bounds, pos, query):
        self.bounds, self.query = bounds, query
        self.ox, self.oy, self.gw, self.gh = cases.sp_geometry(bounds)
        ix, iy = cases.sp_scale(pos[:, 0]), cases.sp_scale(pos[:, 1])
        qx, qy = cases.sp_scale(query[:, 0]), cases.sp_scale(query[:, 1])
        self.d2 = (ix[None, :] - qx[:, None]) ** 2 + (iy[None, :] - qy[:, None]) ** 2
        self.cx = np.clip((ix - self.ox) >> 12, 0, self.gw - 1)            # _bg_cell_x_from_int: clamped into the grid
        self.cy = np.clip((iy - self.oy) >> 12, 0, self.gh - 1)
        cell = self.cy * self.gw + self.cx
        self.pool = np.lexsort((-np.arange(len(pos)), cell))
        self.cell_start = np.searchsorted(cell[self.pool], np.arange(self.gw * self.gh + 1))

    def hits(self, r):
        """(extent, [nq, n] bool): inside the circle, inclusive -- and nothing for a box that misses the grid."""
        e = cases.sp_extent(self.bounds, self.query, r)
        return e, (self.d2 <= e["ir"] * e["ir"]) & ~e["miss"][:, None]

    def candidates(self, e, k):
        """uids in the order query k visits them (bitmap_grid.h:1408-1466: coarse blocks row-major, fine rows inside a
        block, cells left to right; the whole pool for a wide query)."""
        if e["wide"][k]:
            return self.pool
        cx_lo, cx_hi, cy_lo, cy_hi = (int(e[n][k]) for n in ("cx_lo", "cx_hi", "cy_lo", "cy_hi"))
        segs = [np.zeros(0, np.int64)]
        for cyc in range(cy_lo >> 3, (cy_hi >> 3) + 1):
            for cxc in range(cx_lo >> 3, (cx_hi >> 3) + 1):
                fx0, fx1 = max(cxc * 8, cx_lo), min(cxc * 8 + 8, cx_hi + 1)
                for fy in range(max(cyc * 8, cy_lo), min(cyc * 8 + 8, cy_hi + 1)):
                    segs.append(self.pool[self.cell_start[fy * self.gw + fx0]:self.cell_start[fy * self.gw + fx1]])
        return np.concatenate(segs)


@functools.lru_cache(maxsize=None)
def model_of(name):
    bounds, pos, query, _pairs = cases.spatial_cases()[name]
    return Model(bounds, pos, query)


def check_against_model(name, r, cap, counts, ids, ordered=6):
    """The reference-free check of one result: the SET of every uncapped list is the brute-force set, a capped list
    holds `cap` distinct hits; and the ORDER of up to `ordered` capped and `ordered` uncapped non-empty lists is the
    model's visiting order."""
    m = model_of(name)
    e, hit = m.hits(r)
    nhit = hit.sum(1)
    assert np.array_equal(counts, np.minimum(nhit, cap)), (name, r, cap, np.flatnonzero(counts != np.minimum(nhit, cap))[:8])
    got = np.zeros_like(hit)
    rows = np.repeat(np.arange(len(counts)), counts)
    cols = ids[np.arange(ids.shape[1])[None, :] < counts[:, None]]
    assert (cols < hit.shape[1]).all(), (name, r, cap)
    got[rows, cols] = True
    assert got.sum(1).tolist() == counts.tolist(), (name, r, cap, "an id twice in one list")
    full = nhit <= cap
    assert np.array_equal(got[full], hit[full]), (name, r, cap, np.flatnonzero(full)[(got[full] != hit[full]).any(1)][:8])
    assert not (got & ~hit).any(), (name, r, cap)
    capped = np.flatnonzero(nhit > cap)[:ordered]
    sample = np.flatnonzero((nhit > 1) & (nhit <= cap))
    for k in list(capped) + list(sample[::max(1, len(sample) // ordered)][:ordered]):
        c = m.candidates(e, k)
        exp = c[hit[k, c]][:cap]
        assert np.array_equal(ids[k, :counts[k]], exp), (name, r, cap, int(k))


def coverage():
    """How many queries of the case matrix take each path, from the reference's rule alone (cases.sp_extent, Model)."""
    cov = dict.fromkeys(["cols_1", "cols_2", "cols_3_4", "cols_5_8", "cols_gt8_not_wide", "wide", "miss",
                         "ir_le_16000_not_wide", "ir_gt_16000_not_wide", "cap_binds_in_first_64", "cap_binds_after_64",
                         "hit_exactly_at_r", "partial_last_block_3_or_more_cols", "rows_gt8_not_wide",
                         "wide_one_step_above", "not_wide_one_step_below", "hits_in_gt8_block_columns",
                         "small_build", "large_build", "cell_of_300", "scan_blocks_gt256", "far_clamped_entity_in_reach", "wide_by_equality"], 0)
    for name, (bounds, pos, query, pairs) in cases.spatial_cases().items():
        m = model_of(name)
        ncells = m.gw * m.gh
        cov["small_build" if len(pos) <= 1024 and ncells <= 8192 else "large_build"] += 1
        cov["cell_of_300"] += int(np.diff(m.cell_start).max() >= 300)
        cov["scan_blocks_gt256"] += int((ncells + 255) // 256 > 256)
        seen = set()
        for r, cap in pairs:
            e, hit = m.hits(r)
            nhit = hit.sum(1)
            capped = np.flatnonzero(nhit >= cap)
            for k in capped[:4]:
                c = m.candidates(e, k)
                at = np.flatnonzero(hit[k, c])[cap - 1]                     # the candidate that fills the cap
                cov["cap_binds_in_first_64" if at < 64 else "cap_binds_after_64"] += 1
            if r in seen:
                continue
            seen.add(r)
            seg = ~e["miss"] & ~e["wide"]                                    # the segment passes
            cov["miss"] += int(e["miss"].sum())
            cov["wide"] += int(e["wide"].sum())
            for key, lo, hi in (("cols_1", 1, 1), ("cols_2", 2, 2), ("cols_3_4", 3, 4), ("cols_5_8", 5, 8), ("cols_gt8_not_wide", 9, 1 << 30)):
                cov[key] += int((seg & (e["ncx"] >= lo) & (e["ncx"] <= hi)).sum())
            cov["rows_gt8_not_wide"] += int((seg & (e["ncy"] > 8)).sum())
            if 15990 <= e["ir"] <= 16000:
                cov["ir_le_16000_not_wide"] += int((seg & (nhit > 0)).sum())
            if 16000 < e["ir"] <= 16010:
                cov["ir_gt_16000_not_wide"] += int((seg & (nhit > 0)).sum())
            if e["ir"] > 0:
                cov["hit_exactly_at_r"] += int((hit & (m.d2 == e["ir"] * e["ir"])).any(1).sum())
            cov["partial_last_block_3_or_more_cols"] += int((seg & (e["ncx"] >= 3) & (e["cx_hi"] == m.gw - 1) & (m.gw % 8 != 0)
                                                            & (nhit > 0)).sum())
            for k in np.flatnonzero(seg & (e["ncx"] > 8)):
                cov["hits_in_gt8_block_columns"] += int(len(np.unique(m.cx[hit[k]] >> 3)) > 8)
            # an entity clamped into a border cell the query reaches, too far away for a 32-bit square (181 wu)
            if e["ir"] <= 16000:
                for k in np.flatnonzero(seg):
                    c = m.candidates(e, k)
                    cov["far_clamped_entity_in_reach"] += int(len(c) > 0 and m.d2[k, c].max() >= 1 << 31)
            centre = int(np.flatnonzero((query == np.float32(cases.sp_centre(bounds))).all(1))[0])
            cov["wide_by_equality"] += int((e["on_rule"] & (nhit > 1)).sum())
            if len(pos) > 1 and r not in (0.0, 10.0, 30.0, 62.5, 62.51, 200.0, 400.0, 530.0, 1400.0, -1.0):
                cov["wide_one_step_above" if e["wide"][centre] else "not_wide_one_step_below"] += 1
    return cov


def assert_covered():
    cov = coverage()
    empty = [k for k, v in cov.items() if v == 0]
    assert not empty, (empty, cov)
    # (every world has one radius on each side of its own wide threshold)
    assert cov["wide_one_step_above"] == cov["not_wide_one_step_below"] == len(CASES) - 1, cov
    return cov


# ---------------------------------------------------------------------------------------------
# expected lists, computed once per process
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated(name, r, cap):
    bounds, pos, query, _pairs = cases.spatial_cases()[name]
    return navoracle.spatial_query(1, 1, pos, query, r, cap, bounds=bounds)


@functools.lru_cache(maxsize=None)
def referenced(name, r, cap):
    bounds, pos, query, _pairs = cases.spatial_cases()[name]
    return pfref.spatial_query(bounds, pos, query, r, cap)


def lists_differ(ac, ai, bc, bi):
    """None, or the first query whose count or first `count` ids differ."""
    if not np.array_equal(ac, bc):
        return int(np.flatnonzero(ac != bc)[0]), int(ac[ac != bc][0]), int(bc[ac != bc][0])
    live = np.arange(ai.shape[1])[None, :] < ac[:, None]
    bad = ((ai != bi) & live).any(1)
    return (int(np.flatnonzero(bad)[0]), "ids") if bad.any() else None


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_device_lists_equal_restatement_reference_and_model(navlib, name):
    bounds, pos, query, pairs = cases.spatial_cases()[name]
    ctx = navlib.NavContext(1, 1)
    try:
        for r, cap in pairs:
            gc, gi = ctx.spatial_query(pos, query, r, cap, bounds=bounds)
            assert lists_differ(gc, gi, *restated(name, r, cap)) is None, (name, r, cap, lists_differ(gc, gi, *restated(name, r, cap)))
            if pfref.available():
                assert lists_differ(gc, gi, *referenced(name, r, cap)) is None, (name, r, cap, lists_differ(gc, gi, *referenced(name, r, cap)))
            check_against_model(name, r, cap, gc, gi)
    finally:
        ctx.close()


def test_case_matrix_reaches_every_path():
    """At least one query of the matrix (more, in fact: the counts are in the failure message) per segment-pass shape,
    per distance arm, per side of the wide rule, per build, a cap that binds inside the first 64 candidates and one that
    binds after them, a hit exactly at distance r -- counted from the reference's rule, not by the code under test."""
    assert_covered()


def test_builds_do_not_leak_between_worlds(navlib):
    """One context through worlds that alternate the one-workgroup build, the five-launch build (whose counters the
    previous build's k_sp_scan_add has to have cleaned, over ITS cell count) and grid sizes that regrow the buffers:
    every list equals the one a fresh context gives.  Three radii per world: a narrow one, the widest that is not
    wide, and the pool scan -- between them they read every cell_start entry and every pool record of the build."""
    def run(ctx, name):
        bounds, pos, query, pairs = cases.spatial_cases()[name]
        radii = sorted({r for r, _c in pairs})
        picks = [(30.0, 128), (radii[-3] if len(pos) > 1 else 62.5, len(pos) + 5), (radii[-1], len(pos) + 5)]
        return [(r, cap) + ctx.spatial_query(pos, query, r, cap, bounds=bounds) for r, cap in picks]

    shared = navlib.NavContext(1, 1)
    try:
        for visit, name in enumerate(LEAK_ORDER):
            got = run(shared, name)
            fresh_ctx = navlib.NavContext(1, 1)
            try:
                fresh = run(fresh_ctx, name)
            finally:
                fresh_ctx.close()
            for (r, cap, gc, gi), (_r, _cap, fc, fi) in zip(got, fresh):
                assert lists_differ(gc, gi, fc, fi) is None, (visit, name, r, cap, lists_differ(gc, gi, fc, fi))
                assert lists_differ(gc, gi, *restated(name, r, cap)) is None, (visit, name, r, cap)
    finally:
        shared.close()
