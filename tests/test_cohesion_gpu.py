"""k_cohesion, k_coh_plan and the lane regrouping (csrc/cohesion_kernels.hip) on the worlds of tests/cohesion_worlds.py:
probes whose vpref IS fl(0.15f * cohesion) with |com - me| between the two clamps, flocks in clusters 890-930 wu from each
other's boxes (every survivor count of the tile walk, carried tails, waves of active and inactive quads), 1 .. 513 flocks
with empty ones in front, in the middle and at the end, and 4 096 and more probe/mate lengths through coh_batch's own square
root, t and side paths.  tests/test_cohesion_cpu.py checks without a GPU that the worlds hold all that.

Every world is stepped three ticks on one context with the positions kept: tick 0 runs the identity grouping, ticks 1 and
2 the regrouped lanes (coh_regroup_due, step_api.hip).  vpref_xz and vel_xz equal the restatement's as uint32 on every tick."""
import ctypes as C

import numpy as np
import pytest

from oracle import navoracle
from tests import cohesion_worlds as cw

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def _oracle(W, hz, arrays=None, work=None, tag=""):
    key = (W.name, hz, work, tag)
    if key not in _EXPECTED:
        _EXPECTED[key] = navoracle.OracleNav(W.cost()).agent_step(W.arrays if arrays is None else arrays, hz=hz, work=work, nthreads=16)
    return _EXPECTED[key]


def _context(navlib, W):
    ctx = navlib.NavContext(W.w, W.h)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, W.cost())
    return ctx


def _step(navlib, ctx, W, hz, arrays=None, work=None, epoch=0):
    a = dict(W.arrays if arrays is None else arrays, static_epoch=epoch)
    w, keep = navlib.make_world(W.w, W.h, a, hz=hz)
    if work is not None:
        w.work_begin, w.work_end = work
    out = {k: np.full((W.n, 2), np.nan, np.float32) for k in ("vel_xz", "vpref_xz")}
    so = navlib.StepOut()
    for k, arr in out.items():
        setattr(so, k, arr.ctypes.data)
    assert navlib.lib().navhip_agent_step(ctx._h, C.byref(w), C.byref(so)) == 0
    return out


def _check(got, exp, W, tag, work=None):
    b, e = work if work is not None else (0, W.n)
    for k in ("vpref_xz", "vel_xz"):
        g, x = got[k][b:e].view(np.uint32), exp[k][b:e].view(np.uint32)
        bad = b + np.flatnonzero((g != x).any(1))
        assert len(bad) == 0, (W.name, tag, k, len(bad), bad[:8], W.arrays["flock"][bad[:8]], got[k][bad[:4]], exp[k][bad[:4]])


def _three_ticks(navlib, W, hz):
    ctx = _context(navlib, W)
    exp = _oracle(W, hz)
    for tick in range(3):
        _check(_step(navlib, ctx, W, hz), exp, W, tick)
    return ctx, exp


@pytest.mark.parametrize("hz", [20, 1])
def test_window_probes(navlib, hz):
    """Flocks of 2, 3, 17, 33, 257 and 300 members (the last with 258 mates out of range: a carried
    tail), 310 probes with smf / 15 < |com - me| < smf at this tick rate: the sum shows
    in vpref at full precision."""
    W = cw.get("window%d" % hz)
    ctx, exp = _three_ticks(navlib, W, hz)
    ctx.close()
    assert np.abs(exp["vpref_xz"][W.probes]).max(1).min() > 0


def test_arith_lengths(navlib):
    """Lengths from 1e-20 to 300 wu, len == 16.0 and its neighbours, coincident members, 0 < ss < 2^-90, batches with one,
    several and no lane on the `close` and on the `odd` path."""
    W = cw.get("arith")
    ctx, exp = _three_ticks(navlib, W, 20)
    ctx.close()
    assert np.abs(exp["vpref_xz"][W.probes]).max(1).min() > 0


def test_far_clusters(navlib):
    """Survivor counts 0, 1, 15, 16, 17, 31, 32 and 33 per tile, an empty tile between two others, own members in carried
    tails and in the second and third tile, waves of active and inactive quads; a fourth tick with the positions of two
    clusters swapped member by member under unchanged flock tables: the carried grouping, built for the old positions, puts
    both ends of the map into one wave and is only a hint (tests/test_cohesion_cpu.py: its survivor counts are not those of
    a fresh grouping)."""
    W = cw.get("far_clusters")
    ctx, exp = _three_ticks(navlib, W, 20)
    swapped = W.swapped()
    _check(_step(navlib, ctx, W, 20, arrays=swapped), _oracle(W, 20, arrays=swapped, tag="swapped"), W, "swapped")
    ctx.close()
    assert np.abs(exp["vel_xz"]).max() > 0


@pytest.mark.parametrize("nf", cw.PLAN_SHAPES)
def test_plan_shapes(navlib, nf):
    """1, 63, 64, 65, 256, 257 and 513 flocks of 0-20 members, empty flocks first, in a run in the middle and last, flocks
    of one, flocks that are all idle; then a slab (twice: the second call runs the grouping the first one left) whose
    range leaves flocks without a member inside, and the whole range again."""
    W = cw.get("plan_%d" % nf)
    ctx, exp = _three_ticks(navlib, W, 20)
    b, e, epoch = W.slab
    slab = _oracle(W, 20, work=(b, e))
    for k in range(2):
        _check(_step(navlib, ctx, W, 20, work=(b, e), epoch=epoch), slab, W, ("slab", k), work=(b, e))
    _check(_step(navlib, ctx, W, 20), exp, W, "whole again")
    ctx.close()
    assert np.abs(exp["vel_xz"]).max() > 0
