"""The work-list dispatch of the agent step at its neighbour-count boundaries (csrc/agent_kernels.hip: k_agent_mid sorts
the agents into eight lists of 64 sub-lists; k_cp_small, k_cp_rows -- main and retry launch --, k_cp_heavy -- team and
wave-per-problem form -- and k_agent_full work out from the counters which agent each unit holds: unit_totals, first_above,
next_unit's static rounds and ticket stripes, the ticket counter of the workgroup problems, two alternating counter sets).
None of it is ClearPath mathematics; off by one, an agent is stepped twice, not at all, or read from the wrong sub-list.

The worlds are tests/dispatch_worlds.py (every agent's neighbour count known beforehand; tests/test_dispatch_worlds_cpu.py
checks that without a GPU).  The reference is the restatement oracle (navoracle.OracleNav.agent_step).  Every step:
  * vel_xz, vpref_xz, new_pos_xz, vdes_xz and status equal the oracle's bit for bit, over all rows of the stepped slab;
  * the outputs are the caller's arrays, filled with a sentinel beforehand: no sentinel survives inside the slab -- every
    row was written at least once (a second write of the same value would not show; a still or held entity's row is
    written too: velocity 0, navhip.h) --, every row outside it keeps the sentinel;
  * navhip_last_step_lists equals the histogram of the intended counts: the device's sorting is tied to the world, not
    only to the end result."""
import ctypes as C

import numpy as np
import pytest

from oracle import navoracle
from tests import cases
from tests import dispatch_worlds as dw

pytestmark = pytest.mark.gpu

FLOATS = ("vel_xz", "new_pos_xz", "vdes_xz", "vpref_xz")
SENTINEL = np.float32(np.nan).view(np.uint32)
_EXPECTED = {}


def _oracle(W, hz=20, work=None):
    """The oracle's outputs for a world, computed once per (world, hz, slab) and shared between the tests."""
    key = (W.name, hz, work)
    if key not in _EXPECTED:
        _EXPECTED[key] = navoracle.OracleNav(W.cost()).agent_step(cases.step_arrays(W.world, W.vdes), hz=hz, work=work, nthreads=16)
    return _EXPECTED[key]


def _context(navlib, W):
    ctx = navlib.NavContext(W.w, W.h)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, W.cost())
    return ctx


def _step(navlib, ctx, W, hz=20, work=None):
    """One host-buffer step into caller-owned, sentinel-filled outputs."""
    w, keep = navlib.make_world(W.w, W.h, cases.step_arrays(W.world, W.vdes), hz=hz)
    if work is not None:
        w.work_begin, w.work_end = work
    out = {k: np.full((W.n, 2), np.nan, np.float32) for k in FLOATS}
    out["status"] = np.full(W.n, 0xAA, np.uint8)
    so = navlib.StepOut()
    for k, a in out.items():
        setattr(so, k, a.ctypes.data)
    assert navlib.lib().navhip_agent_step(ctx._h, C.byref(w), C.byref(so)) == 0
    return out


def _check(navlib, ctx, W, hz=20, work=None, lists=True, tag=None):
    got = _step(navlib, ctx, W, hz, work)
    exp = _oracle(W, hz, work)
    b, e = work if work is not None else (0, W.n)
    inside = np.zeros(W.n, bool)
    inside[b:e] = True
    for k in FLOATS:
        g, x = got[k].view(np.uint32), exp[k].view(np.uint32)
        bad = np.flatnonzero(inside & (g != x).any(1))
        assert len(bad) == 0, (W.name, tag, k, len(bad), bad[:8], W.count[bad[:8]], got[k][bad[:4]], exp[k][bad[:4]])
        assert not (g[inside] == SENTINEL).any(), (W.name, tag, k, "a row of the slab was not written")
        assert (g[~inside] == SENTINEL).all(), (W.name, tag, k, "a row outside the slab was written")
    assert np.array_equal(got["status"][inside], exp["status"][inside]), (W.name, tag)
    assert (got["status"][~inside] == 0xAA).all(), (W.name, tag)
    if lists:
        assert list(ctx.last_step_lists()) == W.lists(work), (W.name, tag, work)
    return got


@pytest.mark.parametrize("name", ["ladder", "ladder_garrisoned"])
def test_ladder_of_neighbour_counts(navlib, name):
    """0, 1, 2 | 3, 4 | 5, 8 | 9, 16 | 17, 32 | 33, 63, 64 neighbours and both caps, twelve agents and more at each; the
    variant with garrisoned entities inside some clusters (the irregular list beside the others).  The whole range, a slab
    whose bounds are no multiples of 64 and cut through clusters (twice: the second one starts where the first ended), and
    a step at 10 Hz, on one context."""
    W = dw.get(name)
    ctx = _context(navlib, W)
    got = _check(navlib, ctx, W, tag="whole")
    assert np.abs(got["vel_xz"]).max() > 0
    for work in ((37, 411), (411, W.n - 29)):
        assert work[0] % 64 and work[1] % 64
        _check(navlib, ctx, W, work=work, tag="slab")
    _check(navlib, ctx, W, hz=10, tag="10 Hz")
    ctx.close()


def test_sparse_lists_take_turns_on_one_context(navlib):
    """Five worlds with one agent on ROW2 | four on ROW0 | five on ROW1 | one with 17 neighbours and nobody with 33+ (an
    empty heavy half in front of the wave half of k_cp_heavy's table) | one with 34 and nobody with 17-32 -- stepped one
    after the other on ONE context, then in reverse order: every step reads the counter set its predecessor's k_cp_heavy
    cleared, after lists that were empty.  In between a world in which nobody has a neighbour (a step that launches and
    leaves every list empty) and an empty slab (nothing is launched: the parity must not flip, the lists of the step before
    stay the latest).  Every step against the oracle and against a context of its own."""
    worlds = [dw.get(name) for name in dw.SPARSE]
    none = dw.get("no_neighbours")
    shared = _context(navlib, worlds[0])
    seq = worlds + [none] + worlds[::-1] + [none]
    for k, W in enumerate(seq):
        got = _check(navlib, shared, W, tag=k)
        fresh = _context(navlib, W)
        alone = _step(navlib, fresh, W)
        assert list(fresh.last_step_lists()) == W.lists()
        fresh.close()
        for key in FLOATS + ("status",):
            assert np.array_equal(got[key].view(np.uint8), alone[key].view(np.uint8)), (k, W.name, key)
        if k % 3 == 1:
            # an empty slab (begin = end > 0; 0, 0 would mean everybody): no row written, the lists unchanged
            _check(navlib, shared, W, work=(5, 5), tag=(k, "empty slab"), lists=False)
            assert list(shared.last_step_lists()) == W.lists()
    shared.close()


def test_one_list_full_deals_units_out_statically(navlib):
    """36 864 agents with 5 neighbours: 9 216 units on ROW2 alone, 2.25 per wave of the main k_cp_rows launch (1 024
    workgroups of four) -- next_unit deals the first round out by wave number (static_rounds = 9 216 / 4 096 - 1 = 1) and
    the other 5 120 by ticket over the 32 stripes.  (The oracle with 16 threads: 0.06 s.)"""
    W = dw.get("one_list_full")
    ctx = _context(navlib, W)
    _check(navlib, ctx, W)
    ctx.close()


def test_solo_heavy_takes_a_problem_per_wave(navlib):
    """8 208 agents with 17 neighbours, nobody with 33+: k_cp_heavy's table starts with an empty heavy half, and from
    CP_SOLO_MIN = 8 192 problems on every wave takes problems of its own -- the first nblk * 4 = 2 056 by wave number, the
    rest by ticket.  (The oracle with 16 threads: 0.07 s.)"""
    W = dw.get("solo_heavy")
    ctx = _context(navlib, W)
    _check(navlib, ctx, W)
    ctx.close()


def test_retry_flood_puts_a_quarter_of_the_agents_on_the_retry_list(navlib):
    """8 192 agents with 3 neighbours (nwork a multiple of 4 096), the one in the middle of every quad without an
    admissible candidate in k_cp_small's single attempt: 2 048 and more entries on the retry list -- 512 units and more for
    the 256 waves of the retry launch, static_rounds = 1.  The retry counters (navhip_debug_cp_attempts, as bench.py
    reads them) count every problem that did not return in its first attempt: here the retry launch's.  (Some 32 entries
    per sub-list of the retry list: its capacity, nh_worklist_cap, is not approached by this or any other test.)"""
    W = dw.get("retry_flood")
    att = (C.c_ulonglong * 9)()
    ctx = _context(navlib, W)
    assert navlib.lib().navhip_debug_cp_attempts(att, 1) == 0
    _check(navlib, ctx, W)
    assert navlib.lib().navhip_debug_cp_attempts(att, 1) == 0
    ctx.close()
    retried = sum(att[i] for i in range(8))
    print("retry_flood: retried", retried, list(att))
    assert retried >= dw.RETRY_ESTABLISHED, list(att)


def test_a_jam_between_two_sparse_steps(navlib):
    """ladder, solo_heavy, ladder on ONE context (the ladder in the middle of solo_heavy's map): the scratch regrows from
    690 to 8 208 agents, and the counters and tickets of a jam are followed by a step with a few agents on every list."""
    ctx = _context(navlib, dw.get("solo_heavy"))
    for k, name in enumerate(("ladder_wide", "solo_heavy", "ladder_wide")):
        _check(navlib, ctx, dw.get(name), tag=k)
    ctx.close()
