"""The ClearPath search on structured problems (tests/cp_lattice_problems.py: lattices, equal-distance rings, neighbours
exactly on the agent) WITHOUT a GPU: the premises of the problems -- they really tie --, then the device's own search
sources on the host emulator (tests/hostsim: clearpath_grp<64>, <16>, the workgroup form, the serial search) and the
restatement oracle against G_ClearPath_NewVelocity (clearpath.c:694) of the reference build, bit for bit on every
problem.  tests/test_cp_lattice_gpu.py runs the same problems through the gfx950 build."""
import numpy as np
import pytest

from oracle import navoracle, pfref
from tests import cp_lattice_problems as lp
from tests import hostsim

pytestmark = [pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present"),
              pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build")]

expected, mismatches = lp.expected, lp.mismatches


def _assert_same(got, exp, tag, idx=None):
    bad = mismatches(got, exp)
    names = [lp.NAMES[i if idx is None else idx[i]] for i in bad[:6]]
    assert len(bad) == 0, (tag, len(bad), names, got[bad[:3]], exp[bad[:3]])


def test_problems_are_exact_and_named():
    ent, des, dyn, nd, stat, ns = lp.problems()
    assert 300 <= len(ent) <= 400 and len(set(lp.NAMES)) == len(lp.NAMES) == len(ent)
    assert (ent[:, 0] == lp.OFFSET[0]).all() and (ent[:, 1] == lp.OFFSET[1]).all()
    for arr in (ent, des, dyn, stat):
        assert np.array_equal(arr * 8, np.rint(arr * 8))                 # multiples of 1/8
    assert set(np.unique(nd + ns)) >= {8, 9, 10, 11, 12, 24} and (nd + ns <= 16).sum() > 100 and (nd + ns > 16).sum() > 100
    assert ((nd > 0) & (ns > 0)).sum() > 80


def test_premises_hold():
    """The problems have what they were built for: 10 and more with a tie between the winning candidate and another
    admissible one, with two equally far neighbours of one list at a removal, with a vertical side ray; 50 and more whose
    first attempt fails."""
    p = lp.premises(lp.problems())
    print("cp_lattice premises:", p)
    assert p["candidate_tie"] >= 10 and p["removal_tie"] >= 10 and p["vertical_ray"] >= 10, p
    assert p["retried"] >= 50, p


def test_restatement_equals_reference():
    ent, des, dyn, nd, stat, ns = lp.problems()
    _assert_same(navoracle.clearpath(ent, des, dyn, nd, stat, ns), expected(), "navoracle")


def test_wave_search_on_the_emulator_equals_reference():
    """clearpath_grp<64> (k_cp_heavy's wave-per-problem form, k_agent_full) on every problem; 50 and more retried."""
    P = lp.problems()
    hostsim.group_attempts(reset=True)
    got, ops = hostsim.clearpath_group(64, *P)
    att = hostsim.group_attempts()
    _assert_same(got, expected(), "grp<64>")
    print("cp_lattice grp<64> attempts:", att)
    assert sum(att[0:8]) >= 50, att


def test_row_search_on_the_emulator_equals_reference():
    """clearpath_grp<16> (k_cp_rows) on the problems with 16 neighbours and fewer."""
    P = lp.problems()
    idx = np.flatnonzero(P[3] + P[5] <= 16)
    assert len(idx) > 100
    hostsim.group_attempts(reset=True)
    got, ops = hostsim.clearpath_group(16, *lp.select(P, idx))
    att = hostsim.group_attempts()
    _assert_same(got, expected()[idx], "grp<16>", idx)
    assert sum(att[0:8]) >= 5, att


def test_team_search_on_the_emulator_equals_reference():
    """clearpath_grp<64, true>: a workgroup of four waves per problem (k_cp_heavy outside a jam)."""
    P = lp.problems()
    hostsim.group_attempts(reset=True)
    got, ops = hostsim.clearpath_team(*P)
    att = hostsim.group_attempts()
    _assert_same(got, expected(), "team")
    assert sum(att[0:8]) >= 50, att


def test_serial_search_equals_reference_where_it_finds_a_candidate():
    """clearpath_light (k_cp_small's single attempt per thread): where it reports a candidate, that is the reference's."""
    P = lp.problems()
    got, found = hostsim.clearpath_light(*P)
    idx = np.flatnonzero(found != 0)
    assert len(idx) >= len(P[0]) - lp.premises(P)["retried"] - 5 and len(idx) > 250, len(idx)
    _assert_same(got[idx], expected()[idx], "light", idx)
