"""The gfx950 build of the ClearPath search on structured problems (tests/cp_lattice_problems.py): agents inside lattices
with one common velocity, rings of equally far neighbours, duplicate cones, neighbours exactly on the agent -- candidates
that tie in distance, removals that tie, vertical side rays.  The wave-per-problem form, the 16-lane row form (16
neighbours and fewer) and the workgroup form each equal G_ClearPath_NewVelocity (clearpath.c:694) of the reference build
bit for bit on every problem; tests/test_cp_lattice_cpu.py checks the premises and the same sources on the emulator."""
import ctypes as C

import numpy as np
import pytest

from oracle import pfref
from tests import cp_lattice_problems as lp

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]


@pytest.mark.parametrize("rows", [False, True, "team"], ids=["wave", "rows", "team"])
def test_structured_problems_equal_reference(navlib, rows):
    P = lp.problems()
    exp = lp.expected()
    idx = np.flatnonzero(P[3] + P[5] <= 16) if rows is True else np.arange(len(exp))
    assert len(idx) > 100
    att = (C.c_ulonglong * 9)()
    assert navlib.lib().navhip_debug_cp_attempts(att, 1) == 0
    ctx = navlib.NavContext(1, 1)
    got = ctx.G_ClearPath_NewVelocity(*lp.select(P, idx), rows=rows)
    ctx.close()
    assert navlib.lib().navhip_debug_cp_attempts(att, 1) == 0
    bad = lp.mismatches(got, exp[idx])
    assert len(bad) == 0, (rows, len(bad), [lp.NAMES[idx[i]] for i in bad[:6]], got[bad[:3]], exp[idx][bad[:3]])
    retried = sum(att[i] for i in range(8))
    print("cp_lattice", rows, "retried", retried, list(att))
    # (tests/test_cp_lattice_cpu.py: 56 problems fail their first attempt, 8 of them among those of the row form)
    assert retried >= (5 if rows is True else 50), list(att)
