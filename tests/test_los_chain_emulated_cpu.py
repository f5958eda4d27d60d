"""tests/test_los_chain_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_attack_fields_emulated_cpu.py runs its file).  The pool of a chain is the test's own tensor -- host memory
here -- so the run goes without the strict pointer check, like the tick tests of tests/test_emulated_cpu.py.  The 3 x 3-chunk map with every
blocker batch in both modes, the build and the rejections: the ballots of the stale-slot compaction go through
the emulator's rendezvous, the level order through its in-order launches.  Every selected test has to PASS: a skip counts
as a failure here."""
import os
import re
import subprocess
import sys

import pytest

from oracle import pfref
from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_los_chain_gpu.py"
SELECT = "3x3 or rejects"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build"),
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]


def test_los_chain_tests_pass_on_the_emulated_library():
    lib = hostsim.build_navhip_emu()
    env = dict(os.environ, NAVHIP_LIB=lib)
    env.pop("EMU_STRICT_POINTERS", None)
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-p", "no:cacheprovider", FILE, "-k", SELECT]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = "\n".join(r.stdout.strip().splitlines()[-25:])
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert "failed" not in last and "error" not in last and "skipped" not in last, tail
    m = re.search(r"(\d+) passed, (\d+) deselected", last)
    # the 3 x 3 map: 1 build + 5 batches x 2 modes + (f) x 2 modes; the rejections.  Left out: the 5 x 2 map, and the two
    # tick tests (four minutes on the emulator)
    assert m and int(m.group(1)) == 1 + 10 + 2 + 1 and int(m.group(2)) == 1 + 10 + 2 + 2, tail
