"""tests/test_arrival_build_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_arrival_flock_emulated_cpu.py runs its file).  The workgroup of k_arrival_build is four emulated waves: wave 0's
dq_flood, the one-lane heap, the rank sorts behind barriers, the ballots of the thinning pass and of the filter's
compaction go through the emulator's rendezvous; k_arrival_flock runs behind it in its first-build mode.  Every test of the
file has to PASS: a skip counts as a failure here."""
import os
import re
import subprocess
import sys

import pytest

from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_arrival_build_gpu.py"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build")]


def test_arrival_build_tests_pass_on_the_emulated_library():
    lib = hostsim.build_navhip_emu()
    env = dict(os.environ, NAVHIP_LIB=lib)
    env.pop("EMU_STRICT_POINTERS", None)
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-p", "no:cacheprovider", FILE]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = "\n".join(r.stdout.strip().splitlines()[-25:])
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert "failed" not in last and "error" not in last and "skipped" not in last and "deselected" not in last, tail
    m = re.search(r"(\d+) passed", last)
    # the worlds x 8, the chain, the zones without room, argument errors
    assert m and int(m.group(1)) == 8 + 1 + 1 + 1, tail
