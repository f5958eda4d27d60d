"""tests/test_arrival_flock_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_arrival_velocity_emulated_cpu.py runs its file).  The device buffers of the resident calls are the test's own
tensors -- host memory here -- so the run goes without the strict pointer check.  The workgroup of k_arrival_flock is four
emulated waves: its barriers, the level-synchronous flood's __syncthreads_or and the shuffles of the (distance, index)
minimum go through the emulator's rendezvous.  Every test of the file has to PASS: a skip counts as a failure here."""
import os
import re
import subprocess
import sys

import pytest

from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_arrival_flock_gpu.py"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build")]


def test_arrival_flock_tests_pass_on_the_emulated_library():
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
    # the worlds x 10, the chain, host rows, the cap as a host row, argument errors
    assert m and int(m.group(1)) == 10 + 1 + 1 + 1 + 1, tail
