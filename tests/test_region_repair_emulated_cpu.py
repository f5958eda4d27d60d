"""tests/test_region_repair_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_order_queries_emulated_cpu.py runs its file).  k_region_repair is one emulated workgroup of 256 lanes per row: the
flood's and the relaxation's __syncthreads_or loops and the barrier the serial arm's idle lanes wait at go through the
emulator's rendezvous.  The device buffers of the resident form are the test's own host tensors.  Every test of the file
has to PASS: a skip counts as a failure here.  No case is dropped or shrunk for the emulator (times: the GPU file)."""
import os
import re
import subprocess
import sys

import pytest

from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_region_repair_gpu.py"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build")]


def test_region_repair_tests_pass_on_the_emulated_library():
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
    # the thirteen cases alone, the four shapes, the empty calls, the handed-back rows, the refusals, the four chains
    assert m and int(m.group(1)) == 13 + 4 + 1 + 1 + 1 + 4, tail
