"""tests/test_arrival_velocity_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_dest_queries_emulated_cpu.py runs its file).  The device buffers of the resident calls are the test's own
tensors -- host memory here -- so the run goes without the strict pointer check.  The ballots of the pad ring and the
shuffles of the slot scans' key minimum go through the emulator's rendezvous, rows of one wave in different arms of the
rule included.  Every test of the file has to PASS: a skip counts as a failure here."""
import os
import re
import subprocess
import sys

import pytest

from oracle import pfref
from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_arrival_velocity_gpu.py"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build"),
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]


def test_arrival_velocity_tests_pass_on_the_emulated_library():
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
    # zone worlds x 2, row shapes x 8, frontier / sealed zone, ties and floats, debounce chain, into the step, argument errors
    assert m and int(m.group(1)) == 2 + 8 + 1 + 1 + 1 + 1 + 1, tail
