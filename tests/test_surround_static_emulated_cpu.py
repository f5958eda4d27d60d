"""tests/test_surround_static_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_dest_queries_emulated_cpu.py runs its file).  The device buffers of the resident chain are the test's own
tensors -- host memory here -- so the run goes without the strict pointer check.  The static arm goes through the
emulator's rendezvous: the DPP row moves of the dilation, the LDS rows the lanes read back, the ballot of the touching test,
the floods and the key minima of the pick.  The cap case runs on a smaller box (NAVHIP_STATIC_SMALL_CAP: its premise, the
count of 2 048 entries, is dropped there by that name).  Every test of the file has to PASS: a skip counts as a failure
here."""
import os
import re
import subprocess
import sys

import pytest

from oracle import pfref
from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_surround_static_gpu.py"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build"),
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]


def test_static_surround_tests_pass_on_the_emulated_library():
    lib = hostsim.build_navhip_emu()
    env = dict(os.environ, NAVHIP_LIB=lib, NAVHIP_STATIC_SMALL_CAP="1")
    env.pop("EMU_STRICT_POINTERS", None)
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-p", "no:cacheprovider", FILE]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = "\n".join(r.stdout.strip().splitlines()[-25:])
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert "failed" not in last and "error" not in last and "skipped" not in last and "deselected" not in last, tail
    m = re.search(r"(\d+) passed", last)
    # axis-aligned, rotated + tie, chunk corner + edge, two islands, nothing reachable, the cap, the window,
    # mixed batches x 5, table handling, resident chain, argument errors
    assert m and int(m.group(1)) == 7 + 5 + 3, tail
