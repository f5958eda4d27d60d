"""tests/test_faction_changed_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_los_chain_emulated_cpu.py runs its file).  The pool of a chain is the test's own tensor -- host memory here --
so the run goes without the strict pointer check.  The flags of every batch on both layers, the faction chain and the
mixed chain in both refresh modes, the rejections and NAVHIP_REQ_IF_CHANGED on both field kernels: the ballots of
k_refresh_touched and k_los_mark go through the emulator's rendezvous.  Every selected test has to PASS: a skip counts as
a failure here."""
import os
import re
import subprocess
import sys

import pytest

from oracle import pfref
from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_faction_changed_gpu.py"
SELECT = "not wide_level"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build"),
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]


def test_faction_changed_tests_pass_on_the_emulated_library():
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
    # the flags: 4 batches + sticky + no factions plane; the chains: 1 build + 3 batches x 2 modes; the rejections;
    # IF_CHANGED x 2 kernels.  Left out: the wide level x 2 modes (2 200 LOS fields each on one host thread)
    assert m and int(m.group(1)) == 4 + 1 + 1 + 1 + 6 + 1 + 2 and int(m.group(2)) == 2, tail
