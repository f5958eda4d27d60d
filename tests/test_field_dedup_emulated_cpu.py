"""tests/test_field_dedup_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_attack_fields_emulated_cpu.py runs its file).  The classing pass's compare-and-swap, exchange and ballot go
through the emulator's atomics and rendezvous.  Every case runs and has to PASS: a skip counts as a failure here.

Two runs: the host-buffer cases with the strict pointer check; the scratch-reuse case, whose buffers are the test's own
tensors -- host memory here -- without it."""
import os
import re
import subprocess
import sys

import pytest

from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_field_dedup_gpu.py"
OWN_TENSORS = "three_builds_in_flight"
# mixed classes: 2 worlds x 2 modes; then near-duplicates, the mergeable flag, never merged, IF_CHANGED, pool slots,
# integration fields, table pressure, smallest lists: 2 modes each | scratch reuse: 2 modes
COUNTS = {True: 4 + 8 * 2, False: 2}

pytestmark = pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build")


@pytest.mark.parametrize("strict", [True, False])
def test_field_dedup_tests_pass_on_the_emulated_library(strict):
    lib = hostsim.build_navhip_emu()
    env = dict(os.environ, NAVHIP_LIB=lib)
    env.pop("EMU_STRICT_POINTERS", None)
    if strict:
        env["EMU_STRICT_POINTERS"] = "1"
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-p", "no:cacheprovider", FILE,
           "-k", ("not " if strict else "") + OWN_TENSORS]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = "\n".join(r.stdout.strip().splitlines()[-25:])
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert "failed" not in last and "error" not in last and "skipped" not in last, tail
    m = re.search(r"(\d+) passed, (\d+) deselected", last)
    assert m and int(m.group(1)) == COUNTS[strict] and int(m.group(2)) == COUNTS[not strict], tail
