"""tests/test_attack_fields_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_emulated_cpu.py runs the other parity files), with the strict pointer check.  Only the test at benchmark size
is left out, and every other one has to PASS: a skip counts as a failure here."""
import os
import re
import subprocess
import sys

import pytest

from oracle import pfref
from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_attack_fields_gpu.py"
AT_SIZE = FILE + "::test_attacking_fields_at_benchmark_size"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build"),
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]


def test_attacking_path_tests_pass_on_the_emulated_library():
    lib = hostsim.build_navhip_emu()
    env = dict(os.environ, NAVHIP_LIB=lib, EMU_STRICT_POINTERS="1")
    base = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-p", "no:cacheprovider", FILE, "--deselect", AT_SIZE]
    r = subprocess.run(base + ["--collect-only"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    m = re.search(r"(\d+)/(\d+) tests collected \(1 deselected\)", r.stdout)
    assert r.returncode == 0 and m, r.stdout[-2000:]
    selected = int(m.group(1))
    assert selected == int(m.group(2)) - 1 and selected >= 20
    cmd = list(base)
    try:
        import xdist  # noqa: F401
        cmd += ["-n", str(min(8, os.cpu_count() or 1))]
    except ImportError:
        pass
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    tail = "\n".join(r.stdout.strip().splitlines()[-25:])
    assert r.returncode == 0, tail
    last = r.stdout.strip().splitlines()[-1]
    assert "failed" not in last and "error" not in last and "skipped" not in last, tail
    assert int(last.split(" passed")[0].split()[-1]) == selected, tail
