"""tests/test_seek_fields_gpu.py WITHOUT a GPU: the library's own sources on the host emulator (tests/hostsim, the way
tests/test_region_repair_emulated_cpu.py runs its file).  k_seek_seeds is one emulated workgroup of 256 lanes per request; its
ballots, shuffles, the DPP row moves of the contours and the workgroup prefix sum go through the emulator's rendezvous, and
k_region_field follows it on the same (serial) stream.  The device buffers of the resident form are the test's own host
tensors.  Every test of the file has to PASS: a skip counts as a failure here.  No case is dropped for the emulator, the
4 097-entity rectangle of the hand-placed world included (its entities are swept, three of them rasterised)."""
import os
import re
import subprocess
import sys

import pytest

from tests import hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_seek_fields_gpu.py"

pytestmark = [pytest.mark.skipif(not hostsim.group_available(), reason="no clang++ (ROCm LLVM) for the host build")]


def test_seek_field_tests_pass_on_the_emulated_library():
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
    # the five worlds in both forms, the second call, the empty call with the refusals, the fields sampled by the step
    assert m and int(m.group(1)) == 5 + 5 + 1 + 1 + 1, tail
