"""CPU checks of the drop-in boundary: libnavhip.so builds, loads, exports every symbol that
include/navhip.h declares, its PODs have the layout the ctypes mirror assumes, its host-only
entry points answer, and -- without a GPU -- every compute entry point fails LOUDLY (no CPU
fallback inside the product)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "navhip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(navhip_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound(navlib):
    L = navlib.lib()
    names = _declared()
    assert len(names) >= 25
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, "declared in include/navhip.h but not exported: %s" % missing
    unbound = [n for n in names if n not in navlib._SIGS]
    assert not unbound, "exported but not mirrored in navhip.py: %s" % unbound
    ghost = [n for n in navlib._SIGS if n not in names]
    assert not ghost, "navhip.py binds undeclared symbols: %s" % ghost
    # ... and nothing else leaves the library: kernels, launch helpers and C++ internals stay local
    # (csrc/navhip.map), every dynamic symbol it defines is declared in the header
    out = subprocess.run(["nm", "-D", "--defined-only", navlib.LIB_PATH], stdout=subprocess.PIPE, text=True,
                         check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.split()[1] in "TDBW")
    extra = [n for n in exported if n not in names]
    assert not extra, "exported but not declared in include/navhip.h: %s" % extra


def _header_records():
    """{C type name: member names in order} of every record include/navhip.h defines."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"typedef struct (navhip_\w+) \{(.*?)\} \1;", src, re.S):
        decls = [d for d in m.group(2).split(";") if d.strip()]
        out[m.group(1)] = [re.search(r"(\w+)\s*$", part).group(1) for d in decls for part in d.split(",")]
    return out


def _mirror_members(rec):
    """[(C member designator, offset)] of a record of navhip.RECORDS: every member, those of nested structures included."""
    if isinstance(rec, np.dtype):
        return [(name, rec.fields[name][1]) for name in rec.names]
    out, todo = [], [("", 0, rec)]
    while todo:
        prefix, base, cls = todo.pop()
        for name, typ in cls._fields_:
            off = base + getattr(cls, name).offset
            out.append((prefix + name, off))
            if issubclass(typ, C.Structure):
                todo.append((prefix + name + ".", off, typ))
    return out


def test_header_is_plain_c_and_layouts_match(navlib, tmp_path):
    """The header must compile as C99 (the reference's host language) and the PODs crossing the
    boundary must have the sizes/offsets the Python mirror uses: every record of navhip.RECORDS, every member."""
    from oracle import navoracle
    header = _header_records()
    # the mirror names every record the header defines (navhip_counters crosses as COUNTER_NAMES), member for member
    assert sorted(navlib.RECORDS) == sorted(set(header) - {"navhip_counters"})
    for cname, rec in navlib.RECORDS.items():
        mine = list(rec.names) if isinstance(rec, np.dtype) else [f[0] for f in rec._fields_]
        assert mine == header[cname], cname
    assert list(navlib.COUNTER_NAMES) == header["navhip_counters"]
    lines = ['printf("sizeof.%s %%zu\\n", sizeof(%s));' % (c, c) for c in header]
    lines += ["P(%s, %s);" % (c, f) for c, rec in navlib.RECORDS.items() for f, _ in _mirror_members(rec)]
    prog = tmp_path / "layout.c"
    prog.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "navhip.h"
#define P(T, f) printf(#T "." #f " %zu\\n", offsetof(T, f))
int main(void){
    ''' + "\n    ".join(lines) + '''
    return 0;
}''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I",
                           os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    got = {k: int(v) for k, v in got.items()}
    for cname, rec in navlib.RECORDS.items():
        assert got["sizeof." + cname] == (rec.itemsize if isinstance(rec, np.dtype) else C.sizeof(rec)), cname
        for f, off in _mirror_members(rec):
            assert got[cname + "." + f] == off, (cname, f)
    assert got["sizeof.navhip_field_req"] == navlib.FIELD_REQ_DTYPE.itemsize == 32
    assert got["sizeof.navhip_circle"] == navlib.CIRCLE_DTYPE.itemsize == 24
    assert got["sizeof.navhip_arrival_zone"] == C.sizeof(navlib.ArrivalZone) == 48
    assert got["sizeof.navhip_counters"] == 8 * len(navlib.COUNTER_NAMES)
    # the oracle restates the records it passes on its own (it does not import the product package)
    assert C.sizeof(navoracle.World) == got["sizeof.navhip_world"]
    assert C.sizeof(navoracle.StepOut) == got["sizeof.navhip_step_out"]
    for name in ("FIELD_REQ_DTYPE", "CIRCLE_DTYPE", "LOS_REQ_DTYPE", "REGION_REQ_DTYPE"):
        assert getattr(navoracle, name) == getattr(navlib, name), name


def _ff_id_expected(r):
    """N_FlowFieldID restated from field.c:1952-1975 (independent of the C code under test)."""
    if r["type"] == 0:
        return ((int(r["layer"]) << 60) | (0 << 56) | ((int(r["next_iid"]) & 0xf) << 48)
                | ((int(r["port_iid"]) & 0xf) << 40) | (int(r["port_r0"]) << 34)
                | (int(r["port_c0"]) << 28) | (int(r["port_r1"]) << 22) | (int(r["port_c1"]) << 16)
                | (int(r["chunk_r"]) << 8) | int(r["chunk_c"]))
    return ((int(r["layer"]) << 60) | (1 << 56) | (int(r["tile_r"]) << 24) | (int(r["tile_c"]) << 16)
            | (int(r["chunk_r"]) << 8) | int(r["chunk_c"]))


def test_flow_field_id_bit_layout(navlib):
    rng = np.random.RandomState(0)
    reqs = navlib.make_reqs(64)
    reqs["layer"] = rng.randint(0, 12, 64)
    reqs["type"] = rng.randint(0, 2, 64)
    for f in ("tile_r", "tile_c", "port_r0", "port_c0", "port_r1", "port_c1", "chunk_r", "chunk_c"):
        reqs[f] = rng.randint(0, 64, 64)
    reqs["port_iid"] = rng.randint(0, 40, 64)
    reqs["next_iid"] = rng.randint(0, 40, 64)
    ids = [navlib.N_FlowFieldID(reqs[i]) for i in range(64)]
    assert ids == [_ff_id_expected(reqs[i]) for i in range(64)]
    # distinct requests of one chunk never collide on the cache key
    assert len(set(ids)) == 64


def test_flow_field_id_matches_the_reference(navlib):
    """navhip_flow_field_id / navhip_region_field_id against the reference's own N_FlowFieldID
    (field.c:1952) through oracle/_ref: the planner's real request stream (real portals, island ids
    above 15) plus every region target kind."""
    from oracle import pfref
    from tests import cases
    if not (pfref.available() or os.path.isdir("/root/reference")):
        pytest.skip("oracle/_ref not built and /root/reference absent")
    grid, nav = cases.ref_nav_for(4, 3, seed=21)
    reqs_t = cases.tile_requests(grid, 16, seed=5)
    reqs_p, _b, _a = cases.planner_requests(nav, grid, pairs=10, seed=9)
    ref_reqs = np.concatenate([reqs_t, reqs_p])
    assert (ref_reqs["type"] == 0).sum() > 8
    for layer in (0, 3, 11):
        ref_reqs["layer"] = 0                      # (the portals are those of layer 0)
        want = [nav.flow_field_id(r) for r in ref_reqs]
        mine = cases.reqs_from_ref(navlib, ref_reqs)
        got = [navlib.N_FlowFieldID(mine[i]) for i in range(len(mine))]
        assert got == want
        # the layer field only enters through the top nibble (field.c:1956,1969)
        mine["layer"] = layer
        got_l = [navlib.N_FlowFieldID(mine[i]) for i in range(len(mine))]
        assert got_l == [(w & ~(0xf << 60)) | (layer << 60) for w in want]
    rng = np.random.RandomState(2)
    for _ in range(200):
        layer, cr, cc = int(rng.randint(12)), int(rng.randint(64)), int(rng.randint(64))
        fac, uid = int(rng.randint(15)), int(rng.randint(1 << 20))
        ar, ac, rad = int(rng.randint(64 * 64)), int(rng.randint(64 * 64)), int(rng.randint(1, 200))
        for kind, a, b, c in ((navlib.FFID_ENEMIES, fac, 0, 0), (navlib.FFID_ENTITY, uid, 0, 0),
                              (navlib.FFID_ZONE, ar, ac, rad)):
            assert navlib.N_RegionFieldID(kind, layer, cr, cc, a, b, c) \
                == pfref.RefNav.region_field_id(kind, layer, cr, cc, a, b, c), (kind, a, b, c)
    assert navlib.N_RegionFieldID(3, 0, 1, 1, 0) == 0          # TARGET_PORTALMASK has no cache key
    nav.close()


def test_invalid_arguments_are_rejected(navlib):
    L = navlib.lib()
    h = C.c_void_p()
    assert L.navhip_ctx_create(C.byref(h), 0, 4, 0) == -1          # NAVHIP_ERR_INVALID
    assert L.navhip_ctx_create(C.byref(h), 65, 4, 0) == -1         # 6-bit chunk ids, nav.c:841
    assert L.navhip_ctx_create(None, 4, 4, 0) == -1
    assert L.navhip_sync(None) == -1
    assert L.navhip_build_fields(None, None, 1, None, None) == -1
    assert L.navhip_device(None) == -1
    assert L.navhip_plane_dev(None, 0, 0) is None
    assert L.navhip_last_error(None) == b""
    # the state pass (csrc/state_kernels.hip): no context, no answer
    w = navlib.World()
    assert L.navhip_heading_gate(None, C.byref(w), C.byref(navlib.GateIn()), None, None, None) == -1
    assert L.navhip_heading_gate_dev(None, C.byref(w), C.byref(navlib.GateIn()), None, None, None, None) == -1
    assert L.navhip_settled_count(None, C.byref(w), 1, None, None) == -1
    assert L.navhip_arrival_settle(None, C.byref(w), C.byref(navlib.SettleIn()), C.byref(navlib.SettleOut())) == -1
    assert L.navhip_arrival_settle_dev(None, C.byref(w), C.byref(navlib.SettleIn()), C.byref(navlib.SettleOut()), None) == -1
    assert L.navhip_state_update_aux(None, C.byref(w), C.byref(navlib.StateAuxIn()), None, None, None) == -1
    assert L.navhip_state_update_aux_dev(None, C.byref(w), C.byref(navlib.StateAuxIn()), None, None, None, None) == -1
    assert L.navhip_state_pass(None, C.byref(w), C.byref(navlib.StatePassIn()), C.byref(navlib.StatePassOut())) == -1


def _gpu_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_gpu_visible(), reason="a GPU is present: the loud-failure path cannot be seen")
def test_no_gpu_means_loud_failure_not_cpu_fallback(navlib):
    """The product path must refuse to run without the device: no CPU fallback, no oracle."""
    with pytest.raises(navlib.NavHipError):
        navlib.NavContext(2, 2, device=0)
    src = open(os.path.join(ROOT, "permafrost-engine_amd", "navhip.py")).read() \
        + open(os.path.join(ROOT, "permafrost-engine_amd", "tick.py")).read() \
        + open(os.path.join(ROOT, "permafrost-engine_amd", "dist.py")).read()
    assert "oracle" not in src, "product code must not import the oracle"


def test_product_sources_do_not_reference_the_oracle():
    pkg = os.path.join(ROOT, "permafrost-engine_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".c", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "pfref" not in txt and "navoracle" not in txt, f


def _device_kernels(lib_path, tmp_path):
    """{kernel name: (allocated VGPRs, LDS bytes)} of the gfx950 code objects embedded in the built library (the
    HSA metadata notes, read with the ROCm LLVM tools; None when they are not there)."""
    import re
    import shutil
    import subprocess
    objdump, readelf = (os.path.join("/opt/rocm/lib/llvm/bin", t) for t in ("llvm-objdump", "llvm-readelf"))
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        return None
    work = os.path.join(str(tmp_path), "co")
    os.makedirs(work, exist_ok=True)
    shutil.copy(lib_path, work)                      # (--offloading extracts next to its input)
    subprocess.run([objdump, "--offloading", os.path.basename(lib_path)], cwd=work, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL, check=False)
    out = {}
    for f in os.listdir(work):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([readelf, "--notes", f], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                               text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            vgpr = re.search(r"\.vgpr_count:\s+(\d+)", block)
            lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
            if name and vgpr and lds:
                out[name.group(1)] = (int(vgpr.group(1)), int(lds.group(1)))
    return out or None


def test_persistent_clearpath_kernels_share_their_allocation_granules(tmp_path):
    """Hole inheritance: k_cp_heavy's persistent workgroups move into the register and LDS ranges that
    k_cp_rows' workgroups leave behind and keep them for the whole launch.  A k_cp_rows wave with fewer allocated
    registers, or a k_cp_rows workgroup with less LDS, leaves holes k_cp_heavy cannot use: a quarter of its waves
    for the whole launch (4.9 -> 6.1 ms per tick in the crowded world).  The built code objects must keep the two
    matched -- whatever the compiler's register allocation did this time."""
    from permafrost_engine_amd import build as nb
    lib = os.environ.get("NAVHIP_LIB") or os.path.join(os.path.dirname(nb.__file__), "libnavhip.so")
    if not os.path.exists(lib):
        pytest.skip("libnavhip.so not built")
    ks = _device_kernels(lib, tmp_path)
    if ks is None:
        pytest.skip("ROCm LLVM tools not available")
    rows = [v for k, v in ks.items() if "k_cp_rows" in k]
    heavy = [v for k, v in ks.items() if "k_cp_heavy" in k]
    assert len(rows) == 1 and len(heavy) == 1, sorted(ks)[:8]
    alloc = lambda v: (v + 7) // 8 * 8                # (the hardware allocates registers in granules of 8 per lane)
    assert alloc(rows[0][0]) == alloc(heavy[0][0]) == 128, (rows, heavy)
    assert rows[0][1] >= heavy[0][1], (rows, heavy)
    assert 4 * rows[0][1] <= 160 * 1024 and 4 * heavy[0][1] <= 160 * 1024      # four workgroups per CU, by LDS


def test_profile_stamps_cover_the_files_they_list(tmp_path):
    """profiles/traffic.json and sq_counters.json are quoted by bench.py only for the kernel code they were
    measured on: the stamp lists the sources it covers.  A translation unit added later leaves it valid; a
    change to a covered file (or its removal) does not; comments and whitespace do not count."""
    import json
    import shutil
    sys.path.insert(0, ROOT)
    import bench
    csrc = os.path.join(ROOT, "permafrost-engine_amd", "csrc")
    for name in ("traffic.json", "sq_counters.json"):
        stamp = json.load(open(os.path.join(ROOT, "profiles", name)))
        assert stamp["files"] == sorted(stamp["files"]) and "agent_kernels.hip" in stamp["files"]
        # the sha is over the units that can change the measured kernels: every header, the units that define or
        # name one of them, the host units; a unit with other kernels only (the state pass) is not among them
        cov = stamp["covers"]
        assert set(cov) <= set(stamp["files"]) and "agent_kernels.hip" in cov and "agent_math.h" in cov
        assert cov == bench.stamp_units(stamp["files"], bench.stamp_kernels(stamp)) or not bench.stamp_is_current(stamp)
        if not bench.stamp_is_current(stamp):
            # not an error of the tree: bench.py then prints "traffic": null, "traffic_stale": true and no counters;
            # the next PMC session (scripts/gpu_job.sh pmc + summarize_prof.py) restamps
            import warnings
            warnings.warn(name + " was measured on other kernel code than this tree's: bench.py will not quote it")
    d = str(tmp_path / "csrc")
    os.makedirs(d)
    for f in bench.csrc_files(csrc):
        shutil.copy(os.path.join(csrc, f), d)
    files, sha = bench.csrc_files(d), bench.csrc_sha(d)
    assert sha == bench.csrc_sha(csrc)
    open(os.path.join(d, "later_unit.hip"), "w").write("__global__ void k_later() {}\n")
    assert bench.csrc_sha(d) != sha and bench.csrc_sha(d, files) == sha
    with open(os.path.join(d, "agent_math.h"), "a") as f:
        f.write("// a comment\n\n")
    assert bench.csrc_sha(d, files) == sha
    with open(os.path.join(d, "agent_math.h"), "a") as f:
        f.write("#define NH_SOMETHING_ELSE 1\n")
    assert bench.csrc_sha(d, files) != sha
    os.remove(os.path.join(d, "agent_math.h"))
    assert bench.csrc_sha(d, files).startswith("missing:")
    # a unit whose kernels were not measured and that names no measured kernel is outside a stamp's cover
    cov = bench.stamp_units(bench.csrc_files(csrc), ["k_agent_mid", "k_field_bfs"], csrc)
    assert "state_kernels.hip" not in cov and "agent_kernels.hip" in cov and "field_kernels.hip" in cov
    assert "tick_api.hip" in cov and "navhip_api.hip" in cov and all(f in cov for f in bench.csrc_files(csrc) if f.endswith(".h"))
    assert bench.stamp_units(bench.csrc_files(csrc), [], csrc) == bench.csrc_files(csrc)


def test_c_host_example_compiles_as_c99(tmp_path):
    """examples/c_host_tick.c -- the plain C host of navhip_tick_run -- against include/navhip.h and the HIP runtime's C
    API, as C99 with warnings as errors (not -pedantic: the HIP headers use unnamed unions; it RUNS in tests/test_c_host_gpu.py)."""
    import shutil
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if shutil.which("gcc") is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime_api.h")):
        pytest.skip("no gcc / HIP headers")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(rocm, "include"), "-c", os.path.join(ROOT, "examples", "c_host_tick.c"),
                        "-o", str(tmp_path / "c_host_tick.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_makefile_builds_what_build_py_builds():
    """csrc/Makefile (libnavhip.so for a C build system, no Python) lists the sources and the code-generation flags of
    permafrost_engine_amd/build.py: the arithmetic flags are part of the parity contract."""
    import re
    from permafrost_engine_amd import build as nb
    mk = open(os.path.join(os.path.dirname(nb.__file__), "csrc", "Makefile")).read().replace("\\\n", " ")
    srcs = re.search(r"^SOURCES\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert srcs == nb.SOURCES
    flags = re.search(r"^FLAGS\s*=\s*(.*)$", mk, re.M).group(1).split()
    want = [f for f in nb.FLAGS if not f.startswith("-I")]
    assert [f for f in flags if not f.startswith("-I")] == want


def test_staging_tables_cover_every_array_and_slots_are_named():
    """csrc/navhip_internal.h keeps ONE list of the arrays of navhip_world (nh_world_rows) and one of navhip_step_out
    (nh_out_rows) for every host-buffer path: each pointer member declared in include/navhip.h has exactly one row, and
    nothing in csrc/ indexes the context's staging slots by a bare number."""
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    csrc = os.path.join(ROOT, "permafrost-engine_amd", "csrc")
    internal = open(os.path.join(csrc, "navhip_internal.h")).read()
    for struct, macro in (("navhip_world", "NH_WROW"), ("navhip_step_out", "NH_OROW")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        members = re.findall(r"\*\s*(\w+)\s*;", body)
        assert len(members) == len(set(members)) and members
        rows = re.findall(r"\b%s\((\w+)," % macro, internal)
        rows = [r for r in rows if r != "member"]                      # (the macro's own definition)
        assert sorted(rows) == sorted(members), (struct, sorted(set(members) ^ set(rows)))
    slots = re.search(r"enum nh_stage_slot \{(.*?)\};", internal, re.S).group(1)
    slots = re.findall(r"\b(NH_STAGE_\w+)", re.sub(r"//[^\n]*", "", slots))
    assert len(slots) == len(set(slots)) and slots[-1] == "NH_STAGE_COUNT"
    row_slots = re.findall(r"\bNH_[WO]ROW\([^)]*?(NH_STAGE_\w+)", internal)
    assert len(row_slots) == len(set(row_slots)) == 27 + 5, "two arrays share a staging slot"
    assert not [s for s in row_slots if s.startswith("NH_STAGE_CALL")], "an array that outlives its call sits in call-local scratch"
    bare = re.compile(r"stage\[[0-9]|stage_reserve\([^,]*, *[0-9]|_SLOT +[0-9]")
    hits = []
    for f in sorted(os.listdir(csrc)):
        for i, line in enumerate(open(os.path.join(csrc, f), errors="replace"), 1):
            if bare.search(line):
                hits.append("%s:%d: %s" % (f, i, line.strip()))
    assert not hits, "staging slots indexed by number:\n" + "\n".join(hits)


# the members of navhip_ctx that were the agent step's state between calls before struct nh_step_state held them
OLD_STEP_STATE = ("aux", "aux_main", "ev_regroup", "snapshot_held", "join0_signalled", "lists_signalled", "start_flag", "start_seq",
                  "step_end_signalled", "step_end_on", "front_stream", "regroup_pending", "serial_step", "coh_flocks", "coh_members",
                  "coh_parity", "coh_unique", "coh_regroup_key", "coh_regroup_age", "scratch_moves", "wl_parity", "lists_pinned",
                  "sp_builds", "pre", "profiling", "ev", "ev_valid")


def test_step_host_code_is_one_unit_with_named_scratch_and_one_state_struct():
    """The host side of the agent step is csrc/step_api.hip, a unit without kernels; its scratch is ctx->step.buf[], one
    buffer per name of enum nh_step_buf, never indexed by a bare number; what the step keeps between calls is struct
    nh_step_state and nothing of it is left in navhip_ctx; navhip_state_update stages through the state unit's plan, and
    its eight staging slots are gone."""
    csrc = os.path.join(ROOT, "permafrost-engine_amd", "csrc")
    strip = lambda s: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))      # noqa: E731
    internal = strip(open(os.path.join(csrc, "navhip_internal.h")).read())
    # scratch arrays of the step, under their old names and the new one, indexed by a digit
    bare = re.compile(r"\b(?:sp|nbr|wl|arrived|buf)\[[0-9]")
    hits, sin = [], []
    for f in sorted(os.listdir(csrc)):
        for i, line in enumerate(open(os.path.join(csrc, f), errors="replace"), 1):
            if bare.search(line):
                hits.append("%s:%d: %s" % (f, i, line.strip()))
            if "NH_STAGE_SIN_" in line:
                sin.append("%s:%d" % (f, i))
    assert not hits, "step scratch indexed by number:\n" + "\n".join(hits)
    assert not sin, sin
    names = re.search(r"enum nh_step_buf \{(.*?)\};", internal, re.S).group(1)
    names = re.findall(r"\b(NH_SB_\w+)", names)
    assert len(names) == len(set(names)) == 19 and names[-1] == "NH_SB_COUNT"         # 10 hash + 3 walk + midrec + 2 lists + 2 cohesion
    step_src = open(os.path.join(csrc, "step_api.hip")).read()
    assert "__global__" not in step_src and "hipLaunchKernelGGL" not in step_src
    for moved in ("navhip_agent_prefetch_dev_ex", "navhip_agent_step_dev", "navhip_stream_wait_stage", "navhip_agent_step",
                  "navhip_spatial_query", "navhip_step_lists_peek"):
        assert re.search(r"^int %s\(" % moved, step_src, re.M), moved
        assert not re.search(r"^int %s\(" % moved, open(os.path.join(csrc, "navhip_api.hip")).read(), re.M), moved
    assert re.search(r"^int navhip_state_update\(", open(os.path.join(csrc, "state_kernels.hip")).read(), re.M)
    # every old member: declared inside struct nh_step_state, named nowhere else in the header (`ev` is also what struct
    # nh_handover calls its events: for that one name, nowhere else in navhip_ctx)
    m = re.search(r"struct nh_step_state \{(.*?)\n\};", internal, re.S)
    state, rest = m.group(1), internal[:m.start()] + internal[m.end():]
    ctx_body = re.search(r"struct navhip_ctx \{(.*?)\n\};", internal, re.S).group(1)
    assert re.search(r"\bnh_step_state\s+step\s*;", ctx_body)
    for name in OLD_STEP_STATE:
        assert re.search(r"\b%s\b" % name, state), name
        assert not re.search(r"\b%s\b" % name, ctx_body if name == "ev" else rest), name


def test_pool_and_submit_are_two_units_with_one_of_each_helper():
    """csrc/pool_api.hip is the resident field pool and nothing else; the asynchronous host-buffer step, the page-locked
    memory helpers and the one place that asks the runtime about a pointer are csrc/submit_api.hip, a unit without
    kernels; navhip_build_fields stages in the call-local slots, so navhip_ctx keeps no scratch of its own for it."""
    csrc = os.path.join(ROOT, "permafrost-engine_amd", "csrc")
    submit = open(os.path.join(csrc, "submit_api.hip")).read()
    pool = open(os.path.join(csrc, "pool_api.hip")).read()
    for entry in ("int navhip_agent_step_submit", "int navhip_agent_step_poll", "int navhip_agent_step_wait", "void *navhip_host_alloc"):
        assert re.search(r"^%s\(" % re.escape(entry), submit, re.M), entry
    assert "__global__" not in submit and "hipLaunchKernelGGL" not in submit
    for gone in ("nh_async", "hipHostMalloc", "POOL_FAIL", "POOL_HIPCHK", "fresh_slots", "<< 12"):
        assert gone not in pool, gone
    asks = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))
            for _ in re.findall("hipPointerGetAttributes", open(os.path.join(csrc, f)).read())]
    assert asks == ["submit_api.hip"], asks
    strip = lambda s: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))      # noqa: E731
    internal = strip(open(os.path.join(csrc, "navhip_internal.h")).read())
    ctx_body = re.search(r"struct navhip_ctx \{(.*?)\n\};", internal, re.S).group(1)
    each_buf = re.search(r"nh_ctx_each_buf\(navhip_ctx \*ctx, F f\)\s*\{(.*?)\n\}", internal, re.S).group(1)
    for name in ("d_reqs", "d_dirs", "d_integ"):
        assert not re.search(r"\b%s\b" % name, ctx_body) and not re.search(r"\b%s\b" % name, each_buf), name


def test_map_unit_holds_map_state_only_with_one_plane_table_and_one_staging_path():
    """csrc/navhip_api.hip is the context, the planes with their derived masks, the blockers and the field builds: the
    stream fronts live in stream_set.hip, the host-pointer utilities over the agent kernels in step_api.hip, and the unit
    includes no agent header and opens extern "C" once; the planes are described by a table (no switch over the plane
    number), guarded by a static_assert on NAVHIP_PLANE_COUNT; the four staging helpers are defined side by side."""
    csrc = os.path.join(ROOT, "permafrost-engine_amd", "csrc")
    units = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}
    api = units["navhip_api.hip"]
    assert "agent_internal.h" not in api and "agent_thread.h" not in api
    assert len(re.findall(r'extern\s+"C"\s*\{', api)) == 1
    assert not re.search(r"switch\s*\(\s*plane\s*\)", api)
    assert re.search(r"static_assert\([^;]*plane_rows[^;]*NAVHIP_PLANE_COUNT", api, re.S)
    moved = {"navhip_stream_beside": "stream_set.hip", "navhip_stream_main": "stream_set.hip",
             "navhip_stream_create_partial": "stream_set.hip", "navhip_region_lookup": "step_api.hip",
             "navhip_clearpath": "step_api.hip", "navhip_clearpath_rows": "step_api.hip", "navhip_clearpath_team": "step_api.hip",
             "clearpath_batch": "step_api.hip"}
    for name, unit in moved.items():
        homes = [f for f, src in units.items() if re.search(r"^(?:static )?int %s\(" % name, src, re.M)]
        assert homes == [unit], (name, homes)
    helpers = ("nh_ensure", "nh_ensure_buf", "nh_stage_reserve", "nh_stage_in")
    homes = {h: [f for f, src in units.items() if re.search(r"^int %s\(" % h, src, re.M)] for h in helpers}
    assert all(len(v) == 1 for v in homes.values()) and len(set(v[0] for v in homes.values())) == 1, homes
    for entry in ("navhip_upload_plane", "navhip_upload_chunk", "navhip_download_plane", "navhip_build_fields",
                  "navhip_build_los", "navhip_build_region_fields", "navhip_blockers_circles"):
        assert re.search(r"^int %s\(" % entry, api, re.M), entry


def test_agent_kernel_units_hold_their_own_kernels_and_one_unit_includes_the_group_header():
    """The agent step's kernels live in four units: the build side of the spatial hash (spatial_kernels.hip), the cohesion
    term (cohesion_kernels.hip), the arrival arm of the state pass (state_kernels.hip) and the step proper
    (agent_kernels.hip).  agent_group.h defines a device variable and is included by one unit only; the state unit's
    launcher is its own; the two scan kernels are reached from outside through nh_launch_scan, never by name."""
    csrc = os.path.join(ROOT, "permafrost-engine_amd", "csrc")
    units = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}
    headers = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".h")}
    home = {"spatial_kernels.hip": ("k_sp_bbox", "k_sp_count", "k_sp_scan_local", "k_sp_scan_add", "k_sp_scatter", "k_sp_place",
                                    "k_sp_build_small"),
            "cohesion_kernels.hip": ("k_coh_plan", "k_coh_bin", "k_coh_scatter", "k_cohesion", "k_zero_i32"),
            "state_kernels.hip": ("k_arrived_compact", "k_state_update")}
    for unit, kernels in home.items():
        for k in kernels:
            # (from __global__ to the kernel's name: attributes and the return type, no body or statement in between)
            defined = [f for f, src in units.items() if re.search(r"__global__[^;{}]*?\b%s\s*\(" % k, src)]
            assert defined == [unit], (k, defined)
    including = [f for f, src in units.items() if re.search(r'#include\s+"agent_group\.h"', src)]
    assert including == ["agent_kernels.hip"], including
    assert not [f for f, src in headers.items() if "nh_launch_state_update" in src]
    assert re.search(r"^static void nh_launch_state_update\(", units["state_kernels.hip"], re.M)
    for k in ("k_sp_scan_local", "k_sp_scan_add"):
        named = [f for f, src in {**units, **headers}.items() if k in src]
        assert named == ["spatial_kernels.hip"], (k, named)


def test_state_staging_tables_cover_every_array():
    """The units whose host-buffer forms stage whole structs (csrc/state_kernels.hip, arrival_flock_kernels.hip,
    arrival_build_kernels.hip) do so from ONE list per struct on the plan of csrc/stage_plan.h (sk_gate_rows,
    sk_state_rows, sk_aux_rows, sk_pass_out_rows, sk_settle_in_rows, sk_settle_out_rows, av_*_rows, af_*_rows,
    ab_*_rows): each pointer member declared in include/navhip.h has exactly one row in the list of its struct, with the
    element size of its declared type, and each list is guarded by a static_assert on the size of its struct."""
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    csrc = os.path.join(ROOT, "permafrost-engine_amd", "csrc")
    plan = open(os.path.join(csrc, "stage_plan.h")).read()
    assert re.search(r"#define NH_COVERS\(tab, T, scalar_bytes\) \\\n\s*static_assert\(sizeof\(T\) == ", plan)
    width = {"float": 4, "int32_t": 4, "uint32_t": 4, "int16_t": 2, "uint8_t": 1, "uint64_t": 8}
    units = {"state_kernels.hip": ("navhip_gate_in", "navhip_state_in", "navhip_state_aux_in", "navhip_state_pass_out",
                                   "navhip_settle_in", "navhip_settle_out", "navhip_arrival_vel_in", "navhip_arrival_vel_out"),
             "arrival_flock_kernels.hip": ("navhip_arrival_flock_in", "navhip_arrival_flock_out"),
             "arrival_build_kernels.hip": ("navhip_arrival_build_in", "navhip_arrival_build_out")}
    for unit, structs in units.items():
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "stage_plan.h"' in src and "struct nh_plan" not in src, unit
        rows = re.findall(r"\bNH_ROW(?:_PAD|_OUT|_OUT_PAD|_OUT_RANGE|_IO)?\((navhip_\w+),\s*(\w+),\s*([\w() ]+?),\s*(?:NH_LEN|SK_PER)_\w+,\s*(?:NH_ON|SK)_\w+", src)
        assert sorted(set(s for s, _, _ in rows)) == sorted(structs), unit
        for struct in structs:
            body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
            members = {}
            for decl in re.findall(r"(?:const\s+)?(\w+)\s*(\*[^;]*);", body):
                for name in re.findall(r"\*\s*(\w+)", decl[1]):
                    members[name] = decl[0]
            assert members
            mine = [(m, e) for s, m, e in rows if s == struct]
            assert sorted(m for m, _ in mine) == sorted(members), (struct, sorted(set(members) ^ set(m for m, _ in mine)))
            for m, e in mine:
                if members[m] in width:            # a row's element is a whole number of the declared type: [n][2] floats = 8
                    assert int(e) % width[members[m]] == 0, (struct, m, e)
                else:
                    assert e == "sizeof(%s)" % members[m], (struct, m, e)
        tables = re.findall(r"^const nh_row (\w+_rows)\[\]", src, re.M)
        guards = re.findall(r"^NH_COVERS\((\w+_rows), (navhip_\w+),", src, re.M)
        assert len(tables) == len(structs) and sorted(tables) == sorted(t for t, _ in guards), unit
        assert sorted(s for _, s in guards) == sorted(structs), unit
