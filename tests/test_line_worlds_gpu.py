"""The agent step of the gfx950 build where units really stand (tests/line_worlds.py): on tile lines, tile corners and exact
tile centres, on chunk seams and chunk corners (where many coincide), on watersheds of the flow field, in formations on a
3-wu lattice -- the arms of csrc/agent_math.h (tile_for_point at x == base, sample_flow with dx == 0, with wc == 0.5 and
cancelling taps, taps and probes across seams, into chunks without a field, the position accept on a line) and of
csrc/agent_group.h (ties, coincident neighbours, a separation sum of zero) that no position of the form tile centre +
uniform(-1.5, 1.5) reaches.  tests/test_line_worlds_cpu.py asserts that the worlds reach them.

No tolerance anywhere: every output of EVERY agent equals the restatement oracle's bit for bit; vdes and vel of the clean
point-seek agents (a field under them, not FD_NONE) equal N_DesiredPointSeekVelocity / move_velocity_work of the reference
build bit for bit, 60 and more of every kind; with the host's fallbacks filled in, vel of every moving agent does."""
import numpy as np
import pytest

from oracle import pfref
from tests import dispatch_worlds as dw
from tests import line_worlds as lw
from tests.test_line_worlds_cpu import clean, with_host_fallbacks

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]

OUTPUTS = ("vel_xz", "new_pos_xz", "vdes_xz", "vpref_xz", "status")


def _upload(navlib, nav):
    ctx = navlib.NavContext(nav.w, nav.h)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, nav.plane(0))
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, nav.plane(1))
    ctx.upload_plane(0, navlib.PLANE_LOCAL_ISLANDS, nav.plane(3))
    return ctx


def _check_world(navlib, L):
    ctx = _upload(navlib, L.nav)
    out = ctx.agent_step(L.arrays)
    lists = ctx.last_step_lists()
    full = ctx.agent_step(with_host_fallbacks(L, out["status"]))
    ctx.close()
    # ---- against the restatement: every output of every agent
    exp = L.oracle()
    for key in OUTPUTS:
        g, x = out[key].view(np.uint8).reshape(L.n, -1), exp[key].view(np.uint8).reshape(L.n, -1)
        bad = np.flatnonzero((g != x).any(1))
        assert len(bad) == 0, (L.name, key, len(bad), bad[:8], L.kind[bad[:8]], out[key][bad[:4]], exp[key][bad[:4]])
    assert np.abs(out["vel_xz"]).max() > 0
    # ---- against the reference: the clean point-seek agents, every kind
    ok = clean(L, out["status"])
    per_kind = np.bincount(L.kind[ok], minlength=lw.KINDS)
    print(L.name, "clean per kind:", per_kind.tolist())
    assert (per_kind[:lw.KINDS if L.name == "lines" else 1] >= 60).all(), per_kind
    for key, ref in (("vdes_xz", L.ref_vdes), ("vel_xz", L.ref_vel)):
        bad = np.flatnonzero(ok & (out[key].view(np.uint32) != ref.view(np.uint32)).any(1))
        assert len(bad) == 0, (L.name, key, len(bad), bad[:8], L.kind[bad[:8]], out[key][bad[:4]], ref[bad[:4]])
    # ... and, the fallbacks of the reported agents supplied by the host, every moving agent
    mv = L.moving()
    bad = np.flatnonzero(mv & (full["vel_xz"].view(np.uint32) != L.ref_vel.view(np.uint32)).any(1))
    assert len(bad) == 0, (L.name, "all moving", len(bad), bad[:8], L.kind[bad[:8]], full["vel_xz"][bad[:4]], L.ref_vel[bad[:4]])
    assert np.all(full["vel_xz"][~mv] == 0)
    return out, lists


def test_lines_world(navlib):
    L = lw.lines()
    out, _ = _check_world(navlib, L)
    # the MOVED bit == the reference's position tests at pos + vel, for every computed agent that stands on a line
    pos, nav = L.world["pos_xz"], L.nav
    on_line = L.moving() & np.isin(L.kind, (1, 2, 3, 6, 7))
    assert on_line.sum() > 700
    landed = 0
    for uid in np.flatnonzero(on_line):
        v = out["vel_xz"][uid]
        npos = pos[uid] + v
        assert np.array_equal(npos, out["new_pos_xz"][uid]) or not (out["status"][uid] & navlib.ST_MOVED)
        acc = bool(np.linalg.norm(v) > 0) and nav.position_pathable(npos) and (nav.position_blocked(pos[uid]) or not nav.position_blocked(npos))
        assert bool(out["status"][uid] & navlib.ST_MOVED) == acc, (uid, L.kind[uid], pos[uid], v)
        landed += bool(np.mod(float(npos[0]), 4.0) == 0 or np.mod(float(npos[1]), 4.0) == 0)
    print("lines: agents whose pos + vel is on a tile line again:", landed)


def test_formation_world(navlib):
    L = lw.formation()
    out, lists = _check_world(navlib, L)
    assert list(lists) == dw.list_histogram(L.count, L.searching, L.irregular), lists
