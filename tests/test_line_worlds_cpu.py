"""The worlds of tests/line_worlds.py WITHOUT a GPU: their premises -- the agents really stand on tile lines, centres, seams and
watersheds, counted with a numpy model of M_Tile_DescForPoint2D / n_interpolated_flow_dir --, and the restatement oracle's
agent step against move_velocity_work of the reference build on them.  tests/test_line_worlds_gpu.py steps the same worlds
on the device."""
import numpy as np
import pytest

from oracle import pfref
from tests import dispatch_worlds as dw
from tests import line_worlds as lw

pytestmark = pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")

FLOORS = {"dx_zero": 20, "dz_zero": 20, "weight_half": 20, "taps_cancel": 20, "tap_in_other_chunk": 20,
          "tap_in_chunk_without_slot": 5, "probe_in_other_chunk": 20}
ST_FIELD = 0x06                     # NAVHIP_ST_FIELD_MISS | NAVHIP_ST_FIELD_NONE


def with_host_fallbacks(L, status):
    """The world's arrays with vdes_xz as the host completes it: NaN (the step samples) but for the agents the step reported
    as without a field or on FD_NONE -- theirs from the reference's own fallbacks (nav.c:3483-3554), which the step leaves to
    the host (navhip_collect_misses)."""
    vdes = np.full((L.n, 2), np.nan, np.float32)
    flagged = (status & ST_FIELD) != 0
    vdes[flagged] = L.ref_vdes[flagged]
    return dict(L.arrays, vdes_xz=vdes)


def clean(L, status):
    """Point-seek agents with a field under them that is not FD_NONE there."""
    return L.point_seek() & ((status & ST_FIELD) == 0)


def test_tile_model_on_lines_seams_and_the_rim():
    """The numpy model itself: x == base of a tile and of a chunk belong to the tile / chunk that starts there, the map's
    own boundary coordinates are on the map (tile 64 clamped to 63), one step beyond is not."""
    x = np.array([512.0, 508.0, 256.0, 255.99998, 0.0, -512.0, -512.0001, 512.0001], np.float32)
    on, cr, cc, tr, tc = lw.tile_of(4, 4, x, np.full(len(x), -512.0, np.float32))
    assert on.tolist() == [True] * 6 + [False, False]
    assert cc[:6].tolist() == [0, 0, 1, 1, 2, 3] and tc[:6].tolist() == [0, 1, 0, 0, 0, 63] and (tr[:6] == 0).all()
    on, cr, cc, tr, tc = lw.tile_of(4, 4, np.zeros(3, np.float32), np.array([512.0, 256.0, 252.0], np.float32))
    assert on.all() and cr.tolist() == [3, 3, 2] and tr.tolist() == [63, 0, 63]


def test_lines_world_premises():
    L = lw.lines()
    p = lw.premises(L)
    print("lines premises:", p, "planted on watersheds:", L.planted)
    for k, floor in FLOORS.items():
        assert p[k] >= floor, (k, p)
    pos = L.world["pos_xz"].astype(np.float64)
    k = L.kind
    # the kinds are where the table says (the agents moved onto watersheds keep their kind's line)
    assert (np.mod(pos[k == 1], 4.0) == 0).all() and (np.mod(pos[k == 2][:, 0], 4.0) == 0).all() and (np.mod(pos[k == 3][:, 1], 4.0) == 0).all()
    assert (np.mod(pos[k == 4], 4.0) == 2).all() and (np.mod(pos[k == 5][:, 0], 4.0) == 2).all()
    assert (np.mod(pos[k == 6], 256.0) == 0).all() and (np.mod(pos[k == 7][:, 0], 256.0) == 0).all()
    assert (np.abs(pos) <= 4 * 128.0 - 12.0).all()
    # many agents coincide on the chunk corners
    _, counts = np.unique(pos[k == 6], axis=0, return_counts=True)
    assert len(counts) == 9 and counts.max() >= 10
    vel = L.world["vel_xz"].astype(np.float64)
    assert (np.mod(vel[::3] * 2, 1.0) == 0).all() and (np.abs(vel[::3]).max(1) > 0).sum() > 100


def test_formation_world_premises():
    L = lw.formation()
    p = lw.premises(L)
    print("formation premises:", p)
    assert p["dx_zero"] >= 20 and p["dz_zero"] >= 20 and p["weight_half"] >= 20, p
    hist = dw.list_histogram(L.count, L.searching, L.irregular)
    print("formation lists:", hist)
    assert all(h >= 10 for h in hist[:5]) and hist[5] == 0, hist
    # blocks of 5 x 5, 7 x 7 and 9 x 9 are there: 24 neighbours in the middle of the first, both caps' sum in the last
    sizes = np.bincount(L.world["flock"])
    assert {25, 49, 81} <= set(sizes.tolist()) and L.count.max() >= 32 and (L.count == 24).any()


@pytest.mark.parametrize("name", ["lines", "formation"])
def test_restatement_step_equals_reference(name):
    """navoracle's agent_step on the world, sampling the reference's cached fields itself: vdes and vel of every clean
    point-seek agent are the reference's bit for bit, each kind with 60 and more of them; with the host's fallbacks filled
    in for the agents it reports, vel is the reference's for EVERY moving agent."""
    from tests import cases
    L = getattr(lw, name)()
    out = L.oracle()
    ok = clean(L, out["status"])
    per_kind = np.bincount(L.kind[ok], minlength=lw.KINDS)
    print(name, "clean per kind:", per_kind.tolist())
    assert (per_kind[:lw.KINDS if name == "lines" else 1] >= 60).all(), per_kind
    for key, ref in (("vdes_xz", L.ref_vdes), ("vel_xz", L.ref_vel)):
        bad = np.flatnonzero(ok & (out[key].view(np.uint32) != ref.view(np.uint32)).any(1))
        assert len(bad) == 0, (key, len(bad), bad[:8], L.kind[bad[:8]], out[key][bad[:3]], ref[bad[:3]])
    full = cases.oracle_nav_from_ref(L.nav).agent_step(with_host_fallbacks(L, out["status"]))
    mv = L.moving()
    assert mv.sum() > L.n // 2
    bad = np.flatnonzero(mv & (full["vel_xz"].view(np.uint32) != L.ref_vel.view(np.uint32)).any(1))
    assert len(bad) == 0, (len(bad), bad[:8], L.kind[bad[:8]], full["vel_xz"][bad[:3]], L.ref_vel[bad[:3]])
    assert np.all(full["vel_xz"][~mv] == 0)
