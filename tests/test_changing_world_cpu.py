"""The script of changing worlds (tests/changing_world.py) on the host: every tick's snapshot is well-formed, the
script does what the GPU test relies on, and -- where oracle/_ref is built -- the C restatement that the GPU test
compares with matches the reference's own move_velocity_work in the unusual states the script creates."""
import os

import numpy as np
import pytest

from oracle import navoracle, pfref
from permafrost_engine_amd import synth
from tests import cases
from tests import changing_world as cw

needs_ref = pytest.mark.skipif(not (pfref.available() or os.path.isdir("/root/reference")),
                               reason="oracle/_ref not built and /root/reference absent")


@pytest.fixture(scope="module")
def ticks():
    return cw.script()


def test_script_ticks_are_well_formed(ticks):
    half = cw.W * 128.0
    for tk in ticks:
        n, k = tk.n, tk.n_flocks
        offs, mem = tk.flock_offsets, tk.flock_members
        assert offs[0] == 0 and offs[-1] == len(mem) and (np.diff(offs) >= 0).all(), tk.t
        assert ((mem >= 0) & (mem < n)).all(), tk.t
        assert len(np.unique(mem)) == len(mem), tk.t                      # a uid in at most one flock
        assert len(mem) == n and (tk.flock >= 0).all()                      # ... and here in exactly one
        for f in range(k):
            assert (tk.flock[mem[offs[f]:offs[f + 1]]] == f).all(), (tk.t, f)
        assert tk.flock_target_xz.shape == (k, 2)
        assert (np.abs(tk.flock_target_xz) < half).all(), tk.t
        for name in cw.ENTITY_ARRAYS:
            assert len(tk.ent[name]) == n, (tk.t, name)
        assert tk.spawn_pos.shape == (n - tk.n_carry, 2) == tk.spawn_vel.shape
        assert (np.abs(tk.spawn_pos) < half).all()
        assert tk.hz in (10, 20)
        if tk.form is not None:
            assert all(len(tk.form[name]) == n for name in cw.FORM_ARRAYS)
        else:
            assert not np.isin(tk.ent["state"], (cw.MOVING_IN_FORMATION, cw.ARRIVING_TO_CELL)).any(), tk.t


def test_script_covers_the_changes(ticks):
    """What the GPU test relies on the script for: each change happens, at least once."""
    k = [tk.n_flocks for tk in ticks]
    n = [tk.n for tk in ticks]
    above = [i for i, x in enumerate(k) if x > 64]
    assert above and k[0] <= 64 and any(x <= 64 for x in k[above[-1]:]), k     # 64 flocks crossed both ways
    assert max(n) >= 2 * n[0] and n[-1] < max(n), n                           # spawns past x2, deaths
    assert any(np.diff(tk.flock_offsets).min() == 0 for tk in ticks)           # an empty flock
    hz = [tk.hz for tk in ticks]
    assert hz[0] == 20 and 10 in hz and hz[-1] == 20
    assert any(tk.form is not None for tk in ticks) and ticks[-1].form is None
    # flock sizes change at equal n_flocks and n_ents; two units swap flocks at equal offsets
    same_counts = [(a, b) for a, b in zip(ticks, ticks[1:]) if (a.n, a.n_flocks) == (b.n, b.n_flocks)]
    assert any(not np.array_equal(a.flock_offsets, b.flock_offsets) for a, b in same_counts)
    assert any(np.array_equal(a.flock_offsets, b.flock_offsets) and not np.array_equal(a.flock_members, b.flock_members)
               for a, b in same_counts)
    flags = [tk.ent["flags"] for tk in ticks]
    assert any(((f & cw.FLAG_COMBAT_HELD) != 0).any() for f in flags)
    assert any(((f & cw.FLAG_GARRISONED) != 0).any() for f in flags)
    assert any((tk.ent["state"] == cw.ARRIVED).mean() > 0.15 for tk in ticks)


def _trajectory(ticks, onav, upto):
    """Positions / velocities of ticks 0..upto as the restatement steps them."""
    pos = vel = np.zeros((0, 2), np.float32)
    out = {}
    for tk in ticks[:upto + 1]:
        pos, vel = tk.start_rows(pos, vel)
        out[tk.t] = (pos, vel)
        o = onav.agent_step(tk.arrays(pos, vel), hz=tk.hz, nthreads=4)
        pos, vel = o["new_pos_xz"], o["vel_xz"]
    return out


@needs_ref
def test_restatement_matches_reference_on_script_ticks(ticks):
    """The restatement against the reference's move_velocity_work on the ticks with an empty flock and hz 10 (5),
    70 flocks with a mix of ARRIVED / COMBAT_HELD / GARRISONED units (7), 72 flocks with the formation arm (9), and
    hz 10 again after spawns and deaths (14); the flock member order is the reference's own."""
    grid, nav = cases.ref_nav_for(cw.W, cw.W, seed=21)
    assert np.array_equal(grid, cw.grid())
    onav = cases.oracle_nav_from_ref(nav)
    picked = (5, 7, 9, 14)
    traj = _trajectory(ticks, onav, max(picked))
    half = cw.W * 128.0
    for t in picked:
        tk = ticks[t]
        pos, vel = traj[t]
        world = {"pos_xz": pos, "vel_xz": vel, "flock": tk.flock, "flock_target_xz": tk.flock_target_xz}
        world.update({name: tk.ent[name] for name in cw.ENTITY_ARRAYS})
        mv, _ = cases.ref_move_for(nav, world, hz=tk.hz)
        try:
            if tk.form is not None:
                f = tk.form
                mv.set_formation(f["form_ready"], f["cell_pos_xz"], f["form_cohesion_xz"], f["form_align_xz"],
                                 f["form_drag_xz"])
            vdes = tk.ent["vdes_xz"]
            exp_vel = mv.velocity(vdes)
            order = [mv.flock_order(f) for f in range(tk.n_flocks)]
        finally:
            pfref.RefMove.unload()
        arrays = cases.step_arrays(world, vdes, order)
        if tk.form is not None:
            arrays.update(tk.form)
        out = onav.agent_step(arrays, hz=tk.hz, nthreads=4)
        # still units and the map edge left out, as in the other pins (tests/test_fullsize_ref_gpu.py::_check_agents:
        # for an off-map probe the reference reads an uninitialised tile_desc)
        moving = ~np.isin(tk.ent["state"], (cw.ARRIVED, 4))
        edge = (np.abs(pos[:, 0]) > half - 4.0) | (np.abs(pos[:, 1]) > half - 4.0)
        assert edge.sum() < 0.01 * tk.n + 20, edge.sum()
        rows = moving & ~edge
        assert rows.sum() > tk.n // 2
        bad = np.flatnonzero((out["vel_xz"].view(np.uint32) != exp_vel.view(np.uint32)).any(1) & rows)
        assert len(bad) == 0, (t, tk.events, len(bad), bad[:5])
