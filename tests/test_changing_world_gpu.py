"""The agent step tick by tick on a world that changes between ticks (tests/changing_world.py), in every schedule
the engine and the tick drive it with.  The step carries state from tick to tick on one context -- the cohesion
lane grouping, the prefetch key, scratch buffers grown on demand, the work-list and slab-box parities, the
hand-over sequence numbers -- and none of it may show in a result.  Every tick of every schedule is compared,
bit for bit, with
  * the C restatement (oracle/navoracle.c) on the exact inputs the device saw that tick, and
  * a context created for that tick alone and stepped once on the same inputs (no carried state at all)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from oracle import navoracle
from permafrost_engine_amd import synth
from tests import changing_world as cw

pytestmark = pytest.mark.gpu

OUTS = ("vel_xz", "new_pos_xz", "vdes_xz", "status")
SCHEDULES = ("blocking", "device", "prefetch", "follows", "follows_events", "abandoned", "slab_epoch", "slab_no_epoch")


@pytest.fixture(scope="module")
def env():
    g = cw.grid()
    planes = (synth.to_chunks(g), np.zeros((cw.W, cw.W, 64, 64), np.uint16), synth.to_chunks(synth.local_islands(g)))
    return {"planes": planes, "ticks": cw.script(), "onav": navoracle.OracleNav(*planes), "expected": {}}


def _context(navlib, env):
    ctx = navlib.NavContext(cw.W, cw.W)
    for plane, arr in zip((navlib.PLANE_COST_BASE, navlib.PLANE_BLOCKERS, navlib.PLANE_LOCAL_ISLANDS), env["planes"]):
        ctx.upload_plane(0, plane, arr)
    return ctx


def _host_step(navlib, ctx, arrays, hz, work=None):
    """navhip_agent_step (host buffers) with every output, on the uid slab `work` (None: all)."""
    w, keep = navlib.make_world(cw.W, cw.W, arrays, hz)
    if work is not None:
        w.work_begin, w.work_end = work
    n = w.n_ents
    out = {k: np.zeros((n, 2), np.float32) for k in ("vel_xz", "new_pos_xz", "vdes_xz")}
    out["status"] = np.zeros(n, np.uint8)
    so = navlib.StepOut()
    so.vel_xz, so.new_pos_xz = out["vel_xz"].ctypes.data, out["new_pos_xz"].ctypes.data
    so.vdes_xz, so.status = out["vdes_xz"].ctypes.data, out["status"].ctypes.data
    ctx._chk(navlib.lib().navhip_agent_step(ctx._h, C.byref(w), C.byref(so)), "navhip_agent_step")
    return out


def _expected(navlib, env, tick, pos, vel, work=None):
    """(restatement, cold context) for these inputs -- computed once: every schedule that is right sees the same."""
    key = (tick.t, work, hashlib.sha1(pos.tobytes() + vel.tobytes()).hexdigest())
    if key not in env["expected"]:
        a = tick.arrays(pos, vel)
        exp = env["onav"].agent_step(a, hz=tick.hz, work=work, nthreads=8)
        cold = _context(navlib, env)
        got = _host_step(navlib, cold, a, tick.hz, work)
        cold.close()
        env["expected"][key] = (exp, got)
    return env["expected"][key]


def _bits_equal(got, exp):
    if got.dtype == np.uint8:
        return got == exp
    same = got.view(np.uint32) == exp.view(np.uint32)
    return (same | (np.isnan(got) & np.isnan(exp))).all(axis=-1)


def _check(navlib, env, tick, pos, vel, out, schedule, work=None):
    rows = slice(None) if work is None else slice(*work)
    exp, cold = _expected(navlib, env, tick, pos, vel, work)
    for ref, name in ((exp, "restatement"), (cold, "cold context")):
        for k in OUTS:
            ok = _bits_equal(out[k][rows], ref[k][rows])
            assert ok.all(), "%s, tick %d %s (work %s): %s differs from the %s in %d rows, first %s" % (
                schedule, tick.t, tick.events, work, k, name, int((~ok).sum()), np.flatnonzero(~ok)[:6])


# ---------------------------------------------------------------------------------------------
# device buffers of one snapshot
# ---------------------------------------------------------------------------------------------
class _DevSet:
    """Device copies of every snapshot array but positions and velocities, at the script's largest size."""

    def __init__(self, ticks, torch):
        self.torch = torch
        nmax, fmax = max(t.n for t in ticks), max(t.n_flocks for t in ticks)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")     # noqa: E731
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        self.t = {"radius": z(nmax, f32), "max_speed": z(nmax, f32), "speed": z(nmax, f32),
                  "flags": z(nmax, i32), "state": z(nmax, u8), "has_dest_los": z(nmax, u8),
                  "vdes_xz": z((nmax, 2), f32), "flock": z(nmax, i32), "flock_target_xz": z((fmax, 2), f32),
                  "flock_offsets": z(fmax + 1, i32), "flock_members": z(nmax, i32),
                  "form_ready": z(nmax, u8), "cell_pos_xz": z((nmax, 2), f32), "form_cohesion_xz": z((nmax, 2), f32),
                  "form_align_xz": z((nmax, 2), f32), "form_drag_xz": z((nmax, 2), f32)}

    def load(self, tick, keep=None):
        """Copy the tables of `tick` in.  keep=None: synchronous copies; else non-blocking copies from pinned
        host memory on the current stream, the host buffers appended to `keep`."""
        a = tick.arrays(np.zeros((tick.n, 2), np.float32), np.zeros((tick.n, 2), np.float32))
        for k, dst in self.t.items():
            if a.get(k) is None:
                continue
            src = self.torch.from_numpy(np.ascontiguousarray(a[k]).view(_view_dtype(a[k])))
            if keep is None:
                dst[:len(src)].copy_(src)
            else:
                src = src.pin_memory()
                keep.append(src)
                dst[:len(src)].copy_(src, non_blocking=True)

    def world(self, navlib, tick, pos, vel, work=None, epoch=0):
        n, k = tick.n, tick.n_flocks
        a = {name: t[:n] for name, t in self.t.items()}
        a["flock_target_xz"], a["flock_offsets"] = self.t["flock_target_xz"][:k], self.t["flock_offsets"][:k + 1]
        a["flock_members"] = self.t["flock_members"][:int(tick.flock_offsets[-1])]
        if tick.form is None:
            for name in cw.FORM_ARRAYS:
                a[name] = None
        a["pos_xz"], a["vel_xz"] = pos[:n], vel[:n]
        a["static_epoch"] = epoch
        w, keep = navlib.make_world(cw.W, cw.W, a, hz=tick.hz)
        if work is not None:
            w.work_begin, w.work_end = work
        return w, keep


def _view_dtype(a):
    return np.int32 if a.dtype == np.uint32 else a.dtype


def _step_out(navlib, vel, pos, vdes, status):
    so = navlib.StepOut()
    so.vel_xz, so.new_pos_xz, so.vdes_xz, so.status = vel.data_ptr(), pos.data_ptr(), vdes.data_ptr(), status.data_ptr()
    return so


def _outputs(torch, nmax):
    return {"vel_xz": torch.zeros((nmax, 2), device="cuda"), "new_pos_xz": torch.zeros((nmax, 2), device="cuda"),
            "vdes_xz": torch.zeros((nmax, 2), device="cuda"), "status": torch.zeros(nmax, dtype=torch.uint8, device="cuda")}


def _host(t, n):
    return t[:n].cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------
# the schedules: each returns [(tick, pos, vel, outputs, work)] per stepped call, and the (n_flocks, n_ents) the
# device was handed per tick
# ---------------------------------------------------------------------------------------------
def _run_blocking(navlib, env):
    ctx = _context(navlib, env)
    res, seen = [], []
    pos = vel = np.zeros((0, 2), np.float32)
    for tick in env["ticks"]:
        pos, vel = tick.start_rows(pos, vel)
        w, _ = navlib.make_world(cw.W, cw.W, tick.arrays(pos, vel), tick.hz)
        seen.append((w.n_flocks, w.n_ents))
        out = _host_step(navlib, ctx, tick.arrays(pos, vel), tick.hz)
        res.append((tick, pos, vel, out, None))
        pos, vel = out["new_pos_xz"], out["vel_xz"]
    ctx.close()
    return res, seen


def _run_synced(navlib, env, prefetch, abandon=False):
    """Device-resident step on the context's stream, the host synchronising after every tick and changing the
    snapshot arrays in place.  prefetch: agent_prefetch_dev (flags 0: the front on the side streams) first.
    abandon: the snapshots alternate between two buffer sets, and every third tick prefetches the LAST tick's
    snapshot (still intact in the other set) before it steps its own."""
    import torch
    ticks = env["ticks"]
    nmax = max(t.n for t in ticks)
    ctx = _context(navlib, env)
    s = ctx.stream
    sets = [_DevSet(ticks, torch) for _ in range(2 if abandon else 1)]
    pv = [(torch.zeros((nmax, 2), device="cuda"), torch.zeros((nmax, 2), device="cuda")) for _ in sets]
    o = _outputs(torch, nmax)
    so = _step_out(navlib, o["vel_xz"], o["new_pos_xz"], o["vdes_xz"], o["status"])
    res, seen, prev_world = [], [], None
    pos = vel = np.zeros((0, 2), np.float32)
    for tick in ticks:
        pos, vel = tick.start_rows(pos, vel)
        i = tick.t % len(sets)
        sets[i].load(tick)
        pv[i][0][:tick.n].copy_(torch.from_numpy(pos))
        pv[i][1][:tick.n].copy_(torch.from_numpy(vel))
        torch.cuda.synchronize()
        w, keep = sets[i].world(navlib, tick, pv[i][0], pv[i][1])
        seen.append((w.n_flocks, w.n_ents))
        if abandon and prev_world is not None and tick.t % 3 == 2:
            ctx.agent_prefetch_dev(prev_world[0], stream=s)            # never stepped: drained by the step below
        elif prefetch:
            ctx.agent_prefetch_dev(w, stream=s)
        ctx.agent_step_dev(w, so, stream=s)
        ctx.sync()
        torch.cuda.synchronize()
        out = {k: _host(v, tick.n) for k, v in o.items()}
        res.append((tick, pos, vel, out, None))
        pos, vel = out["new_pos_xz"], out["vel_xz"]
        prev_world = (w, keep)
    ctx.close()
    return res, seen


def _run_follows(navlib, env):
    """The tick loop of an engine that owns its snapshot: PREFETCH_FRONT_INLINE | SNAPSHOT_HELD, and FOLLOWS_STEP
    from tick 1 on; the host never waits inside the run.  Step t reads positions / velocities from ring entry t and
    writes them to entry t+1 (the rows a spawn adds are in place before the run); its vdes / status go to ring entry
    t.  The tables rotate through THREE buffer sets: tick t+1's are written before step t is enqueued (FOLLOWS_STEP:
    the snapshot was final when the last step ended), into the set of tick t-2 (SNAPSHOT_HELD: a snapshot stays
    untouched until the next step has been enqueued -- the set of tick t-1 is still held then)."""
    import torch
    ticks = env["ticks"]
    T, nmax = len(ticks), max(t.n for t in ticks)
    ctx = _context(navlib, env)
    s = ctx.stream
    ring_pos = torch.zeros((T + 1, nmax, 2), device="cuda")
    ring_vel = torch.zeros((T + 1, nmax, 2), device="cuda")
    ring_vdes = torch.zeros((T, nmax, 2), device="cuda")
    ring_status = torch.zeros((T, nmax), dtype=torch.uint8, device="cuda")
    for tick in ticks:
        if tick.n > tick.n_carry:
            ring_pos[tick.t, tick.n_carry:tick.n].copy_(torch.from_numpy(tick.spawn_pos))
            ring_vel[tick.t, tick.n_carry:tick.n].copy_(torch.from_numpy(tick.spawn_vel))
    sets = [_DevSet(ticks, torch) for _ in range(3)]
    sets[0].load(ticks[0])
    torch.cuda.synchronize()
    keep, seen = [], []
    flags = navlib.PREFETCH_FRONT_INLINE | navlib.PREFETCH_SNAPSHOT_HELD
    with torch.cuda.stream(torch.cuda.ExternalStream(s)):
        for tick in ticks:
            t = tick.t
            if t + 1 < T:
                sets[(t + 1) % 3].load(ticks[t + 1], keep)
            w, k = sets[t % 3].world(navlib, tick, ring_pos[t], ring_vel[t])
            keep.append((w, k))
            seen.append((w.n_flocks, w.n_ents))
            so = _step_out(navlib, ring_vel[t + 1], ring_pos[t + 1], ring_vdes[t], ring_status[t])
            keep.append(so)
            ctx.agent_prefetch_dev(w, stream=s, flags=flags | (navlib.PREFETCH_FOLLOWS_STEP if t else 0))
            ctx.agent_step_dev(w, so, stream=s)
    ctx.sync()
    torch.cuda.synchronize()
    # (torch frees pinned host memory behind an event it records on every stream that copied from it: free the
    # staging buffers while the context's stream still exists)
    keep.clear()
    torch.cuda.synchronize()
    res = []
    for tick in ticks:
        t, n = tick.t, tick.n
        out = {"vel_xz": _host(ring_vel[t + 1], n), "new_pos_xz": _host(ring_pos[t + 1], n),
               "vdes_xz": _host(ring_vdes[t], n), "status": _host(ring_status[t], n)}
        res.append((tick, _host(ring_pos[t], n), _host(ring_vel[t], n), out, None))
    ctx.close()
    return res, seen


def _run_slab(navlib, env, with_epoch):
    """Two ranks, one context each, split the uids at a boundary that moves from tick to tick (prefetch + device
    step, the host synchronising between calls).  with_epoch: static_epoch is bumped whenever the flock tables
    change (the caller's promise that an unchanged epoch means unchanged tables); else 0."""
    import torch
    ticks = env["ticks"]
    nmax = max(t.n for t in ticks)
    ctxs = [_context(navlib, env) for _ in range(2)]
    dset = _DevSet(ticks, torch)
    dpos, dvel = torch.zeros((nmax, 2), device="cuda"), torch.zeros((nmax, 2), device="cuda")
    outs = [_outputs(torch, nmax) for _ in ctxs]
    res, seen, epoch, last_tables = [], [], 0, None
    pos = vel = np.zeros((0, 2), np.float32)
    for tick in ticks:
        pos, vel = tick.start_rows(pos, vel)
        if tick.tables_key() != last_tables:
            epoch, last_tables = epoch + 1, tick.tables_key()
        dset.load(tick)
        dpos[:tick.n].copy_(torch.from_numpy(pos))
        dvel[:tick.n].copy_(torch.from_numpy(vel))
        torch.cuda.synchronize()
        cut = cw.slab_cut(tick)
        npos, nvel = np.zeros_like(pos), np.zeros_like(vel)
        for ctx, o, work in zip(ctxs, outs, ((0, cut), (cut, tick.n))):
            w, keep = dset.world(navlib, tick, dpos, dvel, work=work, epoch=epoch if with_epoch else 0)
            so = _step_out(navlib, o["vel_xz"], o["new_pos_xz"], o["vdes_xz"], o["status"])
            ctx.agent_prefetch_dev(w, stream=ctx.stream)
            ctx.agent_step_dev(w, so, stream=ctx.stream)
            ctx.sync()
            torch.cuda.synchronize()
            out = {k: _host(v, tick.n) for k, v in o.items()}
            res.append((tick, pos, vel, out, work))
            npos[work[0]:work[1]], nvel[work[0]:work[1]] = out["new_pos_xz"][work[0]:work[1]], out["vel_xz"][work[0]:work[1]]
        seen.append((w.n_flocks, w.n_ents))
        pos, vel = npos, nvel
    for ctx in ctxs:
        ctx.close()
    return res, seen


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_changing_world_tick_by_tick(navlib, env, schedule, monkeypatch):
    if schedule == "blocking":
        res, seen = _run_blocking(navlib, env)
    elif schedule in ("device", "prefetch", "abandoned"):
        res, seen = _run_synced(navlib, env, prefetch=schedule != "device", abandon=schedule == "abandoned")
    elif schedule in ("follows", "follows_events"):
        if schedule == "follows_events":
            monkeypatch.setenv("NAVHIP_HANDOVER", "events")            # (read when a context gets its side streams)
        res, seen = _run_follows(navlib, env)
    else:
        res, seen = _run_slab(navlib, env, with_epoch=schedule == "slab_epoch")
    # the script did what it says: the flock count crossed 64 both ways, the entity count more than doubled
    kf, ne = [s[0] for s in seen], [s[1] for s in seen]
    first_above = next(i for i, k in enumerate(kf) if k > 64)
    assert kf[0] <= 64 and any(k <= 64 for k in kf[first_above:]), kf
    assert max(ne) >= 2 * ne[0] and ne[-1] < max(ne), ne
    moved = {}
    for tick, pos, vel, out, work in res:
        _check(navlib, env, tick, pos, vel, out, schedule, work)
        rows = np.arange(tick.n) if work is None else np.arange(*work)
        m = moved.setdefault(tick.t, np.zeros(tick.n, bool))
        m[rows] = (out["status"][rows] & navlib.ST_MOVED) != 0
    assert len(moved) == len(env["ticks"])
    for t, m in moved.items():
        assert m.mean() > 0.5, "tick %d: only %.2f of the agents moved" % (t, m.mean())
