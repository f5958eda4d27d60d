"""navhip_arrival_flock_update / _dev (csrc/arrival_flock_kernels.hip, k_arrival_flock) against tests/arrival_flock_model.py,
the plain model of the built-zone branch of G_Arrival_UpdateFlock that tests/test_arrival_flock_cpu.py holds against the
reference: the zone table, the companion, slot_ring, the members' arrival state and the status, bit for bit, host form
and resident form (in place).  Every world asserts its own premise from the model (premises(), shared with the CPU file)."""
import ctypes as C

import numpy as np
import pytest

from tests import arrival_flock_model as afm
from tests import arrival_flock_worlds as aw
from tests import arrival_velocity_model as avm

pytestmark = [pytest.mark.gpu]

F = np.float32
WORLDS = {"shapes": aw.shapes_world, "cap": aw.cap_world, "footprints": aw.footprints_world, "ties": aw.ties_world,
          "frontier": aw.frontier_world, "period": aw.period_world, "fill_below": aw.fill_below_world,
          "batch_1": lambda: aw.batch_world(1), "batch_2": lambda: aw.batch_world(2), "batch_50": lambda: aw.batch_world(50)}
_BUILT = {}


def world(name):
    """The world and the model's answer for it, computed once and left unchanged."""
    if name not in _BUILT:
        W = WORLDS[name]()
        _BUILT[name] = (W, afm.update_flocks(W.map, W.zones, W.keys, W.pos, W.members))
    return _BUILT[name]


def _dev():
    import torch
    from permafrost_engine_amd import tick
    return torch.device("cpu") if tick.EMULATED else torch.device("cuda", 0)


def _sync():
    import torch
    if _dev().type == "cuda":
        torch.cuda.synchronize()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what=""):
    """(zones, members, status) of a call against the model's, every output bit for bit."""
    gz, gm, gs = got
    wz, wm, ws = want
    assert np.array_equal(gs, ws), (what, "status", gs, ws)
    for i, (g, w) in enumerate(zip(gz, wz)):
        for f in afm.ZONE_OUT:
            a, b = (F(g[f]).view(np.uint32), F(w[f]).view(np.uint32)) if f in ("unit_radius", "fill_frac") else (int(g[f]), int(w[f]))
            assert a == b, (what, "zone", i, f, g[f], w[f])
        bad = np.flatnonzero(np.asarray(g["slot_ring"]) != np.asarray(w["slot_ring"]))
        assert len(bad) == 0, (what, "zone", i, "slot_ring", bad[:8], g["slot_ring"][bad[:8]], w["slot_ring"][bad[:8]])
    for i, (g, w) in enumerate(zip(gm, wm)):
        for f in afm.MEMBER_OUT:
            a, b = _bits(g[f]), _bits(w[f])
            assert a.shape == b.shape, (what, "members of zone", i, f, a.shape, b.shape)
            bad = np.flatnonzero((a != b).reshape(len(a), max(a.size // max(len(a), 1), 1)).any(1))
            assert len(bad) == 0, (what, "members of zone", i, f, bad[:8], g[f][bad[:4]], w[f][bad[:4]])


def context(navlib, W):
    ctx = navlib.NavContext(W.w, W.h)
    for layer, b in W.blockers.items():
        ctx.upload_plane(layer, navlib.PLANE_COST_BASE, np.ones((W.h, W.w, 64, 64), np.uint8))
        ctx.upload_plane(layer, navlib.PLANE_BLOCKERS, b)
    return ctx


class Resident:
    """Everything of the call as device tensors; the outputs ARE the inputs (in place)."""

    def __init__(self, navlib, ctx, W, zones=None, members=None):
        import torch
        self.navlib, self.ctx, self.dev = navlib, ctx, _dev()
        self.t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.dev)      # noqa: E731
        zones, members = W.zones if zones is None else zones, W.members if members is None else members
        self.d_pos = self.t(W.pos, F)
        self.world, self.keep = navlib.make_world(W.w, W.h, {"pos_xz": self.d_pos})
        zs, slots, ring, kk = navlib._pack_zones(zones, W.keys)
        fs, cat = navlib.pack_flocks(zones, members)
        self.nz, self.nm, self.n_slots, self.n_keys = len(zones), len(cat["uid"]) - 1, len(ring) - 1, len(kk) - 1
        raw = lambda s: np.frombuffer(bytes(s), np.uint8).copy()             # noqa: E731
        self.d = {"zones": self.t(raw(zs), np.uint8), "flocks": self.t(raw(fs), np.uint8), "slots_xz": self.t(slots, F),
                  "slot_ring": self.t(ring, np.int32), "region_keys": self.t(kk.view(np.int64), np.int64)}
        self.d.update({k: self.t(v, v.dtype) for k, v in cat.items()})
        self.d_status = torch.full((max(1, self.nz),), 0x55, dtype=torch.uint8, device=self.dev)

    def call(self, stream=None):
        fi, fo = self.navlib.ArrivalFlockIn(), self.navlib.ArrivalFlockOut()
        fi.n_zones, fi.nm, fi.n_slots, fi.n_keys = self.nz, self.nm, self.n_slots, self.n_keys
        for k, v in self.d.items():
            setattr(fi, k, v.data_ptr())
        for k in ("zones", "flocks", "slot_ring", "substate", "sink_valid", "sink_xz"):
            setattr(fo, k, self.d[k].data_ptr())
        fo.status = self.d_status.data_ptr()
        self.ctx.arrival_flock_update_dev(self.world, fi, fo, stream)

    def read(self):
        nl = self.navlib
        zs = (nl.ArrivalZone * max(1, self.nz)).from_buffer_copy(self.d["zones"].cpu().numpy().tobytes())
        fs = (nl.ArrivalFlock * max(1, self.nz)).from_buffer_copy(self.d["flocks"].cpu().numpy().tobytes())
        res = {k: self.d[k].cpu().numpy() for k in ("slot_ring", "substate", "sink_valid", "sink_xz")}
        res["status"] = self.d_status.cpu().numpy()
        return nl.unpack_flocks(zs, fs, res, self.nz)


# ---------------------------------------------------------------------------------------------
# what every world is there to show, asserted from the model alone (the CPU file asserts the same)
# ---------------------------------------------------------------------------------------------
def premises(name, W, want):
    wz, wm, ws = want
    zin, min_ = W.zones, W.members
    assert not ws.any(), name
    n = getattr(W, "names", {})

    def slot_dists(i):
        z = zin[i]
        entry = afm.entry_point(z, W.pos, min_[i])
        return afm.geodesic_dist(W.map, W.keys[i], entry, z["slots_xz"]), entry
    if name == "shapes":
        assert [len(z["slot_ring"]) for z in zin[:5]] == list(aw.SLOT_COUNTS)
        for i in (5, 6):                                                     # M == 0, num_rows == 0: the counter, nothing else
            assert wz[i]["realloc_counter"] == 0 and wz[i]["num_rows"] == zin[i]["num_rows"] and wz[i]["fill_frac"] == 0
            assert np.array_equal(wm[i]["sink_valid"], min_[i]["sink_valid"]) and np.array_equal(wm[i]["substate"], min_[i]["substate"])
        assert wz[7]["layer"] == 1 and wz[0]["radius"] == afm.zone_radius(4, 2.5) != zin[0]["radius"]
        # slots under blockers count: of layer 1 for zone 7, whose layer-0 blockers do not
        b1 = sum(W.map.blocked(1, *s) for s in zin[7]["slots_xz"])
        b0 = sum(W.map.blocked(0, *s) for s in zin[7]["slots_xz"])
        assert b1 > 0 and b0 > 0 and wz[7]["fill_frac"] >= F(b1) / F(40)
        committed = {int(s) for i in range(5) for s, t in zip(min_[i]["substate"], wm[i]["substate"]) if s != t}
        stayed = {int(s) for i in range(5) for s, t, v, done in zip(min_[i]["substate"], wm[i]["substate"], wm[i]["sink_valid"], min_[i]["settled"])
                  if s == t and v and not done}
        assert committed == {0, 1} and stayed == {2, 3}                      # all four substates among the units committed
        assert any(z["num_rows"] > 1 for z in wz[:5])
    if name == "cap":
        assert len(W.keys[0]) == 4096 == len(zin[0]["slots_xz"]) and len(min_[0]["uid"]) == 3 and wz[0]["num_rows"] > 8
    if name == "footprints":
        (g, maxd, _), entry = slot_dists(n["c_shape"])
        s = zin[n["c_shape"]]["slots_xz"]
        e = np.hypot(s[:, 0] - entry[0], s[:, 1] - entry[1])
        assert any(g[i] < g[j] and e[i] > e[j] + 4 for i in range(len(s)) for j in range(len(s)))     # geodesic != straight order
        (g, maxd, _), _ = slot_dists(n["two_parts"])
        assert (g < 0).sum() > 3 and (g >= 0).sum() > 3
        assert (wz[n["two_parts"]]["slot_ring"][g < 0] == wz[n["two_parts"]]["num_rows"] - 1).all() and wz[n["two_parts"]]["num_rows"] > 2
        (g, _, _), _ = slot_dists(n["off_region"])
        assert (g[-4:] == -1).all() and (g[:-4] >= 0).all()
        (g, _, kd), _ = slot_dists(n["hole"])
        assert min(kd) >= 0 and len(W.keys[n["hole"]]) == 72
        for k in ("chunk_corner", "edge", "corner"):
            assert wz[n[k]]["num_rows"] > 1
        assert len({int(key) >> 32 for key in W.keys[n["chunk_corner"]]}) == 4                       # four chunks
    if name == "ties":
        i = n["four"]
        assert wm[i]["sink_valid"].tolist() == [1, 1, 1] and np.array_equal(wm[i]["sink_xz"][1], zin[i]["slots_xz"][1])
        assert np.array_equal(wm[i]["sink_xz"][2], zin[i]["slots_xz"][1]) and wz[i]["fill_frac"] == F(1) / F(5)
        e = afm.entry_point(zin[n["entry"]], W.pos, min_[n["entry"]])
        assert afm.source_key(W.map, W.keys[n["entry"]], e) == 0
        d = [F(F(c[0] - e[0]) ** 2 + F(c[1] - e[1]) ** 2) for c in (afm.tile_centre(W.map, int(k)) for k in W.keys[n["entry"]][:2])]
        assert d[0] == d[1]
        assert wz[n["entry"]]["slot_ring"].tolist() == [5, 4, 3, 2, 1, 0]
        i = n["coincident"]
        assert wz[i]["fill_frac"] == F(1) / F(4) and np.array_equal(wm[i]["sink_xz"][1], zin[i]["slots_xz"][2])
    if name == "frontier":
        z = lambda k: wz[n[k]]                                               # noqa: E731
        assert (z("exact_cap")["active_row"], z("exact_cap")["stall_counter"], z("exact_cap")["prev_occ"]) == (1, 0, 1)
        assert z("three_rows")["active_row"] == 3 and z("three_rows")["prev_occ"] == 0
        assert (z("stall_18")["active_row"], z("stall_18")["stall_counter"]) == (0, 19)
        assert (z("stall_19")["active_row"], z("stall_19")["stall_counter"]) == (1, 0)
        assert (z("last_row")["active_row"], z("last_row")["stall_counter"]) == (1, 20)
        assert (z("crowd_0")["active_row"], z("crowd_0")["stall_counter"]) == (0, 0)
        assert z("rising")["stall_counter"] == 0 and z("not_rising")["stall_counter"] == 6
        assert z("fill_above")["num_rows"] == 2 and z("fill_exact")["num_rows"] == 2 and z("fill_exact")["active_row"] == 0
        assert z("blocked_l0")["fill_frac"] == F(5) / F(8) and z("blocked_l0")["active_row"] == 1
        assert z("blocked_l1")["fill_frac"] == F(3) / F(8) and z("blocked_l1")["layer"] == 1
    if name == "fill_below":
        a, b = wz[n["fill_below"]], wz[n["fill_exact"]]
        assert not np.array_equal(a["slot_ring"], zin[n["fill_below"]]["slot_ring"]) and a["active_row"] == 0
        assert np.array_equal(b["slot_ring"], zin[n["fill_exact"]]["slot_ring"]) and b["active_row"] == 1
    if name == "period":
        for c in range(4):
            z = wz[n["counter_%d" % c]]
            assert z["realloc_counter"] == (c + 1) % 4 and (z["active_row"] == 1) == (c == 3) and z["radius"] == afm.zone_radius(8, 1.0)
            assert (wm[n["counter_%d" % c]]["substate"] != min_[n["counter_%d" % c]]["substate"]).any() == (c == 3)
        for k, phase in (("none_of_0", afm.DONE), ("settled_1", afm.DONE), ("unsettled_1", afm.FILLING), ("none_of_300", afm.FILLING),
                         ("some_of_300", afm.FILLING), ("all_of_300", afm.DONE)):
            z, zi = wz[n[k]], zin[n[k]]
            assert z["phase"] == phase, k
            if phase == afm.DONE:                                            # nothing else changes, not even layer, radius, unit_radius
                assert all(F(z[f]).view(np.uint32) == F(zi[f]).view(np.uint32) for f in afm.ZONE_OUT if f != "phase"), k
            else:
                assert z["radius"] != zi["radius"] and z["unit_radius"] == F(1.5) and z["realloc_counter"] == 0
    if name.startswith("batch_"):
        done = [i for i, z in enumerate(wz) if z["phase"] == afm.DONE]
        count = len(zin)
        assert done == (sorted({0, count // 2, count - 1}) if count >= 3 else []) and len(zin) == int(name[6:])


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_worlds_host_form_and_resident_in_place(navlib, name):
    W, want = world(name)
    premises(name, W, want)
    ctx = context(navlib, W)
    same(ctx.arrival_flock_update({"pos_xz": W.pos}, W.zones, W.keys, W.members), want, name + ", host form")
    R = Resident(navlib, ctx, W)
    _sync()
    R.call()
    ctx.sync()
    same(R.read(), want, name + ", resident")
    ctx.close()


# ---------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------
def model_chain(calls=12):
    """The model over `calls` calls of the chain world: per call (zones in, members in, positions, the model's answer)."""
    W = aw.chain_world()
    steps = []
    for call in range(calls):
        want = afm.update_flocks(W.map, W.zones, W.keys, W.pos, W.members)
        steps.append((W.zones, W.members, W.pos.copy(), want))
        aw.chain_step(W, want[0], want[1], call)
    return W, steps


_CHAIN = []


def chain():
    if not _CHAIN:
        _CHAIN.append(model_chain())
    return _CHAIN[0]


def chain_premises(steps):
    first, last = steps[0][3][0], steps[-1][3][0]
    settled = [int(s[1][0]["settled"].sum()) for s in steps]
    assert settled[0] == 0 and settled[-1] > 8 and sorted(settled) == settled
    fills = [float(s[0][0]["fill_frac"]) for s in steps]
    assert fills[0] < 0.25 <= fills[-1]                                      # the zone re-orients, then freezes
    assert last[0]["active_row"] >= 1 or last[0]["fill_frac"] > first[0]["fill_frac"]
    assert [s[3][0][0]["realloc_counter"] for s in steps[:5]] == [0, 1, 2, 3, 0]


def test_chain_of_twelve_calls_host_and_resident_then_the_velocity_call(navlib):
    """Members walk to their sinks and settle by script between calls.  The host form call by call; the resident chain with
    the zone table, the companion, the rings and the members' state living in device arrays in place (the script uploads
    positions and settled flags only); then navhip_arrival_velocity_dev on the same device arrays == model after model."""
    import torch
    W, steps = chain()
    chain_premises(steps)
    ctx = context(navlib, W)
    for call, (zones, mems, pos, want) in enumerate(steps):
        same(ctx.arrival_flock_update({"pos_xz": pos}, zones, W.keys, mems), want, "host chain, call %d" % call)
    zones0, mems0, pos0, _ = steps[0]
    W0 = aw.chain_world()
    R = Resident(navlib, ctx, W0)
    _sync()
    for call, (zones, mems, pos, want) in enumerate(steps):
        R.d_pos.copy_(torch.from_numpy(pos))
        R.d["settled"][:R.nm].copy_(torch.from_numpy(np.concatenate([m["settled"] for m in mems])))
        _sync()
        R.call()
    ctx.sync()
    same(R.read(), steps[-1][3], "resident chain")
    # ---- the velocity call on the same device arrays: the member rows are the query rows
    zones, mems, pos, want = steps[-1]
    after = [dict(z, **{k: za[k] for k in afm.ZONE_OUT}, slot_ring=za["slot_ring"]) for z, za in zip(zones, want[0])]
    nq = R.nm
    cat = lambda f: np.concatenate([m[f] for m in want[1]])                  # noqa: E731
    units = {"uid": np.concatenate([m["uid"] for m in mems]), "zone": np.concatenate([np.full(len(m["uid"]), i, np.int32) for i, m in enumerate(mems)]),
             "has_dest_los": np.zeros(nq, np.uint8), "substate": cat("substate"), "sink_valid": cat("sink_valid"), "sink_xz": cat("sink_xz"),
             "los_latched": np.ones(nq, np.uint8), "los_hyst": np.zeros(nq, np.int32)}
    none = np.full(len(zones), -1, np.int32)
    v_want = avm.desired_velocity(W.map, after, W.keys, none, none, pos, units)
    assert (v_want["arm"] == "beeline").sum() > 3 and (v_want["status"] == 0).all()
    t = R.t
    extra = {"zone": t(units["zone"], np.int32), "has_dest_los": t(units["has_dest_los"], np.uint8), "los_latched": t(units["los_latched"], np.uint8),
             "los_hyst": t(units["los_hyst"], np.int32), "zone_row": t(none, np.int32), "com_row": t(none, np.int32)}
    out = {"vdes_xz": torch.zeros((nq, 2), dtype=torch.float32, device=R.dev), "status": torch.zeros(nq, dtype=torch.uint8, device=R.dev),
           "los_latched": torch.zeros(nq, dtype=torch.uint8, device=R.dev), "los_hyst": torch.zeros(nq, dtype=torch.int32, device=R.dev)}
    vi, vo = navlib.ArrivalVelIn(), navlib.ArrivalVelOut()
    vi.n_zones, vi.nq, vi.n_slots, vi.n_keys = R.nz, nq, R.n_slots, R.n_keys
    for k in ("zones", "slots_xz", "slot_ring", "region_keys", "uid", "substate", "sink_valid", "sink_xz"):
        setattr(vi, k, R.d[k].data_ptr())
    for k, v in extra.items():
        setattr(vi, k, v.data_ptr())
    for k in ("substate", "sink_valid", "sink_xz"):
        setattr(vo, k, R.d[k].data_ptr())
    for k, v in out.items():
        setattr(vo, k, v.data_ptr())
    _sync()
    ctx.arrival_velocity_dev(R.world, vi, vo)
    ctx.sync()
    assert np.array_equal(out["vdes_xz"].cpu().numpy().view(np.uint32), v_want["vdes_xz"].view(np.uint32))
    assert np.array_equal(out["status"].cpu().numpy(), v_want["status"])
    for f in ("substate", "sink_valid", "sink_xz"):
        assert np.array_equal(_bits(R.d[f].cpu().numpy()[:nq]), _bits(v_want[f])), f
    ctx.close()


# ---------------------------------------------------------------------------------------------
# NAVHIP_AF_HOST rows, argument errors
# ---------------------------------------------------------------------------------------------
def host_rows_world():
    """Zones the device leaves to the host between zones it decides: a layer without a blockers plane, a uid outside the
    world (above and below), phase INACTIVE and DONE, num_rows above the cap, active_row outside the rows."""
    W = aw.World(2, 2)
    n = W.names = {}
    n["ok_0"] = aw.row_zone(W, 4, 4, (4, 4), (4, 0), 3)
    n["layer"] = aw.row_zone(W, 8, 4, (4, 4), (4, 0), 3, layer=2)
    n["uid_high"] = aw.row_zone(W, 12, 4, (4, 4), (4, 0), 3)
    n["uid_neg"] = aw.row_zone(W, 16, 4, (4, 4), (4, 0), 3)
    n["inactive"] = aw.row_zone(W, 20, 4, (4, 4), (4, 0), 3, phase=afm.INACTIVE)
    n["done"] = aw.row_zone(W, 24, 4, (4, 4), (4, 0), 3, phase=afm.DONE)
    n["rows"] = aw.row_zone(W, 28, 4, (4, 4), (4, 0), 3, num_rows=5000)
    n["active_row"] = aw.row_zone(W, 32, 4, (4, 4), (4, 0), 3, active_row=2)
    n["ok_1"] = aw.row_zone(W, 36, 4, (4, 4), (4, 0), 3)
    W.done()
    W.members[n["uid_high"]]["uid"][2] = len(W.pos)
    W.members[n["uid_neg"]]["uid"][0] = -1
    return W


def test_host_rows_of_both_forms(navlib):
    W = host_rows_world()
    want = afm.update_flocks(W.map, W.zones, W.keys, W.pos, W.members)
    n = W.names
    assert want[2].tolist() == [0] + [afm.AF_HOST] * 7 + [0]
    for i in range(1, 8):                                                    # every output repeats its input
        assert all(want[0][i][f] == W.zones[i][f] for f in afm.ZONE_OUT)
        assert all(np.array_equal(want[1][i][f], W.members[i][f]) for f in afm.MEMBER_OUT)
    assert want[0][n["ok_1"]]["active_row"] == 1
    ctx = context(navlib, W)
    same(ctx.arrival_flock_update({"pos_xz": W.pos}, W.zones, W.keys, W.members), want, "host form")
    R = Resident(navlib, ctx, W)
    _sync()
    R.call()
    ctx.sync()
    same(R.read(), want, "resident")
    ctx.close()


def test_more_slots_or_keys_than_the_cap_is_a_host_row(navlib):
    W = aw.World(4, 4)
    tiles = aw.rect(10, 10, 65, 64)                                          # 4 160 keys
    slots = np.array([aw.xz(4, 4, r, c) for r, c in tiles[:40]], F)
    W.add(aw.zone(4, 4, tiles, slots), [(aw.xz(4, 4, 11, 11), 0, 0, 0, (0, 0))])
    small = aw.rect(100, 100, 8, 8)
    many = np.array([aw.xz(4, 4, 100 + (i // 8) % 8, 100 + i % 8) for i in range(4097)], F)
    W.add(aw.zone(4, 4, small, many), [(aw.xz(4, 4, 101, 101), 0, 0, 0, (0, 0))])
    W.add(aw.zone(4, 4, small, many[:10]), [(aw.xz(4, 4, 101, 101), 0, 0, 0, (0, 0))])
    W.done()
    want = afm.update_flocks(W.map, W.zones, W.keys, W.pos, W.members)
    assert want[2].tolist() == [afm.AF_HOST, afm.AF_HOST, 0] and want[1][2]["sink_valid"][0] == 1
    ctx = context(navlib, W)
    same(ctx.arrival_flock_update({"pos_xz": W.pos}, W.zones, W.keys, W.members), want, "host form")
    ctx.close()


def test_argument_errors(navlib):
    """Each refusal is NAVHIP_ERR_ARG, names its reason and leaves the outputs untouched."""
    W = aw.World(2, 2)
    aw.row_zone(W, 4, 4, (4, 4), (4, 0), 3)
    W.done()
    ctx = context(navlib, W)
    seen = {}
    outs = ("zones", "flocks", "slot_ring", "substate", "sink_valid", "sink_xz", "status")

    def refused(word, patch, keys=None):
        def damage(fi, fo, zs, fs):
            seen["out"] = []
            for name in outs:
                a = (C.c_uint8 * 4).from_address(getattr(fo, name))
                C.memset(a, 7, 1 if name == "status" else 4)
                seen["out"].append(a)
            patch(fi, fo, zs, fs)
        with pytest.raises(navlib.NavHipError) as e:
            ctx.arrival_flock_update({"pos_xz": W.pos}, W.zones, keys or W.keys, W.members, patch=damage)
        assert "(%d)" % navlib.ERR_ARG in str(e.value) and word in str(e.value), str(e.value)
        for a, name in zip(seen["out"], outs):
            k = 1 if name == "status" else 4
            assert bytes(a[:k]) == b"\x07" * k, name

    _, _, status = ctx.arrival_flock_update({"pos_xz": W.pos}, W.zones, W.keys, W.members)      # (fine as it is)
    assert (status == 0).all()
    for member in ("zones", "flocks", "slots_xz", "slot_ring", "region_keys", "uid", "settled", "substate", "sink_valid", "sink_xz"):
        refused("missing", lambda fi, fo, zs, fs, f=member: setattr(fi, f, None))
    for member in outs:
        refused("missing", lambda fi, fo, zs, fs, f=member: setattr(fo, f, None))
    refused("nm < 0", lambda fi, fo, zs, fs: setattr(fi, "nm", -1))
    refused("slot range", lambda fi, fo, zs, fs: setattr(zs[0], "slot_end", 9))
    refused("slot range", lambda fi, fo, zs, fs: setattr(zs[0], "slot_begin", -1))
    refused("key range", lambda fi, fo, zs, fs: setattr(zs[0], "key_end", len(W.keys[0]) + 1))
    refused("member range", lambda fi, fo, zs, fs: setattr(fs[0], "member_end", 8))
    refused("member range", lambda fi, fo, zs, fs: setattr(fs[0], "member_begin", -2))
    refused("not ascending", lambda fi, fo, zs, fs: None, keys=[W.keys[0][::-1].copy()])
    refused("not ascending", lambda fi, fo, zs, fs: None, keys=[np.concatenate([W.keys[0][:2], W.keys[0][1:]])])
    ctx.close()
