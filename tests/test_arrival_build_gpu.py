"""navhip_arrival_zone_build / _dev (csrc/arrival_build_kernels.hip, k_arrival_build, and k_arrival_flock's first-build mode)
against tests/arrival_build_model.py, the plain model of the `!built` branch of G_Arrival_UpdateFlock that
tests/test_arrival_build_cpu.py holds against the reference: the zone table, the companion, slots, rings, keys, axis, com,
com_dest_id, the members' arrival state and the status, bit for bit, host form and resident form (in place).  Every world
asserts its own premise from the model (arrival_build_worlds.premises, shared with the CPU file)."""
import ctypes as C

import numpy as np
import pytest

from tests import arrival_build_model as abm
from tests import arrival_build_worlds as bw
from tests import arrival_flock_model as afm
from tests import arrival_velocity_model as avm
from tests.test_arrival_flock_gpu import _bits, _dev, _sync

pytestmark = [pytest.mark.gpu]

F = np.float32
ZONE_F = ("centre_x", "centre_z", "unit_radius", "fill_frac")
ZONE_I = ("radius", "layer", "active_row", "num_rows", "slot_begin", "key_begin")
FLOCK_I = ("phase", "realloc_counter", "stall_counter", "prev_occ", "total_members", "layer", "member_begin", "member_end")


def context(navlib, W):
    ctx = navlib.NavContext(W.w, W.h)
    for layer in W.blockers:
        ctx.upload_plane(layer, navlib.PLANE_COST_BASE, W.cost[layer])
        ctx.upload_plane(layer, navlib.PLANE_BLOCKERS, W.blockers[layer])
    return ctx


def same(navlib, W, got, want, what=""):
    """What a call left (the dict of NavContext.arrival_zone_build) against the model's answers, every output bit for bit."""
    zs_in, slots_in, ring_in, keys_in = navlib._pack_zones(W.zones, [z["room_keys"] for z in W.zones])
    fs_in, cat = navlib.pack_flocks(W.zones, W.members)
    status = np.asarray(got["status"])[:len(want)]
    assert status.tolist() == [r["status"] for r in want], (what, status.tolist())
    for i, r in enumerate(want):
        z, f, zi, fi = got["zs"][i], got["fs"][i], zs_in[i], fs_in[i]
        tag = (what, "zone", i)
        mb, me = fi.member_begin, fi.member_end
        for name in afm.MEMBER_OUT:
            assert np.array_equal(_bits(np.asarray(got[name])[mb:me]), _bits(np.asarray(r["members"][name]))), tag + (name,)
        if r["status"] != 0:                                                 # every output repeats its input
            assert bytes(z) == bytes(zi) and bytes(f) == bytes(fi), tag
            assert np.array_equal(_bits(np.asarray(got["slots_xz"])[zi.slot_begin:zi.slot_end]), _bits(slots_in[zi.slot_begin:zi.slot_end])), tag
            assert np.array_equal(np.asarray(got["slot_ring"])[zi.slot_begin:zi.slot_end], ring_in[zi.slot_begin:zi.slot_end]), tag
            assert np.array_equal(np.asarray(got["region_keys"])[zi.key_begin:zi.key_end], keys_in[zi.key_begin:zi.key_end]), tag
            # axis, com and dest id have no input to repeat: they are not written (the callers fill them with -7 / 7)
            assert np.asarray(got["axis_xz"])[i].tolist() == [-7.0, -7.0] and np.asarray(got["com_xz"])[i].tolist() == [-7.0, -7.0], tag
            assert int(np.asarray(got["com_dest_id"])[i]) == 7, tag
            continue
        wz = r["zone"]
        exp = dict(wz, centre_x=wz["centre_xz"][0], centre_z=wz["centre_xz"][1], slot_begin=zi.slot_begin, key_begin=zi.key_begin,
                   total_members=fi.total_members, member_begin=mb, member_end=me)
        for name in ZONE_F:
            assert F(getattr(z, name)).view(np.uint32) == F(exp[name]).view(np.uint32), tag + (name, getattr(z, name), exp[name])
        for name in ZONE_I:
            assert getattr(z, name) == int(exp[name]), tag + (name, getattr(z, name), exp[name])
        for name in FLOCK_I:
            assert getattr(f, name) == int(exp[name]), tag + (name, getattr(f, name), exp[name])
        assert F(f.row_height).view(np.uint32) == F(wz["row_height"]).view(np.uint32) and F(f.unit_radius).view(np.uint32) == F(fi.unit_radius).view(np.uint32), tag
        assert z.slot_end - z.slot_begin == len(wz["slots_xz"]) and z.key_end - z.key_begin == len(r["keys"]), \
            tag + (z.slot_end - z.slot_begin, len(wz["slots_xz"]), z.key_end - z.key_begin, len(r["keys"]))
        gs = np.asarray(got["slots_xz"])[z.slot_begin:z.slot_end]
        bad = np.flatnonzero((_bits(gs) != _bits(np.asarray(wz["slots_xz"], F).reshape(-1, 2))).any(1))
        assert len(bad) == 0, tag + ("slots_xz", bad[:8], gs[bad[:4]], wz["slots_xz"][bad[:4]])
        assert np.array_equal(np.asarray(got["slot_ring"])[z.slot_begin:z.slot_end], wz["slot_ring"]), tag + ("slot_ring",)
        assert np.array_equal(np.asarray(got["region_keys"])[z.key_begin:z.key_end], r["keys"]), tag + ("region_keys",)
        # what the room holds behind the new ranges is not touched
        assert np.array_equal(_bits(np.asarray(got["slots_xz"])[z.slot_end:zi.slot_end]), _bits(slots_in[z.slot_end:zi.slot_end])), tag
        assert np.array_equal(np.asarray(got["region_keys"])[z.key_end:zi.key_end], keys_in[z.key_end:zi.key_end]), tag
        assert np.array_equal(_bits(np.asarray(got["axis_xz"])[i]), _bits(r["axis"])), tag + ("axis", got["axis_xz"][i], r["axis"])
        assert np.array_equal(_bits(np.asarray(got["com_xz"])[i]), _bits(r["com"])), tag + ("com", got["com_xz"][i], r["com"])
        assert int(np.asarray(got["com_dest_id"])[i]) == r["com_dest_id"], tag + ("com_dest_id",)


class Resident:
    """Everything of the call as device tensors; the outputs ARE the inputs (in place) where the call has an input."""

    def __init__(self, navlib, ctx, W):
        import torch
        self.navlib, self.ctx, self.dev, self.W = navlib, ctx, _dev(), W
        self.t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.dev)      # noqa: E731
        self.d_pos = self.t(W.pos, F)
        self.world, self.keep = navlib.make_world(W.w, W.h, {"pos_xz": self.d_pos})
        zs, slots, ring, kk = navlib._pack_zones(W.zones, [z["room_keys"] for z in W.zones])
        fs, cat = navlib.pack_flocks(W.zones, W.members)
        self.nz, self.nm, self.n_slots, self.n_keys = len(W.zones), len(cat["uid"]) - 1, len(ring) - 1, len(kk) - 1
        raw = lambda s: np.frombuffer(bytes(s), np.uint8).copy()             # noqa: E731
        self.d = {"zones": self.t(raw(zs), np.uint8), "flocks": self.t(raw(fs), np.uint8), "slots_xz": self.t(slots, F),
                  "slot_ring": self.t(ring, np.int32), "region_keys": self.t(kk.view(np.int64), np.int64),
                  "target_xz": self.t(np.concatenate([W.targets, np.zeros((1, 2), F)]), F)}
        self.d.update({k: self.t(v, v.dtype) for k, v in cat.items()})
        self.o = {"axis_xz": torch.full((self.nz + 1, 2), -7.0, dtype=torch.float32, device=self.dev),
                  "com_xz": torch.full((self.nz + 1, 2), -7.0, dtype=torch.float32, device=self.dev),
                  "com_dest_id": torch.full((self.nz + 1,), 7, dtype=torch.int32, device=self.dev),
                  "status": torch.full((max(1, self.nz),), 0x55, dtype=torch.uint8, device=self.dev)}

    def call(self, stream=None):
        bi, bo = self.navlib.ArrivalBuildIn(), self.navlib.ArrivalBuildOut()
        bi.n_zones, bi.nm, bi.n_slots, bi.n_keys = self.nz, self.nm, self.n_slots, self.n_keys
        for k, v in self.d.items():
            setattr(bi, k, v.data_ptr())
        for k in ("zones", "flocks", "slots_xz", "slot_ring", "region_keys", "substate", "sink_valid", "sink_xz"):
            setattr(bo, k, self.d[k].data_ptr())
        for k, v in self.o.items():
            setattr(bo, k, v.data_ptr())
        self.ctx.arrival_zone_build_dev(self.world, bi, bo, stream)

    def read(self):
        nl = self.navlib
        res = {k: self.d[k].cpu().numpy() for k in ("slots_xz", "slot_ring", "substate", "sink_valid", "sink_xz")}
        res["region_keys"] = self.d["region_keys"].cpu().numpy().view(np.uint64)
        res.update({k: v.cpu().numpy() for k, v in self.o.items()})
        res["com_dest_id"] = res["com_dest_id"].view(np.uint32)
        res["zs"] = (nl.ArrivalZone * max(1, self.nz)).from_buffer_copy(self.d["zones"].cpu().numpy().tobytes())
        res["fs"] = (nl.ArrivalFlock * max(1, self.nz)).from_buffer_copy(self.d["flocks"].cpu().numpy().tobytes())
        return res


# the rows the host form refuses before it launches: their room is the caller's mistake there, a HOST row on the device
ROOM_ROWS = ("host_room_keys", "host_room_slots")


@pytest.mark.parametrize("name", sorted(bw.WORLDS))
def test_worlds_host_form_and_resident_in_place(navlib, name):
    W, want = bw.world(name)
    bw.premises(name, W, want)
    ctx = context(navlib, W)
    R = Resident(navlib, ctx, W)
    _sync()
    R.call()
    ctx.sync()
    same(navlib, W, R.read(), want, name + ", resident")
    if any(k in W.names for k in ROOM_ROWS):
        with pytest.raises(navlib.NavHipError) as e:
            ctx.arrival_zone_build({"pos_xz": W.pos}, W.zones, W.members, W.targets)
        assert "too little room" in str(e.value)
        keep = [i for k, i in sorted(W.names.items(), key=lambda kv: kv[1]) if k not in ROOM_ROWS]
        sub = bw.World(W.w, W.h)
        sub.blockers, sub.cost, sub.map, sub.pos = W.blockers, W.cost, W.map, W.pos
        sub.zones, sub.members, sub.targets = [W.zones[i] for i in keep], [W.members[i] for i in keep], W.targets[keep]
        W, want = sub, [want[i] for i in keep]
    same(navlib, W, ctx.arrival_zone_build({"pos_xz": W.pos}, W.zones, W.members, W.targets), want, name + ", host form")
    ctx.close()


def test_build_then_eight_flock_updates_then_the_velocity_call_on_the_same_arrays(navlib):
    """The chain on resident arrays: the build, eight navhip_arrival_flock_update_dev calls in place -- the zone table equals
    the flock model run eight times on the build model's answer -- then navhip_arrival_velocity_dev on the same device arrays
    (the member rows are the query rows) == tests/arrival_velocity_model.py on the zones the two models left."""
    import torch
    W, want = bw.world("open")
    ctx = context(navlib, W)
    R = Resident(navlib, ctx, W)
    _sync()
    R.call()
    fi, fo = navlib.ArrivalFlockIn(), navlib.ArrivalFlockOut()
    fi.n_zones, fi.nm, fi.n_slots, fi.n_keys = R.nz, R.nm, R.n_slots, R.n_keys
    for k in ("zones", "flocks", "slots_xz", "slot_ring", "region_keys", "uid", "settled", "substate", "sink_valid", "sink_xz"):
        setattr(fi, k, R.d[k].data_ptr())
    for k in ("zones", "flocks", "slot_ring", "substate", "sink_valid", "sink_xz"):
        setattr(fo, k, R.d[k].data_ptr())
    fo.status = R.o["status"].data_ptr()
    for _ in range(8):
        ctx.arrival_flock_update_dev(R.world, fi, fo)
    ctx.sync()
    got = R.read()
    after, mems = [], []
    for i, r in enumerate(want):
        z = dict(r["zone"], arg_layer=W.zones[i]["arg_layer"], arg_unit_radius=W.zones[i]["arg_unit_radius"],
                 arg_total_members=W.zones[i]["arg_total_members"])
        mem = dict(W.members[i], **r["members"])
        for _ in range(8):
            z, out, status = afm.update_flock(W.map, z, r["keys"], W.pos, mem)
            assert status == 0
            mem = dict(mem, **out)
        gz, gf = got["zs"][i], got["fs"][i]
        assert (gz.active_row, gz.num_rows, gf.realloc_counter, gf.stall_counter, gf.prev_occ, gf.phase) == \
            (z["active_row"], z["num_rows"], z["realloc_counter"], z["stall_counter"], z["prev_occ"], z["phase"]), i
        assert F(gz.fill_frac).view(np.uint32) == F(z["fill_frac"]).view(np.uint32)
        assert np.array_equal(got["slot_ring"][gz.slot_begin:gz.slot_end], z["slot_ring"])
        for name in afm.MEMBER_OUT:
            assert np.array_equal(_bits(got[name][gf.member_begin:gf.member_end]), _bits(mem[name])), (i, name)
        after.append(z)
        mems.append(mem)
    # ---- the velocity call: it reads the zone table, the slots, rings and keys the build wrote
    nq, nz = R.nm, R.nz
    cat = lambda f: np.concatenate([m[f] for m in mems])                     # noqa: E731
    units = {"uid": cat("uid"), "zone": np.concatenate([np.full(len(m["uid"]), i, np.int32) for i, m in enumerate(mems)]),
             "has_dest_los": np.zeros(nq, np.uint8), "substate": cat("substate"), "sink_valid": cat("sink_valid"), "sink_xz": cat("sink_xz"),
             "los_latched": np.ones(nq, np.uint8), "los_hyst": np.zeros(nq, np.int32)}
    none = np.full(nz, -1, np.int32)
    v_want = avm.desired_velocity(W.map, after, [r["keys"] for r in want], none, none, W.pos, units)
    assert (v_want["arm"] == "beeline").sum() > 3 and len(set(v_want["arm"])) >= 2, sorted(set(v_want["arm"]))
    t = R.t
    extra = {"zone": t(units["zone"], np.int32), "has_dest_los": t(units["has_dest_los"], np.uint8), "los_latched": t(units["los_latched"], np.uint8),
             "los_hyst": t(units["los_hyst"], np.int32), "zone_row": t(none, np.int32), "com_row": t(none, np.int32)}
    out = {"vdes_xz": torch.zeros((nq, 2), dtype=torch.float32, device=R.dev), "status": torch.zeros(nq, dtype=torch.uint8, device=R.dev),
           "los_latched": torch.zeros(nq, dtype=torch.uint8, device=R.dev), "los_hyst": torch.zeros(nq, dtype=torch.int32, device=R.dev)}
    vi, vo = navlib.ArrivalVelIn(), navlib.ArrivalVelOut()
    vi.n_zones, vi.nq, vi.n_slots, vi.n_keys = nz, nq, R.n_slots, R.n_keys
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


def test_host_form_asks_no_room_of_zones_it_will_not_build(navlib):
    """A batch of zones that wait (nobody near, three members) or are the host's (a layer without planes, a uid outside the
    world), each with one slot and one key of room: the host form polls them like the resident form."""
    W = bw.World(2, 2)
    t = W.p(64, 64)
    W.add("nobody_near", t, [W.p(10, 10), W.p(120, 10), W.p(10, 120), W.p(120, 120)], total=40, room=(1, 1))
    W.add("total_3", t, bw.crowd(W, 70, 64, 6), total=3, room=(1, 1))
    W.add("host_layer", t, bw.crowd(W, 70, 64, 6, seed=2), total=40, layer=2, room=(1, 1))
    W.add("host_uid", t, bw.crowd(W, 70, 64, 6, seed=3), total=40, room=(1, 1))
    W.done()
    W.members[W.names["host_uid"]]["uid"][0] = -1
    want = abm.build_zones(W.map, W.zones, W.pos, W.members, W.targets)
    assert [r["status"] for r in want] == [abm.AB_WAIT, abm.AB_WAIT, abm.AB_HOST, abm.AB_HOST]
    ctx = context(navlib, W)
    same(navlib, W, ctx.arrival_zone_build({"pos_xz": W.pos}, W.zones, W.members, W.targets), want, "host form")
    R = Resident(navlib, ctx, W)
    _sync()
    R.call()
    ctx.sync()
    same(navlib, W, R.read(), want, "resident")
    ctx.close()


def test_argument_errors(navlib):
    """Each refusal is NAVHIP_ERR_ARG, names its reason and leaves the outputs untouched."""
    W, _ = bw.world("edges")
    ctx = context(navlib, W)
    seen = {}
    outs = ("zones", "flocks", "slots_xz", "slot_ring", "region_keys", "axis_xz", "com_xz", "com_dest_id", "substate", "sink_valid",
            "sink_xz", "status")

    def refused(word, patch):
        def damage(bi, bo, zs, fs):
            seen["out"] = []
            for name in outs:
                a = (C.c_uint8 * 4).from_address(getattr(bo, name))
                C.memset(a, 9, 1 if name == "status" else 4)
                seen["out"].append(a)
            patch(bi, bo, zs, fs)
        with pytest.raises(navlib.NavHipError) as e:
            ctx.arrival_zone_build({"pos_xz": W.pos}, W.zones, W.members, W.targets, patch=damage)
        assert "(%d)" % navlib.ERR_ARG in str(e.value) and word in str(e.value), str(e.value)
        for a, name in zip(seen["out"], outs):
            k = 1 if name == "status" else 4
            assert bytes(a[:k]) == b"\x09" * k, name

    for member in ("zones", "flocks", "target_xz", "slots_xz", "slot_ring", "region_keys", "uid", "settled", "substate", "sink_valid", "sink_xz"):
        refused("missing", lambda bi, bo, zs, fs, f=member: setattr(bi, f, None))
    for member in outs:
        refused("missing", lambda bi, bo, zs, fs, f=member: setattr(bo, f, None))
    refused("nm < 0", lambda bi, bo, zs, fs: setattr(bi, "nm", -1))
    refused("slot range", lambda bi, bo, zs, fs: setattr(zs[0], "slot_begin", -1))
    refused("key range", lambda bi, bo, zs, fs: setattr(zs[0], "key_begin", -3))
    refused("member range", lambda bi, bo, zs, fs: setattr(fs[0], "member_begin", -2))
    refused("too little room", lambda bi, bo, zs, fs: setattr(zs[1], "key_end", zs[1].key_end - 1))
    refused("too little room", lambda bi, bo, zs, fs: setattr(zs[1], "slot_end", zs[1].slot_end - 1))
    ctx.close()
