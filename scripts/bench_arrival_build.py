"""Time navhip_arrival_zone_build_dev (k_arrival_build + k_arrival_flock's first-build mode) with events around 20 calls
after 5, and the reference's own time for the same builds on one core: the seconds spent inside the exported N_* calls of
the first build (tests/test_arrival_build_cpu.py's Ref.seconds_in_the_reference; when oracle/_ref is present).  The
resident calls write to buffers of their own, so every call sees INACTIVE zones.
    (a) one zone at the 4 096-tile budget   (b) 64 zones of 25 members   (c) 256 zones of 25 members
Prints one JSON line per case."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from tests import arrival_build_model as abm  # noqa: E402
from tests import arrival_build_worlds as bw  # noqa: E402

F = np.float32


def build(n_zones, n_members, ur, rng):
    W = bw.World(2, 2)
    W.block([(int(r), int(c)) for r, c in rng.randint(0, 128, (300, 2))])
    for z in range(n_zones):
        r, c = (64, 64) if n_zones == 1 else (int(rng.randint(8, 120)), int(rng.randint(8, 120)))
        W.add("z%d" % z, W.p(r, c, rng.uniform(-1.9, 1.9, 2)), bw.crowd(W, min(r + 5, 124), c, n_members, seed=z), ur=ur)
    return W.done()


def timed(fn, side):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(side)
    for _ in range(20):
        fn()
    e1.record(side)
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000 / 20, 1)


def case(navlib, name, W):
    ctx = navlib.NavContext(W.w, W.h)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, W.cost[0])
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, W.blockers[0])
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    zs, slots, ring, kk = navlib._pack_zones(W.zones, [z["room_keys"] for z in W.zones])
    fs, cat = navlib.pack_flocks(W.zones, W.members)
    raw = lambda s: np.frombuffer(bytes(s), np.uint8).copy()                 # noqa: E731
    d_pos = t(W.pos)
    world, keep = navlib.make_world(W.w, W.h, {"pos_xz": d_pos})
    nz = len(W.zones)
    ins = {"zones": t(raw(zs)), "flocks": t(raw(fs)), "slots_xz": t(slots), "slot_ring": t(ring), "region_keys": t(kk.view(np.int64)),
           "target_xz": t(np.concatenate([W.targets, np.zeros((1, 2), F)]))}
    ins.update({k: t(v) for k, v in cat.items()})
    outs = {k: torch.zeros_like(ins[k]) for k in ("zones", "flocks", "slots_xz", "slot_ring", "region_keys", "substate", "sink_valid", "sink_xz")}
    outs.update(axis_xz=torch.zeros((nz, 2), device=dev), com_xz=torch.zeros((nz, 2), device=dev),
                com_dest_id=torch.zeros(nz, dtype=torch.int32, device=dev), status=torch.zeros(nz, dtype=torch.uint8, device=dev))
    bi, bo = navlib.ArrivalBuildIn(), navlib.ArrivalBuildOut()
    bi.n_zones, bi.nm, bi.n_slots, bi.n_keys = nz, len(cat["uid"]) - 1, len(ring) - 1, len(kk) - 1
    for k, v in ins.items():
        setattr(bi, k, v.data_ptr())
    for k, v in outs.items():
        setattr(bo, k, v.data_ptr())
    side = torch.cuda.Stream()
    res = {"case": name, "zones": nz, "members": bi.nm, "room_slots": bi.n_slots, "room_keys": bi.n_keys}
    res["dev_us_per_call"] = timed(lambda: ctx.arrival_zone_build_dev(world, bi, bo, side.cuda_stream), side)
    status = outs["status"].cpu().numpy()
    res["built"], res["host_rows"] = int((status == 0).sum()), int((status == abm.AB_HOST).sum())
    zo = (navlib.ArrivalZone * nz).from_buffer_copy(outs["zones"].cpu().numpy().tobytes())
    res["keys_out"], res["slots_out"] = sum(z.key_end - z.key_begin for z in zo), sum(z.slot_end - z.slot_begin for z in zo)
    ctx.close()
    from oracle import pfref
    if pfref.available():
        from tests import test_arrival_build_cpu as ref
        R = ref.Ref(W)
        for i, z in enumerate(W.zones):
            total, ur = z["arg_total_members"], z["arg_unit_radius"]
            area = abm.region_area(abm.afm.zone_radius(total, ur))
            centre = R.closest_pathable(0, W.targets[i])
            flood = R.connected(0, centre, area)
            keys = R.keys(flood)
            axis = abm.approach_axis(W.pos, W.members[i], W.targets[i])
            thinned, _, _ = abm.thin(flood, centre, axis, total, F(F(1.85) * ur))
            kept = [s for s in thinned if R.segment(centre, s, keys)]
            com = R.closest_pathable(0, abm.centre_of_mass(np.array(kept, F).reshape(-1, 2)))
            R.dest_id(com, 0)
        res["reference_nav_calls_us_one_core"] = round(R.seconds_in_the_reference * 1e6, 1)      # the N_* calls only, all zones
        R.close()
    return res


def main():
    ge.build_navhip()
    from permafrost_engine_amd import navhip as navlib
    torch.cuda.init()
    rng = np.random.RandomState(2)
    for name, (nz, nm, ur) in (("a", (1, 4, 64.0)), ("b", (64, 25, 1.0)), ("c", (256, 25, 1.0))):
        print(json.dumps(case(navlib, name, build(nz, nm, ur, rng))), flush=True)


if __name__ == "__main__":
    main()
