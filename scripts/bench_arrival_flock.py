"""Time navhip_arrival_flock_update (host buffers) and navhip_arrival_flock_update_dev (k_arrival_flock) with events around
20 calls after 5, every zone at its fourth call, once with every zone re-orienting (fill_frac 0) and once frozen
(fill_frac 0.5); for the frozen case also the reference's G_Arrival_UpdateFlock on one core over the same zones (when
oracle/_ref is present).  The resident calls write to buffers of their own, so every call sees the same input.
    (a) 8 zones x 64 members x 64 slots   (b) 50 zones x 300 members x 300 slots, 1 200 keys   (c) one zone of 1 563
    members and slots at the key cap.  Prints one JSON line per case."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from tests import arrival_flock_worlds as aw  # noqa: E402

W = H = 4
F = np.float32


def build(n_zones, n_members, n_slots, rows, cols, frozen, rng):
    Wd = aw.World(W, H)
    for z in range(n_zones):
        # (footprints may overlap: zones are independent of each other)
        r0, c0 = 4 + (z * 29) % (W * 64 - rows - 8), 4 + (z * 53) % (W * 64 - cols - 8)
        tiles = aw.rect(r0, c0, rows, cols)
        pick = rng.permutation(len(tiles))[:n_slots]
        slots = np.array([aw.xz(W, H, *tiles[i], rng.uniform(-1.5, 1.5, 2)) for i in pick], F)
        nrows = 6
        zone = aw.zone(W, H, tiles, slots, fill=0.5 if frozen else 0.0, rings=rng.randint(0, nrows, n_slots) if frozen else None,
                       num_rows=nrows if frozen else 1, active_row=2 if frozen else 0, row_height=F(8.0), total=n_members)
        Wd.block([tiles[i] for i in pick[::17]], 0)
        Wd.add(zone, aw.crowd(Wd, rng, tiles, n_members, slots, p_settled=0.4, outside=0.1))
    return Wd.done()


def timed(fn, side, sync):
    """Events on `side`, the stream the resident calls run on (the host form waits for its own stream: wall clock)."""
    for _ in range(5):
        fn()
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(side)
    for _ in range(20):
        fn()
    e1.record(side)
    sync()
    wall = (time.perf_counter() - t0) * 1e6 / 20
    return round(e0.elapsed_time(e1) * 1000 / 20, 1), round(wall, 1)


def case(navlib, name, Wd, frozen):
    ctx = navlib.NavContext(W, H)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, np.ones((H, W, 64, 64), np.uint8))
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, Wd.blockers[0])
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    zs, slots, ring, kk = navlib._pack_zones(Wd.zones, Wd.keys)
    fs, cat = navlib.pack_flocks(Wd.zones, Wd.members)
    raw = lambda s: np.frombuffer(bytes(s), np.uint8).copy()                 # noqa: E731
    d_pos = t(Wd.pos)
    world, keep = navlib.make_world(W, H, {"pos_xz": d_pos})
    ins = {"zones": t(raw(zs)), "flocks": t(raw(fs)), "slots_xz": t(slots), "slot_ring": t(ring), "region_keys": t(kk.view(np.int64))}
    ins.update({k: t(v) for k, v in cat.items()})
    outs = {k: torch.zeros_like(ins[k]) for k in ("zones", "flocks", "slot_ring", "substate", "sink_valid", "sink_xz")}
    outs["status"] = torch.zeros(len(Wd.zones), dtype=torch.uint8, device=dev)
    fi, fo = navlib.ArrivalFlockIn(), navlib.ArrivalFlockOut()
    fi.n_zones, fi.nm, fi.n_slots, fi.n_keys = len(Wd.zones), len(cat["uid"]) - 1, len(ring) - 1, len(kk) - 1
    for k, v in ins.items():
        setattr(fi, k, v.data_ptr())
    for k, v in outs.items():
        setattr(fo, k, v.data_ptr())
    side = torch.cuda.Stream()                                               # (a stream of its own: 0 would mean the context's)
    stream = side.cuda_stream
    res = {"case": name, "frozen": frozen, "zones": len(Wd.zones), "members": fi.nm, "slots": fi.n_slots, "keys": fi.n_keys}
    torch.cuda.synchronize()
    res["dev_us_per_call"], _ = timed(lambda: ctx.arrival_flock_update_dev(world, fi, fo, stream), side, torch.cuda.synchronize)
    _, res["host_form_wall_us_per_call"] = timed(lambda: ctx.arrival_flock_update({"pos_xz": Wd.pos}, Wd.zones, Wd.keys, Wd.members), side,
                                                 torch.cuda.synchronize)
    res["host_rows"] = int((outs["status"].cpu().numpy() != 0).sum())
    ctx.close()
    from oracle import pfref
    if frozen and pfref.available():
        from tests import test_arrival_flock_cpu as ref
        R = ref.Ref(Wd)
        for z, keys, mem in zip(Wd.zones, Wd.keys, Wd.members):
            R.update(z, keys, Wd.pos, mem)
        res["reference_us_one_core"] = round(R.seconds_in_the_reference * 1e6, 1)    # inside G_Arrival_UpdateFlock only, all zones
        R.close()
    return res


def main():
    ge.build_navhip()
    from permafrost_engine_amd import navhip as navlib
    torch.cuda.init()
    rng = np.random.RandomState(2)
    for name, (nz, nm, ns, rows, cols) in (("a", (8, 64, 64, 10, 10)), ("b", (50, 300, 300, 30, 40)), ("c", (1, 1563, 1563, 64, 64))):
        for frozen in (False, True):
            print(json.dumps(case(navlib, name, build(nz, nm, ns, rows, cols, frozen, rng), frozen)), flush=True)


if __name__ == "__main__":
    main()
