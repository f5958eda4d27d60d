"""Time navhip_arrival_velocity_dev (k_arrival_velocity, the dense output form) with events around 20 calls after 5, for
64 units in 8 zones and for 1 000 units in 50 zones of about 300 slots; prints one JSON line per case.  Synthetic zones on an
open 4 x 4 map: square footprints, a slot on three tiles in four, units of every substate in and around them."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

W = H = 4
F = np.float32


def xz(r, c):
    return F(W * 128.0) - F(4 * c + 2), F(-H * 128.0) + F(4 * r + 2)


def case(navlib, ctx, n_zones, n_units, side, rng):
    zones, keys = [], []
    per_row = (W * 64 - 8) // (side + 4)
    for z in range(n_zones):
        r0, c0 = 4 + (z // per_row) * (side + 4), 4 + (z % per_row) * (side + 4)
        tiles = [(r0 + i // side, c0 + i % side) for i in range(side * side)]
        slots = np.array([xz(r, c) for r, c in tiles if rng.rand() < 0.75], F).reshape(-1, 2)
        zones.append({"layer": 0, "centre_xz": xz(r0 + side // 2, c0 + side // 2), "radius": side // 2, "unit_radius": 1.0,
                      "fill_frac": 0.5, "active_row": 1, "num_rows": 4, "slots_xz": slots,
                      "slot_ring": rng.randint(0, 4, len(slots)).astype(np.int32)})
        keys.append(np.array(sorted(((r >> 6) << 48) | ((c >> 6) << 32) | ((r & 63) << 16) | (c & 63) for r, c in tiles), np.uint64))
    zs, slots, ring, kk = navlib._pack_zones(zones, keys)
    zone = rng.randint(0, n_zones, n_units).astype(np.int32)
    centre = np.array([zones[z]["centre_xz"] for z in zone], F)
    pos = np.clip(centre + rng.normal(0, side * 2.5, (n_units, 2)), -W * 128 + 8, W * 128 - 8).astype(F)
    sink = np.array([zones[z]["slots_xz"][rng.randint(len(zones[z]["slots_xz"]))] for z in zone], F)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    pool = rng.randint(0, 9, (2 * W * H, 4096)).astype(np.uint8)
    com = np.tile(np.arange(W * H, dtype=np.int32), (n_zones, 1))
    reg = np.tile(np.arange(W * H, 2 * W * H, dtype=np.int32), (n_zones, 1))
    d = {"pos_xz": t(pos), "flock_field_slot": t(com), "region_field_slot": t(reg), "field_pool": t(pool)}
    world, keep = navlib.make_world(W, H, d)
    world.n_flocks = n_zones
    vi, vo = navlib.ArrivalVelIn(), navlib.ArrivalVelOut()
    vi.n_zones, vi.nq, vi.n_slots, vi.n_keys = n_zones, n_units, len(ring) - 1, len(kk) - 1
    rows = np.arange(n_zones, dtype=np.int32)
    ins = {"zones": t(np.frombuffer(bytes(zs), np.uint8).copy()), "slots_xz": t(slots), "slot_ring": t(ring),
           "region_keys": t(kk.view(np.int64)), "zone_row": t(rows), "com_row": t(rows), "uid": t(np.arange(n_units, dtype=np.int32)),
           "zone": t(zone), "has_dest_los": t(rng.randint(0, 2, n_units).astype(np.uint8)),
           "substate": t(rng.randint(0, 4, n_units).astype(np.uint8)), "sink_valid": t((rng.rand(n_units) < 0.7).astype(np.uint8)),
           "sink_xz": t(sink), "los_latched": t(rng.randint(0, 2, n_units).astype(np.uint8)),
           "los_hyst": t(rng.randint(0, 12, n_units).astype(np.int32))}
    outs = {"status": torch.zeros(n_units, dtype=torch.uint8, device=dev), "substate": torch.zeros(n_units, dtype=torch.uint8, device=dev),
            "sink_valid": torch.zeros(n_units, dtype=torch.uint8, device=dev), "sink_xz": torch.zeros((n_units, 2), device=dev),
            "los_latched": torch.zeros(n_units, dtype=torch.uint8, device=dev),
            "los_hyst": torch.zeros(n_units, dtype=torch.int32, device=dev),
            "dense_vdes_xz": torch.full((n_units, 2), float("nan"), device=dev)}
    for k, v in ins.items():
        setattr(vi, k, v.data_ptr())
    for k, v in outs.items():
        setattr(vo, k, v.data_ptr())
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        ctx.arrival_velocity_dev(world, vi, vo, stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        ctx.arrival_velocity_dev(world, vi, vo, stream)
    e1.record()
    torch.cuda.synchronize()
    st = outs["status"].cpu().numpy()
    return {"zones": n_zones, "units": n_units, "slots_per_zone": int(len(ring) - 1) // n_zones, "us_per_call": round(e0.elapsed_time(e1) * 1000 / 20, 2),
            "decided": int((st == 0).sum()), "com_miss": int((st == 1).sum()), "host": int((st == 0x80).sum())}


def main():
    ge.build_navhip()
    from permafrost_engine_amd import navhip as navlib
    torch.cuda.init()
    ctx = navlib.NavContext(W, H)
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, np.ones((H, W, 64, 64), np.uint8))
    ctx.upload_plane(0, navlib.PLANE_BLOCKERS, (np.random.RandomState(1).rand(H, W, 64, 64) < 0.05).astype(np.uint16))
    rng = np.random.RandomState(2)
    for n_zones, n_units, side in ((8, 64, 8), (50, 1000, 20)):
        print(json.dumps(case(navlib, ctx, n_zones, n_units, side, rng)))
    ctx.close()


if __name__ == "__main__":
    main()
