#!/usr/bin/env python3
"""What the order-time nav queries cost on the device (navhip_order_queries_dev, csrc/order_query_kernels.hip) against the
reference's own calls for the same rows on one core of this machine's CPU (oracle/_ref through ctypes: N_LocationsReachable,
N_ClosestReachableInRange, N_ClosestReachableDest, N_DestIDForPos), timed around the calls only.

    python scripts/bench_order_queries.py [--rows 10000] [--calls 20]
    rocprofv3 --kernel-trace --stats -d <dir> -o oq --output-format csv -- python scripts/bench_order_queries.py

The world is configs[2]'s of bench.py (16 x 16 chunks, 1024 x 1024 cells).  Three batches of --rows rows each:
    reachable   NAVHIP_OQ_REACHABLE, a third of the clicks on impassable ground (off the source's island)
    in_range    NAVHIP_OQ_IN_RANGE | NAVHIP_OQ_REACHABLE, ranges 20 .. 60
    range_120   NAVHIP_OQ_IN_RANGE | NAVHIP_OQ_REACHABLE, range 120 (a box of 61 x 61 tiles, above the 2048-tile cap)
The device call is timed with events around one call on an idle stream (the median of --calls).  The reference loop holds
its arguments ready and runs three times; the best is the loop without cold caches.  The answers are compared, bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--map", type=int, default=16)
    args = ap.parse_args()
    import torch
    from oracle import pfref
    from permafrost_engine_amd import navhip, synth, tick
    from tests.test_order_queries_cpu import Vec3, _lib, v2
    if not tick.EMULATED and not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    Event = tick.tcuda.Event
    T = tick.NavTick(chunk_w=args.map, fields_per_rank=64, agents_per_rank=2_000)
    ctx, s, W, n = T.ctx, T.stream, args.map, args.rows
    nav = pfref.RefNav(synth.to_chunks(T.grid))
    ctx.upload_plane(0, navhip.PLANE_ISLANDS, nav.plane(pfref.PLANE_ISLANDS, 0))
    L, priv, mp = _lib(), _lib().pfref_nav_private(nav._h), Vec3(*[float(v) for v in nav.map_pos])
    rng = np.random.RandomState(77)
    free = np.argwhere(T.grid != 255)
    walls = np.argwhere(T.grid == 255)
    pick = lambda cells, k: synth.cell_centre(W, W, *cells[rng.randint(len(cells), size=k)].T).astype(np.float32)    # noqa: E731
    res = {"world": {"map": W, "cells": int(T.grid.size), "impassable": int(len(walls))}, "rows": n, "calls": args.calls}
    batches = {"reachable": (navhip.OQ_REACHABLE, None), "in_range": (navhip.OQ_IN_RANGE | navhip.OQ_REACHABLE, (20.0, 60.0)),
               "range_120": (navhip.OQ_IN_RANGE | navhip.OQ_REACHABLE, (120.0, 120.0))}
    for name, (flags, ranges) in batches.items():
        q = np.zeros(n, navhip.ORDER_QUERY_DTYPE)
        src, dst = pick(free, n), pick(free, n)
        if ranges is None:
            off = rng.rand(n) < 1.0 / 3.0
            dst[off] = pick(walls, int(off.sum()))
        else:
            q["range"] = rng.uniform(ranges[0], ranges[1], n).astype(np.float32)
        q["src_x"], q["src_z"], q["dst_x"], q["dst_z"] = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
        q["faction"], q["flags"] = navhip.FACTION_NONE, flags
        d_q = torch.from_numpy(q.view(np.uint8).reshape(n, 32)).to(T.dev)
        d_dest = torch.zeros((n, 2), dtype=torch.float32, device=T.dev)
        d_id = torch.zeros(n, dtype=torch.int32, device=T.dev)
        d_status = torch.zeros(n, dtype=torch.uint8, device=T.dev)
        T.sync()
        ms = []
        for k in range(3 + args.calls):
            e0, e1 = Event(enable_timing=True), Event(enable_timing=True)
            e0.record(s)
            ctx.order_queries_dev(d_q, n, d_dest, d_id, d_status, stream=s.cuda_stream)
            e1.record(s)
            e1.synchronize()
            if k >= 3:
                ms.append(e0.elapsed_time(e1))
        # the reference: the same rows, one core, the arguments made beforehand
        a = [(v2(src[i]), v2(dst[i]), float(q["range"][i])) for i in range(n)]
        host, stage = [], {}
        for _ in range(3):
            out = np.zeros((n, 2), np.float32)
            ids, same_island = np.zeros(n, np.uint32), np.zeros(n, bool)
            t_in, t_re, t_rest = 0.0, 0.0, 0.0
            for i, (vs, vd, r) in enumerate(a):
                t0 = time.perf_counter()
                same_island[i] = L.N_LocationsReachable(priv, 0, mp, vs, vd)
                t1 = time.perf_counter()
                t = L.N_ClosestReachableInRange(priv, mp, vs, vd, r, 0) if flags & navhip.OQ_IN_RANGE else vd
                t2 = time.perf_counter()
                d = L.N_ClosestReachableDest(priv, 0, mp, vs, t)
                t3 = time.perf_counter()
                ids[i] = L.N_DestIDForPos(priv, mp, d, 0)
                t4 = time.perf_counter()
                out[i] = (d.x, d.z)
                t_in, t_re, t_rest = t_in + (t2 - t1), t_re + (t3 - t2), t_rest + (t1 - t0) + (t4 - t3)
            host.append((t_in + t_re + t_rest) * 1e3)
            if host[-1] == min(host):
                stage = {"in_range_ms": round(t_in * 1e3, 3), "reachable_ms": round(t_re * 1e3, 3), "rest_ms": round(t_rest * 1e3, 3)}
        got, got_id, status = d_dest.cpu().numpy(), d_id.cpu().numpy().view(np.uint32), d_status.cpu().numpy()
        done = status != navhip.OQ_HOST
        equal = np.array_equal(got[done].view(np.uint32), out[done].view(np.uint32)) and np.array_equal(got_id[done], ids[done]) \
            and np.array_equal((status[done] & navhip.OQ_SAME_ISLAND) != 0, same_island[done])
        res[name] = {"device_call_ms_median": round(float(np.median(ms)), 4), "device_call_ms_min": round(min(ms), 4),
                     "device_call_ms_max": round(max(ms), 4), "reference_loop_ms_best": round(min(host), 3),
                     "reference_loop_ms_all": [round(h, 3) for h in host], "reference_stages_of_best": stage,
                     "rows_left_to_host": int((~done).sum()), "rows_moved": int((got[done] != dst[done]).any(1).sum()),
                     "rows_no_tile": int(((status & navhip.OQ_NO_TILE) != 0)[done].sum()), "answers_equal": bool(equal)}
    T.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
