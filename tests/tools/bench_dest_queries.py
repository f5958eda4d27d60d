"""What the destination queries cost (navhip_dest_queries_dev, csrc/dest_query_kernels.hip) against the host loop they
replace: the reference's N_ClosestPathable + n_closest_island_tiles per destination, through oracle.pfref, on this
machine's CPU.

    python tests/tools/bench_dest_queries.py [--calls 30]
    rocprofv3 --kernel-trace --stats -d <dir> -o dq --output-format csv -- python tests/tools/bench_dest_queries.py

The world is configs[2]'s of bench.py (16 x 16 chunks, 64 flow-field destinations) under configs[4]'s 10 000 obstacles,
queried right behind one batch of its obstacle stream: F = 64 (the world's own flock destinations) and F = 1 024
(destinations drawn the same way).  The device call is timed with HIP events around one call on an idle stream (the
median of --calls; under rocprofv3 the kernel times are in its statistics, by kernel name); the host loop with the host's
clock, ctypes call overhead included (a few microseconds against the tens a query takes).  The answers are compared too."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--map", type=int, default=16)
    ap.add_argument("--obstacles", type=int, default=10_000)
    args = ap.parse_args()
    import torch
    from oracle import pfref
    from permafrost_engine_amd import navhip, synth, tick
    if not tick.EMULATED and not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    Event = tick.tcuda.Event
    T = tick.NavTick(chunk_w=args.map, fields_per_rank=64, agents_per_rank=2_000, obstacles=args.obstacles, obstacle_ticks=2)
    ctx, s, W = T.ctx, T.stream, args.map
    nav = pfref.RefNav(synth.to_chunks(T.grid))
    ctx.upload_plane(0, navhip.PLANE_ISLANDS, nav.plane(pfref.PLANE_ISLANDS, 0))
    # one batch of the obstacle stream, then the queries: the reference works on the planes the batch left
    ctx.blockers_circles_dev(T.d_moves[0], T.n_moves, stream=s.cuda_stream)
    T.sync()
    nav.set_blockers(ctx.download_plane(0, navhip.PLANE_BLOCKERS), 0)
    res = {"world": {"map": W, "obstacles": args.obstacles, "moves_in_batch": int(T.n_moves)}, "calls": args.calls}
    own = T.t["flock_target_xz"].cpu().numpy()
    more = synth.destinations(T.grid, 1024, seed=4242)
    for F, targets in ((64, own), (1024, synth.cell_centre(W, W, more[:, 0], more[:, 1]))):
        assert len(targets) == F
        q = np.zeros(F, navhip.DEST_QUERY_DTYPE)
        q["x"], q["z"], q["flags"] = targets[:, 0], targets[:, 1], navhip.DQ_NEAREST | navhip.DQ_TILES
        d_q = torch.from_numpy(q.view(np.uint8).reshape(F, 16)).to(T.dev)
        d_nearest = torch.zeros((F, 2), dtype=torch.float32, device=T.dev)
        d_off = torch.zeros(F + 1, dtype=torch.int32, device=T.dev)
        d_tiles = torch.zeros((navhip.DQ_MAX_TILES * F, 2), dtype=torch.int16, device=T.dev)
        d_status = torch.zeros(F, dtype=torch.uint8, device=T.dev)
        T.sync()
        call = lambda: ctx.dest_queries_dev(d_q, F, d_nearest, d_off, d_tiles, navhip.DQ_MAX_TILES * F, d_status,   # noqa: E731
                                            stream=s.cuda_stream)
        ms = []
        for k in range(3 + args.calls):
            e0, e1 = Event(enable_timing=True), Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            e1.synchronize()
            if k >= 3:
                ms.append(e0.elapsed_time(e1))
        # the host loop, three times: the best is the loop without cold caches
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref = [(nav.closest_pathable(t), nav.dest_island_tiles(t)) for t in targets]
            host.append((time.perf_counter() - t0) * 1e3)
        off, status = d_off.cpu().numpy(), d_status.cpu().numpy()
        got_nearest, got_tiles = d_nearest.cpu().numpy(), d_tiles.cpu().numpy()
        same = True
        for i, (p, tl) in enumerate(ref):
            if status[i]:
                continue
            exp = np.array([np.nan, 0.0], np.float32) if p is None else p
            same = same and np.array_equal(got_nearest[i].view(np.uint32), exp.view(np.uint32)) \
                and np.array_equal(got_tiles[off[i]:off[i + 1]], tl)
        res["F%d" % F] = {"device_call_ms_median": round(float(np.median(ms)), 4), "device_call_ms_min": round(min(ms), 4),
                          "device_call_ms_max": round(max(ms), 4), "host_loop_ms_best": round(min(host), 3),
                          "host_loop_ms_all": [round(h, 3) for h in host], "rows_left_to_host": int((status != 0).sum()),
                          "blocked_targets": int(sum(p is None or not np.array_equal(p, t) for (p, _), t in zip(ref, targets))),
                          "tiles": int(off[-1]), "answers_equal": bool(same)}
    T.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
