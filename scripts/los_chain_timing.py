"""What a resident LOS chain costs on the device (navhip_los_chain_*, csrc/los_chain_api.hip), in isolation: HIP events
around ONE call on an otherwise idle stream, the median of `--calls` calls (with the smallest and the largest).

    python scripts/los_chain_timing.py [--calls 50] [--map 16 --fields 64 --obstacles 10000]

The world is configs[4]'s -- configs[2]'s map, destinations and planner LOS chain (16 384 slots) under 10 000 obstacles --
so that one tick of its obstacle stream can be applied:
  (i)   refresh with no chunk flagged changed: what every tick with a chain pays (the mark launch + one launch per level
        whose blocks all end at once);
  (ii)  refresh behind one tick of the obstacle stream, both modes, with the fields it rebuilds.  The changed-chunk flags
        are left standing between the calls, so every call rebuilds the same set;
  (iii) build of the whole chain, against the per-level loop tick.py runs at start-up (_build_los_pool: one
        navhip_build_los_dev per level from an index_select copy of the predecessors).  That loop synchronises with the
        host between levels, so both are also timed with the host's clock around call + synchronise."""
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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--map", type=int, default=16)
    ap.add_argument("--fields", type=int, default=64)
    ap.add_argument("--obstacles", type=int, default=10_000)
    ap.add_argument("--agents", type=int, default=2_000, help="(the chain does not depend on them)")
    args = ap.parse_args()
    import torch
    from permafrost_engine_amd import navhip, tick
    if not tick.EMULATED and not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    Event = tick.tcuda.Event        # (HIP events; on the host emulator of tests/hostsim, a rehearsal, the host's clock)
    T = tick.NavTick(chunk_w=args.map, fields_per_rank=args.fields, agents_per_rank=args.agents, obstacles=args.obstacles,
                     obstacle_ticks=2, los=True, los_repair="downstream")
    if T.los_chain is None:
        raise SystemExit("no planner LOS fixture for this world")
    chain, s = T.los_chain, T.stream
    T.sync()

    def spread(ms):
        ms = sorted(ms)
        return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}

    def by_events(call, n=args.calls, warm=3):
        out = []
        for k in range(warm + n):
            e0, e1 = Event(enable_timing=True), Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            e1.synchronize()
            if k >= warm:
                out.append(e0.elapsed_time(e1))
        return spread(out)

    def by_host(call, n, warm=1):
        out = []
        for k in range(warm + n):
            T.sync()
            t0 = time.perf_counter()
            call()
            T.sync()
            if k >= warm:
                out.append((time.perf_counter() - t0) * 1e3)
        return spread(out)

    st0 = chain.stats()
    res = {"slots": st0.slots, "levels": st0.levels, "world": vars(args)}
    assert not T.ctx.changed_chunks(0).any()
    for name, flags in (("reference", 0), ("downstream", navhip.LOS_REFRESH_DOWNSTREAM)):
        res["refresh_nothing_changed_" + name] = by_events(lambda: chain.refresh(flags, stream=s.cuda_stream))
    assert chain.stats().rebuilt == st0.rebuilt
    # (iii) before the planes move: both builds give the pool that is there already
    before = T.los_pool.clone()
    res["build_chain"] = by_events(lambda: chain.build(stream=s.cuda_stream))
    assert torch.equal(before, T.los_pool)
    res["build_chain_host_clock"] = by_host(lambda: chain.build(stream=s.cuda_stream), 10)
    other = torch.zeros_like(T.los_pool)
    res["build_per_level_loop_host_clock"] = by_host(lambda: T._build_los_pool(other), 10)
    assert torch.equal(before, other)
    # (ii) one tick of the obstacle stream
    T.ctx.blockers_circles_dev(T.d_moves[0], T.n_moves, stream=s.cuda_stream)
    T.sync()
    res["changed_chunks"] = int(T.ctx.changed_chunks(0).sum())
    for name, flags in (("reference", 0), ("downstream", navhip.LOS_REFRESH_DOWNSTREAM)):
        r0 = chain.stats().rebuilt
        chain.refresh(flags, stream=s.cuda_stream)
        per_call = chain.stats().rebuilt - r0
        res["refresh_one_obstacle_tick_" + name] = dict(by_events(lambda: chain.refresh(flags, stream=s.cuda_stream)), rebuilt=per_call)
    T._build_los_pool(other)
    res["downstream_equals_fresh_build"] = bool(torch.equal(other, T.los_pool))
    T.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
