#!/usr/bin/env python3
"""navhip_build_fields_dev alone on one stream, at the benchmark's size (16 x 16 chunks, 64 destinations: 16 384 requests):

  planner_list    the benchmark's request list as it is: each distinct record about nine times over
  no_duplicates   the same list with _pad = the request's index: 16 384 records of which no two are equal, the work of every
                  one unchanged -- what a caller sends whose own cache is keyed by field id.  Here the classing pass
                  (k_field_classes + the reset of its table) is pure overhead: compare against the parent library
                  (NAVHIP_LIB) to read it off.

Prints one JSON object; times are per build, from events on the build's stream."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge            # noqa: E402
ge.build_navhip()
from permafrost_engine_amd import navhip, synth   # noqa: E402


def main():
    import torch
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    W, K, reps = 16, 64, 20
    grid = synth.cost_grid(W, W, seed=1234)
    dests = synth.destinations(grid, K, seed=42)
    ctx = navhip.NavContext(W, W)
    ctx.upload_plane(0, navhip.PLANE_COST_BASE, synth.to_chunks(grid))
    ctx.upload_plane(0, navhip.PLANE_BLOCKERS, np.zeros((W, W, 64, 64), np.uint16))
    ctx.relabel_local_islands(0)
    cols = synth.planner_requests(grid, dests)
    if cols is None:
        cols = synth.whole_map_requests(grid, dests, synth.from_chunks(ctx.download_plane(0, navhip.PLANE_LOCAL_ISLANDS)))
    reqs = navhip.make_reqs(len(cols["type"]))
    for k in synth.REQ_FIELDS:
        reqs[k] = cols[k]
    n = len(reqs)
    unique = reqs.copy()
    unique["_pad"] = np.arange(n)
    assert n <= 65536 and len(np.unique(unique)) == n
    pool = torch.zeros((n, 4096), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    out = {"requests": n, "distinct_records": int(len(np.unique(reqs))), "reps": reps,
           "library": os.path.basename(os.environ.get("NAVHIP_LIB", "")) or "libnavhip.so (in-tree)"}
    fields = {}
    for name, r in (("planner_list", reqs), ("no_duplicates", unique)):
        d_reqs = torch.from_numpy(r.view(np.uint8).reshape(n, 32).copy()).to(dev)
        torch.cuda.synchronize()
        times = []
        for k in range(reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            ctx.build_fields_dev(d_reqs, n, pool, stream=st.cuda_stream)
            e1.record(st)
            st.synchronize()
            if k >= 3:
                times.append(e0.elapsed_time(e1))
        out[name] = {"ms_min": min(times), "ms_median": float(np.median(times)), "ms_max": max(times),
                     "split_bfs_generic": list(ctx.last_fields_split())}
        fields[name] = pool.clone()
    assert torch.equal(fields["planner_list"], fields["no_duplicates"])
    ctx.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
