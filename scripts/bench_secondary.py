#!/usr/bin/env python3
"""The kernels outside the headline tick at a size that matters, for `rocprofv3 --kernel-trace --stats`
(scripts/gpu_job.sh <tag> secondary -> profiles/archive/r03_secondary_kernel_stats_*.csv) and as wall-clock rates:

  k_field_generic     16 384 chunk fields on a map whose passable cells cost 1..4 (the BFS kernel declines
                      every chunk: all requests take the LDS relaxation), device resident
  k_region_field      256 enemy-seek style jobs (128 x 128 padded region -> 64 x 64 window, ~40 seeds each):
                      one asynchronous field batch of the reference (MAX_FIELD_TASKS, nav.c:88)
  k_blockers_circles  10 000 circles (configs[4]'s obstacle count) + k_refresh_touched + k_local_islands
  k_local_islands     the relabel of every chunk of the map
  k_los_field         4 096 destination-chunk LOS fields
  field_attacking     the 16 384 chunk fields of the benchmark map as ATTACKING paths (faction 0 at war with faction 1)
                      on a map held by 4 000 units of three factions: k_field_bfs (mode 0), k_field_generic (mode 1)
                      and the same requests without a faction, with navhip_last_fields_split beside each; and the
                      blocker update of 10 000 circles with a resident factions plane (k_refresh_touched keeps the
                      faction rows current)
  k_region_repair     64 and 256 nearest-pathable repairs of cell arrival fields (dim 96) on a map with blocked blobs, per
                      call: the resident form, the host-buffer form, and the round trip of the slots that a host-side
                      repair would need instead.  The reference's own time for the same requests on one core:
                      tests/tools/bench_region_repair.py
  seek_fields         256 enemy-seek jobs (kind 0) on the configs[2] map with 100 000 entities of 3 factions, per call:
                      navhip_build_seek_fields_dev with events round the call; its field part as navhip_build_region_fields_dev
                      replayed on the very seed lists (uploaded once, events round it), the seed part as the difference; the
                      parent's route for the grid half, navhip_build_region_fields fed by uploaded seeds (host buffers); and,
                      where oracle/_ref is present, the reference's async batch of the same jobs all on the CPU and with the
                      binding on (N_HIP_RegionRequest: the frontier extraction on the host, then one region build on the
                      device) -- the binding's batch less the parent's region call is the host's seed extraction
Prints one JSON object."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge            # noqa: E402
ge.build_navhip()
from permafrost_engine_amd import navhip, synth   # noqa: E402


def timed(fn, reps=5):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def field_attacking(torch, dev):
    """Chunk fields with a faction against the same requests without one, and against the generic kernel."""
    W, K = 16, 64
    grid = synth.cost_grid(W, W, seed=1234)
    dests = synth.destinations(grid, K, seed=42)
    ctx = navhip.NavContext(W, W)
    ctx.upload_plane(0, navhip.PLANE_COST_BASE, synth.to_chunks(grid))
    ctx.upload_plane(0, navhip.PLANE_BLOCKERS, np.zeros((W, W, 64, 64), np.uint16))
    ctx.upload_plane(0, navhip.PLANE_FACTIONS, np.zeros((W, W, 15, 64, 64), np.uint8))
    ctx.relabel_local_islands(0)
    cols = synth.planner_requests(grid, dests)             # the benchmark's request fixture
    if cols is None:
        cols = synth.whole_map_requests(grid, dests, synth.from_chunks(ctx.download_plane(0, navhip.PLANE_LOCAL_ISLANDS)))
    plain = navhip.make_reqs(len(cols["type"]))
    for k in synth.REQ_FIELDS:
        plain[k] = cols[k]
    attack = plain.copy()
    attack["faction_id"], attack["enemies"] = 0, 0b010
    c = synth.faction_circles(grid, 4000, seed=11)
    circ = np.zeros(4000, navhip.CIRCLE_DTYPE)
    for k in ("x", "z", "radius", "faction_id"):
        circ[k] = c[k]
    circ["delta"] = 1
    ctx.N_BlockersUpdate(circ)
    pool = torch.zeros((len(plain), 4096), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)
    has_split = hasattr(navhip.lib(), "navhip_last_fields_split")        # (an A/B build of an older revision)
    res = {"chunk_fields": len(plain), "circles": len(circ), "what": "faction 0, enemies 0b010; 1024x1024 map, three factions"}
    fields = {}
    for name, reqs, mode, reps in (("attack_mode0", attack, 0, 10), ("attack_mode1", attack, 1, 3), ("plain_mode0", plain, 0, 10),
                                   ("attack_mode0_again", attack, 0, 10)):
        d_reqs = torch.from_numpy(reqs.view(np.uint8).reshape(len(reqs), 32)).to(dev)
        ctx.set_field_kernel(mode)

        def run():
            ctx.build_fields_dev(d_reqs, len(reqs), pool, stream=st.cuda_stream)
            st.synchronize()
        t = timed(run, reps=reps)
        res[name] = {"ms": t * 1e3, "split_bfs_generic": list(ctx.last_fields_split()) if has_split else None}
        fields[name] = pool.clone()
    ctx.set_field_kernel(0)
    assert torch.equal(fields["attack_mode0"], fields["attack_mode1"]) and torch.equal(fields["attack_mode0"], fields["attack_mode0_again"])
    res["attack_fields_differing_from_plain"] = int((fields["attack_mode0"] != fields["plain_mode0"]).any(1).sum().item())
    res["attack_mode0_over_plain_mode0"] = res["attack_mode0"]["ms"] / res["plain_mode0"]["ms"]
    res["attack_mode1_over_mode0"] = res["attack_mode1"]["ms"] / res["attack_mode0"]["ms"]

    # the blocker update with faction counters: 10 000 circles in, the same out
    rng = np.random.RandomState(5)
    cells = synth.passable_cells(grid)
    pos = synth.cell_centre(W, W, *cells[rng.randint(len(cells), size=10_000)].T)
    big = np.zeros(10_000, navhip.CIRCLE_DTYPE)
    big["x"], big["z"] = pos[:, 0], pos[:, 1]
    big["radius"] = rng.uniform(2.0, 6.0, 10_000)
    big["faction_id"] = rng.randint(0, 3, 10_000)
    undo = big.copy()
    big["delta"], undo["delta"] = 1, -1

    def blk():
        ctx.N_BlockersUpdate(big)
        ctx.N_BlockersUpdate(undo)
    t = timed(blk, reps=5)
    res["blockers_circles_with_factions"] = {"circles_per_call": 10_000, "ms_per_call_host_api": t * 1e3 / 2}
    ctx.close()
    return res


def region_repair(torch, dev):
    """navhip_repair_region_fields[_dev] per call against the transfers of a repair on the host."""
    from tests.tools import bench_region_repair as brr
    res = {"what": "dim %d, %d x %d chunks, 400 blocked blobs; requests of tests/tools/bench_region_repair.py" % (brr.DIM, brr.MAP, brr.MAP)}
    stride = brr.DIM * brr.DIM // 2
    for n in (64, 256):
        cases = brr.world(n)
        ctx = navhip.NavContext(brr.MAP, brr.MAP)
        ctx.upload_plane(0, navhip.PLANE_COST_BASE, synth.to_chunks(cases[0]["cost"]))
        ctx.upload_plane(0, navhip.PLANE_BLOCKERS, synth.to_chunks(cases[0]["blk"]))
        reqs = np.zeros(n, navhip.REGION_REPAIR_REQ_DTYPE)
        reqs["dim"] = brr.DIM
        reqs["centre_abs_r"], reqs["centre_abs_c"] = np.array([c["centre"] for c in cases]).T
        reqs["start_abs_r"], reqs["start_abs_c"] = np.array([c["start"] for c in cases]).T
        fields = np.random.RandomState(1).randint(0, 256, (n, stride)).astype(np.uint8)
        d_reqs = torch.from_numpy(reqs.view(np.uint8).reshape(n, 20)).to(dev)
        d_io = torch.from_numpy(fields).to(dev)
        d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(device=dev)
        pinned = torch.empty((n, stride), dtype=torch.uint8).pin_memory()

        def resident():
            ctx.repair_region_fields_dev(d_reqs, n, brr.DIM, None, d_io, stride, d_st, stream=st.cuda_stream)
            st.synchronize()

        def round_trip():
            with torch.cuda.stream(st):
                pinned.copy_(d_io, non_blocking=True)
                st.synchronize()                     # (the host's repair would run here)
                d_io.copy_(pinned, non_blocking=True)
            st.synchronize()
        res["n%d" % n] = {"ms_resident": timed(resident, reps=20) * 1e3,
                          "ms_host_api": timed(lambda: ctx.repair_region_fields(reqs, None, fields, stride), reps=10) * 1e3,
                          "ms_round_trip_of_the_slots_pinned": timed(round_trip, reps=20) * 1e3,
                          "host_rows": int((d_st.cpu().numpy() == navhip.RR_HOST).sum())}
        ctx.close()
    return res


def seek_fields(torch, dev):
    """navhip_build_seek_fields_dev against the host's seed extraction and the parent's region build."""
    W, n, nj = 16, 100_000, 256
    rng = np.random.RandomState(7)
    grid = synth.cost_grid(W, W, seed=1234)
    cells = synth.passable_cells(grid)
    pick = cells[rng.choice(len(cells), size=n, replace=False)]
    pos = (synth.cell_centre(W, W, pick[:, 0], pick[:, 1]) + rng.uniform(-1.5, 1.5, (n, 2))).astype(np.float32)
    radius = rng.choice([1.0, 1.0, 2.5, 4.0], size=n).astype(np.float32)
    faction = rng.randint(0, 3, n).astype(np.int32)
    flags = np.full(n, navhip.ENTITY_FLAG_MOVABLE | navhip.ENTITY_FLAG_COMBATABLE, np.uint32)
    flags[rng.rand(n) < 0.1] &= ~np.uint32(navhip.ENTITY_FLAG_COMBATABLE)
    masks = np.zeros(16, np.uint16)
    masks[:3] = (0b110, 0b001, 0b010)
    jobs = [(cr, cc, f) for cr in range(W) for cc in range(W) for f in range(3)]
    jobs = [jobs[i] for i in rng.choice(len(jobs), nj, replace=False)]                  # distinct: the reference builds a job once
    reqs = np.zeros(nj, navhip.SEEK_REQ_DTYPE)
    reqs["chunk_r"], reqs["chunk_c"], reqs["faction_id"] = np.array(jobs).T
    ctx = navhip.NavContext(W, W)
    ctx.upload_plane(0, navhip.PLANE_COST_BASE, synth.to_chunks(grid))
    ctx.upload_plane(0, navhip.PLANE_BLOCKERS, np.zeros((W, W, 64, 64), np.uint16))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)
    world, keep = navhip.make_world(W, W, {"pos_xz": t(pos), "radius": t(radius), "flags": t(flags.view(np.int32))})
    game, keep2 = navhip.make_seek_game(t(faction), masks)
    d_reqs = t(reqs.view(np.uint8).reshape(nj, 12))
    d_io = torch.zeros((nj, 4096), dtype=torch.uint8, device=dev)
    d_st = torch.zeros(nj, dtype=torch.uint8, device=dev)
    d_bits = torch.zeros((nj, 2048), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)

    def by_events(fn, reps=20):
        fn(); st.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st); fn(); b.record(st); st.synchronize()
            ms.append(a.elapsed_time(b))
        return {"ms_mean": float(np.mean(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}

    total = by_events(lambda: ctx.build_seek_fields_dev(world, game, d_reqs, nj, d_io, 4096, d_st, d_bits, stream=st.cuda_stream))
    status, fields = d_st.cpu().numpy(), d_io.cpu().numpy()
    bits = np.unpackbits(d_bits.cpu().numpy(), axis=1, bitorder="little").reshape(nj, 128, 128)
    # the same seed lists as the host would upload them
    rr = np.zeros(nj, navhip.REGION_REQ_DTYPE)
    seeds = []
    for j, (cr, cc, f) in enumerate(jobs):
        br, bc = ((cr - 1) * 64 + 32 if cr else 0), ((cc - 1) * 64 + 32 if cc else 0)
        sd = np.argwhere(bits[j]) + (br, bc)
        rr[j] = (0, 1, 0, br, bc, 128, 128, 32 if cr else 0, 32 if cc else 0, sum(len(x) for x in seeds), len(sd), 0, 0)
        seeds.append(sd.astype(np.int16))
    seeds = np.concatenate(seeds)
    d_rr, d_seeds = t(rr.view(np.uint8).reshape(nj, 32)), t(seeds)
    d_io2 = torch.zeros((nj, 4096), dtype=torch.uint8, device=dev)
    part = by_events(lambda: ctx.build_region_fields_dev(d_rr, nj, 128, d_seeds, None, d_io2, 4096, stream=st.cuda_stream))
    assert np.array_equal(d_io2.cpu().numpy(), fields)
    zeros = np.zeros((nj, 4096), np.uint8)
    parent = timed(lambda: ctx.build_region_fields(rr, seeds, inout=zeros, out_stride=4096), reps=10) * 1e3
    res = {"what": "256 distinct kind-0 jobs, layer 0, 1024x1024 map (configs[2]), 100 000 entities, 3 factions, radii 1 / 2.5 / 4",
           "host_rows": int((status != 0).sum()), "seeds_per_job_mean": float(bits.reshape(nj, -1).sum(1).mean()),
           "fields_not_trivial": int(fields.any(1).sum()),
           "seek_fields_dev_events": total, "field_part_events": part,
           "seed_part_ms_mean_by_difference": total["ms_mean"] - part["ms_mean"],
           "parent_region_fields_host_api_ms": parent, "seed_upload_bytes": int(seeds.nbytes)}
    ctx.close()
    from oracle import pfref
    if pfref.available():
        nav = pfref.RefNav(synth.to_chunks(grid))
        nav.game_load(pos, radius, faction, flags)
        for f in range(16):
            pfref.set_enemy_factions(f, int(masks[f]))
        centre = synth.cell_centre(W, W, np.array([j[0] for j in jobs]) * 64 + 32, np.array([j[1] for j in jobs]) * 64 + 32)
        batch = np.array([(pfref.ASYNC_ENEMY_SEEK, 0, f, c[0], c[1], 0, 0) for (cr, cc, f), c in zip(jobs, centre)],
                         dtype=pfref.ASYNC_REQ_DTYPE)
        assert nav.hip_init()
        try:
            def ref_batch(binding):
                ms, got = [], None
                for _ in range(4):
                    nav.cache_clear()
                    pfref.RefNav.hip_mode(binding, 1)
                    t0 = time.perf_counter()
                    got = nav.async_batch(batch)
                    ms.append((time.perf_counter() - t0) * 1e3)
                return min(ms[1:]), got
            cpu_ms, ref = ref_batch(False)
            bind_ms, _ = ref_batch(True)
            same = sum(np.array_equal(ref[navhip.N_RegionFieldID(navhip.FFID_ENEMIES, 0, cr, cc, f)].reshape(4096), fields[j])
                       for j, (cr, cc, f) in enumerate(jobs) if status[j] == 0)
            res.update({"reference_async_batch_all_cpu_ms": cpu_ms, "reference_async_batch_binding_on_ms": bind_ms,
                        "host_seed_extraction_ms_binding_less_parent_region_call": bind_ms - parent,
                        "device_fields_equal_to_reference": int(same), "jobs_decided": int((status == 0).sum())})
        finally:
            pfref.RefNav.hip_mode(False)
            pfref.RefNav.hip_shutdown()
            pfref.RefNav.game_unload()
            for f in range(16):
                pfref.set_enemy_factions(f, 0)
            nav.close()
    return res


def main():
    import torch
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    if "--seek-only" in sys.argv:
        print(json.dumps({"seek_fields": seek_fields(torch, dev)}, indent=1))
        return
    if "--region-repair-only" in sys.argv:
        print(json.dumps({"region_repair": region_repair(torch, dev)}, indent=1))
        return
    if "--attacking-only" in sys.argv:
        print(json.dumps({"field_attacking": field_attacking(torch, dev)}, indent=1))
        return
    W, K = 16, 64
    rng = np.random.RandomState(5)
    grid = synth.cost_grid(W, W, seed=1234)
    out = {}

    # ---- generic field kernel: non-unit costs everywhere
    costly = grid.copy()
    passable = costly != 255
    costly[passable] = rng.randint(1, 5, size=int(passable.sum())).astype(np.uint8)
    ctx = navhip.NavContext(W, W)
    ctx.upload_plane(0, navhip.PLANE_COST_BASE, synth.to_chunks(costly))
    ctx.upload_plane(0, navhip.PLANE_BLOCKERS, np.zeros((W, W, 64, 64), np.uint16))
    ctx.relabel_local_islands(0)
    liid = synth.from_chunks(ctx.download_plane(0, navhip.PLANE_LOCAL_ISLANDS))
    dests = synth.destinations(grid, K, seed=42)
    cols = synth.whole_map_requests(grid, dests, liid)
    reqs = navhip.make_reqs(len(cols["type"]))
    for k in synth.REQ_FIELDS:
        reqs[k] = cols[k]
    d_reqs = torch.from_numpy(reqs.view(np.uint8).reshape(len(reqs), 32)).to(dev)
    pool = torch.zeros((len(reqs), 4096), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(device=dev)

    def gen():
        ctx.build_fields_dev(d_reqs, len(reqs), pool, stream=st.cuda_stream)
        st.synchronize()
    t = timed(gen, reps=10)
    out["field_generic"] = {"chunk_fields": len(reqs), "ms": t * 1e3, "cells_per_s": len(reqs) * 4096 / t,
                            "what": "cost_base 1..4 on every passable cell: k_field_bfs declines all, k_field_generic builds all"}
    assert int((pool != 0).sum().item()) > len(reqs) * 1000
    ctx.close()

    # ---- the rest on the benchmark map
    ctx = navhip.NavContext(W, W)
    ctx.upload_plane(0, navhip.PLANE_COST_BASE, synth.to_chunks(grid))
    ctx.upload_plane(0, navhip.PLANE_BLOCKERS, np.zeros((W, W, 64, 64), np.uint16))
    t = timed(lambda: ctx.relabel_local_islands(0), reps=10)
    out["local_islands_whole_map"] = {"chunks": W * W, "ms": t * 1e3, "chunks_per_s": W * W / t}

    # region fields: one async batch of 256 jobs
    nj = 256
    rr = np.zeros(nj, navhip.REGION_REQ_DTYPE)
    seeds = []
    cells = synth.passable_cells(grid)
    for j in range(nj):
        cr, cc = rng.randint(1, W - 1), rng.randint(1, W - 1)
        rr["out_mode"][j] = 1
        rr["base_abs_r"][j], rr["base_abs_c"][j] = (cr - 1) * 64 + 32, (cc - 1) * 64 + 32
        rr["rdim"][j] = rr["cdim"][j] = 128
        rr["roff"][j] = rr["coff"][j] = 32
        rr["seed_begin"][j] = len(seeds)
        k = 40
        sr = rng.randint(rr["base_abs_r"][j], rr["base_abs_r"][j] + 128, k)
        sc = rng.randint(rr["base_abs_c"][j], rr["base_abs_c"][j] + 128, k)
        seeds += list(zip(sr, sc))
        rr["seed_count"][j] = k
    seeds = np.array(seeds, np.int16)
    t = timed(lambda: ctx.build_region_fields(rr, seeds, out_stride=4096), reps=5)
    out["region_fields_async_batch"] = {"jobs": nj, "ms_host_api": t * 1e3, "jobs_per_s": nj / t,
                                        "what": "128x128 padded regions, 64x64 window out, 40 seeds each; host buffers"}

    # blockers: 10 000 circles in, the same out
    pos = synth.cell_centre(W, W, *cells[rng.randint(len(cells), size=10_000)].T)
    circ = np.zeros(10_000, navhip.CIRCLE_DTYPE)
    circ["x"], circ["z"] = pos[:, 0], pos[:, 1]
    circ["radius"] = rng.uniform(2.0, 6.0, 10_000)
    undo = circ.copy()
    circ["delta"], undo["delta"] = 1, -1

    def blk():
        ctx.N_BlockersUpdate(circ)
        ctx.N_BlockersUpdate(undo)
    t = timed(blk, reps=5)
    out["blockers_circles"] = {"circles_per_call": 10_000, "ms_per_call_host_api": t * 1e3 / 2,
                               "circles_per_s": 20_000 / t,
                               "what": "k_blockers_circles + k_refresh_touched + k_local_islands of the touched chunks"}

    # LOS
    pick = cells[rng.randint(len(cells), size=4096)]
    lr = np.zeros(4096, navhip.LOS_REQ_DTYPE)
    lr["faction_id"] = 0xF
    lr["chunk_r"] = lr["target_chunk_r"] = pick[:, 0] // 64
    lr["chunk_c"] = lr["target_chunk_c"] = pick[:, 1] // 64
    lr["target_tile_r"], lr["target_tile_c"] = pick[:, 0] % 64, pick[:, 1] % 64
    t = timed(lambda: ctx.N_LOSFieldCreate(lr), reps=3)
    out["los_fields"] = {"fields": 4096, "ms_host_api": t * 1e3, "fields_per_s": 4096 / t}
    ctx.close()
    out["field_attacking"] = field_attacking(torch, dev)
    out["region_repair"] = region_repair(torch, dev)
    out["seek_fields"] = seek_fields(torch, dev)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
