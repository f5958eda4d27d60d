"""The workload plan of tick.NavTick (permafrost_engine_amd.plan) by itself: host only, no library, no device.  Every
table a benchmark line rests on -- the per-rank request slices, the rows that travel, the slot tables, the obstacle
move stream, the level order of the LOS chain -- is checked here against what it has to mean."""
import collections
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from permafrost_engine_amd import navhip, plan, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _job(chunk_w=2, world=1, fpr=3, apr=300, rank=0, straddle=0.0, **kw):
    """(layout, grid, destinations, agents, request stream) as NavTick plans them, the island plane from numpy."""
    lay = plan.layout(chunk_w, world)
    grid = synth.cost_grid(lay.Wt, lay.H, seed=1234)
    dests, ag = plan.population(grid, lay, world, fpr, apr, 20, straddle=straddle)
    rq = plan.request_stream(grid, lay, dests, ag["flock"], synth.local_islands(grid), rank, world, fpr, apr, **kw)
    return lay, grid, dests, ag, rq


def _chunk(rq, lay):
    return rq.reqs["chunk_r"].astype(np.int64) * lay.Wt + rq.reqs["chunk_c"]


def _check_region_records(rq, lay, q):
    """Every record of region q's slice names chunks of region q (its own, and the next one of a portal target)."""
    b, e = rq.req_bounds[q]
    r0, r1, c0, c1 = (v // 64 for v in plan.region_cells(lay, q))
    r = rq.reqs[b:e]
    assert e > b
    assert ((r["chunk_r"] >= r0) & (r["chunk_r"] < r1) & (r["chunk_c"] >= c0) & (r["chunk_c"] < c1)).all()
    p = r[r["type"] == navhip.TARGET_PORTAL]
    assert len(p) and ((p["next_chunk_r"] >= r0) & (p["next_chunk_r"] < r1)
                       & (p["next_chunk_c"] >= c0) & (p["next_chunk_c"] < c1)).all()


@pytest.mark.parametrize("world", [2, 4])
def test_regions_slice_the_request_stream(world):
    lay, grid, dests, ag, rq = _job(chunk_w=2, world=world, fpr=3, apr=300, tile_exchange="all")
    n_req = len(rq.reqs)
    assert (lay.Wt, lay.H) == ((4, 2) if world == 2 else (4, 4)) and rq.tile_exchange == "all"
    assert rq.req_bounds[0][0] == 0 and rq.req_bounds[-1][1] == n_req and len(rq.req_bounds) == world
    assert all(rq.req_bounds[q][1] == rq.req_bounds[q + 1][0] for q in range(world - 1))      # rank order, no gap
    assert rq.xchg_bounds == rq.req_bounds and rq.n_requests_served == n_req
    for q in range(world):
        _check_region_records(rq, lay, q)
        b, e = rq.req_bounds[q]
        assert (rq.dest_of_req[b:e] // 3 == q).all()                    # a region's requests are its own destinations'
        r0, r1, c0, c1 = plan.region_cells(lay, q)
        d = dests[q * 3:(q + 1) * 3]
        assert ((d[:, 0] >= r0) & (d[:, 0] < r1) & (d[:, 1] >= c0) & (d[:, 1] < c1)).all()
    assert np.array_equal(rq.slot_tbl[rq.dest_of_req, _chunk(rq, lay)], np.arange(n_req))
    assert (rq.slot_tbl >= 0).sum() == n_req and rq.slot_tbl.shape == (3 * world, lay.nchunks)


def test_travelling_tiles_lead_every_rank_slice():
    from permafrost_engine_amd import dist as pdist
    fpr, apr = 4, 400
    lay, grid, dests, ag, rq = _job(chunk_w=2, world=2, fpr=fpr, apr=apr, straddle=0.25)
    travels = pdist.travelling_destinations(ag["flock"], apr, fpr, 2 * fpr)
    assert rq.tile_exchange == "auto" and travels.any() and not travels.all()
    inside = np.zeros(len(rq.reqs), bool)
    for q in range(2):
        (b, e), (xb, xe) = rq.req_bounds[q], rq.xchg_bounds[q]
        assert xb == b and b < xe < e                                    # a prefix of the rank's slice
        inside[xb:xe] = True
        _check_region_records(rq, lay, q)
    assert np.array_equal(inside, travels[rq.dest_of_req])
    assert np.array_equal(rq.slot_tbl[rq.dest_of_req, _chunk(rq, lay)], np.arange(len(rq.reqs)))
    other = _job(chunk_w=2, world=2, fpr=fpr, apr=apr, straddle=0.25, rank=1)[4]       # every rank plans the same stream
    assert other.req_bounds == rq.req_bounds and other.xchg_bounds == rq.xchg_bounds
    assert other.reqs.tobytes() == rq.reqs.tobytes() and np.array_equal(other.slot_tbl, rq.slot_tbl)


@pytest.mark.parametrize("rank", [0, 1])
def test_rank_aligned_flocks_plan_their_own_region_only(rank):
    fpr, apr = 4, 400
    lay, grid, dests, ag, rq = _job(chunk_w=2, world=2, fpr=fpr, apr=apr, rank=rank)
    assert not plan.travelling_destinations(ag["flock"], apr, fpr, 2 * fpr).any()
    assert rq.tile_exchange == "none"
    assert rq.req_bounds[rank] == (0, len(rq.reqs)) and rq.req_bounds[1 - rank] == (0, 0)
    assert (rq.dest_of_req // fpr == rank).all()
    _check_region_records(rq, lay, rank)


def test_shared_fields_point_every_destination_at_one_copy():
    plain = _job(chunk_w=4, fpr=8, apr=300)[4]
    lay, grid, dests, ag, shared = _job(chunk_w=4, fpr=8, apr=300, share_fields=True)
    chunk = _chunk(plain, lay)
    slots = shared.slot_tbl[plain.dest_of_req, chunk]
    assert (slots >= 0).all() and shared.reqs[slots].tobytes() == plain.reqs.tobytes()      # byte for byte
    distinct = {plain.reqs[i].tobytes() for i in range(len(plain.reqs))}
    assert len(shared.reqs) == len(distinct) and shared.n_requests_served == len(plain.reqs)
    assert shared.req_bounds == [(0, len(shared.reqs))] and shared.xchg_bounds == [(0, len(shared.reqs))]
    assert (shared.slot_tbl >= 0).sum() == (plain.slot_tbl >= 0).sum()
    # slots in first-occurrence order: the first stream position of every slot's record grows with the slot
    first = np.full(len(shared.reqs), len(plain.reqs))
    np.minimum.at(first, slots, np.arange(len(plain.reqs)))
    assert (np.diff(first) > 0).all() and np.array_equal(shared.dest_of_req, plain.dest_of_req[first])
    with pytest.raises(ValueError):
        _job(chunk_w=2, world=2, fpr=3, apr=300, share_fields=True)
    with pytest.raises(ValueError):
        _job(chunk_w=2, fpr=3, apr=300, share_fields=True, obstacles=5)


def test_obstacle_requests_are_live_and_conditional():
    rq = _job(chunk_w=2, fpr=3, apr=300, obstacles=5)[4]
    assert (rq.reqs["flags"] == navhip.REQ_LIVE_IIDS | navhip.REQ_IF_CHANGED).all()
    assert (_job(chunk_w=2, fpr=3, apr=300)[4].reqs["flags"] & (navhip.REQ_LIVE_IIDS | navhip.REQ_IF_CHANGED) == 0).all()


@pytest.mark.parametrize("obstacles,move_frac,ticks", [(40, 0.1, 6), (40, 0.01, 3), (7, 0.5, 5)])
def test_obstacle_moves_replay_over_the_start_circles(obstacles, move_frac, ticks):
    lay = plan.layout(2, 1)
    grid = synth.cost_grid(2, 2, seed=1234)
    circ, moves = plan.obstacle_stream(grid, lay, obstacles, move_frac, ticks)
    nmove = max(1, int(round(obstacles * move_frac)))
    assert circ.dtype == navhip.CIRCLE_DTYPE and len(circ) == obstacles and (circ["delta"] == 1).all()
    assert moves.shape == (ticks, 2 * nmove) and moves.dtype == navhip.CIRCLE_DTYPE
    assert ((circ["radius"] >= 2.0) & (circ["radius"] < 6.0)).all()

    def key(c):
        return (float(c["x"]), float(c["z"]), float(c["radius"]))
    present = collections.Counter(key(c) for c in circ)
    for t in range(ticks):
        assert (moves[t, :nmove]["delta"] == -1).all() and (moves[t, nmove:]["delta"] == 1).all()
        for c in moves[t]:
            if c["delta"] == -1:
                assert present[key(c)] > 0, "tick %d removes a circle that is not there" % t
            present[key(c)] += int(c["delta"])
        assert sum(present.values()) == obstacles and min(present.values()) >= 0
    mp = synth.map_pos(2, 2)                       # (every landing place is a passable cell centre of this map)
    col = ((mp[0] - moves["x"]) / 4.0 - 0.5).round().astype(int)
    row = ((moves["z"] - mp[2]) / 4.0 - 0.5).round().astype(int)
    assert (grid[row, col] != synth.COST_IMPASSABLE).all()


def test_los_layout_orders_the_chain_by_level():
    grid = synth.cost_grid(4, 4, seed=1234)
    dests = synth.destinations(grid, 1, seed=42)
    lc = synth.planner_los(grid, dests)
    assert lc is not None, "data/los_cfg0.npz is the fixture of this world"
    lay = plan.layout(4, 1)
    ll = plan.los_layout(lc, dests, lay, 1)
    n = len(lc["dest"])
    r = ll.reqs
    assert r.dtype == navhip.LOS_REQ_DTYPE and len(r) == n and n > 1
    assert ll.bounds[0] == 0 and ll.bounds[-1] == n and (np.diff(ll.bounds) >= 0).all()
    assert len(ll.bounds) - 1 == ll.level.max() + 1 > 1
    for L in range(len(ll.bounds) - 1):
        assert (ll.level[ll.bounds[L]:ll.bounds[L + 1]] == L).all()
    # the slot table is the inverse of the order: record i of the chain sits in slot tbl[dest, chunk]
    slots = ll.slot_tbl[lc["dest"], lc["chunk_r"] * lay.Wt + lc["chunk_c"]]
    assert np.array_equal(np.sort(slots), np.arange(n)) and (ll.slot_tbl >= 0).sum() == n
    assert np.array_equal(r["chunk_r"][slots], lc["chunk_r"]) and np.array_equal(r["chunk_c"][slots], lc["chunk_c"])
    assert np.array_equal(r["prev_dr"][slots], lc["prev_dr"]) and np.array_equal(r["prev_dc"][slots], lc["prev_dc"])
    dest_of_slot = np.empty(n, np.int64)
    dest_of_slot[slots] = lc["dest"]
    assert np.array_equal(r["target_chunk_r"] * 64 + r["target_tile_r"], dests[dest_of_slot, 0])
    assert np.array_equal(r["target_chunk_c"] * 64 + r["target_tile_c"], dests[dest_of_slot, 1])
    first = ll.level == 0
    assert (ll.chain_prev[first] == -1).all() and (r["prev_dr"][first] == 0).all() and (r["prev_dc"][first] == 0).all()
    later = np.flatnonzero(~first)
    p = ll.prev_slot[later]
    assert np.array_equal(ll.chain_prev[later], p) and ll.chain_prev.dtype == np.int32
    assert np.array_equal(ll.level[p], ll.level[later] - 1)
    assert np.array_equal(r["chunk_r"][p], r["chunk_r"][later] + r["prev_dr"][later])
    assert np.array_equal(r["chunk_c"][p], r["chunk_c"][later] + r["prev_dc"][later])
    assert np.array_equal(dest_of_slot[p], dest_of_slot[later])


def test_layout_limits_and_region_cells():
    assert plan.layout(16, 16)[3:] == (4, 64, 64, 4096) and plan.layout(16, 8, shared_map=True)[2:] == (1, 1, 16, 16, 256)
    with pytest.raises(ValueError):
        plan.layout(17, 16)
    lay = plan.layout(2, 4)
    assert [plan.region_cells(lay, q) for q in range(4)] == [(0, 128, 0, 128), (0, 128, 128, 256), (128, 256, 0, 128),
                                                             (128, 256, 128, 256)]
    assert plan.region_cells(plan.layout(2, 4, shared_map=True), 3) == (0, 128, 0, 128)


def test_the_plan_needs_neither_torch_nor_the_library():
    code = ("import sys; import permafrost_engine_amd.plan; from permafrost_engine_amd import navhip; "
            "assert 'torch' not in sys.modules, 'torch'; assert navhip._lib is None, 'library loaded'; print('host only')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host only" in r.stdout, r.stdout
