"""The map planes of a context (csrc/navhip_api.hip): whole-plane and single-chunk uploads of two layers at once, seen by
the next chunk-field build through the derived row masks -- a partial list of dirty chunks per layer, through the one
list buffer the layers share --, the read-back, the non-unit-cost mark a chunk upload raises and a whole-plane upload
takes back, and the answers of the host-side checks in front of every launch (NAVHIP_ERR_INVALID,
NAVHIP_ERR_NOT_UPLOADED).  Fields are compared bit for bit with the restatement (oracle/navoracle.c).

Host buffers only: the file also runs on the host emulator (tests/test_emulated_cpu.py)."""
import numpy as np
import pytest

from oracle import navoracle

pytestmark = pytest.mark.gpu

W, H = 3, 2                 # chunks: w != h, so chunk_r * w + chunk_c cannot be written the other way round unnoticed
LAYERS = (0, 1)
TARGET = (31, 33)           # the target tile of every request: passable and free in every chunk made here


def _chunk(rng, cost3=False):
    """One chunk: (cost [64][64] u8, 1 or impassable -- or 3 in places --, blockers [64][64] u16)."""
    cost = np.where(rng.rand(64, 64) < 0.2, 0xFF, 1).astype(np.uint8)
    if cost3:
        cost[(rng.rand(64, 64) < 0.3) & (cost == 1)] = 3
    blockers = np.where(rng.rand(64, 64) < 0.05, rng.randint(1, 4, (64, 64)), 0).astype(np.uint16)
    cost[TARGET] = 1
    blockers[TARGET] = 0
    return cost, blockers


def _planes(seed):
    """{layer: [cost [H][W][64][64], blockers [H][W][64][64]]}, unit costs."""
    rng = np.random.RandomState(seed)
    out = {}
    for layer in LAYERS:
        chunks = [_chunk(rng) for _ in range(W * H)]
        out[layer] = [np.stack([c[k] for c in chunks]).reshape(H, W, 64, 64) for k in (0, 1)]
    return out


def _reqs(navlib):
    """One TARGET_TILE request per chunk and layer."""
    reqs = navlib.make_reqs(len(LAYERS) * W * H)
    i = 0
    for layer in LAYERS:
        for r in range(H):
            for c in range(W):
                reqs[i]["layer"], reqs[i]["type"] = layer, navlib.TARGET_TILE
                reqs[i]["chunk_r"], reqs[i]["chunk_c"] = r, c
                reqs[i]["tile_r"], reqs[i]["tile_c"] = TARGET
                i += 1
    return reqs


def _upload_all(navlib, ctx, planes):
    for layer in LAYERS:
        ctx.upload_plane(layer, navlib.PLANE_COST_BASE, planes[layer][0])
        ctx.upload_plane(layer, navlib.PLANE_BLOCKERS, planes[layer][1])


def _build_and_compare(navlib, ctx, planes, reqs, what):
    """The twelve fields of the context against the restatement over `planes`; returns the split of the build."""
    onav = navoracle.OracleNav(planes[0][0].copy(), planes[0][1].copy(), layer=0)
    for layer in LAYERS[1:]:
        onav.set_layer(layer, planes[layer][0].copy(), planes[layer][1].copy())
    exp, _ = onav.build_fields(reqs.view(navoracle.FIELD_REQ_DTYPE))
    dirs, _ = ctx.N_FlowFieldUpdate(reqs)
    bad = np.flatnonzero((dirs != exp).reshape(len(reqs), -1).any(1))
    assert bad.size == 0, "%s: fields of requests %s differ" % (what, bad)
    split = ctx.last_fields_split()
    assert sum(split) == len(reqs), (what, split)
    return split


def _patched_context(navlib):
    """A context whose layer 0 got the cost of two chunks and whose layer 1 got the blockers of a third chunk by
    navhip_upload_chunk after the whole planes; returns (ctx, planes as the device holds them, reqs, first split)."""
    planes, reqs = _planes(11), _reqs(navlib)
    ctx = navlib.NavContext(W, H)
    _upload_all(navlib, ctx, planes)
    split0 = _build_and_compare(navlib, ctx, planes, reqs, "whole planes")
    rng = np.random.RandomState(12)
    for (r, c) in ((0, 1), (1, 2)):                                   # two of the six chunks of layer 0: cost
        planes[0][0][r, c] = _chunk(rng)[0]
        ctx.upload_chunk(0, navlib.PLANE_COST_BASE, r, c, planes[0][0][r, c])
    planes[1][1][1, 0] = _chunk(rng)[1]                               # another chunk, layer 1: blockers
    ctx.upload_chunk(1, navlib.PLANE_BLOCKERS, 1, 0, planes[1][1][1, 0])
    return ctx, planes, reqs, split0


def test_chunk_uploads_reach_the_next_build_and_the_read_back(navlib):
    """Two layers dirty at once, each with a partial list of chunks; then a chunk with a cost of 3."""
    ctx, planes, reqs, split0 = _patched_context(navlib)
    assert _build_and_compare(navlib, ctx, planes, reqs, "after chunk uploads") == split0
    for layer in LAYERS:
        assert np.array_equal(ctx.download_plane(layer, navlib.PLANE_COST_BASE), planes[layer][0])
        assert np.array_equal(ctx.download_plane(layer, navlib.PLANE_BLOCKERS), planes[layer][1])
    planes[0][0][1, 1] = _chunk(np.random.RandomState(13), cost3=True)[0]
    assert (planes[0][0][1, 1] == 3).any()
    ctx.upload_chunk(0, navlib.PLANE_COST_BASE, 1, 1, planes[0][0][1, 1])
    split = _build_and_compare(navlib, ctx, planes, reqs, "a chunk with a cost of 3")
    # include/navhip.h, navhip_set_field_kernel: the generic relaxation builds the requests of chunks with other costs
    assert split == (split0[0] - 1, split0[1] + 1)
    assert np.array_equal(ctx.download_plane(0, navlib.PLANE_COST_BASE), planes[0][0])
    ctx.close()


def test_whole_plane_upload_after_chunk_uploads_takes_the_cost_mark_back(navlib):
    ctx, planes, reqs, split0 = _patched_context(navlib)
    planes[0][0][0, 2] = _chunk(np.random.RandomState(14), cost3=True)[0]
    ctx.upload_chunk(0, navlib.PLANE_COST_BASE, 0, 2, planes[0][0][0, 2])
    assert _build_and_compare(navlib, ctx, planes, reqs, "a chunk with a cost of 3")[1] == split0[1] + 1
    planes[0][0] = _planes(15)[0][0]                                  # unit costs again, every chunk of layer 0
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, planes[0][0])
    assert _build_and_compare(navlib, ctx, planes, reqs, "whole plane over the chunk uploads") == split0
    ctx.close()


def test_host_side_checks_refuse_before_anything_is_launched(navlib):
    L, hp = navlib.lib(), navlib._hp
    ctx = navlib.NavContext(2, 2)
    cost = np.ones((2, 2, 64, 64), np.uint8)
    chunk = np.ones((64, 64), np.uint8)
    # nothing uploaded yet
    assert L.navhip_plane_dev(ctx._h, 0, navlib.PLANE_COST_BASE) is None
    back = np.zeros_like(cost)
    assert L.navhip_download_plane(ctx._h, 0, navlib.PLANE_COST_BASE, hp(back), back.nbytes) == navlib.ERR_NOT_UPLOADED
    assert L.navhip_relabel_local_islands(ctx._h, 0) == navlib.ERR_NOT_UPLOADED
    circle = np.zeros(1, navlib.CIRCLE_DTYPE)
    circle["x"], circle["z"], circle["radius"], circle["delta"] = 100.0, -100.0, 4.0, 1
    mx, mz = ctx.map_pos()
    assert L.navhip_blockers_circles(ctx._h, hp(circle), 1, mx, mz) == navlib.ERR_NOT_UPLOADED
    ctx.sync()
    # sizes and ranges
    assert L.navhip_upload_plane(ctx._h, 0, navlib.PLANE_COST_BASE, hp(cost), cost.nbytes - 1) == navlib.ERR_INVALID
    assert "navhip_upload_plane" in ctx.last_error()
    assert L.navhip_plane_dev(ctx._h, 0, navlib.PLANE_COST_BASE) is None
    assert L.navhip_upload_chunk(ctx._h, 0, navlib.PLANE_COST_BASE, 2, 0, hp(chunk), chunk.nbytes) == navlib.ERR_INVALID
    assert L.navhip_upload_chunk(ctx._h, 0, 5, 0, 0, hp(chunk), chunk.nbytes) == navlib.ERR_INVALID
    assert L.navhip_upload_chunk(ctx._h, 0, navlib.PLANE_COST_BASE, 0, 0, hp(chunk), chunk.nbytes - 1) == navlib.ERR_INVALID
    assert "navhip_upload_chunk" in ctx.last_error()
    # a cost plane, and still no local islands for a portal request
    ctx.upload_plane(0, navlib.PLANE_COST_BASE, cost)
    assert L.navhip_plane_dev(ctx._h, 0, navlib.PLANE_COST_BASE) is not None
    assert L.navhip_plane_dev(ctx._h, 0, navlib.PLANE_LOCAL_ISLANDS) is None
    assert L.navhip_plane_dev(ctx._h, 0, 5) is None and L.navhip_plane_dev(ctx._h, navoracle.NLAYERS, 0) is None
    req = navlib.make_reqs(1)
    req["type"] = navlib.TARGET_PORTAL
    dirs = np.zeros((1, 64, 64), np.uint8)
    assert L.navhip_build_fields(ctx._h, hp(req), 1, hp(dirs), None) == navlib.ERR_NOT_UPLOADED
    assert np.array_equal(ctx.download_plane(0, navlib.PLANE_COST_BASE), cost)
    ctx.close()

