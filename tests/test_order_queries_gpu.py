"""navhip_order_queries[_dev] (csrc/order_query_kernels.hip) against the reference build itself, row for row and bit for
bit: the dest as uint32 views, the dest id, the status.  The expected row is the reference's own calls made in sequence
(tests/test_order_queries_cpu.py: Ref.row -- N_LocationsReachable, N_ClosestReachableInRange, N_ClosestReachableDest,
N_DestIDForPos[Attacking]) on the worlds of tests/order_query_worlds.py; the model (tests/order_query_model.py, pinned to
the reference by the CPU file) adds what the reference does not return: NAVHIP_OQ_NO_TILE, and which rows lie beyond the
device's window.  NAVHIP_OQ_HOST may come back for the rows a case names only.

The device gets the ISLANDS planes and, on one layer, cost and blockers planes that the queries must not read.  Host buffers
wherever the API allows; the file also runs on the host emulator (tests/test_order_queries_emulated_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pfref
from tests import order_query_model as om
from tests import order_query_worlds as ow
from tests.test_order_queries_cpu import Ref

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not pfref.available(), reason="oracle/_ref (the reference build) is not present")]

F = np.float32
NAN_BITS = np.array([np.nan, 0.0], F).view(np.uint32)
IR, RE = om.OQ_IN_RANGE, om.OQ_REACHABLE


def _dev():
    import torch
    from permafrost_engine_amd import tick
    return torch.device("cpu") if tick.EMULATED else torch.device("cuda", 0)


class Dev:
    """One world in the reference, in the model and on the device.  The reference's answers are computed once per case."""

    def __init__(self, navlib, name):
        self.navlib, self.ref = navlib, Ref(ow.WORLDS[name]())
        self.W, self.model = self.ref.W, self.ref.model()
        self.ctx = navlib.NavContext(self.W.w, self.W.h)
        self.upload(self.ref)
        self._expected = {}

    def upload(self, ref):
        for layer, nav in ref.navs.items():
            self.ctx.upload_plane(layer, self.navlib.PLANE_ISLANDS, nav.plane(pfref.PLANE_ISLANDS, layer))
            if layer in ref.W.blockers:                                 # (the surround flood would skip these tiles)
                self.ctx.upload_plane(layer, self.navlib.PLANE_COST_BASE, nav.plane(pfref.PLANE_COST, layer))
                self.ctx.upload_plane(layer, self.navlib.PLANE_BLOCKERS, nav.plane(pfref.PLANE_BLOCKERS, layer))

    def queries(self, rows):
        q = np.zeros(len(rows), self.navlib.ORDER_QUERY_DTYPE)
        q[:] = om.make_queries(rows)
        return q

    def expected_rows(self, q):
        """(dest [n][2], id [n], status [n], infos): the reference's answers; NO_TILE and HOST from the model."""
        dest, ids, status, infos = np.zeros((len(q), 2), F), np.zeros(len(q), np.uint32), np.zeros(len(q), np.uint8), []
        for i, r in enumerate(q):
            key = r.tobytes()
            if key not in self._expected:
                md, mid, mstatus, info = self.model.row(r)
                if mstatus == om.OQ_HOST:
                    self._expected[key] = (np.array([np.nan, 0.0], F), 0, om.OQ_HOST, info)
                else:
                    d, did, st = self.ref.row(r)
                    self._expected[key] = (d, did, st | (mstatus & om.OQ_NO_TILE), info)
            dest[i], ids[i], status[i], info = self._expected[key]
            infos.append(info)
        return dest, ids, status, infos

    def resident(self, q):
        import torch
        dev, n = _dev(), len(q)
        d_q = torch.from_numpy(q.view(np.uint8).reshape(n, 32).copy()).to(dev)
        d_dest = torch.full((n, 2), 7.0, dtype=torch.float32, device=dev)
        d_id = torch.full((n,), 7, dtype=torch.int32, device=dev)
        d_status = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        self.ctx.order_queries_dev(d_q, n, d_dest, d_id, d_status)
        self.ctx.sync()
        return d_dest.cpu().numpy(), d_id.cpu().numpy().view(np.uint32), d_status.cpu().numpy()

    def check(self, rows, host_rows=(), resident=False):
        """The device's answers equal the reference's, bit for bit; exactly the rows in host_rows come back NAVHIP_OQ_HOST
        with (NaN, 0) and id 0.  Returns (queries, dest, ids, status, infos) of the reference."""
        q = self.queries(rows)
        dest, ids, status, infos = self.expected_rows(q)
        assert sorted(np.flatnonzero(status == om.OQ_HOST).tolist()) == sorted(host_rows)
        for i in host_rows:
            assert dest[i].view(np.uint32).tolist() == NAN_BITS.tolist() and ids[i] == 0
        for got in ([self.ctx.order_queries(q)] + ([self.resident(q)] if resident else [])):
            assert np.array_equal(got[2], status), (got[2].tolist(), status.tolist())
            bad = np.flatnonzero((got[0].view(np.uint32) != dest.view(np.uint32)).any(1) | (got[1] != ids))
            assert len(bad) == 0, [(int(i), q[i], got[0][i].tolist(), dest[i].tolist(), hex(got[1][i]), hex(ids[i])) for i in bad[:6]]
            assert got[1].dtype == np.uint32 and got[2].dtype == np.uint8
        return q, dest, ids, status, infos

    def close(self):
        self.ctx.close()
        self.ref.close()


@pytest.fixture(scope="module")
def small(navlib):
    d = Dev(navlib, "small")
    yield d
    d.close()


@pytest.fixture(scope="module")
def big(navlib):
    d = Dev(navlib, "big")
    yield d
    d.close()


def _dst_bits(q):
    return np.stack([q["dst_x"], q["dst_z"]], 1).view(np.uint32)


# ---- the cases ---------------------------------------------------------------------------------------------------------
def test_same_island(small):
    """d == dst bit for bit, SAME_ISLAND set; layers 0 and 2 (different islands), factions 0, 7, 14 and none."""
    q, dest, ids, status, _ = small.check(small.W.cases["same_island"], resident=True)
    plain = (q["flags"] & IR) == 0
    assert np.array_equal(dest.view(np.uint32)[plain], _dst_bits(q)[plain]) and (status == om.OQ_SAME_ISLAND).all()
    assert set((ids & 0xf).tolist()) == {0, 7, 14, 15} and set(((ids >> 4) & 0xf).tolist()) == {0, 2}


def test_click_on_a_blob_and_on_another_island(small):
    """The tile centre of the first hit in queue order; one source stands on an impassable tile (island 0xffff)."""
    q, dest, ids, status, infos = small.check(small.W.cases["blob_and_other_island"], resident=True)
    moved = (dest.view(np.uint32) != _dst_bits(q)).any(1)
    assert moved.sum() >= len(q) - 1 and not (status[moved] & om.OQ_SAME_ISLAND).any()
    # centres: half a tile off the grid in both coordinates
    assert (np.mod(dest[moved], 4.0) == 2.0).all()


def test_queue_order_decides(small):
    """Two tiles of the source's island on one Chebyshev ring, the Euclidean-nearer one later in the queue."""
    q, dest, ids, status, infos = small.check(small.W.cases["queue_order"])
    E = small.ref.model("euclid")
    for r, info, d in zip(q, infos, dest):
        e = E.flood_first(0, info["reachable"]["start"], small.ref.islands(0)[small.model.tile((r["src_x"], r["src_z"]))])
        assert e != info["reachable"]["tile"] and small.model.tile(d) == info["reachable"]["tile"]


def test_nearest_tile_holds_a_blocker(small):
    """ignore_blockers = true: the tile is still the answer, with a blockers plane resident that says it is occupied."""
    q, dest, ids, status, infos = small.check(small.W.cases["blocker"], resident=True)
    blk = small.ctx.download_plane(0, small.navlib.PLANE_BLOCKERS)
    for d in dest:
        r, c = small.model.tile(d)
        assert blk[r >> 6, c >> 6, r & 63, c & 63] > 0


def test_borders_and_corners(small):
    q, dest, ids, status, infos = small.check(small.W.cases["borders"], resident=True)
    assert max(i["reachable"]["depth"] for i in infos if i["reachable"]) == 62


def test_the_lake(big):
    """Wider than the window: the nearest land 63 tiles away is answered, 64 tiles away comes back NAVHIP_OQ_HOST."""
    q, dest, ids, status, infos = big.check(big.W.cases["lake"], host_rows=(1, 2), resident=True)
    assert [i["reachable"]["depth"] for i in infos[:3]] == [63, 64, 64]


def test_in_range_plain(small):
    """Ranges 0.5, 4, 4.01, 17 and 60 from all sides, ties from grid points, a target two tiles from the map's edge."""
    q, dest, ids, status, infos = small.check(small.W.cases["in_range"] + small.W.cases["ties"], resident=True)
    assert not (status & om.OQ_HOST).any() and sum(i["in_range"]["ties"] >= 2 for i in infos) >= 4
    won = np.array([not i["in_range"]["no_tile"] for i in infos]) & ((q["flags"] & RE) == 0)
    assert won.sum() > 20 and (np.mod(dest[won], 4.0) == 0.0).all()                 # corners, not centres


def test_in_range_at_the_cap(big):
    """More than 2048 tiles under the circle: the sources south of the target see the truncated set.  Range 128.01 is
    NAVHIP_OQ_HOST in the resident form and refused by the host form."""
    rows = big.W.cases["cap"]
    q, dest, ids, status, infos = big.check(rows, resident=True)
    assert all(i["in_range"]["n_tiles"] == om.CAP for i in infos)
    over = [(src, dst, 128.01, layer, f, fl) for src, dst, rng, layer, f, fl in rows[-2:]]
    qo = big.queries(rows[:2] + over)
    d, i, s = big.resident(qo)
    assert s[2:].tolist() == [om.OQ_HOST] * 2 and (d[2:].view(np.uint32) == NAN_BITS).all() and not i[2:].any()
    assert np.array_equal(s[:2], status[:2]) and np.array_equal(d[:2].view(np.uint32), dest[:2].view(np.uint32))
    with pytest.raises(big.navlib.NavHipError, match="range"):
        big.ctx.order_queries(qo)


def test_in_range_at_negative_and_zero_ranges(small):
    q, dest, ids, status, infos = small.check(small.W.cases["small_ranges"], resident=True)
    for r, st, i in zip(q, status, infos):
        assert i["in_range"]["n_tiles"] == (1 if r["range"] > -4 else 0)
        assert r["range"] > -4 or st & om.OQ_NO_TILE


def test_no_tile_in_range_then_onto_the_sources_island(small):
    """The composition of do_set_enter_range: the in-range search returns the target, N_ClosestReachableDest moves it."""
    q, dest, ids, status, infos = small.check(small.W.cases["no_tile"], resident=True)
    assert (status & om.OQ_NO_TILE).all()
    plain = (q["flags"] & RE) == 0
    assert np.array_equal(dest.view(np.uint32)[plain], _dst_bits(q)[plain])
    assert (dest.view(np.uint32)[~plain] != _dst_bits(q)[~plain]).any(1).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_sizes(small, n):
    """Mixed flags, layers and factions; the resident form's outputs equal the host form's (both equal the reference)."""
    pool = [r for case in ("same_island", "blob_and_other_island", "ties", "small_ranges", "no_tile", "blocker") for r in small.W.cases[case]]
    rows = [pool[(7 * i) % len(pool)] for i in range(n)]
    q, dest, ids, status, infos = small.check(rows, resident=True)
    if n >= 63:
        assert set(q["flags"].tolist()) == {0, IR, RE, IR | RE} and set(q["layer"].tolist()) == {0, 2}


def test_answers_follow_an_upload(navlib, small):
    """Part of the WEST island is walled off: with the new islands plane uploaded, the same context answers as the
    reference on the new map does; before the upload it answered as on the old one."""
    walled = Ref(ow.WORLDS["small_walled"]())
    rows = walled.W.cases["after_upload"]
    before = small.check(rows)[1]
    d = Dev(navlib, "small")
    d.ref.close()
    d.ref, d.model, d._expected = walled, walled.model(), {}
    d.upload(walled)
    after = d.check(rows, resident=True)[1]
    assert (before.view(np.uint32) != after.view(np.uint32)).any(1).tolist() == [True, False, True, False]
    d.close()


def test_argument_errors(navlib, small):
    """Each is refused with NAVHIP_ERR_ARG and a message, before any launch and with the outputs untouched; the same rows
    in the resident form come back NAVHIP_OQ_HOST with (NaN, 0) and id 0, the good rows beside them answered."""
    L, ctx, xz = navlib.lib(), small.ctx, small.W.xz
    mx, mz = ctx.map_pos()
    good = (xz(10, 10), xz(50, 40), 10.0, 0, om.FACTION_NONE, IR | RE)

    def call(q, n=None, missing=None):
        n = len(q) if n is None else n
        out = [np.full((len(q), 2), 7.0, F), np.full(len(q), 7, np.uint32), np.full(len(q), 7, np.uint8)]
        p = [q.ctypes.data_as(C.c_void_p)] + [a.ctypes.data_as(C.c_void_p) for a in out]
        if missing is not None:
            p[missing] = None
        rc = L.navhip_order_queries(ctx._h, p[0], n, mx, mz, p[1], p[2], p[3])
        return rc, out

    def refused(q, word, **kw):
        rc, out = call(q, **kw)
        assert rc == navlib.ERR_ARG and word in ctx.last_error(), (rc, ctx.last_error())
        assert all((a == 7).all() for a in out)

    def row(**kw):
        src, dst, rng, layer, faction, flags = good
        v = dict(src=src, dst=dst, rng=rng, layer=layer, faction=faction, flags=flags)
        v.update(kw)
        return (v["src"], v["dst"], v["rng"], v["layer"], v["faction"], v["flags"])

    rc, out = call(small.queries([good]))
    assert rc == 0 and out[2][0] == om.OQ_SAME_ISLAND
    for missing in range(4):
        refused(small.queries([good]), "missing", missing=missing)
    refused(small.queries([good]), "negative", n=-1)
    bad = [(row(flags=4), "flags"), (row(flags=IR | RE | 0x80), "flags"), (row(layer=-1), "layer"), (row(layer=12), "layer"),
           (row(layer=1), "islands"), (row(faction=-1), "faction"), (row(faction=16), "faction"),
           (row(src=(np.nan, mz + 4.0)), "NaN"), (row(dst=(mx - 4.0, np.nan)), "NaN"), (row(rng=np.nan), "NaN"),
           (row(src=(mx + 0.5, mz + 10.0)), "source"), (row(src=(mx - 10.0, mz + 512.5)), "source"),
           (row(dst=(mx - 512.5, mz + 10.0)), "destination"), (row(dst=(mx - 10.0, mz - 0.5), flags=IR), "destination"),
           (row(rng=128.01), "range"), (row(rng=1.0e9, flags=0), "range"), (row(rng=np.inf), "range")]
    for r, word in bad:
        refused(small.queries([good, r]), word)
    # the resident form: the same rows, one launch
    q = small.queries([good] + [r for r, _ in bad] + [good])
    d, i, s = small.resident(q)
    want = small.check([good])
    assert s[1:-1].tolist() == [om.OQ_HOST] * len(bad) and (d[1:-1].view(np.uint32) == NAN_BITS).all() and not i[1:-1].any()
    for k in (0, -1):
        assert s[k] == want[3][0] and d[k].view(np.uint32).tolist() == want[1][0].view(np.uint32).tolist() and i[k] == want[2][0]
    # n == 0 is fine in both forms
    assert L.navhip_order_queries(ctx._h, None, 0, mx, mz, None, None, None) == 0
    assert L.navhip_order_queries_dev(ctx._h, None, 0, mx, mz, None, None, None, None) == 0
