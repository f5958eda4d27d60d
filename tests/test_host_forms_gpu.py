"""The seven host-buffer forms that stage through ONE call-local arena (csrc/stage_plan.h, NH_STAGE_CALL0):
navhip_arrival_flock_update, navhip_arrival_zone_build, navhip_dest_queries, navhip_order_queries,
navhip_surround_queries[_ex], navhip_repair_region_fields, navhip_build_seek_fields -- each against its own _dev form on
the same context, byte for byte.  What the answers ARE is held against the models and the reference by each unit's own test
file; here it is the staging: one arena carved differently call after call and growing in between, rows that are empty,
optional arrays that are absent, and which of the forms drop the snapshot a completed host-buffer step left resident.

One 4 x 4 map (the map of tests/arrival_flock_worlds.batch_world) with cost, blockers and islands planes on layer 0 serves
every call.  The file also runs on the host emulator (NAVHIP_LIB), like the files it borrows from."""
import ctypes as C

import numpy as np
import pytest

from tests import arrival_build_worlds as bw
from tests import arrival_flock_worlds as aw
from tests import test_arrival_build_gpu as tab
from tests import test_arrival_flock_gpu as taf
from tests.test_arrival_flock_gpu import _dev, _sync

pytestmark = [pytest.mark.gpu]

F = np.float32
MAP = 4
STRIDE = 4096
SENTINEL = 0xa5


# ---------------------------------------------------------------------------------------------
# the worlds: the smallest of each unit's own tests, on the one map
# ---------------------------------------------------------------------------------------------
def build_world(count, members=8, **kw):
    """`count` INACTIVE zones of tests/arrival_build_worlds on the 4 x 4 map, far enough apart for their rooms; kw: total
    and room of World.add (total_members below 4 makes a zone wait, and a zone that waits needs no room)."""
    W = bw.World(MAP, MAP)
    for k in range(count):
        r, c = 30 + 40 * (k // 5), 30 + 40 * (k % 5)
        W.add("z%d" % k, W.p(r, c, (0.3, -0.6)), bw.crowd(W, r + 6, c, members, seed=50 + k) if members else [], **kw)
    return W.done()


def units(n, seed=3):
    """n movable units on random tiles: the snapshot of the surround and seek calls and of the agent step."""
    rng = np.random.RandomState(seed)
    pos = np.array([aw.xz(MAP, MAP, int(r), int(c), rng.uniform(-1.5, 1.5, 2)) for r, c in rng.randint(8, 248, (n, 2))], F)
    return {"pos_xz": pos, "radius": np.full(n, 1.0, F), "flags": np.full(n, 8, np.uint32)}          # ENTITY_FLAG_MOVABLE


def make_context(navlib):
    c = taf.context(navlib, aw.batch_world(3))
    c.upload_plane(0, navlib.PLANE_ISLANDS, np.ones((MAP, MAP, 64, 64), np.uint16))
    assert int(units(1)["flags"][0]) == navlib.ENTITY_FLAG_MOVABLE
    return c


@pytest.fixture(scope="module")
def ctx(navlib):
    c = make_context(navlib)
    yield c
    c.close()


def t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(_dev())


def full(shape, value, dtype):
    import torch
    return torch.full(shape, value, dtype=dtype, device=_dev())


# ---------------------------------------------------------------------------------------------
# each form: the host call and the _dev call, both as a tuple of byte-comparable arrays
# ---------------------------------------------------------------------------------------------
def flat_flock(got):
    zones, members, status = got
    out = [np.asarray(status)]
    for z in zones:
        out += [np.asarray(z[k]) for k in sorted(z)]
    for m in members:
        out += [np.asarray(m[k]) for k in sorted(m)]
    return out


class Flock:
    def __init__(self, W):
        self.W = W

    def host(self, navlib, ctx):
        W = self.W
        return flat_flock(ctx.arrival_flock_update({"pos_xz": W.pos}, W.zones, W.keys, W.members))

    def dev(self, navlib, ctx):
        R = taf.Resident(navlib, ctx, self.W)
        _sync()
        R.call()
        ctx.sync()
        return flat_flock(R.read())


def flat_build(res, nz):
    keys = ("slots_xz", "slot_ring", "region_keys", "axis_xz", "com_xz", "com_dest_id", "substate", "sink_valid", "sink_xz")
    # (every array has one spare row behind the call's counts, which is the caller's own: not compared)
    out = [np.asarray(res["status"])[:max(nz, 1)]] + [np.asarray(res[k])[:-1] for k in keys]
    return out + [np.frombuffer(bytes(res["zs"]), np.uint8), np.frombuffer(bytes(res["fs"]), np.uint8)]


class Build:
    def __init__(self, W):
        self.W = W

    def host(self, navlib, ctx):
        """The wrapper fills the shared arrays, axis, com and dest id with -7 / 7 and zeroes the member outputs: those three
        are pointed at arrays of SENTINEL bytes here, one row longer than nm like the wrapper's own."""
        W, seen = self.W, {}

        def sentinel(bi, bo, zs, fs):
            self.counts = (bi.n_slots, bi.n_keys, bi.nm)
            for name, width in (("substate", 1), ("sink_valid", 1), ("sink_xz", 8)):
                seen[name] = np.full((bi.nm + 1) * width, SENTINEL, np.uint8)
                setattr(bo, name, seen[name].ctypes.data)

        res = ctx.arrival_zone_build({"pos_xz": W.pos}, W.zones, W.members, W.targets, patch=sentinel)
        for name, a in seen.items():
            assert (a[self.counts[2] * (8 if name == "sink_xz" else 1):] == SENTINEL).all(), name
        res.update(substate=seen["substate"], sink_valid=seen["sink_valid"], sink_xz=seen["sink_xz"].view(F).reshape(-1, 2))
        self.res = res
        return flat_build(res, len(W.zones))

    def dev(self, navlib, ctx):
        R = tab.Resident(navlib, ctx, self.W)
        _sync()
        R.call()
        ctx.sync()
        return flat_build(R.read(), len(self.W.zones))


class Dest:
    def __init__(self, n):
        rng = np.random.RandomState(n)
        self.tiles = rng.randint(8, 248, (n, 2))

    def queries(self, navlib):
        q = np.zeros(len(self.tiles), navlib.DEST_QUERY_DTYPE)
        p = np.array([aw.xz(MAP, MAP, int(r), int(c)) for r, c in self.tiles], F)
        q["x"], q["z"], q["flags"] = p[:, 0], p[:, 1], navlib.DQ_NEAREST | navlib.DQ_TILES
        return q

    def host(self, navlib, ctx):
        nearest, tiles, status = ctx.dest_queries(self.queries(navlib))
        return [nearest, status, np.array([len(x) for x in tiles], np.int32), np.concatenate(tiles + [np.zeros((0, 2), np.int16)])]

    def dev(self, navlib, ctx):
        import torch
        q = self.queries(navlib)
        n = len(q)
        d_nearest, d_off = full((n, 2), 7.0, torch.float32), full((n + 1,), 7, torch.int32)
        d_tiles, d_status = full((navlib.DQ_MAX_TILES * n, 2), 7, torch.int16), full((n,), 7, torch.uint8)
        d_q = t(q.view(np.uint8).reshape(n, 16))
        _sync()
        ctx.dest_queries_dev(d_q, n, d_nearest, d_off, d_tiles, navlib.DQ_MAX_TILES * n, d_status)
        ctx.sync()
        off = d_off.cpu().numpy()
        return [d_nearest.cpu().numpy(), d_status.cpu().numpy(), np.diff(off), d_tiles.cpu().numpy()[:off[-1]]]


class Order:
    def queries(self, navlib):
        q = np.zeros(5, navlib.ORDER_QUERY_DTYPE)
        for i in range(5):
            s, d = aw.xz(MAP, MAP, 20 + 9 * i, 30), aw.xz(MAP, MAP, 200 - 7 * i, 180)
            q[i] = (s[0], s[1], d[0], d[1], 12.0, 0, 15, navlib.OQ_IN_RANGE | navlib.OQ_REACHABLE)
        return q

    def host(self, navlib, ctx):
        return list(ctx.order_queries(self.queries(navlib)))

    def dev(self, navlib, ctx):
        import torch
        q = self.queries(navlib)
        n = len(q)
        d_dest, d_id, d_status = full((n, 2), 7.0, torch.float32), full((n,), 7, torch.int32), full((n,), 7, torch.uint8)
        d_q = t(q.view(np.uint8).reshape(n, 32))
        _sync()
        ctx.order_queries_dev(d_q, n, d_dest, d_id, d_status)
        ctx.sync()
        return [d_dest.cpu().numpy(), d_id.cpu().numpy().view(np.uint32), d_status.cpu().numpy()]


class Surround:
    def __init__(self, n=12):
        self.u = units(n)
        self.vel = np.full((n, 2), 0.25, F)
        self.target = np.array([(i + 1) % n if i % 3 else -1 for i in range(n)], np.int32)

    def host(self, navlib, ctx):
        return list(ctx.surround_queries(self.u, self.vel, self.target))

    def dev(self, navlib, ctx):
        import torch
        n = len(self.target)
        arrays = {"pos_xz": t(self.u["pos_xz"]), "radius": t(self.u["radius"]), "flags": t(self.u["flags"].view(np.int32))}
        w, keep = navlib.make_world(MAP, MAP, arrays)
        d_vel, d_tgt = t(self.vel), t(self.target)
        d_query, d_dest = full((n,), 7, torch.uint8), full((n, 2, 2), 7.0, torch.float32)
        _sync()
        ctx.surround_queries_dev(w, d_vel, None, d_tgt, n, d_query, d_dest)
        ctx.sync()
        return [d_query.cpu().numpy(), d_dest.cpu().numpy()]


class Repair:
    """Requests whose start tile is one of the blocked tiles of the map (a field to repair) -- and, with an overlay, more."""

    def __init__(self, overlay):
        self.overlay = np.array([[41, 40], [41, 41]], np.int16) if overlay else None

    def rows(self, navlib):
        W = aw.batch_world(3)
        reqs = np.zeros(2, navlib.REGION_REPAIR_REQ_DTYPE)
        for i, z in enumerate(W.zones[:2]):
            r, c = z["tiles"][1]                                            # (batch_world blocks tiles[1] of every zone)
            reqs[i] = (0, 0, 16 + 16 * i, r, c, r, c, 0, 0 if self.overlay is None else len(self.overlay))
        inout = np.random.RandomState(5).randint(0, 256, (2, STRIDE)).astype(np.uint8)
        return reqs, inout

    def host(self, navlib, ctx):
        reqs, inout = self.rows(navlib)
        return list(ctx.repair_region_fields(reqs, self.overlay, inout, STRIDE))

    def dev(self, navlib, ctx):
        import torch
        reqs, inout = self.rows(navlib)
        d_reqs, d_io, d_st = t(reqs.view(np.uint8).reshape(2, 20)), t(inout), full((2,), 7, torch.uint8)
        d_ov = None if self.overlay is None else t(self.overlay)
        _sync()
        ctx.repair_region_fields_dev(d_reqs, 2, 32, d_ov, d_io, STRIDE, d_st)
        ctx.sync()
        return [d_io.cpu().numpy(), d_st.cpu().numpy()]


class Seek:
    """Two enemy-seek requests over a snapshot of 40 units of two factions at war; bare: no exclude array, no seed rows."""

    def __init__(self, bare):
        self.bare, self.u = bare, units(40, seed=8)
        self.faction = (np.arange(40) % 2).astype(np.int32)
        self.mask = np.zeros(16, np.uint16)
        self.mask[0], self.mask[1] = 2, 1
        self.exclude = None if bare else (np.arange(40) % 5 == 0).astype(np.uint8)

    def rows(self, navlib):
        reqs = np.zeros(2, navlib.SEEK_REQ_DTYPE)
        reqs[0], reqs[1] = (navlib.SEEK_ENEMIES, 0, 1, 1, 0, -1), (navlib.SEEK_ENEMIES, 0, 2, 1, 1, -1)
        return reqs, np.random.RandomState(6).randint(0, 256, (2, STRIDE)).astype(np.uint8)

    def host(self, navlib, ctx):
        reqs, inout = self.rows(navlib)
        w, keep = navlib.make_world(MAP, MAP, self.u)
        g, keep2 = navlib.make_seek_game(self.faction, self.mask, self.exclude)
        status, bits = np.full(2, 7, np.uint8), np.full((2, 2048), SENTINEL, np.uint8)
        ctx._call("navhip_build_seek_fields", C.byref(w), C.byref(g), navlib._hp(reqs), 2, navlib._hp(inout), STRIDE,
                  navlib._hp(status), None if self.bare else navlib._hp(bits))
        return [inout, status, bits]

    def dev(self, navlib, ctx):
        import torch
        reqs, inout = self.rows(navlib)
        arrays = {"pos_xz": t(self.u["pos_xz"]), "radius": t(self.u["radius"]), "flags": t(self.u["flags"].view(np.int32))}
        w, keep = navlib.make_world(MAP, MAP, arrays)
        g, keep2 = navlib.make_seek_game(t(self.faction), self.mask, None if self.exclude is None else t(self.exclude))
        d_reqs, d_io, d_st = t(reqs.view(np.uint8).reshape(2, 12)), t(inout), full((2,), 7, torch.uint8)
        d_bits = full((2, 2048), SENTINEL, torch.uint8)
        _sync()
        ctx.build_seek_fields_dev(w, g, d_reqs, 2, d_io, STRIDE, d_st, None if self.bare else d_bits)
        ctx.sync()
        return [d_io.cpu().numpy(), d_st.cpu().numpy(), d_bits.cpu().numpy()]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def assert_same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.asarray(x).shape == np.asarray(y).shape and np.array_equal(bits(x), bits(y)), (what, "output", i)


# ---------------------------------------------------------------------------------------------
# 1. one arena, carved by another form in between, smaller and larger
# ---------------------------------------------------------------------------------------------
# The arena of a call is its rows, each rounded up to 256 bytes.  flock_update: 18 rows, of 3 zones 5 - 7 KB; dest_queries:
# 4 rows and 1 KB of tiles per query, 2 KB for one query and 70 KB for 64; zone_build: 25 rows, 6.4 KB at least, about 8 KB
# for three zones; flock_update of one zone 18 rows of 256 bytes (4.6 KB), of 50 zones above 30 KB.  A slot grows to 1.5
# times what is asked and never shrinks: each pair runs on a context of its own, whose slot A's first run sizes, and the
# larger call of the pair asks for more than 1.5 times that, so A's last run finds another buffer.
PAIRS = {"flock_update / dest_queries": (lambda: Flock(aw.batch_world(3)), lambda: Dest(1), lambda: Dest(64)),
         "zone_build / flock_update": (lambda: Build(build_world(3)), lambda: Flock(aw.batch_world(1)),
                                       lambda: Flock(aw.batch_world(50)))}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_shared_arena_changing_sizes(navlib, pair):
    A, small, large = (f() for f in PAIRS[pair])
    ctx = make_context(navlib)
    try:
        first = A.host(navlib, ctx)                                             # (the context's first host-buffer call)
        assert_same(first, A.dev(navlib, ctx), pair + ": A against its _dev form")
        for B in (small, large):
            assert_same(B.host(navlib, ctx), B.dev(navlib, ctx), pair + ": B against its _dev form")
            assert_same(A.host(navlib, ctx), first, pair + ": A again")
        if isinstance(A, Build):
            assert not first[0].any(), "the zones of A were to be built"
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. empty rows, absent arrays
# ---------------------------------------------------------------------------------------------
def flock_world(slots, keys, members):
    """Two FILLING zones without slots, without keys and / or without members."""
    W = aw.World(MAP, MAP)
    rng = np.random.RandomState(11)
    for k in range(2):
        tiles = aw.rect(40 + 30 * k, 40, 4, 5) if keys else []
        sl = np.array([aw.xz(MAP, MAP, 40 + 30 * k + i, 41) for i in range(3)], F) if slots else np.zeros((0, 2), F)
        z = aw.zone(MAP, MAP, tiles, sl, centre=aw.xz(MAP, MAP, 41 + 30 * k, 41), total=4)
        rows = aw.crowd(W, rng, aw.rect(40 + 30 * k, 40, 4, 5), 5, sl if slots else np.zeros((1, 2), F)) if members else []
        W.add(z, rows)
    return W.done()


EMPTY = [(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)]


@pytest.mark.parametrize("slots,keys,members", EMPTY)
def test_empty_rows_flock_update(navlib, ctx, slots, keys, members):
    W = flock_world(slots, keys, members)
    seen = {}

    def sentinel(fi, fo, zs, fs):
        """the output arrays of the call, one row longer than the call's counts, filled beforehand"""
        assert (fi.n_slots, fi.n_keys, fi.nm) == (3 * 2 * slots, 20 * 2 * keys, 5 * 2 * members)
        for name, rows, width in (("slot_ring", fi.n_slots, 4), ("substate", fi.nm, 1), ("sink_valid", fi.nm, 1), ("sink_xz", fi.nm, 8),
                                  ("status", fi.n_zones, 1)):
            seen[name] = (np.full((rows + 1) * width, SENTINEL, np.uint8), rows * width)
            setattr(fo, name, seen[name][0].ctypes.data)

    zones, mem, _ = ctx.arrival_flock_update({"pos_xz": W.pos}, W.zones, W.keys, W.members, patch=sentinel)
    for name, (a, owned) in seen.items():
        assert (a[owned:] == SENTINEL).all(), name
    res = taf.Resident(navlib, ctx, W)
    _sync()
    res.call()
    ctx.sync()
    dz, dm, dstatus = res.read()
    assert np.array_equal(seen["status"][0][:2], dstatus)
    assert np.array_equal(seen["slot_ring"][0][:seen["slot_ring"][1]].view(np.int32), np.concatenate([z["slot_ring"] for z in dz] + [np.zeros(0, np.int32)]))
    for name in ("substate", "sink_valid", "sink_xz"):
        assert np.array_equal(seen[name][0][:seen[name][1]], bits(np.concatenate([bits(m[name]) for m in dm])))
    assert_same(flat_flock((zones, [], [])), flat_flock((dz, [], [])), "the zone table and the companions")


# (slots, keys, members) of the call: zones with room and members are built; zones of three units wait (the gate asks for
# four), need no room and get none where the case says so -- n_slots = 0, n_keys = 0 and nm = 0, each alone and together
BUILD_EMPTY = [(1, 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (0, 0, 1), (0, 0, 0)]


@pytest.mark.parametrize("slots,keys,members", BUILD_EMPTY)
def test_empty_rows_zone_build(navlib, ctx, slots, keys, members):
    """Zones that wait (NAVHIP_AB_WAIT: every output repeats its input, axis / com / dest id keep the caller's -7 / 7) with
    and without room and members; the room of a zone that is built keeps what it held behind the new ranges."""
    built = (slots, keys, members) == (1, 1, 1)
    W = build_world(2) if built else build_world(2, members=3 if members else 0, total=3, room=(4 * slots, 4 * keys))
    B = Build(W)
    host, dev = B.host(navlib, ctx), B.dev(navlib, ctx)
    if not built:
        assert B.counts == (8 * slots, 8 * keys, 6 * members)
    assert_same(host, dev, "zone_build, slots %d keys %d members %d" % (slots, keys, members))
    assert host[0].tolist() == ([0, 0] if built else [navlib_ab_wait(navlib)] * 2)
    if not built:
        assert (host[4] == -7.0).all() and (host[5] == -7.0).all() and (host[6] == 7).all()
    # the spare row the wrapper keeps behind every shared array is nobody's: -7 / 7 as it was filled
    res = B.res
    assert (res["slots_xz"][-1] == -7.0).all() and res["slot_ring"][-1] == -7 and res["region_keys"][-1] == 7
    assert (res["axis_xz"][-1] == -7.0).all() and (res["com_xz"][-1] == -7.0).all() and res["com_dest_id"][-1] == 7


def navlib_ab_wait(navlib):
    return getattr(navlib, "AB_WAIT", 0x01)


def test_empty_rows_repair_without_overlay_and_seek_without_exclude_or_seed_rows(navlib, ctx):
    for form in (Repair(overlay=False), Repair(overlay=True), Seek(bare=True), Seek(bare=False)):
        host, dev = form.host(navlib, ctx), form.dev(navlib, ctx)
        assert_same(host, dev, type(form).__name__)
    assert (Seek(bare=True).host(navlib, ctx)[2] == SENTINEL).all()            # no seed rows asked for: none written


# ---------------------------------------------------------------------------------------------
# 3. the snapshot a completed host-buffer step leaves resident
# ---------------------------------------------------------------------------------------------
def step_arrays(navlib, n=64):
    u = units(n, seed=21)
    offs, members = navlib.flock_csr(np.zeros(n, np.int32), 1)
    return dict(u, vel_xz=np.zeros((n, 2), F), max_speed=np.full(n, 2.0, F), speed=np.full(n, 1.0, F), state=np.zeros(n, np.uint8),
                has_dest_los=np.zeros(n, np.uint8), flock=np.zeros(n, np.int32), flock_target_xz=aw.xz(MAP, MAP, 128, 128).reshape(1, 2),
                flock_offsets=offs, flock_members=members, vdes_xz=np.tile(np.array([[1.0, 0.0]], F), (n, 1)))


def settle_resident(navlib, ctx, arrays):
    """navhip_arrival_settle_resident through the wrapper of navhip_arrival_settle (the same arguments): one unit, one zone."""
    W = aw.batch_world(1)
    one = {"uid": [0], "zone": [0], "new_pos_xz": arrays["pos_xz"][:1], "nsettled": [0], "substate": [0], "sink_valid": [0],
           "sink_xz": np.zeros((1, 2), F), "order_pos_xz": np.zeros((1, 2), F), "progress_anchor_xz": np.zeros((1, 2), F),
           "progress_anchored": [0], "stuck": [0]}
    call = ctx._call
    ctx._call = lambda name, *a: call(name + "_resident" if name == "navhip_arrival_settle" else name, *a)
    try:
        return ctx.arrival_settle(arrays, W.zones, W.keys, one)
    finally:
        del ctx._call


# read from the code before the forms moved: nh_stage_in on a slot in front of NH_STAGE_CALL0 drops the snapshot, and only
# the surround and seek forms stage there (positions, radii and flags, through nh_stage_world); the arrival forms reserved
# their arena without staging into it, the others staged in the call-local slots
DROPS = {"flock_update": False, "zone_build": False, "dest_queries": False, "order_queries": False, "surround_queries": True,
         "repair_region_fields": False, "build_seek_fields": True}
FORMS = {"flock_update": lambda: Flock(aw.batch_world(1)), "zone_build": lambda: Build(build_world(1)), "dest_queries": lambda: Dest(2),
         "order_queries": Order, "surround_queries": Surround, "repair_region_fields": lambda: Repair(overlay=True),
         "build_seek_fields": lambda: Seek(bare=False)}


@pytest.mark.parametrize("name", sorted(FORMS))
def test_resident_snapshot_after_each_host_form(navlib, ctx, name):
    arrays = step_arrays(navlib)
    ctx.agent_step_async(arrays)
    settle_resident(navlib, ctx, arrays)                                        # accepted: the step's snapshot is resident
    FORMS[name]().host(navlib, ctx)
    if DROPS[name]:
        with pytest.raises(navlib.NavHipError) as e:
            settle_resident(navlib, ctx, arrays)
        assert "no completed host-buffer step of this size is resident" in str(e.value)
    else:
        settle_resident(navlib, ctx, arrays)
