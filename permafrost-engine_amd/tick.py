"""The benchmark / demo driver of one navigation tick, everything resident in HBM.

One tick = (1) rebuild every chunk field of this rank's share of the flow fields into the field
pool, (2) [multi-GPU, only the tiles another rank samples] exchange baked tiles, (3) velocity step
+ position accept for this rank's slab of agents, sampling the pool on the device, (4) [multi-GPU]
all-gather the slab results, (5) advance the snapshot (pos <- new_pos, vel <- new velocity).  Nothing is cached
between ticks: the worst case of the reference's tick, where every cached field was invalidated
(N_ApplyDeferredInvalidations, nav.c:2208).

PyTorch supplies device buffers, the stream and torch.distributed; all compute is libnavhip.
"""
import ctypes as C
import os
import time

import numpy as np
import torch

from . import dist as pdist
from . import navhip, plan, synth
from .plan import region_grid        # noqa: F401  (bench.py and the tests read it here)


class _HostCuda:
    """What NavTick uses of torch.cuda, for the ONE case in which "device" memory is host memory: the library under test
    is the host-emulator build of tests/hostsim (NAVHIP_LIB names _navhip_emu.so; test infrastructure, see
    tests/test_emulated_cpu.py).  Everything there runs synchronously and in order, so streams and events carry no state
    beyond a timestamp."""

    class Stream:
        def __init__(self, device=None, priority=0):
            self.cuda_stream = 0x1000           # (an opaque non-null handle: the emulated runtime never looks inside)

        def wait_event(self, event):
            pass

        def wait_stream(self, stream):
            pass

        def synchronize(self):
            pass

    class ExternalStream(Stream):
        def __init__(self, handle, device=None):
            self.cuda_stream = handle or 0x1000

    class Event:
        def __init__(self, enable_timing=False):
            self.t = 0.0

        def record(self, stream=None):
            self.t = time.perf_counter()

        def elapsed_time(self, other):
            return (other.t - self.t) * 1e3

        def synchronize(self):
            pass

    class _Props:
        multi_processor_count = 256

    @staticmethod
    def stream(s):
        import contextlib
        return contextlib.nullcontext()

    @staticmethod
    def set_device(dev):
        pass

    @staticmethod
    def synchronize(dev=None):
        pass

    @staticmethod
    def get_device_properties(dev):
        return _HostCuda._Props()


EMULATED = os.path.basename(os.environ.get("NAVHIP_LIB", "")) == "_navhip_emu.so"
tcuda = _HostCuda if EMULATED else torch.cuda


class NavTick:
    """World layout (weak scaling): `world` REGIONS of chunk_w x chunk_w chunks
    tiling one map (region_grid(world): 1x2, 2x2, 2x4, 4x4 ... regions; a map side is at most 64
    chunks, the reference's 6-bit chunk ids).  Region r -- its
    `fields_per_rank` destinations, the chunk-field requests of those destinations (every chunk of
    the region: the corridor the planner would emit for units and destination inside the region)
    and its `agents_per_rank` agents, flock = destination -- belongs to rank r: the agents a rank
    steps sample the fields that rank built, so the baked tiles only travel when a flock has members
    on another rank (`tile_exchange`).  The map planes and the entity snapshot are replicated; agents
    of neighbouring regions see each other through the all-gathered snapshot.  What that world is -- tiling, obstacles,
    destinations, agents, request stream, slot tables -- is planned on the host by plan.py; this class puts it on the
    device and enqueues the tick."""

    def __init__(self, chunk_w=16, fields_per_rank=64, agents_per_rank=100_000, rank=0, world=1,
                 device=0, hz=20, seed_map=1234, verbose=False, obstacles=0, move_frac=0.01,
                 obstacle_ticks=128, tile_exchange="auto", solo=False, shared_map=False, crowd_cells=0,
                 debug_outputs=False, pipeline_fields=False, exchange="torch", planner_requests=True,
                 straddle=0.0, los=False, flow_velocities=False, share_fields=False, driver="c", serial=None,
                 time_fields=False, los_repair=None):
        self.rank, self.world, self.device_index = rank, world, device
        self.dev = torch.device("cpu") if EMULATED else torch.device("cuda", device)
        tcuda.set_device(self.dev)
        t0 = time.time()
        # ---- the plan (plan.py, host only); the two planes only the library gives come in between ---------------
        lay = plan.layout(chunk_w, world, shared_map)
        self.W = chunk_w                            # region side in chunks
        self.shared_map, self.reg_rows, self.reg_cols = lay.shared_map, lay.reg_rows, lay.reg_cols
        self.Wt, self.H, self.nchunks = lay.Wt, lay.H, lay.nchunks     # whole map, in chunks
        self.K = fields_per_rank * world            # flow fields (destinations) in the whole job
        self.N = agents_per_rank * world            # agents in the whole job
        self.hz = hz
        self.solo = bool(solo)
        # synthetic map, identical on every rank
        self.grid = grid = synth.cost_grid(lay.Wt, lay.H, seed=seed_map)
        self.map_cells = grid.size
        self.n_obstacles = obstacles
        if obstacles:
            # (_circ_host: parity tests replay the start circles through the reference)
            self._circ_host, self._moves_host = plan.obstacle_stream(grid, lay, obstacles, move_frac, obstacle_ticks)
            self.n_moves = self._moves_host.shape[1]
        blockers, liid = self._make_context(grid)
        dests, ag = plan.population(grid, lay, world, fields_per_rank, agents_per_rank, hz, blockers, crowd_cells, straddle)
        rq = plan.request_stream(grid, lay, dests, ag["flock"], liid, rank, world, fields_per_rank, agents_per_rank,
                                 tile_exchange, solo, planner_requests, share_fields, obstacles)
        self.tile_exchange, self.request_source = rq.tile_exchange, rq.request_source
        self.req_bounds, self.xchg_bounds = rq.req_bounds, rq.xchg_bounds      # (xchg: the rows of a rank the others need)
        self.n_requests_served, self._dest_of_req = rq.n_requests_served, rq.dest_of_req
        n_req = len(rq.reqs)
        # field slot = position in the (local) request stream
        self.req_begin, self.req_end = (0, n_req) if solo else self.req_bounds[rank]
        self.n_req_local = self.req_end - self.req_begin
        self.n_req_total = self.n_req_local * world if self.tile_exchange == "none" else n_req
        self.agent_bounds = [pdist.slab(self.N, r, world) for r in range(world)]
        self.a0, self.a1 = (0, self.N) if solo else pdist.slab(self.N, rank, world)

        self.tick_no = 0
        self.overlap = True
        self._make_device_state(rq, dests, ag, liid, debug_outputs)
        self._make_los(los, los_repair, lay, dests)
        self._make_streams(exchange)
        self._make_structs()
        # ---- start-up builds ------------------------------------------------------------------------------------
        if obstacles:
            # the pool starts fully built (untimed), afterwards only changed chunks are repaired
            full = rq.reqs.copy()
            full["flags"] = navhip.REQ_LIVE_IIDS
            d_full = self._dev(full.view(np.uint8).reshape(n_req, 32))
            self.ctx.build_fields_dev(d_full, n_req, self.pool, stream=self.stream.cuda_stream)
            self.stream.synchronize()
        # pipeline_fields: the fields tick t+1 samples are built DURING tick t, on their own stream, into
        # the other half of a double-buffered pool, starting once the narrow, serial front of tick t's
        # agent step (spatial hash + neighbour walk) is through.  Same work per tick -- one rebuild of
        # every chunk field, one step of every agent --, same results (the static map does not depend on
        # the agents); the field builds just stop gating the agent step of their own tick.  (With moving
        # obstacles the blocker updates of tick t+1 would race with the probes of tick t: not pipelined.)
        self.pipeline_fields = bool(pipeline_fields) and not obstacles
        if self.pipeline_fields:
            self._start_pipeline()
        if flow_velocities:
            self._flow_aligned_velocities()
        if not hasattr(self, "velocity_source"):
            self.velocity_source = "N(0, 0.35) per component (synth.agents)"
        self._choose_driver(driver, serial, time_fields)
        if verbose:
            print("[rank %d] setup %.1fs: %d chunk-field requests (%d local), %d agents (%d local)"
                  % (rank, time.time() - t0, n_req, self.n_req_local, self.N, self.a1 - self.a0), flush=True)

    def _make_context(self, grid):
        """The context with the map planes uploaded.  Returns the two planes of the plan that only the library gives:
        the blocker plane behind the start circles (None without obstacles) and the local-island plane."""
        Wt, H = self.Wt, self.H
        self.ctx = navhip.NavContext(Wt, H, device=self.device_index)
        self.ctx.upload_plane(0, navhip.PLANE_COST_BASE, synth.to_chunks(grid))
        self.ctx.upload_plane(0, navhip.PLANE_BLOCKERS, np.zeros((H, Wt, 64, 64), np.uint16))
        blockers = None
        if self.n_obstacles:
            self.ctx.N_BlockersUpdate(self._circ_host)
            self.ctx.changed_chunks(0, clear=True)
            blockers = synth.from_chunks(self.ctx.download_plane(0, navhip.PLANE_BLOCKERS))
        self.ctx.relabel_local_islands(0)           # n_update_local_island_field on the device
        return blockers, synth.from_chunks(self.ctx.download_plane(0, navhip.PLANE_LOCAL_ISLANDS))

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _make_device_state(self, rq, dests, ag, liid, debug_outputs):
        """The request stream, the move stream, the pool, the snapshot (self.t) and the step's outputs on the device;
        self.host keeps what they were made from."""
        dev, n, n_req = self._dev, self.N, len(rq.reqs)
        offs, members = navhip.flock_csr(ag["flock"], self.K)
        targets = synth.cell_centre(self.Wt, self.H, dests[:, 0], dests[:, 1])
        if self.n_obstacles:
            self.d_moves = dev(self._moves_host.view(np.uint8).reshape(len(self._moves_host), self.n_moves, 24))
        self.d_reqs = dev(rq.reqs.view(np.uint8).reshape(n_req, 32))
        self.pool = torch.zeros((n_req, 4096), dtype=torch.uint8, device=self.dev)
        self.t = {
            "pos_xz": dev(ag["pos"]), "vel_xz": dev(ag["vel"]), "radius": dev(ag["radius"]),
            "max_speed": dev(ag["max_speed"]), "speed": dev(ag["speed"]),
            "flags": dev(np.full(n, navhip.ENTITY_FLAG_MOVABLE, np.uint32)),
            "state": dev(np.zeros(n, np.uint8)), "has_dest_los": dev(np.zeros(n, np.uint8)),
            "flock": dev(ag["flock"]), "flock_target_xz": dev(targets.astype(np.float32)),
            "flock_offsets": dev(offs), "flock_members": dev(members),
            "flock_field_slot": dev(rq.slot_tbl), "field_pool": self.pool,
        }
        self.new_pos = torch.zeros((n, 2), dtype=torch.float32, device=self.dev)
        self.new_vel = torch.zeros((n, 2), dtype=torch.float32, device=self.dev)
        self.status = torch.zeros(n, dtype=torch.uint8, device=self.dev)
        self.res4 = torch.zeros((n, 4), dtype=torch.float32, device=self.dev) if self.world > 1 else None
        # (parity tests: the desired direction / preferred velocity every agent was stepped with)
        self.vdes_out = torch.zeros((n, 2), dtype=torch.float32, device=self.dev) if debug_outputs else None
        self.vpref_out = torch.zeros((n, 2), dtype=torch.float32, device=self.dev) if debug_outputs else None
        # host copies of what the job was built from (parity tests replay it through the reference)
        self.host = {"reqs": rq.reqs, "dest_of_req": rq.dest_of_req, "slot_tbl": rq.slot_tbl, "dests": dests,
                     "targets": targets.astype(np.float32), "flock": ag["flock"], "flock_offsets": offs,
                     "flock_members": members, "radius": ag["radius"], "max_speed": ag["max_speed"],
                     "speed": ag["speed"], "liid": liid}

    def _make_los(self, los, los_repair, lay, dests):
        """"has_dest_los computed by the reference LOS code".
        los=True: the LOS fields of every (destination, chunk) the reference planner would hold -- its own
        N_LOSFieldCreate chain, from the fixture -- are built on the device (navhip_build_los_dev, level by level
        along the chain) and every agent's has_dest_los is answered per tick from them (NAVHIP_LOS_LOOKUP:
        N_HasDestLOS, nav.c:4026).  Built once at start-up like the reference's LOS cache (a static map).
        los_repair: what happens to those fields when blockers move.  None = nothing (the fields of the start-up planes
        answer for ever); "reference" = behind every blocker batch the fields of the changed chunks are rebuilt, each from
        whatever its predecessor holds (the reference's cache: fieldcache.c:526-535, nav.c:2026-2039); "downstream" = and
        every field built from a rebuilt one, so that the pool is the one a fresh build on the current planes gives
        (navhip_los_chain_*, csrc/los_chain_api.hip)"""
        if los_repair not in (None, "reference", "downstream"):
            raise ValueError("los_repair: None, 'reference' or 'downstream'")
        self.los_repair = los_repair
        self.los_chain = None
        self.los_source = "has_dest_los = 0 for every agent (no LOS fields)"
        self.n_los = 0
        if los:
            lc = synth.planner_los(self.grid, dests) if (self.world == 1 or self.shared_map) else None
            if lc is None:
                self.los_source = "has_dest_los = 0: no planner LOS fixture for this world"
            else:
                self._build_los(plan.los_layout(lc, dests, lay, self.K))

    def _make_streams(self, exchange):
        # the agent chain: the library's own stream (a hardware queue to itself, the same one for every context of the
        # process -- navhip_stream_main; NAVTICK_TORCH_STREAM=1: a stream of torch's pool, as rounds 1-5 had it, for the A/B)
        if os.environ.get("NAVTICK_TORCH_STREAM") == "1":
            self.stream = tcuda.Stream(device=self.dev, priority=-1)
        else:
            self.stream = tcuda.ExternalStream(self.ctx.stream_main(), device=self.dev)
        # multi-GPU: the slab all-gather of tick t runs on its own stream and is only awaited by the
        # snapshot consumers of tick t+1 (spatial hash + cohesion, then the agent step); the field
        # builds of tick t+1 do not read positions and overlap with it
        self.pipelined = self.world > 1 and not self.solo
        # (the library's own streams for everything beside the agent chain: each has a hardware queue to itself, on a pipe of
        # the command processor that self.stream's queue does not sit on -- navhip_stream_beside)
        self.comm = tcuda.ExternalStream(self.ctx.stream_beside(self.stream.cuda_stream), device=self.dev) if self.pipelined else None
        # exchange = "navhip": the slab all-gather goes through the library's own C entry point
        # (navhip_comm_allgather_step_dev: librccl called directly -- what a C host uses) instead of
        # torch.distributed; rank 0's communicator id travels over the process group that launched us
        self.exchange_mode = exchange if self.pipelined else "none"
        if self.exchange_mode == "navhip":
            import torch.distributed as tdist
            box = [navhip.comm_unique_id() if self.rank == 0 else None]
            tdist.broadcast_object_list(box, src=0)
            self.ctx.comm_init(self.rank, self.world, box[0])
            self._bounds = np.array([b for b, _ in self.agent_bounds] + [self.N], np.int32)
        self.ev_step = tcuda.Event()
        self.ev_comm = tcuda.Event()
        self._comm_pending = False
        self._stepped = False

    def _start_pipeline(self):
        """pipeline_fields: the field stream, the second pool, and the fields of tick 0."""
        # Where the builds of tick t+1 run inside tick t is a scheduling choice, measured (round 3, after the
        # front of the step had become a third shorter; 20 ticks after 5 / 100 ticks, ms per tick):
        #   configs[2] (16 384 chunk fields, 0.09 ms alone): behind the NEIGHBOUR WALK on 5 of the 8 XCDs
        #     0.316-0.320 / 0.455-0.460 (128 ... 176 CUs all the same); on 192: 0.327 / 0.472; on all 256:
        #     0.336 / 0.477; started with the tick on 192 (round 2's choice): 0.340 / 0.483.  The front --
        #     spatial hash, neighbour walk: the critical path -- then only shares the chip with the cohesion
        #     kernel, and the ClearPath phase keeps three XCDs to itself.
        #   configs[3] (131 072 chunk fields, 0.58 ms alone -- as long as the rest of the tick): started
        #     WITH THE TICK on ALL compute units 0.97; with the tick on 224 / 192: 1.01 / 1.08; behind the
        #     neighbour walk on 224 / 160: 0.99 / 1.20.
        #   configs[1] (4 096 chunk fields, 45 us): no difference (0.259-0.265).
        ncu_all = tcuda.get_device_properties(self.dev).multi_processor_count
        long_build = self.n_req_local >= 65536
        ncu = int(os.environ.get("NAVTICK_FIELD_CUS", str(ncu_all if long_build else ncu_all * 5 // 8)))
        if 0 < ncu < ncu_all:
            self.fstream = tcuda.ExternalStream(self.ctx.stream_beside(self.stream.cuda_stream, ncu_all - ncu, ncu), device=self.dev)
        else:
            self.fstream = tcuda.ExternalStream(self.ctx.stream_beside(self.stream.cuda_stream), device=self.dev)
        self.fields_after = os.environ.get("NAVTICK_FIELDS_AFTER", "start" if long_build else "neighbours")
        # nothing wide is enqueued on self.stream between prefetch and step: the front stays on it
        # ... and the snapshot buffers ping-pong: the one a step read is next written by the ClearPath
        # kernels of the following step
        self.prefetch_flags = navhip.PREFETCH_FRONT_INLINE | navhip.PREFETCH_SNAPSHOT_HELD
        self.pool_next = torch.zeros_like(self.pool)
        self.ev_fields, self.ev_fields_next = tcuda.Event(), tcuda.Event()
        self.fev = []
        self._build_fields(self.pool, self.stream)        # the fields of tick 0 (start-up, untimed)
        with tcuda.stream(self.stream):
            self._exchange_tiles(self.pool)
        self.ev_fields.record(self.stream)
        self.stream.synchronize()

    def _choose_driver(self, driver, serial, time_fields):
        # driver: who enqueues a tick.  "c" = the library's own loop (navhip_tick_*, csrc/tick_api.hip: ONE call per tick,
        # the schedule below in C) -- for every world whose baked tiles do not travel; "python" = this file's compute() /
        # exchange() / advance(), the reference implementation of that schedule, which the C loop is tested against.
        # serial (C driver only; NAVTICK_SERIAL=1): the whole tick on ONE stream, no side streams and no events -- the
        # host side shrinks to 48 us per tick, the tick does not (0.455 against 0.342 ms at configs[2]: the overlap of
        # cohesion / ClearPath / field builds is gone; profiles/r05_host_overhead_c.txt).  An option for a host that
        # wants one stream, not a default.
        self.driver = driver if (self.tile_exchange == "none" or self.solo) else "python"
        if serial is None:
            serial = os.environ.get("NAVTICK_SERIAL") == "1"
        self.serial = bool(serial)
        # time_fields (C driver): HIP events on the FIELD stream around the builds of every fourth tick -- how long the
        # builds take inside the tick, beside the agent step (navhip_tick_info.fields_ms; field_build_times())
        self.time_fields = bool(time_fields)
        self._ctick = None
        self.tick_driver = "python (tick.py)"
        self.ev = []                   # (phase, start_event, end_event) of the timed steps
        self.tick_ev = []              # one event at the start of every tick_every-th recorded tick
        self.tick_every, self._tick_rec = 5, 0
        self.record = False
        self.mark_every = 20

    def _build_fields(self, pool, stream):
        """This rank's slice of the request stream into its rows of `pool`, on `stream`."""
        if self.n_req_local:
            self.ctx.build_fields_dev(self.d_reqs[self.req_begin:self.req_end], self.n_req_local,
                                      pool[self.req_begin:self.req_end], stream=stream.cuda_stream)

    def _exchange_tiles(self, pool):
        """The tile rows of `pool` that travel, to every rank (on torch's current stream)."""
        if self.tile_exchange != "none" and not self.solo:
            pdist.exchange_rows(pool, self.xchg_bounds, self.rank, self.world)

    def _build_los(self, ll):
        """The planner's LOS chain on the device, laid out by plan.los_layout: one navhip_build_los_dev per level, each
        field from its predecessor."""
        n = len(ll.reqs)
        d_reqs = self._dev(ll.reqs.view(np.uint8).reshape(n, 16))
        d_prev_slot = self._dev(ll.prev_slot)
        self.los_pool = torch.zeros((n, 4096), dtype=torch.uint8, device=self.dev)
        self._los_build_args = (d_reqs, d_prev_slot, ll.bounds)
        self._build_los_pool(self.los_pool)
        self.t["los_pool"] = self.los_pool
        self.t["flock_los_slot"] = self._dev(ll.slot_tbl)
        self.t["has_dest_los"] = torch.full((self.N,), navhip.LOS_LOOKUP, dtype=torch.uint8, device=self.dev)
        levels = len(ll.bounds) - 1
        self.host["los"] = {"reqs": ll.reqs, "slot_tbl": ll.slot_tbl, "levels": levels, "prev_slot": ll.prev_slot,
                            "level": ll.level}
        self.n_los = n
        self.los_source = ("device lookup (NAVHIP_LOS_LOOKUP) in %d LOS fields built by navhip_build_los from the "
                           "reference planner's N_LOSFieldCreate chain (fixture), %d levels" % (n, levels))
        if self.los_repair is not None:
            self.los_chain = self.ctx.los_chain_create(ll.reqs, ll.chain_prev, self.los_pool)
            self.los_flags = navhip.LOS_REFRESH_DOWNSTREAM if self.los_repair == "downstream" else 0
            self.los_source += ("; kept current behind every blocker batch by navhip_los_chain_refresh (%s)"
                                % ("the changed chunks' fields and every field built from them" if self.los_flags else
                                   "the changed chunks' fields only, as the reference's cache"))
        else:
            self.los_source += "; never rebuilt (los_repair=None)"

    def _build_los_pool(self, pool):
        """Every LOS field of the chain into `pool` from the planes as they are now: one navhip_build_los_dev per level,
        the predecessors gathered from the level before."""
        d_reqs, d_prev_slot, bounds = self._los_build_args
        tcuda.synchronize(self.dev)
        for L in range(len(bounds) - 1):
            b, e = int(bounds[L]), int(bounds[L + 1])
            if e == b:
                continue
            d_prev = pool.index_select(0, d_prev_slot[b:e]) if L > 0 else None
            tcuda.synchronize(self.dev)     # (torch's stream -> the library's: start-up, untimed)
            self.ctx.build_los_dev(d_reqs[b:e], e - b, d_prev, pool[b:e])
            self.ctx.sync()

    def _los_refresh(self, stream):
        # (one place for the Python schedule's refresh: tests put a full build here to hold the refresh against)
        self.los_chain.refresh(self.los_flags, stream=stream)

    def _flow_aligned_velocities(self):
        """initial velocity = 0.5 max along the sampled flow direction + N(0, 0.1).  The
        directions are the ones the device samples (one untimed step of the start-up pool); seed 11."""
        n = self.N
        keep = self.vdes_out, self.vpref_out
        self.vdes_out = torch.zeros((n, 2), dtype=torch.float32, device=self.dev)
        self.vpref_out = torch.zeros((n, 2), dtype=torch.float32, device=self.dev)
        if not self.pipeline_fields and not self.n_obstacles:
            self._build_fields(self.pool, self.stream)
        self._make_structs()
        wb, we = self.world_s.work_begin, self.world_s.work_end
        self.world_s.work_begin, self.world_s.work_end = 0, n          # (every rank samples every agent: replicated)
        self.ctx.agent_step_dev(self.world_s, self.out_s, stream=self.stream.cuda_stream)
        self.stream.synchronize()
        self.ctx.sync()
        vdes = self.vdes_out.cpu().numpy()
        rng = np.random.RandomState(11)
        speed = self.host["max_speed"][:, None] / float(self.hz)
        vel = (0.5 * speed * vdes + rng.normal(0.0, 0.1, size=(n, 2))).astype(np.float32)
        self.t["vel_xz"] = torch.from_numpy(vel).to(self.dev)
        if self.world > 1 and not self.solo:
            # (a rank only holds the fields its own agents sample: every rank keeps its slab's rows)
            pdist.exchange_rows(self.t["vel_xz"], self.agent_bounds, self.rank, self.world)
        self.vdes_out, self.vpref_out = keep
        self.world_s.work_begin, self.world_s.work_end = wb, we
        self._make_structs()
        self.velocity_source = "0.5 max_speed/hz along the sampled flow direction + N(0, 0.1) (SURVEY 8(d))"

    def _make_structs(self):
        arrays = dict(self.t)
        # (a rank that steps a slab: this driver never changes its flock tables -- the promise that lets the
        # library carry the cohesion term's lane grouping from tick to tick, navhip.h: static_epoch)
        if (self.a0, self.a1) != (0, self.N):
            arrays["static_epoch"] = 1
        self.world_s, self._keep = navhip.make_world(self.Wt, self.H, arrays, hz=self.hz)
        self.world_s.work_begin, self.world_s.work_end = self.a0, self.a1
        self.out_s = navhip.StepOut()
        self.out_s.vel_xz = self.new_vel.data_ptr()
        self.out_s.new_pos_xz = self.new_pos.data_ptr()
        self.out_s.status = self.status.data_ptr()
        if self.vdes_out is not None:
            self.out_s.vdes_xz = self.vdes_out.data_ptr()
            self.out_s.vpref_xz = self.vpref_out.data_ptr()

    def _mark(self, name):
        # phase timing by HIP events on the launch stream, on every `mark_every`-th recorded tick:
        # timing events are not free (a marker packet between back-to-back kernels; six per tick
        # cost ~4 % of the tick when recorded every tick)
        if not self.record or self.tick_no % self.mark_every:
            return None
        e = tcuda.Event(enable_timing=True)
        e.record(self.stream)
        return (name, e)

    # ---- the C driver ---------------------------------------------------------------------------------------------
    def _c_tick(self):
        """The navhip_tick of the current buffers (made on first use; dropped whenever the Python path steps)."""
        if self._ctick is not None:
            return self._ctick
        d = navhip.TickDesc()
        C.memmove(C.byref(d.world), C.byref(self.world_s), C.sizeof(navhip.World))
        d.pos_xz_1, d.vel_xz_1 = self.new_pos.data_ptr(), self.new_vel.data_ptr()
        d.status = self.status.data_ptr()
        if self.vdes_out is not None:
            d.vdes_xz, d.vpref_xz = self.vdes_out.data_ptr(), self.vpref_out.data_ptr()
        d.n_reqs, d.req_slot0 = self.n_req_local, self.req_begin
        d.dev_reqs = self.d_reqs[self.req_begin:self.req_end].data_ptr() if self.n_req_local else None
        keep = [self.world_s, self._keep, self.new_pos, self.new_vel, self.status, self.d_reqs, self.pool]
        d.stream = self.stream.cuda_stream
        if self.pipeline_fields:
            d.field_pool_1 = self.pool_next.data_ptr()
            d.field_stream = self.fstream.cuda_stream
            d.fields_stage = navhip.STAGE_START if self.fields_after == "start" else navhip.STAGE_NEIGHBOURS
            keep.append(self.pool_next)
        if self.n_obstacles:
            d.dev_moves, d.n_moves, d.n_move_ticks = self.d_moves.data_ptr(), self.n_moves, int(self.d_moves.shape[0])
            d.move_tick0 = self.tick_no % int(self.d_moves.shape[0])
        if self.pipelined and self.exchange_mode == "navhip":
            self._bounds_c = np.ascontiguousarray(self._bounds, np.int32)
            d.bounds = self._bounds_c.ctypes.data
            d.comm_stream = self.comm.cuda_stream
        # (the snapshot arrays are this object's own: nothing else writes them or enqueues on its stream between ticks)
        d.flags = ((navhip.TICK_SERIAL if self.serial else 0) | (navhip.TICK_TIME_FIELDS if self.time_fields else 0)
                   | navhip.TICK_OWNS_SNAPSHOT)
        self._ctick = navhip.Tick(self.ctx, d, keep)
        if self.los_chain is not None:
            self._ctick.set_los_chain(self.los_chain, self.los_flags)
        self._ctick_tick0 = self.tick_no
        self.tick_driver = "c (navhip_tick_run%s)" % (", one stream" if self.serial else "")
        return self._ctick

    def field_build_times(self):
        """(sum of milliseconds, samples) of the field builds the C tick has timed so far (time_fields=True)."""
        if self._ctick is None:
            return 0.0, 0
        info = self._ctick.info()
        return info.fields_ms * info.fields_samples, int(info.fields_samples)

    def _c_tick_drop(self):
        if self._ctick is not None:
            self._ctick.sync()
            self.c_tick_info = self._ctick.info()
            self._ctick.close()
            self._ctick = None
            if self.pipeline_fields:
                # (the Python path's event of "this tick's fields are built": they are -- everything was waited for)
                self.ev_fields.record(self.stream)
            self._make_structs()

    def _step_c(self):
        T = self._c_tick()
        if self.pipelined and self.exchange_mode != "navhip":
            # torch.distributed between the two halves of the C tick: the tick starts behind the previous exchange
            if self._comm_pending:
                self.stream.wait_event(self.ev_comm)
            T.compute()
            self.ev_step.record(self.stream)
            self.exchange()
            T.advance()
        else:
            T.run(1)
        # the Python view of the ping-pong; where it differs from advance():
        #   the pools swap only when the C tick builds ahead (on one stream it builds in place: tick_api.hip, `ahead`)
        #   ev_fields is not swapped: only the Python schedule waits for it, and _c_tick_drop records it afresh
        #   no _make_structs: the C tick holds its own two sets
        self._swap_buffers(self.pipeline_fields and not self.serial)
        self.tick_no += 1

    def _swap_buffers(self, pools):
        """Ping-pong the snapshot: what the step wrote is the next tick's positions and velocities; `pools`: and the
        pool built ahead is the one the next tick samples."""
        self.t["pos_xz"], self.new_pos = self.new_pos, self.t["pos_xz"]
        self.t["vel_xz"], self.new_vel = self.new_vel, self.t["vel_xz"]
        if pools:
            self.pool, self.pool_next = self.pool_next, self.pool
            self.t["field_pool"] = self.pool

    def step(self):
        """One tick, asynchronous on self.stream."""
        use_c = self.driver == "c" and not (self.record and self.mark_every <= 1)
        if self.record:
            # one timing event every `tick_every` ticks: an event on the agent stream is a packet on the
            # tick's critical path (recording every tick cost 1.5-2 % of the tick)
            if self._tick_rec % self.tick_every == 0:
                e = tcuda.Event(enable_timing=True)
                e.record(self.stream)
                self.tick_ev.append(e)
            self._tick_rec += 1
        if use_c:
            return self._step_c()
        self._c_tick_drop()
        self.compute()
        self.exchange()
        self.advance()

    def compute(self):
        """Field builds + velocity step of this rank's share (everything up to the exchange)."""
        s = self.stream
        self._marks = marks = []
        if self.pipelined and self.overlap:
            # behind the previous tick's all-gather, concurrently with the field builds below
            with tcuda.stream(self.comm):
                self.ctx.agent_prefetch_dev(self.world_s, stream=self.comm.cuda_stream)
        if self.pipeline_fields:
            return self._compute_pipelined(marks)
        with tcuda.stream(s):
            # snapshot-only parts of the agent step (spatial hash, cohesion: they read no nav plane)
            # start now on the library's side streams and overlap with the blocker updates and the
            # field builds below
            if self.overlap and not self.pipelined:
                self.ctx.agent_prefetch_dev(self.world_s, stream=s.cuda_stream)
            if self.n_obstacles:
                marks.append(self._mark("blockers"))
                t = self.tick_no % self.d_moves.shape[0]
                self.ctx.blockers_circles_dev(self.d_moves[t], self.n_moves, stream=s.cuda_stream)
                if self.los_chain is not None:
                    self._los_refresh(s.cuda_stream)
            marks.append(self._mark("fields"))
            self._build_fields(self.pool, s)
            if self.n_obstacles:
                self.ctx.clear_changed(stream=s.cuda_stream)
            marks.append(self._mark("gather_tiles"))
            self._exchange_tiles(self.pool)
            marks.append(self._mark("agents"))
            if self._comm_pending:
                s.wait_event(self.ev_comm)            # the other ranks' rows of the snapshot
            self.ctx.agent_step_dev(self.world_s, self.out_s, stream=s.cuda_stream)
            marks.append(self._mark("gather_agents"))
            self.ev_step.record(s)

    def _compute_pipelined(self, marks):
        s, f = self.stream, self.fstream
        # In a jam the workgroup ClearPath searches hold every register of the chip for milliseconds: a build
        # that starts behind the neighbour walk has not got its workgroups resident by then, finishes after
        # them, and the next step waits for it (crowded world: 5.3 -> 6.8 ms per tick).  The list lengths of
        # the last steps arrive in pinned memory without a wait: from a jam's worth of such searches on, the
        # builds start with the tick.
        stage = self.fields_after
        if stage == "neighbours" and self.ctx.step_lists_peek()[4] >= 8192:
            stage = "start"
        if stage == "start" and self.pipelined:
            f.wait_stream(s)                      # (the end of the previous tick)
        if not self.pipelined:
            with tcuda.stream(s):
                # (this object's arrays and stream: the snapshot of a tick is the output of the last one)
                follows = navhip.PREFETCH_FOLLOWS_STEP if self._stepped else 0
                self.ctx.agent_prefetch_dev(self.world_s, stream=s.cuda_stream, flags=self.prefetch_flags | follows)
        with tcuda.stream(s):
            marks.append(self._mark("agents"))
            s.wait_event(self.ev_fields)                  # this tick's fields (built during the last one)
            if self._comm_pending:
                s.wait_event(self.ev_comm)
            self.ctx.agent_step_dev(self.world_s, self.out_s, stream=s.cuda_stream)
            self._stepped = True
            marks.append(self._mark("gather_agents"))
            if self.pipelined:
                self.ev_step.record(s)
        # the fields of the NEXT tick: enqueued behind the step (whose own wait for the cohesion term is the launch that
        # says "the neighbour walk is done"), started by the device as soon as that is so
        timed = self.record and self.tick_no % self.mark_every == 0
        with tcuda.stream(f):
            if stage == "neighbours":
                self.ctx.stream_wait_stage(f.cuda_stream, navhip.STAGE_NEIGHBOURS)
            elif not self.pipelined:
                # (the start of the prefetch just enqueued: the end of the previous tick, without
                # another event on the agent stream)
                self.ctx.stream_wait_stage(f.cuda_stream, navhip.STAGE_START)
            if timed:
                e0 = tcuda.Event(enable_timing=True)
                e0.record(f)
            self._build_fields(self.pool_next, f)
            if timed:
                e1 = tcuda.Event(enable_timing=True)
                e1.record(f)
            self._exchange_tiles(self.pool_next)
            if timed:
                e2 = tcuda.Event(enable_timing=True)
                e2.record(f)
                self.fev.append((e0, e1, e2))
            self.ev_fields_next.record(f)

    def _comm_behind_step(self):
        # the exchange stream behind the step's outputs: the word the step stored in device memory when it ended (2-3 us),
        # or -- a step that ran on one stream has none -- the event recorded behind it (12 us between two queues)
        if not self.ctx.stream_wait_stage(self.comm.cuda_stream, navhip.STAGE_END, check=False):
            self.comm.wait_event(self.ev_step)

    def exchange(self):
        """The slab results (new position + velocity) of every rank -> every rank."""
        if not self.pipelined:
            return
        if self.exchange_mode == "navhip":
            self._comm_behind_step()
            self.ctx.comm_allgather_step_dev(self.new_pos, self.new_vel, self._bounds, stream=self.comm.cuda_stream)
            self.ev_comm.record(self.comm)
            self._comm_pending = True
            return
        with tcuda.stream(self.comm):
            self._comm_behind_step()
            # ONE collective per tick: this rank's rows of [new position | new velocity] (16 B per
            # agent) packed into one buffer, all-gathered, unpacked
            b, e = self.agent_bounds[self.rank]
            self.res4[b:e, 0:2] = self.new_pos[b:e]
            self.res4[b:e, 2:4] = self.new_vel[b:e]
            pdist.exchange_rows(self.res4, self.agent_bounds, self.rank, self.world)
            self.new_pos.copy_(self.res4[:, 0:2])
            self.new_vel.copy_(self.res4[:, 2:4])
            self.ev_comm.record(self.comm)
        self._comm_pending = True

    def advance(self):
        """Advance the snapshot: ping-pong the position / velocity buffers."""
        with tcuda.stream(self.stream):
            self._marks.append(self._mark("end"))
            self._swap_buffers(self.pipeline_fields)
            if self.pipeline_fields:
                self.ev_fields, self.ev_fields_next = self.ev_fields_next, self.ev_fields
            self._make_structs()
        if self.record and self._marks and self._marks[0] is not None:
            self.ev.append(self._marks)
        self.tick_no += 1

    def phase_ms(self):
        """Average HIP-event duration of every phase over the recorded steps."""
        out = {}
        for marks in self.ev:
            for (n0, e0), (n1, e1) in zip(marks[:-1], marks[1:]):
                out.setdefault(n0, []).append(e0.elapsed_time(e1))
        for e0, e1, e2 in getattr(self, "fev", []):
            out.setdefault("fields", []).append(e0.elapsed_time(e1))
            out.setdefault("gather_tiles", []).append(e1.elapsed_time(e2))
        return {k: float(np.mean(v)) for k, v in out.items()}

    def tick_ms(self):
        """GPU-timeline milliseconds per tick, one value per window of tick_every recorded ticks (start
        event to start event)."""
        return [a.elapsed_time(b) / self.tick_every for a, b in zip(self.tick_ev[:-1], self.tick_ev[1:])]

    def sync(self):
        if self._ctick is not None:
            self._ctick.sync()
        if self.comm is not None:
            self.comm.synchronize()
        if self.pipeline_fields:
            self.fstream.synchronize()
        self.stream.synchronize()
        tcuda.synchronize(self.dev)

    def close(self):
        self.sync()
        if self._ctick is not None:
            self.c_tick_info = self._ctick.info()
            self._ctick.close()
            self._ctick = None
        if self.los_chain is not None:
            self.los_chain.close()
            self.los_chain = None
        self.ctx.close()
