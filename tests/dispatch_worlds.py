"""Worlds for the ClearPath work-list dispatch (csrc/agent_kernels.hip: k_agent_mid's eight work lists and the kernels
that draw their units from them), built so that every agent's ClearPath neighbour count is known beforehand.  Pure numpy;
the shared source of tests/test_dispatch_worlds_cpu.py (which recomputes the counts from the positions) and
tests/test_dispatch_gpu.py.  Test infrastructure only.

The building block is a CLUSTER: members inside a disc of diameter below 10 wu, the clusters on a lattice of 70 wu, so
that neither the r = 10 query (find_neighbours, movement.c:2768) nor the r = 30 query (separation_force, :1690) of one
cluster sees another.  Inside a cluster everybody is everybody's neighbour:

    fast     state MOVING, |vel| >= 0.4          a work item; a DYNAMIC neighbour of the others
    slow     state MOVING, |vel| <= 0.2          a work item; a STATIC neighbour (CLEARPATH_STILL_SPEED = 0.3)
    arrived  state ARRIVED, vel = 0              no ClearPath search (velocity 0); a STATIC neighbour
    held     state MOVING, |vel| >= 0.4, ENTITY_FLAG_COMBAT_HELD: velocity 0 without a search (movement.c:3404); a DYNAMIC
             neighbour -- what gives ONE agent dynamic neighbours that do not search themselves
    garrisoned (flag, on a fast or an arrived member): nobody's neighbour (filter_garrisoned, position.c:100); the device
             steps every searching agent that has one within r = 30 -- itself included -- on the irregular list

A searching member therefore has min(32, fast + held others) dynamic and min(32, slow + arrived others) static neighbours
(MAX_NEIGHBOURS = 32 each), garrisoned others not counted.  The uids are a fixed permutation of the build order: the members
of a cluster lie in many waves of k_agent_mid and so in many sub-lists.  Maps are all passable (cost 1) and hold no
blockers; every agent keeps 12 wu and more off the map edge (see cases.make_agents)."""
import numpy as np

f32 = np.float32
SPACING = 70.0              # wu between cluster centres
EDGE = 17.0                 # centre to map edge: 12 wu for the tile probes + the cluster's radius
MAX_NEIGHBOURS = 32
STATE_MOVING, STATE_ARRIVED = 0, 2
FLAG_MOVABLE, FLAG_GARRISONED, FLAG_COMBAT_HELD = 1 << 3, 1 << 18, 1 << 21
FAST, SLOW, ARRIVED, HELD = 0, 1, 2, 3
# neighbour count -> slot of navhip_last_step_lists: rows of 1-2, 3-4, 5-8, 9-16, then 17-64; [5] is the irregular list
LIST_EDGES = (2, 4, 8, 16, 64)
LIST_IRREGULAR = 5


class DispatchWorld:
    """world: a cases.make_agents-style dict (cases.step_arrays(world, vdes) takes it); w, h: the map in chunks; n_dyn,
    n_stat: the ClearPath neighbour counts the builder intends for every agent (after the caps); searching: the agent
    runs move_velocity_work's ClearPath call (it is neither still nor held); irregular: a garrisoned entity within r = 30."""

    def __init__(self, name, w, h, world, vdes, n_dyn, n_stat, searching, irregular, cluster):
        self.name, self.w, self.h, self.world, self.vdes = name, w, h, world, vdes
        self.n_dyn, self.n_stat, self.searching, self.irregular, self.cluster = n_dyn, n_stat, searching, irregular, cluster

    @property
    def n(self):
        return len(self.n_dyn)

    @property
    def count(self):
        return self.n_dyn + self.n_stat

    def cost(self):
        """The cost plane [h][w][64][64]: every tile passable."""
        return np.ones((self.h, self.w, 64, 64), np.uint8)

    def lists(self, work=None):
        """What navhip_last_step_lists has to report after a step of `work` = (begin, end) (None: everybody)."""
        return list_histogram(self.count, self.searching, self.irregular, work)


def list_histogram(count, searching, irregular, work=None):
    """Agents per reported work list: searching agents with 1-2, 3-4, 5-8, 9-16 and 17-64 neighbours, the irregular ones
    (whatever their count; an agent without neighbours is on no list unless it is irregular)."""
    sel = np.asarray(searching).copy()
    if work is not None:
        sel[:work[0]] = False
        sel[work[1]:] = False
    out = [0] * 6
    out[LIST_IRREGULAR] = int((sel & irregular).sum())
    c = np.asarray(count)[sel & ~irregular]
    lo = 0
    for k, hi in enumerate(LIST_EDGES):
        out[k] = int(((c > lo) & (c <= hi)).sum())
        lo = hi
    return out


def map_for(n_clusters):
    """(chunks per side, lattice points per side) of the smallest square map that holds n_clusters at 70 wu spacing."""
    per = int(np.ceil(np.sqrt(n_clusters)))
    side = (per - 1) * SPACING + 2 * EDGE
    return max(1, int(np.ceil(side / 256.0))), per


def lattice(w, per, n_clusters):
    """Centres of the first n_clusters lattice points, row by row, the lattice centred on a w x w-chunk map."""
    assert (per - 1) * SPACING + 2 * EDGE <= 256.0 * w and per * per >= n_clusters
    k = np.arange(n_clusters)
    c = np.stack([k % per, k // per], 1) * SPACING - (per - 1) * SPACING / 2.0
    return c + 0.25                                # (off the tile corners and the 16-wu cell boundaries)


def disc_offsets(m, radius, phase):
    """m distinct points inside a disc of `radius` (a sunflower spiral turned by `phase`)."""
    k = np.arange(m)
    r = radius * np.sqrt((k + 0.5) / m)
    a = k * 2.399963229728653 + phase
    return np.stack([r * np.cos(a), r * np.sin(a)], 1)


def _radius_of(m):
    return min(4.6, 1.6 * np.sqrt(m))


def build(name, w, specs, seed, per=None, spread=None, agents_per_flock=192, garrison=None, ring=None):
    """specs: one (fast, slow, arrived[, held]) per cluster, in lattice order.  spread(m): the disc radius of a cluster of m
    members.  garrison: {cluster index: member indices} to flag (members are ordered fast, slow, arrived, held)."""
    rng = np.random.RandomState(seed)
    ncl = len(specs)
    if per is None:
        per = int(np.ceil(np.sqrt(ncl)))
    centres = lattice(w, per, ncl)
    spread = spread or _radius_of
    garrison = garrison or {}
    pos, kind, cl, garr, offs = [], [], [], [], []
    for c, spec in enumerate(specs):
        nf, nsl, na, nh = tuple(spec) + (0,) * (4 - len(spec))
        m = nf + nsl + na + nh
        if ring is None:
            off = disc_offsets(m, spread(m), rng.uniform(0, 2 * np.pi))
            off = off[rng.permutation(m)]          # (which member is fast / slow / arrived does not follow the spiral)
        else:
            # the first member in the middle, the others around it at `ring` wu, evenly but for a jitter
            a = rng.uniform(0, 2 * np.pi) + np.arange(m - 1) * 2 * np.pi / (m - 1) + rng.uniform(-0.15, 0.15, m - 1)
            off = np.stack([np.cos(a), np.sin(a)], 1) * (ring * rng.uniform(0.85, 1.15, (m - 1, 1)))
            off = np.concatenate([rng.uniform(-0.02, 0.02, (1, 2)), off])
        pos.append(centres[c] + off)
        offs.append(off)
        kind.append(np.repeat([FAST, SLOW, ARRIVED, HELD], [nf, nsl, na, nh]))
        cl.append(np.full(m, c))
        g = np.zeros(m, bool)
        g[list(garrison.get(c, ()))] = True
        garr.append(g)
    pos, kind, cl, garr = np.concatenate(pos), np.concatenate(kind), np.concatenate(cl), np.concatenate(garr)
    n = len(pos)
    # velocities: a direction at random, |v| in [0.4, 0.9] (fast) or [0.05, 0.2] (slow): either side of 0.3, not near it
    ang = rng.uniform(0, 2 * np.pi, n)
    if ring is not None:                           # ... or, the members of a ring, towards its middle
        offs = np.concatenate(offs)
        ang = np.where(np.linalg.norm(offs, axis=1) > 0.1, np.arctan2(-offs[:, 1], -offs[:, 0]) + rng.uniform(-0.3, 0.3, n), ang)
    moves = (kind == FAST) | (kind == HELD)
    mag = np.where(moves, rng.uniform(0.4, 0.9, n), np.where(kind == SLOW, rng.uniform(0.05, 0.2, n), 0.0))
    vel = np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    # intended counts, from the composition of the cluster alone
    free = ~garr
    fast_in = np.bincount(cl, moves & free, ncl).astype(int)
    still_in = np.bincount(cl, ~moves & free, ncl).astype(int)
    n_dyn = np.minimum(MAX_NEIGHBOURS, fast_in[cl] - (moves & free))
    n_stat = np.minimum(MAX_NEIGHBOURS, still_in[cl] - (~moves & free))
    searching = (kind == FAST) | (kind == SLOW)
    irregular = np.bincount(cl, garr, ncl)[cl] > 0
    flock = cl // max(1, int(round(agents_per_flock * ncl / max(n, 1))))
    k = int(flock.max()) + 1
    # flock targets: somewhere on the map, away from the members (the arrive force points to them)
    half = 128.0 * w - EDGE
    targets = rng.uniform(-half, half, (k, 2))
    vdes = rng.normal(0, 1, (n, 2))
    vdes /= np.linalg.norm(vdes, axis=1, keepdims=True)
    # uids: a fixed permutation of the build order
    p = rng.permutation(n)
    flags = (FLAG_MOVABLE | np.where(garr, FLAG_GARRISONED, 0) | np.where(kind == HELD, FLAG_COMBAT_HELD, 0)).astype(np.uint32)
    world = {
        "pos_xz": pos[p].astype(f32), "vel_xz": vel[p].astype(f32),
        "radius": np.ones(n, f32), "max_speed": rng.choice([20.0, 15.0, 25.0], n).astype(f32)[p],
        "speed": np.full(n, 20.0, f32), "flags": flags[p],
        "state": np.where(kind == ARRIVED, STATE_ARRIVED, STATE_MOVING).astype(np.uint8)[p],
        "has_dest_los": (rng.rand(n) < 0.3).astype(np.uint8)[p],
        "flock": flock[p].astype(np.int32), "flock_target_xz": targets.astype(f32),
    }
    return DispatchWorld(name, w, w, world, vdes[p].astype(f32), n_dyn[p].astype(np.int32), n_stat[p].astype(np.int32),
                         searching[p], irregular[p], cl[p])


# ---------------------------------------------------------------------------------------------
# the worlds
# ---------------------------------------------------------------------------------------------
# ladder: (fast, slow, arrived) and how many clusters of it; a fast member of it has (fast - 1) + slow + arrived
# neighbours before the caps.  Counts 33-64 need both kinds (32 + 32).
LADDER = (
    ((1, 0, 0), 12),        # 0 neighbours: on no list
    ((2, 0, 0), 6),         # 1                      ROW0
    ((3, 0, 0), 4),         # 2                      ROW0 | ROW1
    ((4, 0, 0), 3),         # 3
    ((5, 0, 0), 3),         # 4                      ROW1 | ROW2
    ((6, 0, 0), 2),         # 5
    ((9, 0, 0), 2),         # 8                      ROW2 | ROW3
    ((10, 0, 0), 2),        # 9
    ((17, 0, 0), 1),        # 16                     ROW3 | WAVE (a workgroup)
    ((18, 0, 0), 1),        # 17
    ((33, 0, 0), 1),        # 32 dynamic             WAVE | HEAVY
    ((33, 0, 1), 1),        # 32 dynamic + 1 static = 33
    ((32, 0, 32), 1),       # 31 + 32 = 63
    ((33, 0, 32), 1),       # 32 + 32 = 64: both lists full
    ((65, 0, 10), 1),       # 64 dynamic (cap: 32) + 10 static = 42
    ((41, 0, 40), 1),       # 40 + 40 (both caps): 64
    # the same edges with static neighbours, and slow members (searching AND static)
    ((1, 0, 1), 2), ((1, 0, 2), 2), ((2, 2, 0), 2), ((1, 1, 3), 2), ((1, 0, 16), 1), ((1, 0, 17), 1), ((2, 3, 4), 1), ((5, 12, 0), 1),
)
LADDER_COUNTS = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)
# clusters of the variant that carry garrisoned members: index into the list of clusters below -> member indices
LADDER_EXTRA = ((3, 0, 0), (6, 0, 0), (10, 0, 2), (18, 0, 0), (33, 0, 20), (4, 1, 1), (2, 0, 0), (1, 0, 0))
LADDER_GARRISONED = ((0,), (1, 4), (0, 11), (2, 3), (0, 40, 52), (5,), (1,), (0,))


def ladder(garrisoned=False, w=4):
    """Every edge of DISP_ROW0 .. DISP_HEAVY (mid_thread_b) and of the 32 / 32 caps on a 4 x 4-chunk map (w: the same
    clusters in the middle of a larger one); garrisoned: ~2 %
    of the agents garrisoned (fast and arrived ones), inside eight clusters of their own -- those clusters' searching
    members are on the irregular list, everybody else is where the plain ladder has it."""
    specs = [s for s, k in LADDER for _ in range(k)] + list(LADDER_EXTRA)
    base = len(specs) - len(LADDER_EXTRA)
    g = {base + i: m for i, m in enumerate(LADDER_GARRISONED)} if garrisoned else None
    return build(("ladder_garrisoned" if garrisoned else "ladder") + ("" if w == 4 else "_wide"), w, specs, seed=101, agents_per_flock=64, garrison=g)


def no_neighbours():
    """40 agents, nobody with a neighbour: every list empty, yet a step that launches."""
    return build("no_neighbours", 2, [(1, 0, 0)] * 40, seed=102)


SPARSE = ("one_on_row2", "four_on_row0", "five_on_row1", "one_wave_no_heavy", "one_heavy_no_wave")


def sparse_lists():
    """Five small worlds on 2 x 2-chunk maps, each with a handful of agents on ONE list.  The neighbours are arrived or
    held members (no search of their own), the singletons around them have no neighbour at all."""
    lone = [(1, 0, 0)] * 9
    return [
        build(SPARSE[0], 2, lone + [(1, 0, 6)] + lone, seed=111),                    # one agent, 6 neighbours: ROW2
        build(SPARSE[1], 2, lone + [(2, 0, 0), (1, 0, 2), (1, 0, 1)], seed=112),     # 1, 1, 2, 1 neighbours: ROW0
        build(SPARSE[2], 2, [(4, 0, 0), (1, 0, 4)] + lone, seed=113),                # 3, 3, 3, 3, 4 neighbours: ROW1
        build(SPARSE[3], 2, lone + [(1, 0, 17)], seed=114),                          # 17 static: WAVE; HEAVY empty
        build(SPARSE[4], 2, [(1, 0, 32, 2)] + lone, seed=115),                       # 2 dynamic + 32 static: HEAVY; WAVE empty
    ]


def one_list_full():
    """36 864 agents in clusters of six: 5 neighbours each, 9 216 units of four on ROW2 alone -- more than twice the
    4 096 waves of the main k_cp_rows launch, so its first round of units is dealt out statically (next_unit) and the rest
    by ticket.  6 144 clusters at 70 wu: a 22 x 22-chunk map."""
    ncl = 36864 // 6
    w, per = map_for(ncl)
    return build("one_list_full", w, [(6, 0, 0)] * ncl, seed=121, per=per)


SOLO_CLUSTERS = 456


def solo_heavy():
    """8 208 agents in clusters of 18: 17 neighbours each, all on the WAVE list and nothing on HEAVY -- from CP_SOLO_MIN =
    8 192 problems on k_cp_heavy gives every wave a problem of its own, here out of the SECOND half of its table, the
    first nblk * 4 by wave number and the rest by ticket."""
    w, per = map_for(SOLO_CLUSTERS)
    return build("solo_heavy", w, [(18, 0, 0)] * SOLO_CLUSTERS, seed=131, per=per)


RETRY_RING = 0.5
# agents of retry_flood whose first attempt fails: what tests/test_dispatch_worlds_cpu.py establishes with the model of
# one attempt (tests/tools/cp_model.py), and the least the device has to report as retried
RETRY_ESTABLISHED = 2048


def retry_flood():
    """8 192 searching agents (nwork a multiple of 4 096: the smallest margin of nh_worklist_cap) in 2 048 quads: one agent
    in the middle of three that stand RETRY_RING = 0.5 wu from it (radius 1: deep inside each other) and move towards it.
    3 neighbours each, all on ROW1.  The three velocity obstacles of the agent in the middle cover every candidate of
    its single attempt (clearpath_small_row): it goes onto the retry list -- 2 048 of them, a quarter of the world; the
    agents of the ring see all their neighbours on one side and find a candidate (all but one of them, with this seed).
    A quarter is some 32 entries per sub-list of the retry list: far from its capacity (nh_worklist_cap), which no test
    comes near.  (Triads and quads at 1.5-2.2 wu, and
    denser ones laid out at random, do not fail: see test_retry_flood_fails_its_first_attempt.)  All four are fast: with
    neighbours of one kind only, a failed attempt ends the reference's retry loop (clearpath.c:704-713) -- velocity 0.
    (With a slow, that is static, agent in the ring some 4 % of the middle agents find a candidate: fewer than 2 048.)"""
    specs = [(4, 0, 0)] * 2048
    w, per = map_for(len(specs))
    return build("retry_flood", w, specs, seed=141, per=per, ring=RETRY_RING)


_WORLDS = {}


def get(name):
    """The world `name`, built once: ladder, ladder_garrisoned, ladder_wide (the ladder on solo_heavy's map), no_neighbours,
    the five of SPARSE, one_list_full, solo_heavy, retry_flood."""
    assert name in NAMES, name
    if name not in _WORLDS:
        if name in SPARSE:
            for W in sparse_lists():
                _WORLDS[W.name] = W
        else:
            make = {"ladder": ladder, "ladder_garrisoned": lambda: ladder(True), "ladder_wide": lambda: ladder(w=map_for(SOLO_CLUSTERS)[0]),
                    "no_neighbours": no_neighbours, "one_list_full": one_list_full, "solo_heavy": solo_heavy,
                    "retry_flood": retry_flood}[name]
            _WORLDS[name] = make()
            assert _WORLDS[name].name == name
    return _WORLDS[name]


NAMES = ("ladder", "ladder_garrisoned", "ladder_wide", "no_neighbours") + SPARSE + ("one_list_full", "solo_heavy", "retry_flood")
