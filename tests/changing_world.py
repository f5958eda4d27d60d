"""A deterministic script of worlds that change from tick to tick, for multi-tick tests of the agent step.

The engine's snapshot is rebuilt every tick (bindings/permafrost/move_hip.c): move orders create flocks, arrivals
dissolve them, units spawn and die, states and flags change.  The script applies one or two such changes per
tick to everything but positions and velocities, which the caller carries from the step's own outputs of the
tick before (rows [0, n_carry); the tail of a tick that spawned comes from the script).

Everything the script decides is known before the first tick -- a caller that does not synchronise with the
device can upload every tick's tables up front.  Deaths drop the highest uids (the survivors keep their uids,
so the carried rows need no gather on the device); every entity is a member of exactly one flock.  Test
infrastructure only."""
import numpy as np

from permafrost_engine_amd import synth
from tests import cases

W = 4                                       # 4 x 4 chunks
N0, K0 = 3000, 6
TICKS = 16
ARRIVED, MOVING_IN_FORMATION, ARRIVING_TO_CELL = 2, 1, 8
FLAG_GARRISONED, FLAG_COMBAT_HELD = 1 << 18, 1 << 21
ENTITY_ARRAYS = ("radius", "max_speed", "speed", "flags", "state", "has_dest_los", "vdes_xz")
FORM_ARRAYS = ("form_ready", "cell_pos_xz", "form_cohesion_xz", "form_align_xz", "form_drag_xz")

# what changes on the way INTO tick t (tick 0 is the start): one or two changes per tick
EVENTS = {
    1: ("split",),
    2: ("merge",),
    3: ("swap", "los"),
    4: ("resize",),
    5: ("empty", "hz10"),
    6: ("split_past_64", "arrive"),
    7: ("resize", "hold_garrison", "hz20"),
    8: ("spawn",),
    9: ("los", "formation_on"),
    10: ("merge_below_64",),
    11: ("resize", "come_back"),
    12: ("die", "formation_off"),
    13: ("swap", "split", "hold_garrison"),
    14: ("resize", "hz10"),
    15: ("refill", "hz20"),
}


def grid():
    return synth.cost_grid(W, W, seed=21, frac_impassable=0.20)


class Tick:
    """One tick of the script: the snapshot minus positions and velocities."""

    def __init__(self, t, n, n_carry, spawn_pos, spawn_vel, ent, flocks, targets, hz, form, events):
        self.t, self.n, self.n_carry, self.hz, self.events = t, n, n_carry, hz, events
        self.spawn_pos, self.spawn_vel = spawn_pos, spawn_vel           # rows [n_carry, n)
        self.ent = ent                                                  # ENTITY_ARRAYS, [n] each
        self.flock_lists = flocks                                       # per flock: uid array (CSR order)
        self.flock_target_xz = np.asarray(targets, np.float32).reshape(-1, 2)
        self.form = form                                                # FORM_ARRAYS or None
        self.n_flocks = len(flocks)
        self.flock = np.full(n, -1, np.int32)
        for f, l in enumerate(flocks):
            self.flock[l] = f
        self.flock_offsets, self.flock_members = _csr(flocks)

    def arrays(self, pos_xz, vel_xz):
        """navhip_world member arrays (host) of this tick for the given positions and velocities."""
        a = {k: self.ent[k] for k in ENTITY_ARRAYS}
        a.update(pos_xz=np.ascontiguousarray(pos_xz, np.float32), vel_xz=np.ascontiguousarray(vel_xz, np.float32),
                 flock=self.flock, flock_target_xz=self.flock_target_xz, flock_offsets=self.flock_offsets,
                 flock_members=self.flock_members)
        if self.form is not None:
            a.update(self.form)
        return a

    def start_rows(self, prev_pos, prev_vel):
        """Positions and velocities of this tick: the previous tick's outputs for the carried rows, the script's
        spawns after them."""
        pos = np.concatenate([prev_pos[:self.n_carry], self.spawn_pos]).astype(np.float32)
        vel = np.concatenate([prev_vel[:self.n_carry], self.spawn_vel]).astype(np.float32)
        return pos, vel

    def tables_key(self):
        return (self.flock_offsets.tobytes(), self.flock_members.tobytes())


def _csr(lists):
    offs = np.zeros(len(lists) + 1, np.int32)
    offs[1:] = np.cumsum([len(l) for l in lists])
    members = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return offs, members


def _new_entities(g, n, k, seed):
    w = cases.make_agents(g, n, k, seed=seed, clustered=True, sigma=60.0)
    rng = np.random.RandomState(seed + 7)
    vdes = rng.normal(0, 1, (n, 2))
    vdes /= np.maximum(np.linalg.norm(vdes, axis=1, keepdims=True), 1e-6)
    vdes[rng.rand(n) < 0.05] = 0
    w["vdes_xz"] = vdes.astype(np.float32)
    return w


def script(seed=11, ticks=TICKS):
    """The list of Tick objects of the script."""
    g = grid()
    rng = np.random.RandomState(seed)
    w0 = _new_entities(g, N0, K0, seed=seed + 30)
    ent = {k: w0[k].copy() for k in ENTITY_ARRAYS}
    flocks = [np.flatnonzero(w0["flock"] == f).astype(np.int32) for f in range(K0)]
    targets = [t for t in w0["flock_target_xz"]]
    passable = synth.passable_cells(g)
    hz, n = 20, N0
    form_flocks = set()
    out = []

    def new_target():
        c = passable[rng.randint(len(passable))]
        return synth.cell_centre(W, W, c[0], c[1]).astype(np.float32)

    def split(f):
        l = flocks[f]
        cut = max(len(l) // 2, 1)
        flocks[f] = l[:cut]
        flocks.append(l[cut:])
        targets.append(new_target())

    def merge(a, b):                                  # b into a; b leaves the table
        flocks[a] = np.sort(np.concatenate([flocks[a], flocks[b]])).astype(np.int32)
        del flocks[b], targets[b]

    def biggest():
        return int(np.argmax([len(l) for l in flocks]))

    for t in range(ticks):
        ev = EVENTS.get(t, ()) if t else ()
        n_carry, spawn_pos, spawn_vel = n, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
        if t == 0:
            n_carry, spawn_pos, spawn_vel = 0, w0["pos_xz"], w0["vel_xz"]
        for e in ev:
            if e == "split":
                split(biggest())
            elif e == "merge":
                merge(0, len(flocks) - 1)
            elif e == "swap":                         # equal offsets: two units trade flocks
                a, b = 0, 1
                i, j = rng.randint(len(flocks[a])), rng.randint(len(flocks[b]))
                flocks[a], flocks[b] = flocks[a].copy(), flocks[b].copy()
                flocks[a][i], flocks[b][j] = flocks[b][j], flocks[a][i]
            elif e == "resize":                       # other flock sizes at equal n_flocks and n_ents
                a, b = biggest(), (biggest() + 1) % len(flocks)
                m = max(len(flocks[a]) // 5, 1)
                flocks[b] = np.sort(np.concatenate([flocks[b], flocks[a][:m]])).astype(np.int32)
                flocks[a] = flocks[a][m:]
            elif e == "empty":                        # a flock with a CSR run of length zero
                flocks[4] = np.sort(np.concatenate([flocks[4], flocks[3]])).astype(np.int32)
                flocks[3] = np.zeros(0, np.int32)
            elif e == "refill":
                f = next(i for i, l in enumerate(flocks) if len(l) == 0)
                b = biggest()
                m = len(flocks[b]) // 3
                flocks[f], flocks[b] = flocks[b][:m], flocks[b][m:]
            elif e == "split_past_64":
                while len(flocks) < 70:
                    split(biggest())
            elif e == "merge_below_64":
                while len(flocks) > 40:
                    merge(len(flocks) - 2, len(flocks) - 1)
            elif e == "spawn":                        # n_ents x 2.3: every scratch buffer of the step grows
                n_new = int(n * 1.3)
                nw = _new_entities(g, n_new, 2, seed=seed + 60)
                uids = np.arange(n, n + n_new, dtype=np.int32)
                spawn_pos, spawn_vel = nw["pos_xz"], nw["vel_xz"]
                for k in ENTITY_ARRAYS:
                    ent[k] = np.concatenate([ent[k], nw[k]])
                home = rng.randint(0, len(flocks) + 2, n_new)  # two new flocks and the old ones (an empty one stays so)
                k_old = len(flocks)
                for f in range(k_old):
                    if len(flocks[f]) == 0:
                        home[home == f] = k_old
                for f in range(k_old):
                    flocks[f] = np.concatenate([flocks[f], uids[home == f]]).astype(np.int32)
                for f in range(2):
                    flocks.append(uids[home == k_old + f])
                    targets.append(new_target())
                n += n_new
            elif e == "die":                          # the highest uids die: buffers are larger than needed
                n = int(n * 0.74)
                n_carry = n
                for k in ENTITY_ARRAYS:
                    ent[k] = ent[k][:n]
                flocks = [l[l < n] for l in flocks]
            elif e == "arrive":                       # a share of the units stop, ...
                ent["state"] = ent["state"].copy()
                ent["state"][(rng.rand(n) < 0.15) & (ent["state"] == 0)] = ARRIVED
            elif e == "come_back":                    # ... and most of them move again
                ent["state"] = ent["state"].copy()
                ent["state"][(ent["state"] == ARRIVED) & (rng.rand(n) < 0.7)] = 0
            elif e == "hold_garrison":
                ent["flags"] = ent["flags"].copy()
                ent["flags"][rng.rand(n) < 0.05] ^= np.uint32(FLAG_COMBAT_HELD)
                ent["flags"][rng.rand(n) < 0.03] ^= np.uint32(FLAG_GARRISONED)
            elif e == "los":
                ent["has_dest_los"] = ent["has_dest_los"].copy()
                ent["has_dest_los"][rng.rand(n) < 0.4] ^= 1
            elif e in ("hz10", "hz20"):
                hz = int(e[2:])
            elif e == "formation_on":                 # the formation arm for three flocks
                form_flocks = {0, 2, len(flocks) - 1}
                ent["state"] = ent["state"].copy()
                for f in form_flocks:
                    l = flocks[f]
                    moving = l[ent["state"][l] == 0]
                    ent["state"][moving[0::2]] = MOVING_IN_FORMATION
                    ent["state"][moving[1::4]] = ARRIVING_TO_CELL
            elif e == "formation_off":
                form_flocks = set()
                ent["state"] = ent["state"].copy()
                ent["state"][np.isin(ent["state"], (MOVING_IN_FORMATION, ARRIVING_TO_CELL))] = 0
            else:
                raise ValueError(e)
        form = None
        if form_flocks:
            frng = np.random.RandomState(seed + 100 + t)
            anchor = np.asarray(targets, np.float32)[_flock_of(flocks, n)]
            form = {
                "form_ready": (frng.rand(n) < 0.85).astype(np.uint8),
                "cell_pos_xz": (anchor + frng.normal(0, 1, (n, 2)) * frng.choice([3.0, 12.0, 45.0], (n, 1))).astype(np.float32),
                "form_cohesion_xz": frng.normal(0, 0.4, (n, 2)).astype(np.float32),
                "form_align_xz": frng.normal(0, 0.4, (n, 2)).astype(np.float32),
                "form_drag_xz": np.where(frng.rand(n, 1) < 0.5, frng.normal(0, 0.3, (n, 2)), 0.0).astype(np.float32),
            }
        out.append(Tick(t, n, n_carry, np.asarray(spawn_pos, np.float32), np.asarray(spawn_vel, np.float32),
                        {k: v.copy() for k, v in ent.items()}, [l.copy() for l in flocks], list(targets), hz, form, ev))
    return out


def _flock_of(flocks, n):
    f = np.zeros(n, np.int64)
    for i, l in enumerate(flocks):
        f[l] = i
    return f


def slab_cut(tick):
    """The uid slab boundary of `tick` for a job split between two ranks: it moves from tick to tick."""
    return int(tick.n * (0.5, 0.3, 0.7, 0.45)[tick.t % 4])
