"""Worlds, a model and wrong models for the cohesion term (csrc/cohesion_kernels.hip: k_cohesion, k_coh_plan and the lane
regrouping).  Pure numpy; the shared source of tests/test_cohesion_cpu.py and tests/test_cohesion_gpu.py.  Test
infrastructure only.

The cohesion force is vtrunc(com - me, smf), com = sum_j pos_j * exp(-6 t_j) / (F - 1) in member order, smf = 0.75 at 20 Hz
and 15 at 1 Hz.  It enters vpref as 0.15 * cohesion beside the arrive and the separation force, and the total is dropped
when it is no longer than 0.01 * smf.  A PROBE is a member for which the restatement reports an arrive and a separation
force of exactly 0 and a final clamp that does not bind (zero velocity, vdes = 0 without line of sight, no movable entity
the r = 30 query returns, speed 100): its vpref is fl(0.15f * cohesion).  A probe IN THE WINDOW has smf / 15 < |com - me| <
smf: neither clamp hides the sum.  Two constructions:
    origin   the probe within smf of the world origin, its mates where their weight is small (150-300 wu away) or -- the
             arith world -- on a line through the origin, with tuner mates placed by a 1-D root find so that com lands
             beside the probe.  Probes next to the origin are within 30 wu of each other: they carry ENTITY_FLAG_GARRISONED,
             which removes them from every neighbour query (filter_garrisoned, position.c:100) and from nothing else.
    tuned    the probe anywhere (340-650 wu from the origin), its mates in pairs mirrored at the ray through the probe, one
             tuner mate on the ray placed by a 1-D root find on the model.
Every non-probe member of those flocks is immovable and ARRIVED (no separation partner, no ClearPath neighbour)."""
import numpy as np

f32, f64 = np.float32, np.float64
STATE_MOVING, STATE_ARRIVED = 0, 2
FLAG_MOVABLE, FLAG_GARRISONED, FLAG_COMBAT_HELD = 1 << 3, 1 << 18, 1 << 21
COH_FAR = f32(906.0)
APW, TILE, BATCH = 16, 256, 16            # members per wave, staged members per tile, queue entries per batch
SURVIVOR_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33)
PLAN_SHAPES = (1, 63, 64, 65, 256, 257, 513)
WINDOW_SIZES = (2, 3, 17, 33, 257)
WRONG_MODELS = ("reverse", "pairwise", "self", "div_f", "t_f32", "sqrt_low", "tail_twice", "drop_200", "box_all", "box_first")


def smf(hz):
    """scaled_max_force as the kernel and the restatement compute it: (float)((double)(0.75f / (float)hz) * 20.0)."""
    return f32(f64(f32(0.75) / f32(hz)) * 20.0)


def active_mask(arrays, work=None):
    """Members that take a cohesion force: point seeking (MOVING here), not combat-held, inside the work range."""
    act = (arrays["state"] == STATE_MOVING) & ((arrays["flags"] & FLAG_COMBAT_HELD) == 0)
    if work is not None:
        act = act.copy()
        act[:work[0]] = False
        act[work[1]:] = False
    return act


# ---------------------------------------------------------------------------------------------
# the kernel's tile walk under the identity grouping (tick 0): a wave is 16 consecutive CSR entries
# ---------------------------------------------------------------------------------------------
def grouping(arrays, w, h, binned_pos=None):
    """A model of the lane grouping k_coh_bin .. k_coh_scatter leave for the next tick: per flock the CSR positions of its
    members, the active ones by the Morton number of their 256-wu block (16 x 16 blocks from the map's corner), the
    others last.  Inside a bin the device's order is whatever its atomics give; here it is the CSR order.  binned_pos:
    the positions the grouping was built from (the tick before), arrays["pos_xz"] when None."""
    offs, mem = arrays["flock_offsets"], arrays["flock_members"]
    pos = arrays["pos_xz"] if binned_pos is None else binned_pos
    act_all = active_mask(arrays)
    out = []
    for f in range(len(offs) - 1):
        m = mem[offs[f]:offs[f + 1]]
        bx = np.floor((pos[m, 0] - f32(-128.0 * w)) * f32(1.0 / 256.0)).astype(int) & 15
        bz = np.floor((pos[m, 1] - f32(-128.0 * h)) * f32(1.0 / 256.0)).astype(int) & 15
        mo = np.zeros(len(m), int)
        for k in range(4):
            mo |= (((bx >> k) & 1) << (2 * k)) | (((bz >> k) & 1) << (2 * k + 1))
        out.append(np.argsort(np.where(act_all[m], mo, 256), kind="stable"))
    return out


def _waves(arrays, box="active", work=None, perm=None):
    """Per wave with an active member: (flock, wave, members, active, keep): members = the flock-local CSR positions of
    the wave's quads, keep[j] = the flock's j-th member passes the kernel's box rule (float32).  box: "active" -- the
    kernel's --, "all" (every quad of the wave), "first" (one quad).  perm: per flock the lane grouping (grouping());
    None: the identity of tick 0."""
    offs, mem, pos = arrays["flock_offsets"], arrays["flock_members"], arrays["pos_xz"]
    act_all = active_mask(arrays, work)
    for f in range(len(offs) - 1):
        m = mem[offs[f]:offs[f + 1]]
        px, pz = pos[m, 0], pos[m, 1]
        act = act_all[m]
        order = np.arange(len(m)) if perm is None else perm[f]
        for wv in range((len(m) + APW - 1) // APW):
            sl = order[wv * APW:wv * APW + APW]
            if not act[sl].any():
                continue
            sel = act[sl] if box == "active" else np.ones(len(sl), bool)
            if box == "first":
                sel = np.zeros(len(sl), bool)
                sel[np.flatnonzero(act[sl])[0]] = True
            bx0, bx1 = px[sl][sel].min(), px[sl][sel].max()
            bz0, bz1 = pz[sl][sel].min(), pz[sl][sel].max()
            dx = np.maximum(np.maximum(bx0 - px, px - bx1), f32(0))
            dz = np.maximum(np.maximum(bz0 - pz, pz - bz1), f32(0))
            keep = ~(dx * dx + dz * dz > COH_FAR * COH_FAR)
            yield f, wv, sl, act, keep


def _queue_walk(keep, n):
    """(survivors per tile, carried[j]: member j waits in a carried tail at least once) for one wave."""
    counts, carry, carried = [], [], np.zeros(n, bool)
    for jb in range(0, n, TILE):
        surv = list(jb + np.flatnonzero(keep[jb:jb + TILE]))
        counts.append(len(surv))
        queue = carry + surv
        whole = len(queue) & ~(BATCH - 1)
        carry = queue[whole:] if jb + TILE < n else []
        carried[carry] = True
    return counts, carried


def tile_survivors(W, box="active", arrays=None, perm=None):
    """{"counts": [(flock, wave, [survivors per 256-member tile])], "zero_between": some wave has a tile without survivors
    between two with some, "self_tail": some active member waits in a carried tail of its own wave, "self_tile": the tile
    numbers in which a wave's own active members lie}."""
    out = {"counts": [], "zero_between": False, "self_tail": False, "self_tile": set()}
    for f, wv, sl, act, keep in _waves(W.arrays if arrays is None else arrays, box, perm=perm):
        counts, carried = _queue_walk(keep, len(keep))
        out["counts"].append((f, wv, counts))
        nz = [k for k, c in enumerate(counts) if c]
        out["zero_between"] |= any(c == 0 for c in counts[nz[0]:nz[-1]])
        own = sl[act[sl]]
        out["self_tail"] |= bool(carried[own].any())
        out["self_tile"] |= set(own // TILE)
    return out


def batch_lanes(W):
    """Per (wave, 16-entry batch) of the flocks that fit one tile and lose nobody to the box rule: the number of lanes --
    (active member, sub-lane); a sub-lane holds the entries k = sub mod 4 -- on the `close` path (a length below 16) and on
    the `odd` path (0 < ss < 2^-90).  Returns two int arrays."""
    a = W.arrays
    close_n, odd_n = [], []
    for f, wv, sl, act, keep in _waves(a):
        n = len(keep)
        if n > TILE or not keep.all():
            continue
        m = a["flock_members"][a["flock_offsets"][f]:a["flock_offsets"][f + 1]]
        px, pz = a["pos_xz"][m, 0], a["pos_xz"][m, 1]
        for i in sl[act[sl]]:
            dx, dz = px - px[i], pz - pz[i]
            ss = dx * dx + dz * dz
            ln = np.sqrt(ss)
            pad = (-n) % BATCH
            c = np.concatenate([ln < 16, np.zeros(pad, bool)]).reshape(-1, 4, 4).any(1)     # [batch][sub]
            o = np.concatenate([(ss != 0) & (ss < f32(2.0 ** -90)), np.zeros(pad, bool)]).reshape(-1, 4, 4).any(1)
            close_n.append(c.sum(1))
            odd_n.append(o.sum(1))
    # (one active member per wave in the arith world: a row is a batch of one wave)
    return np.concatenate(close_n), np.concatenate(odd_n)


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
def _pair_terms(px, pz, variant):
    """ln[i, j], w[i, j] (me = i, mate = j) in the reference's float order: sqrtf(x*x + z*z), t = (float)(((double)len -
    37.5) / 50.0), scale = (float)exp((double)(-6.0f * t))."""
    dx, dz = px[None, :] - px[:, None], pz[None, :] - pz[:, None]
    ss = dx * dx + dz * dz
    ln = np.sqrt(ss)
    if variant == "sqrt_low":
        # (the root one ulp low where it was rounded up: where a native root one ulp short needs the kernel's fix-up)
        up = ln.astype(f64) ** 2 > ss.astype(f64)
        ln = np.where(up, np.nextafter(ln, f32(0)), ln)
    t = ((ln.astype(f64) - 37.5) / 50.0).astype(f32)
    if variant == "t_f32":
        t = np.where(ln < 16, (ln - f32(37.5)) / f32(50.0), t)
    w = np.exp((f32(-6.0) * t).astype(f64)).astype(f32)
    if variant == "drop_200":
        w = np.where(ln > 200, f32(0), w)
    return ln, w


def cohesion_model(arrays, hz, variant=None, work=None):
    """(cohesion[n, 2], com - me [n, 2]) of every flock member, float32, from cohesion_force (movement.c:1653): products and
    running sum in float32 in member order, self skipped, 1.0f / count, vec2_truncate.  variant: one of WRONG_MODELS."""
    offs, mem, pos = arrays["flock_offsets"], arrays["flock_members"], arrays["pos_xz"].astype(f32)
    n = len(pos)
    coh, raw = np.zeros((n, 2), f32), np.zeros((n, 2), f32)
    lim = smf(hz)
    special = {}
    if variant in ("tail_twice", "box_all", "box_first"):
        for f, wv, sl, act, keep in _waves(arrays, {"box_all": "all", "box_first": "first"}.get(variant, "active"), work):
            special.setdefault(f, []).append((sl, keep, _queue_walk(keep, len(keep))[1]))
    for f in range(len(offs) - 1):
        m = mem[offs[f]:offs[f + 1]]
        F = len(m)
        if F < 2:
            continue
        px, pz = pos[m, 0], pos[m, 1]
        ln, w = _pair_terms(px, pz, variant)
        if variant != "self":
            w[m[:, None] == m[None, :]] = 0                    # (curr == uid is skipped: a zero product leaves the sum as it is)
        for sl, keep, carried in special.get(f, ()):
            if variant == "tail_twice":
                w[sl] = np.where(carried[None, :], w[sl] * f32(2), w[sl])
            else:
                w[sl] = np.where(keep[None, :], w[sl], f32(0))
        tx, tz = px[None, :] * w, pz[None, :] * w
        if variant == "pairwise":
            def tree(t):
                while t.shape[1] > 1:
                    if t.shape[1] & 1:
                        t = np.concatenate([t, np.zeros((F, 1), f32)], 1)
                    t = t[:, 0::2] + t[:, 1::2]
                return t[:, 0]
            cx, cz = tree(tx), tree(tz)
        else:
            cx, cz = np.zeros(F, f32), np.zeros(F, f32)
            for j in (range(F - 1, -1, -1) if variant == "reverse" else range(F)):
                cx = cx + tx[:, j]
                cz = cz + tz[:, j]
        inv = f32(1.0) / f32(F if variant == "div_f" else F - 1)
        d = np.stack([cx * inv - px, cz * inv - pz], 1)
        raw[m] = d
        ln_d = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        over = ln_d > lim
        with np.errstate(invalid="ignore", divide="ignore"):
            cl = np.stack([d[:, 0] / ln_d * lim, d[:, 1] / ln_d * lim], 1)
        coh[m] = np.where(over[:, None], cl, d)
    return coh, raw


def vpref_of(coh):
    """What a probe's vpref is: 0 + fl(0.15f * cohesion) (the sum of the three scaled forces starts at +0)."""
    return (coh * f32(0.15) + f32(0)).astype(f32)


def in_window(raw, hz):
    ln = np.sqrt(raw[:, 0].astype(f64) ** 2 + raw[:, 1].astype(f64) ** 2)
    return (ln > f64(smf(hz)) / 15.0 * 1.001) & (ln < f64(smf(hz)) * 0.999)


# ---------------------------------------------------------------------------------------------
# builder
# ---------------------------------------------------------------------------------------------
class CohWorld:
    """arrays: what cases.step_arrays returns (navhip_world members); probes: uids built as probes; tags: label -> uids
    (flock-size classes, arithmetic edges); hz: the tick rates the world is stepped at; slab: (work_begin, work_end,
    static_epoch) of one more call, or None."""

    def __init__(self, name, w, h, arrays, hz, probes=(), tags=None, slab=None):
        self.name, self.w, self.h, self.arrays, self.hz = name, w, h, arrays, tuple(hz)
        self.probes = np.asarray(probes, np.int64)
        self.tags = {k: np.asarray(v, np.int64) for k, v in (tags or {}).items()}
        self.slab = slab

    @property
    def n(self):
        return len(self.arrays["pos_xz"])

    def cost(self):
        return np.ones((self.h, self.w, 64, 64), np.uint8)

    def swapped(self):
        """The same tables with the positions of two clusters swapped member by member: in every flock the two most
        populous 256-wu columns of the map, their members paired in CSR order (the surplus of the larger one stays).  The
        clusters differ in size and extent, so a lane grouping built before the swap puts members of both ends of the map
        into one wave: it is only a hint then."""
        a = dict(self.arrays)
        pos = self.arrays["pos_xz"].copy()
        offs, mem = a["flock_offsets"], a["flock_members"]
        for f in range(len(offs) - 1):
            m = mem[offs[f]:offs[f + 1]]
            col = np.floor((self.arrays["pos_xz"][m, 0] + 128.0 * self.w) / 256.0).astype(int)
            big = np.argsort(-np.bincount(col, minlength=2), kind="stable")[:2]
            one, two = m[col == big[0]], m[col == big[1]]
            k = min(len(one), len(two))
            pos[one[:k]], pos[two[:k]] = self.arrays["pos_xz"][two[:k]], self.arrays["pos_xz"][one[:k]]
        a["pos_xz"] = pos
        return a


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.pos, self.flags, self.state, self.flocks, self.probes, self.tags = [], [], [], [], [], {}

    def add(self, xz, active=True, garrisoned=False, held=False, movable=None):
        movable = active if movable is None else movable
        self.pos.append((float(xz[0]), float(xz[1])))
        self.flags.append((FLAG_MOVABLE if movable else 0) | (FLAG_GARRISONED if garrisoned else 0) | (FLAG_COMBAT_HELD if held else 0))
        self.state.append(STATE_MOVING if active or held else STATE_ARRIVED)
        return len(self.pos) - 1

    def flock(self, members, shuffle=True):
        members = list(members)
        if shuffle:
            members = [members[i] for i in self.rng.permutation(len(members))]
        self.flocks.append(members)

    def probe(self, uid, *tags):
        self.probes.append(uid)
        for t in tags:
            self.tags.setdefault(t, []).append(uid)

    def finish(self, name, w, h, hz, general=False, slab=None):
        """general: random velocities, desired directions and lines of sight (a world without probes)."""
        rng, n, k = self.rng, len(self.pos), len(self.flocks)
        p = rng.permutation(n)                         # uid of the member built i-th: uids do not follow the CSR order
        pos = np.zeros((n, 2), f32)
        pos[p] = np.asarray(self.pos, f64).reshape(n, 2).astype(f32)
        flags, state, flock = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.full(n, -1, np.int32)
        flags[p], state[p] = np.asarray(self.flags, np.uint32), np.asarray(self.state, np.uint8)
        offs = np.zeros(k + 1, np.int32)
        offs[1:] = np.cumsum([len(m) for m in self.flocks])
        mem = p[np.concatenate([np.asarray(m, np.int64) for m in self.flocks] + [np.zeros(0, np.int64)])].astype(np.int32)
        for f in range(k):
            flock[mem[offs[f]:offs[f + 1]]] = f
        assert len(np.unique(mem)) == len(mem) == n and np.abs(pos[:, 0]).max() <= 128.0 * w - 12 and np.abs(pos[:, 1]).max() <= 128.0 * h - 12
        vdes, vel, los = np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.zeros(n, np.uint8)
        if general:
            ang = rng.uniform(0, 2 * np.pi, n)
            vdes = np.stack([np.cos(ang), np.sin(ang)], 1).astype(f32)
            vel = np.where((state == STATE_ARRIVED)[:, None], 0, rng.normal(0, 0.3, (n, 2))).astype(f32)
            los = (rng.rand(n) < 0.3).astype(np.uint8)
        arrays = {"pos_xz": pos, "vel_xz": vel, "radius": np.ones(n, f32), "max_speed": np.full(n, 20.0, f32),
                  "speed": np.full(n, 100.0, f32), "flags": flags, "state": state, "has_dest_los": los, "flock": flock,
                  "flock_target_xz": rng.uniform(-100, 100, (k, 2)).astype(f32), "flock_offsets": offs, "flock_members": mem,
                  "vdes_xz": vdes}
        return CohWorld(name, w, h, arrays, hz, p[np.asarray(self.probes, np.int64)] if self.probes else (),
                        {t: p[np.asarray(v, np.int64)] for t, v in self.tags.items()}, slab)


def _r32(a):
    return np.asarray(a, f64).astype(f32).astype(f64)


def _sum64(me, pts):
    """sum_j pts_j * exp(-6 t_j) in float64: what the root finds work on."""
    pts = np.asarray(pts, f64).reshape(-1, 2)
    d = np.hypot(pts[:, 0] - me[0], pts[:, 1] - me[1])
    return (pts * np.exp(4.5 - 0.12 * d)[:, None]).sum(0)


def _root(g, lo, hi):
    """A root of the monotone g on [lo, hi] by bisection, or None when there is no sign change."""
    glo, ghi = g(lo), g(hi)
    if not glo * ghi < 0:
        return None
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        gm = g(mid)
        if gm * glo > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _tune(me, u, fixed, count, want, side, nt, lo, hi):
    """Positions of nt tuner mates on the line me_r * u -- at radial coordinate side * s, half a unit apart across the line
    -- such that (com - me) . u = want, com over `count` mates: the 1-D root find (positions rounded to float32)."""
    v = np.array([-u[1], u[0]])
    base = _sum64(me, fixed) if len(fixed) else np.zeros(2)

    def place(s):
        return _r32([side * s * u + (k - (nt - 1) / 2.0) * 0.5 * v for k in range(nt)])

    def g(s):
        return ((base + _sum64(me, place(s))) / count - me) @ u - want

    s = _root(g, lo, hi)
    return None if s is None else place(s)


# ---------------------------------------------------------------------------------------------
# window: probes in the window, flocks of 2, 3, 17, 33 and 257 members, mates between 0 and 300 wu
# ---------------------------------------------------------------------------------------------
WINDOW_FLOCKS = {2: (70, 8), 3: (70, 8), 17: (60, 8), 33: (50, 8), 257: (12, 4), 300: (12, 0)}     # size: (tuned, origin) flocks
# the flocks of 300: 258 of the mates 910 wu and more from the probe, interleaved with the others.  Their weight is +0 and
# the box rule drops them: the first tile keeps some 36 members, no multiple of 16, and weighted mates wait in a carried tail
WINDOW_FAR = {300: 258}


def window(hz):
    B = _Builder(300 + hz)
    rng = B.rng
    lim = float(smf(hz))
    sites = []
    for F, (n_tuned, n_origin) in WINDOW_FLOCKS.items():
        for _ in range(n_origin):
            # origin: the probe at lim/15 .. lim from the origin, every mate 150-300 wu away
            a, rho = rng.uniform(0, 2 * np.pi), rng.uniform(0.12, 0.9) * lim
            pr = B.add((rho * np.cos(a), rho * np.sin(a)), garrisoned=True)
            B.probe(pr, "origin", "size%d" % F)
            ang, d = rng.uniform(0, 2 * np.pi, F - 1), rng.uniform(150, 300, F - 1)
            B.flock([pr] + [B.add((d[i] * np.cos(ang[i]), d[i] * np.sin(ang[i])), active=rng.rand() < 0.5) for i in range(F - 1)])
        done = 0
        while done < n_tuned:
            a, P = rng.uniform(0, 2 * np.pi), rng.uniform(340, 650)
            u = np.array([np.cos(a), np.sin(a)])
            me = _r32(P * u)
            if any(np.hypot(*(me - s)) < 40 for s in sites):
                continue                                         # (probes keep 40 wu apart: nobody in anybody's r = 30 query)
            want = rng.uniform(0.15, 0.85) * lim * rng.choice([-1, 1])
            nfar = WINDOW_FAR.get(F, 0)
            nm = F - 2 - nfar
            d, al = rng.uniform(40, 300, (nm + 1) // 2), rng.uniform(0.1, np.pi - 0.1, (nm + 1) // 2)

            def mates(lam):
                pts = []
                for k in range(nm):
                    sg = 1 if k % 2 == 0 else -1
                    ak = a + sg * al[k // 2] if (k // 2) * 2 + 1 < nm else a + (0 if al[k // 2] < np.pi / 2 else np.pi)
                    pts.append(me + lam * d[k // 2] * np.array([np.cos(ak), np.sin(ak)]))
                return _r32(pts).reshape(-1, 2)

            lam = 1.0
            if nm:
                goal = (F - 1) * (P + want) - 1.2 * P              # (the tuner takes a weight near 1.2: some 36 wu off the probe)
                r = _root(lambda l: _sum64(me, mates(l)) @ u - goal, 1e-3, 1.0)
                lam = 1.0 if r is None else r
            fixed = mates(lam)
            if nfar:
                fa, fr = a + np.pi + rng.uniform(-0.2, 0.2, nfar), rng.uniform(930.0 - P, 1000.0, nfar)
                fixed = np.concatenate([fixed, _r32(np.stack([fr * np.cos(fa), fr * np.sin(fa)], 1))])
            tun = _tune(me, u, fixed, F - 1, want, 1, 1, P + 1e-3, P + 500.0)
            if tun is None or np.hypot(*tun[0]) > 1000 or (nm and np.abs(fixed).max() > 1000):
                continue
            sites.append(me)
            pr = B.add(me)
            B.probe(pr, "tuned", "size%d" % F, *(["far_mates"] if nfar else []))
            B.flock([pr] + [B.add(q, active=False) for q in fixed] + [B.add(tun[0], active=False)])
            done += 1
    return B.finish("window%d" % hz, 8, 8, (hz,))


# ---------------------------------------------------------------------------------------------
# arith: 4096 and more probe/mate lengths, every probe next to the origin and in the window
# ---------------------------------------------------------------------------------------------
ARITH_SATS = 15
ULP16 = float(np.spacing(f32(16.0)))


def _arith_flock(B, lens, rho, kind, *tags):
    """One probe at rho * u, satellites at rho +- len on the line through the origin, tuners on that line (_tune).
    kind: "line" (direction at random), "axis" (along x or z: the lengths are exact)."""
    rng = B.rng
    if kind == "axis":
        u = np.array([1.0, 0.0]) if rng.rand() < 0.5 else np.array([0.0, 1.0])
    else:
        a = rng.uniform(0, 2 * np.pi)
        u = np.array([np.cos(a), np.sin(a)])
    me = _r32(rho * u)
    sg = np.where(np.arange(len(lens)) % 2 == 0, 1.0, -1.0)
    if kind == "axis":
        sg[:3] = [1.0, 1.0, -1.0]                                # (16 - ulp is a float below the origin, not above it)
    sats = _r32([(rho + s * l) * u for s, l in zip(sg, lens)]).reshape(-1, 2)
    want = rng.uniform(0.12, 0.6) * rng.choice([-1, 1])
    for nt in range(1, 40):
        count = len(sats) + nt
        need = count * (rho + want) - _sum64(me, sats) @ u
        if abs(need) / nt > 150:
            continue
        tun = _tune(me, u, sats, count, want, 1 if need > 0 else -1, nt, 17.0, 1000.0)
        if tun is not None:
            break
    else:
        return False
    pr = B.add(me, garrisoned=True)
    B.probe(pr, *tags)
    B.flock([pr] + [B.add(q, active=False) for q in sats] + [B.add(q, active=False) for q in tun])
    return True


def arith():
    B = _Builder(77)
    rng = B.rng
    lens = np.concatenate([np.logspace(-20, 0, 2048), np.linspace(1, 300, 2049)[1:]])
    for k in range(0, len(lens), ARITH_SATS):
        ch = lens[k:k + ARITH_SATS]
        # the probe 2^10 of the shortest length from the origin, at most 0.3: every length keeps ten bits and more
        rho = min(0.3, ch.min() * 1024.0) * rng.uniform(0.5, 1.0)
        tags = ["sweep"] + (["tiny_ss"] if ch.min() < 2.0 ** -46 else [])
        assert _arith_flock(B, ch, rho, "line", *tags)
    far = lambda m: rng.uniform(20, 300, m)                                          # noqa: E731
    for i in range(12):
        # len == 16.0 exactly and its two neighbours
        rho = rng.randint(1, 16) / 64.0
        assert _arith_flock(B, np.concatenate([[16.0, 16.0 + ULP16, 16.0 - ULP16 / 2], far(12)]), rho, "axis", "len16")
    for i in range(12):
        # two coincident satellites, and one coincident with the probe
        l = rng.uniform(1, 60)
        assert _arith_flock(B, np.concatenate([[l, 0.0], far(12), [l]])[[0, 1, 14] + list(range(2, 14))], 0.25 * rng.uniform(0.5, 1), "line", "coincident")
    for i in range(24):
        # one satellite below 16 among satellites beyond 20: one lane of one batch on the `close` path
        assert _arith_flock(B, np.concatenate([[rng.uniform(0.5, 15)], far(14)]), 0.2, "line", "one_close")
    for i in range(24):
        # one satellite a few 1e-20 .. 1e-15 away (0 < ss < 2^-90) among satellites beyond 20: one lane on the `odd` path
        l = 10.0 ** rng.uniform(-19.5, -15)
        assert _arith_flock(B, np.concatenate([[l], far(14)]), l * rng.uniform(1, 3), "line", "one_odd", "tiny_ss")
    return B.finish("arith", 8, 8, (20,))


ARITH_EDGES = ("len16", "coincident", "tiny_ss", "one_close", "one_odd")


# ---------------------------------------------------------------------------------------------
# far_clusters: a 8 x 1-chunk map, clusters 890-930 wu from each other's boxes, interleaved member order
# ---------------------------------------------------------------------------------------------
# per flock: the tile of the OBSERVER wave -- 13 active members of the cluster at one end of the map, three inactive ones
# from elsewhere -- and the survivors of every tile in that wave's eyes
FAR_PLANS = ((0, (15, 0, 33)), (0, (16, 1, 17)), (0, (17, 31, 32)), (1, (1, 16, 0)), (2, (33, 0, 15)))
FAR_TILES = (256, 256, 120)


def far_clusters():
    B = _Builder(906)
    rng = B.rng

    def inactive_kw():
        return {"active": False, "movable": True} if rng.rand() < 0.5 else {"active": False, "held": True, "movable": True}

    def some_kw():
        return inactive_kw() if rng.rand() < 0.15 else {"active": True}

    for fi, (obs_tile, plan) in enumerate(FAR_PLANS):
        sx = 1.0 if fi % 2 == 0 else -1.0                        # (every other flock mirrored: the dense end alternates)
        three = fi % 2 == 0                                      # two or three clusters

        def A():
            return (sx * rng.uniform(-1010, -995.5), rng.uniform(-28, 28))

        def B_near():                                            # 890 .. 905.99 from the observer's box
            return (sx * (-995.0 + rng.choice([rng.uniform(890, 905), rng.uniform(905.9, 905.99)])), rng.uniform(-28, 28))

        def B_far():                                             # 906.01 .. 930
            return (sx * (-995.0 + rng.choice([rng.uniform(907, 930), rng.uniform(906.01, 906.1)])), rng.uniform(-28, 28))

        def C():                                                 # 890 and more from the middle cluster's box
            return (sx * rng.uniform(825, 1010), rng.uniform(-110, 110))

        members = []
        for ti, (size, k) in enumerate(zip(FAR_TILES, plan)):
            slots = [None] * size
            free = list(range(size))
            if ti == obs_tile:
                w0 = rng.randint(0, size // APW) * APW
                zext = 30.0 + 2.5 * fi
                own = [(sx * -995.0, -zext), (sx * -995.0, zext)] + [A() for _ in range(11)]
                wave = [B.add(q, active=True) for q in own] + [B.add(C() if three else B_far(), **inactive_kw()) for _ in range(3)]
                for s, uid in zip(range(w0, w0 + APW), [wave[i] for i in rng.permutation(APW)]):
                    slots[s] = uid
                free = [s for s in free if not w0 <= s < w0 + APW]
                k -= 13
            surv = set(rng.choice(free, k, replace=False)) if k else set()
            for s in free:
                if s in surv:
                    slots[s] = B.add(A() if rng.rand() < 0.3 else B_near(), **some_kw())
                else:
                    slots[s] = B.add(C() if three and rng.rand() < 0.5 else B_far(), **some_kw())
            members += slots
        B.flock(members, shuffle=False)
    return B.finish("far_clusters", 8, 1, (20,), general=True)


# ---------------------------------------------------------------------------------------------
# plan_shapes: 1 .. 513 flocks of 0-20 members, empty flocks in front, in the middle and at the end
# ---------------------------------------------------------------------------------------------
def plan_shape(nf):
    B = _Builder(5000 + nf)
    rng = B.rng
    sizes = rng.randint(0, 21, nf)
    if nf == 1:
        sizes[:] = 20
    else:
        sizes[[0, 1, nf // 2, nf // 2 + 1, nf // 2 + 2, nf - 1]] = 0
        sizes[[2, nf // 3, nf - 2]] = 1
        sizes[[3, nf // 4, nf - 3]] = [7, 16, 20]                # (these three: every member idle)
    idle_flocks = () if nf == 1 else (3, nf // 4, nf - 3)
    for f in range(nf):
        kw = [({"active": False, "movable": True} if f in idle_flocks or rng.rand() < 0.15 else {"active": True}) for _ in range(sizes[f])]
        B.flock([B.add(rng.uniform(-490, 490, 2), **k) for k in kw])
    n = int(sizes.sum())
    return B.finish("plan_%d" % nf, 4, 4, (20,), general=True, slab=(n // 3, n // 3 + max(2, n // 8), 7))


_WORLDS = {}
NAMES = ("window20", "window1", "far_clusters", "arith") + tuple("plan_%d" % nf for nf in PLAN_SHAPES)


def get(name):
    """The world `name`, built once."""
    assert name in NAMES, name
    if name not in _WORLDS:
        if name.startswith("window"):
            _WORLDS[name] = window(int(name[6:]))
        elif name.startswith("plan_"):
            _WORLDS[name] = plan_shape(int(name[5:]))
        else:
            _WORLDS[name] = {"far_clusters": far_clusters, "arith": arith}[name]()
    return _WORLDS[name]
