"""Structured ClearPath problems: agents inside regular formations, where exact ties occur.  Pure numpy; the shared
source of tests/test_cp_lattice_cpu.py and tests/test_cp_lattice_gpu.py.  Test infrastructure only.

The random problems of cases.cp_problems never tie.  Units that have arrived stand on tile centres and corners, and
formations are lattices with one common velocity: there the branch and bound of the device search (csrc/agent_group.h)
meets what random floats do not give it --

    * candidates at EQUAL distance from des_v: compute_vnew (clearpath.c:368) keeps the first strict minimum in the order
      intersections (i, j) row-major, then projections; the device's `len == Blen && idx < Bidx` has to pick the same one;
    * neighbours at EQUAL distance from the agent when remove_furthest (clearpath.c:390) drops one: the first strict
      maximum in scan order (dynamic list, then static), the last entry moved into the hole (vec_del) -- what cp_jump
      simulates;
    * DUPLICATE cones, neighbours exactly ON the agent (same_position: no cone), vertical and parallel side rays
      (C_InfiniteLineIntersection's three shapes).

Layout as cases.cp_problems: (ent [nq][5], des [nq][2], dyn [nq][32][5], nd [nq], stat [nq][32][5], ns [nq]), an entity =
(x, z, vx, vz, radius).  Every coordinate is a multiple of 1/8 below 2^10: exact in float32, sums with OFFSET included.
NAMES[i] names problem i.  Three families:

    lattice    the agent on a square lattice of spacing 2 / 2.5 / 3 / 4, 1 ring (8 neighbours) or 2 rings (24), every
               radius 1 or 1.5 (spacing 2 and 2.5 with radius 1.5: touching and overlapping discs, enclosed agents), dynamic
               neighbours with the agent's own velocity, static ones at rest; all dynamic | all static | alternating
               (only a search with BOTH lists non-empty retries, clearpath.c:712)
    ring       the twelve integer points at distance 5, scaled by 0.5 / 0.75 / 1: every neighbour equally far; as a dynamic
               list, a static list, and each of them with every neighbour twice (24 entries, identical cones).  Scale 0.75
               with radius 2.5 + 2.5: the tangent of the neighbours at (+-3, +-2.25) is (0, +-6.25) -- a vertical side ray
    coincident 1-3 neighbours exactly on the agent, first | in the middle | last in their list, among lattice neighbours

premises(problems) counts, from the inputs and the rules of clearpath.c alone (tests/tools/cp_model.py: float32 numpy),
the problems that really have a tie among candidates, a tie at a removal, a vertical side ray."""
import numpy as np

from tests.tools import cp_model

f32 = np.float32
OFFSET = (100.0, -37.0)
MAX_NEIGHBOURS = 32
SPACINGS = (2.0, 2.5, 3.0, 4.0)
VELS = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5))
DES_KINDS = ("axis", "diagonal", "reversed", "zero")
LISTS = ("dyn", "stat", "alt")
# (+-5, 0), (+-4, +-3), (+-3, +-4), (0, +-5), counter-clockwise from (5, 0)
RING5 = ((5, 0), (4, 3), (3, 4), (0, 5), (-3, 4), (-4, 3), (-5, 0), (-4, -3), (-3, -4), (0, -5), (3, -4), (4, -3))


def lattice_offsets(rings):
    """The (2 rings + 1)^2 - 1 lattice points around the origin, row by row (z outer, x inner), in units of the spacing."""
    k = np.arange(-rings, rings + 1)
    zz, xx = np.meshgrid(k, k, indexing="ij")
    pts = np.stack([xx.ravel(), zz.ravel()], 1)
    return pts[(pts != 0).any(1)].astype(np.float64)


def des_for(kind, vel):
    """des_v of a problem: along +x | along the diagonal | against the common velocity (-x for a formation at rest) | 0."""
    if kind == "axis":
        return (0.75, 0.0)
    if kind == "diagonal":
        return (0.5, 0.5)
    if kind == "reversed":
        return (-vel[0] * 1.5, -vel[1] * 1.5) if (vel[0] or vel[1]) else (-0.75, 0.0)
    return (0.0, 0.0)


class _Builder:
    def __init__(self):
        self.rows, self.names = [], []

    def add(self, name, vel, radius, des, dyn, stat):
        """dyn / stat: lists of (dx, dz, vx, vz, radius) relative to the agent."""
        assert len(dyn) <= MAX_NEIGHBOURS and len(stat) <= MAX_NEIGHBOURS, name
        assert name not in self.names, name
        self.names.append(name)
        self.rows.append((vel, radius, des, list(dyn), list(stat)))

    def arrays(self):
        nq = len(self.rows)
        ent = np.zeros((nq, 5), f32)
        des = np.zeros((nq, 2), f32)
        dyn = np.zeros((nq, 32, 5), f32)
        stat = np.zeros((nq, 32, 5), f32)
        nd = np.zeros(nq, np.int32)
        ns = np.zeros(nq, np.int32)
        for i, (vel, radius, d, dl, sl) in enumerate(self.rows):
            ent[i] = (OFFSET[0], OFFSET[1], vel[0], vel[1], radius)
            des[i] = d
            for arr, cnt, lst in ((dyn, nd, dl), (stat, ns, sl)):
                cnt[i] = len(lst)
                for k, (dx, dz, vx, vz, r) in enumerate(lst):
                    arr[i, k] = (OFFSET[0] + dx, OFFSET[1] + dz, vx, vz, r)
        # (exactly representable: the float32 arrays hold what the builder meant)
        for i, (vel, radius, d, dl, sl) in enumerate(self.rows):
            for arr, lst in ((dyn, dl), (stat, sl)):
                for k, (dx, dz, vx, vz, r) in enumerate(lst):
                    assert float(arr[i, k, 0]) == OFFSET[0] + dx and float(arr[i, k, 1]) == OFFSET[1] + dz, self.names[i]
        return ent, des, dyn, nd, stat, ns


def _split(points, vel, radius, lists):
    """Lattice / ring points as neighbour lists: all dynamic (the agent's velocity), all static (at rest), alternating."""
    dyn, stat = [], []
    for k, (x, z) in enumerate(points):
        moving = lists == "dyn" or (lists == "alt" and k % 2 == 0)
        (dyn if moving else stat).append((x, z, vel[0], vel[1], radius) if moving else (x, z, 0.0, 0.0, radius))
    return dyn, stat


def _build():
    B = _Builder()
    # ---- lattices: the full factorial of spacing x rings x radius x lists (48), each with three of the 16 (velocity,
    # des_v) pairs, cycling.  The ENCLOSED ones -- alternating lists (only they retry), two rings deep with radius 1.5 or
    # spacing <= 2.5, or one ring at spacing 2 with radius 1.5; in motion their first attempt finds no admissible
    # candidate (premises() counts them) -- with eight pairs, all of a moving formation
    c = 0
    for sp in SPACINGS:
        for rings in (1, 2):
            for radius in (1.0, 1.5):
                for lists in LISTS:
                    pts = lattice_offsets(rings) * sp
                    enclosed = lists == "alt" and ((rings == 2 and (radius == 1.5 or sp <= 2.5)) or (sp == 2.0 and radius == 1.5))
                    for t in range(8 if enclosed else 3):
                        vi, di = ((1 + t % 3), (c + t) % 4) if enclosed else ((c + t) % 4, (c // 4 + t) % 4)
                        vel = VELS[vi]
                        dyn, stat = _split(pts, vel, radius, lists)
                        B.add("lattice-s%g-r%d-R%g-%s-v%d-%s" % (sp, rings, radius, lists, vi, DES_KINDS[di]), vel, radius,
                              des_for(DES_KINDS[di], vel), dyn, stat)
                    c += 1
    # ---- equal-distance rings: 3 scales x 3 radii x 4 forms x 4 des_v, the velocity cycling
    c = 0
    for scale in (0.5, 0.75, 1.0):
        for radius in (1.0, 1.5, 2.5):
            for form in ("dyn", "stat", "dyn2", "stat2"):
                pts = [(x * scale, z * scale) for x, z in RING5]
                if form.endswith("2"):
                    pts = [p for p in pts for _ in range(2)]           # every neighbour twice, side by side
                for di, kind in enumerate(DES_KINDS):
                    vel = VELS[(c + di) % 4]
                    dyn, stat = _split(pts, vel, radius, form[:-1] if form.endswith("2") else form)
                    B.add("ring-k%g-R%g-%s-v%d-%s" % (scale, radius, form, (c + di) % 4, kind), vel, radius,
                          des_for(kind, vel), dyn, stat)
                c += 1
    # ---- coincident neighbours among the eight of a lattice ring
    c = 0
    for sp in (2.5, 4.0):
        for count in (1, 2, 3):
            for where in ("first", "middle", "last"):
                for lists in ("dyn", "alt"):
                    vel = VELS[1 + c % 3]
                    kind = DES_KINDS[c % 3]
                    dyn, stat = _split(lattice_offsets(1) * sp, vel, 1.0, lists)
                    # the coincident ones go into the dynamic list (with the common velocity), and for the alternating
                    # problems one of them into the static list as well
                    for lst, moving, k in ((dyn, True, count), (stat, False, 1 if lists == "alt" else 0)):
                        on = [(0.0, 0.0, vel[0], vel[1], 1.0) if moving else (0.0, 0.0, 0.0, 0.0, 1.0)] * k
                        at = {"first": 0, "middle": len(lst) // 2, "last": len(lst)}[where]
                        lst[at:at] = on
                    B.add("coincident-s%g-n%d-%s-%s" % (sp, count, where, lists), vel, 1.0, des_for(kind, vel), dyn, stat)
                    c += 1
    return B


_PROBLEMS = None
NAMES = []


def problems():
    """(ent, des, dyn, nd, stat, ns) of all problems, built once; NAMES[i] names problem i."""
    global _PROBLEMS
    if _PROBLEMS is None:
        B = _build()
        NAMES[:] = B.names
        _PROBLEMS = B.arrays()
        assert len(NAMES) <= 400, len(NAMES)
    return _PROBLEMS


_EXPECTED = []


def expected():
    """G_ClearPath_NewVelocity (clearpath.c:694) of the reference build for every problem, computed once."""
    if not _EXPECTED:
        from oracle import pfref
        ent, des, dyn, nd, stat, ns = problems()
        _EXPECTED.append(np.stack([pfref.clearpath_new_velocity(ent[i], des[i], dyn[i, :nd[i]], stat[i, :ns[i]])
                                   for i in range(len(ent))]))
    return _EXPECTED[0]


def mismatches(got, exp):
    """Problems whose velocity is not the expected one bit for bit (NaN in both counts as equal)."""
    both = np.isnan(exp) & np.isnan(got)
    g, x = np.where(both, 0, got).astype(f32).view(np.uint32), np.where(both, 0, exp).astype(f32).view(np.uint32)
    return np.flatnonzero((g != x).any(1))


def select(problems_, idx):
    return tuple(a[idx] for a in problems_)


def subset(step=3):
    """Indices of every step-th problem of each family (a family keeps its first one)."""
    problems()
    out = []
    for fam in ("lattice", "ring", "coincident"):
        idx = [i for i, n in enumerate(NAMES) if n.startswith(fam)]
        out += idx[::step]
    return np.array(out)


# ---------------------------------------------------------------------------------------------
# premises: the reference's rules on the inputs, float32 numpy (tests/tools/cp_model.py)
# ---------------------------------------------------------------------------------------------
def _candidates(ent, des, C):
    """One attempt of clearpath_new_velocity (clearpath.c:552) as lists: None when des_v itself is admissible, else
    (lens, ids, mirror ids) of the admissible candidates in the reference's order -- intersections (i, j) row-major,
    then projections -- id = i * n_rays + j, or n_rays^2 + r for the projection on ray r."""
    n = len(C["ax"])
    ex, ez, d0, d1 = f32(ent[0]), f32(ent[1]), f32(des[0]), f32(des[1])
    if n == 0 or not cp_model.inside_cone(C, np.arange(n), ex + d0, ez + d1).any():
        return None
    px, pz, dx, dz, s = cp_model.rays_of(C)
    nr = 2 * n
    I, J = np.meshgrid(np.arange(nr), np.arange(nr), indexing="ij")
    ok, cx, cz = cp_model.ray_isect(px[I], pz[I], dx[I], dz[I], s[I], px[J], pz[J], dx[J], dz[J], s[J])
    ok &= I != J
    inn = np.zeros(ok.shape, bool)
    for c in range(n):
        inn |= cp_model.inside_cone(C, c, cx, cz)
    adm = ok & ~inn
    clen = cp_model.vlen(d0 - (cx - ex), d1 - (cz - ez))
    plen = dx * d0 + dz * d1
    qx, qz = px + dx * plen, pz + dz * plen
    q_in = np.zeros(nr, bool)
    for c in range(n):
        q_in |= cp_model.inside_cone(C, c, qx, qz)
    qlen = cp_model.vlen(d0 - (qx - ex), d1 - (qz - ez))
    lens = np.concatenate([clen[adm], qlen[~q_in]])
    ids = np.concatenate([(I * nr + J)[adm], nr * nr + np.flatnonzero(~q_in)])
    mirror = np.concatenate([(J * nr + I)[adm], -np.ones(int((~q_in).sum()), np.int64)])
    return lens, ids, mirror


def _analyse(ent, des, dyn, stat):
    """G_ClearPath_NewVelocity (clearpath.c:694) on one problem: (the winner ties with another admissible candidate that
    is not the same two rays the other way round, two neighbours of one list equally far at a removal, a vertical side
    ray in some attempt, failed attempts)."""
    dyn, stat = [np.array(r, f32) for r in dyn], [np.array(r, f32) for r in stat]
    ex, ez = f32(ent[0]), f32(ent[1])
    tie = rem_tie = vertical = False
    failed = 0
    while True:
        nbs = np.array(dyn + stat, f32).reshape(-1, 5)
        isdyn = np.arange(len(nbs)) < len(dyn)
        C = cp_model.make_cones(ent, nbs, isdyn)
        vertical |= bool(np.isnan(C["sl"]).any() or np.isnan(C["sr"]).any())
        cand = _candidates(ent, des, C)
        if cand is None:
            break
        lens, ids, mirror = cand
        if len(lens):
            # compute_vnew (clearpath.c:368): the first strict minimum (a NaN length never wins)
            fin = ~np.isnan(lens)
            if fin.any():
                m = lens[fin].min()
                w = np.flatnonzero(fin & (lens == m))
                tie = bool(((ids[w[1:]] != ids[w[0]]) & (ids[w[1:]] != mirror[w[0]])).any())
            break
        failed += 1
        # remove_furthest (clearpath.c:390): the first strict maximum over dyn then stat; vec_del moves the last entry in
        best, where = -np.inf, None
        for lst in (dyn, stat):
            d = [cp_model.vlen(ex - r[0], ez - r[1]) for r in lst]
            for j, v in enumerate(d):
                if v > best:
                    best, where = v, (lst, j)
        if where is not None:
            for lst in (dyn, stat):
                d = np.array([cp_model.vlen(ex - r[0], ez - r[1]) for r in lst], f32)
                rem_tie |= int((d == best).sum()) >= 2
            lst, j = where
            lst[j] = lst[-1]
            lst.pop()
        if not (len(dyn) > 0 and len(stat) > 0):
            break
    return tie, rem_tie, vertical, failed


def premises(problems_):
    """{"candidate_tie", "removal_tie", "vertical_ray"}: problems whose winning admissible candidate ties in distance with
    another admissible candidate (of another index, and not merely the same pair of rays the other way round); problems
    where two neighbours of one list are equally far at a removal; problems with a vertical side ray.  "retried": problems
    whose first attempt fails, by the same model."""
    ent, des, dyn, nd, stat, ns = problems_
    out = {"candidate_tie": 0, "removal_tie": 0, "vertical_ray": 0, "retried": 0}
    for i in range(len(ent)):
        t, r, v, failed = _analyse(ent[i], des[i], list(dyn[i, :nd[i]]), list(stat[i, :ns[i]]))
        out["candidate_tie"] += t
        out["removal_tie"] += r
        out["vertical_ray"] += v
        out["retried"] += failed > 0
    return out
