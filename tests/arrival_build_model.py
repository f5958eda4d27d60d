"""A plain numpy model of the FIRST build of an arrival zone, the `!built` branch of G_Arrival_UpdateFlock
(arrival.c:784-848), written from the reference's text: arrival_near_goal (:377), arrival_zone_radius (:363),
arrival_region_area (:147), N_ClosestPathable (nav.c:4126), arrival_approach_axis (:236), N_ClosestConnectedPathableTiles
(nav.c:4192) over a heap that follows lib/public/pqueue.h:109-208, N_TileKeysForPositions (nav.c:4304),
arrival_thin_centered_slots (:196), the clear-line filter (:810-817), the centre of mass and N_DestIDForPos (:819-830,
nav.c:3367, n_dest_id nav.c:839), slot_cmp_far_banded (:130).  The tail (:839-847) is tests/arrival_flock_model.py: the
rings and arrival_realloc_slots.  The two qsorts are STABLE sorts (glibc's merge sort; tests/test_arrival_build_cpu.py runs
libc's qsort against this).  Floats are np.float32 operation by operation, double where the reference is.

A zone is a dict as tests/arrival_flock_model.py takes it (phase INACTIVE, arg_layer, arg_unit_radius, arg_total_members)
whose slots_xz / slot_ring / room_keys are its ROOM; members as there.  `wrong`: one of WRONG, a deliberately wrong variant
of one statement."""
import numpy as np

from tests import arrival_flock_model as afm
from tests.arrival_velocity_model import EPS, Map, key_of, segment_within, vlen

F = np.float32
INACTIVE, FILLING = afm.INACTIVE, afm.FILLING
AB_WAIT, AB_HOST = 0x01, 0x80
WINDOW_R, HEAP_NODES, DQ_R = 127, 4096, 63
MAX_SLOTS = 4096
DELTAS8 = ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))     # {r, c}, nav.c:4223
WRONG = ("fifo_ties", "four_connected", "centre_not_pushed", "unstable_sort", "le_spacing", "thin_all", "no_clear_line",
         "pairwise_com", "trunc_band", "ref_centre")


class Host(Exception):
    """What the device leaves to the host."""


class BuildMap(Map):
    """tests/arrival_velocity_model.Map plus the cost plane per layer ([h][w][64][64] u8; 255 = COST_IMPASSABLE)."""

    def __init__(self, w, h, blockers, cost=None):
        Map.__init__(self, w, h, blockers)
        cost = cost or {}
        self.cost = {l: np.asarray(cost.get(l, np.ones((h, w, 64, 64), np.uint8))).reshape(h, w, 64, 64) for l in self.blockers}

    def tile_blocked(self, layer, r, c):
        """n_tile_blocked, nav.c:235"""
        t = (r >> 6, c >> 6, r & 63, c & 63)
        return self.cost[layer][t] == 255 or self.blockers[layer][t] > 0

    def abs_tile(self, x, z):
        t = self.tile(x, z)
        return None if t is None else (t[0] * 64 + t[2], t[1] * 64 + t[3])

    def centre_of(self, r, c):
        return F(self.mx - F(F(F(c) + F(0.5)) * F(4))), F(self.mz + F(F(F(r) + F(0.5)) * F(4)))


def region_area(radius):
    """arrival_region_area, arrival.c:147"""
    area = np.pi * radius * radius + float(F(0.5))
    return int(area) if area < MAX_SLOTS else MAX_SLOTS


def room_needed(total, unit_radius):
    area = region_area(afm.zone_radius(total, unit_radius))
    return min(total, area), area


# ---------------------------------------------------------------------------------------------
# pqueue.h
# ---------------------------------------------------------------------------------------------
class Heap:
    def __init__(self):
        self.prio, self.data, self.size, self.peak = [None], [None], 0, 0

    def push(self, p, d):
        if len(self.prio) < self.size + 2:
            self.prio.append(None)
            self.data.append(None)
        curr = self.size + 1
        parent = curr // 2
        while curr > 1 and self.prio[parent] > p:
            self.prio[curr], self.data[curr] = self.prio[parent], self.data[parent]
            curr, parent = parent, parent // 2
        self.prio[curr], self.data[curr] = p, d
        self.size += 1
        self.peak = max(self.peak, self.size)

    def pop(self):
        out = self.data[1]
        self.prio[1], self.data[1] = self.prio[self.size], self.data[self.size]
        self.size -= 1
        root = 1
        while root != self.size + 1:
            target = self.size + 1
            left, right = root * 2, root * 2 + 1
            if left <= self.size and self.prio[left] < self.prio[target]:
                target = left
            if right <= self.size and self.prio[right] < self.prio[target]:
                target = right
            self.prio[root], self.data[root] = self.prio[target], self.data[target]
            root = target
        return out


class Fifo:
    """WRONG: equal priorities leave in the order they came (a stable priority queue)."""

    def __init__(self):
        self.items, self.seq, self.size, self.peak = [], 0, 0, 0

    def push(self, p, d):
        self.items.append((p, self.seq, d))
        self.seq += 1
        self.size += 1

    def pop(self):
        i = min(range(len(self.items)), key=lambda k: self.items[k][:2])
        self.size -= 1
        return self.items.pop(i)[2]


def connected_tiles(m, layer, cx, cz, maxout, wrong=None, stats=None):
    """N_ClosestConnectedPathableTiles with max_radius = 0: the absolute tiles in out[] order.  Raises Host where the
    device's window or heap end."""
    if maxout <= 0:
        return []
    start = m.abs_tile(cx, cz)
    if start is None:
        return []
    cr, cc = start
    heap = Fifo() if wrong == "fifo_ties" else Heap()
    visited = {start}
    if not (wrong == "centre_not_pushed" and m.tile_blocked(layer, cr, cc)):
        heap.push(F(0), start)
    out, reach = [], 0
    deltas = DELTAS8[:4] if wrong == "four_connected" else DELTAS8
    while heap.size > 0 and len(out) < maxout:
        r, c = heap.pop()
        if not m.tile_blocked(layer, r, c):
            out.append((r, c))
            if len(out) == maxout:
                break
        for dr, dc in deltas:
            nr, nc = r + dr, c + dc
            if nr < 0 or nr >= m.h * 64 or nc < 0 or nc >= m.w * 64:
                continue
            reach = max(reach, abs(nr - cr), abs(nc - cc))
            if reach > WINDOW_R:
                raise Host("window")
            if (nr, nc) in visited:
                continue
            visited.add((nr, nc))
            if m.tile_blocked(layer, nr, nc):
                continue
            px, pz = m.centre_of(nr, nc)
            dx, dz = F(px - cx), F(pz - cz)
            if heap.size + 1 > HEAP_NODES:
                raise Host("heap")
            heap.push(F(F(dx * dx) + F(dz * dz)), (nr, nc))
    if stats is not None:
        stats.update(reach=reach, peak=heap.peak, left=heap.size)
    return out


def closest_pathable(m, layer, x, z):
    """N_ClosestPathable(p) ? snapped : p.  Raises Host for a point that is NaN or off the map (the reference asserts) and
    where the device's 4-connected flood leaves its window of DQ_R tiles."""
    start = m.abs_tile(x, z)
    if start is None:
        raise Host("off the map")
    if not m.tile_blocked(layer, *start):
        return F(x), F(z)
    queue, head, visited = [start], 0, set()
    found = None
    while head < len(queue):
        r, c = queue[head]
        head += 1
        if not m.tile_blocked(layer, r, c):
            found = (r, c)
            break
        for dr, dc in DELTAS8[:4]:
            nr, nc = r + dr, c + dc
            if nr < 0 or nr >= m.h * 64 or nc < 0 or nc >= m.w * 64 or (nr, nc) in visited:
                continue
            visited.add((nr, nc))
            queue.append((nr, nc))
    level = (abs(found[0] - start[0]) + abs(found[1] - start[1])) if found else 1 << 30
    # the device gives up when a level in front of the answer holds an on-map tile outside its window: the nearest such
    # tile lies DQ_R + 1 tiles away along a row or a column, where the map reaches that far
    reach = max(start[0], m.h * 64 - 1 - start[0], start[1], m.w * 64 - 1 - start[1])
    if level - 1 > DQ_R and reach > DQ_R:
        raise Host("dq window")
    if found is None:
        return F(x), F(z)
    return m.bounds((found[0] >> 6, found[1] >> 6, found[0] & 63, found[1] & 63))


def dest_id(m, x, z, layer):
    """N_DestIDForPos (nav.c:3367) with FACTION_ID_NONE"""
    t = m.tile(x, z)
    if t is None:
        raise Host("com off the map")
    return ((t[0] & 0x3f) << 26) | ((t[1] & 0x3f) << 20) | ((t[2] & 0x3f) << 14) | ((t[3] & 0x3f) << 8) | ((layer & 0xf) << 4) | 0xf


def near_goal(pos_xz, mem, target):
    with np.errstate(all="ignore"):
        return any(vlen(F(target[0] - pos_xz[u][0]), F(target[1] - pos_xz[u][1])) < F(150) for u in mem["uid"])


def approach_axis(pos_xz, mem, target):
    with np.errstate(all="ignore"):
        sx, sz = F(0), F(0)
        for u in mem["uid"]:
            sx, sz = F(sx + pos_xz[u][0]), F(sz + pos_xz[u][1])
        n = len(mem["uid"])
        if n > 0:
            inv = F(F(1) / F(n))
            sx, sz = F(sx * inv), F(sz * inv)
        ax, az = F(target[0] - sx), F(target[1] - sz)
        l = vlen(ax, az)
        return (F(ax / l), F(az / l)) if l > EPS else (F(0), F(1))


def stable_order(keys_lt, n, reverse_ties=False):
    """The order a stable sort gives: indices sorted by the comparator `keys_lt(i, j)` = i sorts before j."""
    import functools
    idx = list(range(n))
    cmp = lambda i, j: -1 if keys_lt(i, j) else (1 if keys_lt(j, i) else 0)           # noqa: E731
    if reverse_ties:
        idx.reverse()
    return sorted(idx, key=functools.cmp_to_key(cmp))


def near_ref_keys(slots, ref):
    with np.errstate(all="ignore"):
        dx, dz = slots[:, 0] - F(ref[0]), slots[:, 1] - F(ref[1])
        return (dx * dx + dz * dz).astype(F)


def thin(slots, centre, axis, target, spacing, wrong=None):
    """arrival_thin_centered_slots: (the kept slots in order, the sort keys, the sorted order)"""
    if len(slots) == 0:
        return slots, np.zeros(0, F), []
    fwd = F(F(2) * F(4))
    ref = (F(centre[0] + F(axis[0] * fwd)), F(centre[1] + F(axis[1] * fwd)))
    if wrong == "ref_centre":
        ref = centre
    dd = near_ref_keys(slots, ref)
    order = stable_order(lambda i, j: dd[i] < dd[j], len(slots), wrong == "unstable_sort")
    s = slots[order]
    sp2 = F(F(spacing) * F(spacing))
    kept = []
    for cand in s:
        if len(kept) >= target and wrong != "thin_all":
            break
        if kept:
            k = np.array(kept, F)
            dx, dz = cand[0] - k[:, 0], cand[1] - k[:, 1]
            d2 = (dx * dx + dz * dz).astype(F)
            if ((d2 <= sp2) if wrong == "le_spacing" else (d2 < sp2)).any():
                continue
        kept.append(cand)
    return np.array(kept, F).reshape(-1, 2), dd, order


def band_keys(slots, centre, axis, band_w, wrong=None):
    with np.errstate(all="ignore"):
        rx, rz = (slots[:, 0] - F(centre[0])).astype(F), (slots[:, 1] - F(centre[1])).astype(F)
        q = ((rx * F(axis[0])).astype(F) + (rz * F(axis[1])).astype(F)).astype(F) / F(band_w)
        band = (np.trunc(q) if wrong == "trunc_band" else np.floor(q)).astype(np.int64)
        px, pz = F(-axis[1]), F(axis[0])
        lat = ((rx * px).astype(F) + (rz * pz).astype(F)).astype(F)
    return band, lat


def far_near(slots, centre, axis, band_w, wrong=None):
    if len(slots) == 0:
        return slots
    band, lat = band_keys(slots, centre, axis, band_w, wrong)
    lt = lambda i, j: band[i] > band[j] or (band[i] == band[j] and lat[i] < lat[j])       # noqa: E731
    return slots[stable_order(lt, len(slots), wrong == "unstable_sort")]


def centre_of_mass(slots, wrong=None):
    cx, cz = F(0), F(0)
    if wrong == "pairwise_com" and len(slots):
        x, z = list(slots[:, 0]), list(slots[:, 1])
        while len(x) > 1:
            x = [F(x[i] + x[i + 1]) if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
            z = [F(z[i] + z[i + 1]) if i + 1 < len(z) else z[i] for i in range(0, len(z), 2)]
        cx, cz = x[0], z[0]
    else:
        for s in slots:
            cx, cz = F(cx + s[0]), F(cz + s[1])
    if len(slots):
        cx, cz = F(cx / F(len(slots))), F(cz / F(len(slots)))
    return cx, cz


def structural_host(m, zone, n_ents, mem):
    uid = np.asarray(mem["uid"], np.int64)
    layer = int(zone["arg_layer"])
    ur = F(zone["arg_unit_radius"])
    return (zone["phase"] != INACTIVE or layer not in m.blockers or bool(((uid < 0) | (uid >= n_ents)).any())
            or not (ur > 0 and ur < F(np.inf)))


def build_zone(m, zone, pos_xz, mem, target, wrong=None, stats=None):
    """One call for one zone.  Returns a dict: status; zone (a new dict in tests/arrival_flock_model.py's form: slots_xz,
    slot_ring and the rest as the call leaves them), keys, axis, com, com_dest_id, members (substate, sink_valid, sink_xz);
    `parts` (the intermediate lists, for the tests' premises)."""
    pos_xz = np.asarray(pos_xz, F).reshape(-1, 2)
    n = len(mem["uid"])
    members = {"substate": np.array(mem["substate"], np.uint8), "sink_valid": np.array(mem["sink_valid"], np.uint8),
               "sink_xz": np.array(mem["sink_xz"], F).reshape(n, 2)}
    same = {"status": AB_HOST, "zone": dict(zone), "keys": np.asarray(zone["room_keys"], np.uint64), "axis": None, "com": None,
            "com_dest_id": None, "members": members, "parts": {}}
    if structural_host(m, zone, len(pos_xz), mem):
        return same
    total, ur, layer = int(zone["arg_total_members"]), F(zone["arg_unit_radius"]), int(zone["arg_layer"])
    target = (F(target[0]), F(target[1]))
    if total < 4 or not near_goal(pos_xz, mem, target):
        return dict(same, status=AB_WAIT)
    radius = afm.zone_radius(total, ur)
    area = region_area(radius)
    if len(zone["room_keys"]) < area or len(np.asarray(zone["slots_xz"]).reshape(-1, 2)) < min(total, area):
        return same
    parts = {}
    try:
        centre = closest_pathable(m, layer, *target)
        axis = approach_axis(pos_xz, mem, target)
        tiles = connected_tiles(m, layer, centre[0], centre[1], area, wrong, stats)
        flood = np.array([m.centre_of(r, c) for r, c in tiles], F).reshape(-1, 2)
        keys = np.array(sorted(key_of((r >> 6, c >> 6, r & 63, c & 63)) for r, c in tiles), np.uint64)
        spacing = F(F(1.85) * ur)
        thinned, dd, order = thin(flood, centre, axis, total, spacing, wrong)
        keyset = set(int(k) for k in keys)
        clear = np.array([segment_within(m, keyset, centre[0], centre[1], s[0], s[1]) for s in thinned], bool)
        kept = thinned if wrong == "no_clear_line" else thinned[clear]
        com = centre_of_mass(kept, wrong)
        com = closest_pathable(m, layer, *com)
        did = dest_id(m, com[0], com[1], layer)
        slots = far_near(kept, centre, axis, spacing, wrong)
    except Host:
        return same
    parts.update(tiles=tiles, flood=flood, near_keys=dd, near_order=order, thinned=thinned, clear=clear, kept=kept, area=area)
    z = dict(zone, layer=layer, centre_xz=np.array(centre, F), radius=radius, unit_radius=ur, phase=FILLING,
             slots_xz=slots, slot_ring=np.zeros(len(slots), np.int32), row_height=spacing, active_row=0, num_rows=0,
             stall_counter=0, prev_occ=0, fill_frac=F(0), realloc_counter=0)
    # ---- the tail, arrival.c:839-847
    z["num_rows"], z["slot_ring"] = afm.geodesic_rings(m, z, keys, pos_xz, mem)
    afm.realloc_slots(m, z, keys, pos_xz, mem, members)
    return {"status": 0, "zone": z, "keys": keys, "axis": np.array(axis, F), "com": np.array(com, F), "com_dest_id": did,
            "members": members, "parts": parts}


def build_zones(m, zones, pos_xz, members, targets, wrong=None):
    return [build_zone(m, z, pos_xz, mem, t, wrong) for z, mem, t in zip(zones, members, targets)]
