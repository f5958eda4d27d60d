"""A plain numpy model of the built-zone branch of G_Arrival_UpdateFlock (arrival.c:767-853 without the first build at
:796-848), written from arrival.c:257-302 (arrival_compute_geodesic_rings), :363-375 (arrival_zone_radius), :391-516
(arrival_realloc_slots) and nav.c:4389-4460 (N_RegionGeodesicDist).  Floats are np.float32 operation by operation, double
where the reference is.  tests/test_arrival_flock_cpu.py holds it against the reference's own code.

A zone is a dict: layer, centre_xz, radius, unit_radius, fill_frac, active_row, num_rows, slots_xz, slot_ring (struct
arrival_state as navhip_arrival_zone carries it), phase, realloc_counter, stall_counter, prev_occ, row_height, and the
call's arguments arg_layer, arg_unit_radius, arg_total_members.  Members: a dict of rows uid, settled, substate,
sink_valid, sink_xz in the reference's member order.

`wrong`: one of WRONG, a deliberately wrong variant of one statement -- the tests show that each changes bits.
"""
import numpy as np

from tests.arrival_velocity_model import Map, in_region, key_of      # noqa: F401  (Map: re-exported for the tests)

F = np.float32
INACTIVE, FILLING, DONE = 0, 1, 2
AF_HOST = 0x80
MAX_SLOTS = 4096
REALLOC_PERIOD = 4
STALL_REALLOCS = 80 // REALLOC_PERIOD          # ARRIVAL_ROW_STALL_TICKS / ARRIVAL_REALLOC_PERIOD
WRONG = ("centroid_all", "maxd_keys", "unreached_ring0", "le_settled", "le_sink", "freeze_le", "settled_neighbour")
ZONE_OUT = ("unit_radius", "fill_frac", "radius", "layer", "active_row", "num_rows", "phase", "realloc_counter", "stall_counter",
            "prev_occ")
MEMBER_OUT = ("substate", "sink_valid", "sink_xz")


def zone_radius(nunits, unit_radius):
    """arrival_zone_radius, arrival.c:363"""
    with np.errstate(all="ignore"):
        per_unit = F(F(F(1.85) * F(unit_radius)) / F(4))
        per_unit = F(per_unit * per_unit)
        if per_unit < F(1):
            per_unit = F(1)
        ntiles = F(F(nunits) * per_unit)
        root = np.sqrt(F(np.float64(ntiles) / np.pi))                        # sqrtf of the narrowed double
        return int(F(np.ceil(root)) + F(3)) & 0xffff


def tile_centre(m, key):
    """The tile centre of nav.c:4409-4410"""
    cr, cc, tr, tc = (key >> 48) & 0xffff, (key >> 32) & 0xffff, (key >> 16) & 0xffff, key & 0xffff
    cx = F(m.mx - F(F(F(cc * 64 + tc) + F(0.5)) * F(4)))
    cz = F(m.mz + F(F(F(cr * 64 + tr) + F(0.5)) * F(4)))
    return cx, cz


def source_key(m, keys, entry):
    """Index of the key whose tile centre is nearest the entry: strict `<` from INFINITY, the earliest of equal ones, 0
    when none wins."""
    src, best = 0, F(np.inf)
    with np.errstate(all="ignore"):
        for i, k in enumerate(keys):
            cx, cz = tile_centre(m, int(k))
            dx, dz = F(cx - entry[0]), F(cz - entry[1])
            dd = F(F(dx * dx) + F(dz * dz))
            if dd < best:
                best, src = dd, i
    return src


def flood(m, keys, src):
    """4-connected BFS distances over the sorted key set from keys[src] (nav.c:4419-4442): -1 = unreached."""
    keys = [int(k) for k in keys]
    index = {k: i for i, k in enumerate(keys)}
    dist = [-1] * len(keys)
    if not keys:
        return dist
    dist[src] = 0
    queue, head = [src], 0
    while head < len(queue):
        ci = queue[head]
        head += 1
        k = keys[ci]
        r, c = ((k >> 48) & 0xffff) * 64 + ((k >> 16) & 0xffff), ((k >> 32) & 0xffff) * 64 + (k & 0xffff)
        for dc, dr in ((-1, 0), (1, 0), (0, -1), (0, 1)):                    # deltas[] as {r, c}: {0,-1} {0,+1} {-1,0} {+1,0}
            nr, nc = r + dr, c + dc
            if nr < 0 or nr >= m.h * 64 or nc < 0 or nc >= m.w * 64:        # M_Tile_RelativeDesc
                continue
            ni = index.get(key_of((nr // 64, nc // 64, nr % 64, nc % 64)), -1)
            if ni < 0 or dist[ni] >= 0:
                continue
            dist[ni] = dist[ci] + 1
            queue.append(ni)
    return dist


def geodesic_dist(m, keys, entry, queries):
    """N_RegionGeodesicDist (nav.c:4389): (per-query distance, the largest written or -1, the key distances)."""
    out = np.full(len(queries), -1, np.int32)
    if len(keys) == 0:
        return out, -1, []
    dist = flood(m, keys, source_key(m, keys, entry))
    index = {int(k): i for i, k in enumerate(keys)}
    result = -1
    for q, (x, z) in enumerate(queries):
        t = m.tile(x, z)
        if t is None:
            continue
        idx = index.get(key_of(t), -1)
        if idx >= 0 and dist[idx] >= 0:
            out[q] = dist[idx]
            result = max(result, dist[idx])
    return out, result, dist


def entry_point(zone, pos_xz, mem, wrong=None):
    """The float sum of the unsettled members' positions in member order times 1.0f / cnt; the centre without any."""
    ex, ez, cnt = F(0), F(0), 0
    with np.errstate(all="ignore"):
        for uid, settled in zip(mem["uid"], mem["settled"]):
            if settled and wrong != "centroid_all":
                continue
            ex, ez = F(ex + pos_xz[uid][0]), F(ez + pos_xz[uid][1])
            cnt += 1
        if cnt == 0:
            return F(zone["centre_xz"][0]), F(zone["centre_xz"][1])
        inv = F(F(1) / F(cnt))
        return F(ex * inv), F(ez * inv)


def geodesic_rings(m, zone, keys, pos_xz, mem, wrong=None):
    """arrival_compute_geodesic_rings (arrival.c:257): (num_rows, slot_ring)"""
    slots = np.asarray(zone["slots_xz"], F).reshape(-1, 2)
    M = len(slots)
    if M == 0:
        return 0, np.zeros(0, np.int32)
    gdist, maxd, kdist = geodesic_dist(m, keys, entry_point(zone, pos_xz, mem, wrong), slots)
    if wrong == "maxd_keys":
        maxd = max(kdist) if len(kdist) else -1
    maxd = max(maxd, 0)
    with np.errstate(all="ignore"):
        ring_w = max(int(F(F(F(zone["row_height"]) / F(4)) + F(0.5))), 1)
    num_rows = maxd // ring_w + 1
    ring = np.zeros(M, np.int32)
    for i in range(M):
        g = gdist[i] if gdist[i] >= 0 else (maxd if wrong == "unreached_ring0" else 0)
        ring[i] = min(max((maxd - g) // ring_w, 0), num_rows - 1)
    return num_rows, ring


def _nearest(slots, x, z, allowed=None, le=False):
    """The slot of least dd among `allowed` (strict `<` from INFINITY: the earliest of equal ones); -1 = none."""
    if len(slots) == 0:
        return -1
    with np.errstate(all="ignore"):
        dx, dz = slots[:, 0] - F(x), slots[:, 1] - F(z)
        dd = dx * dx + dz * dz
        ok = dd < F(np.inf)
    if allowed is not None:
        ok &= allowed
    if not ok.any():
        return -1
    dd = np.where(ok, dd, F(np.inf))
    if le:
        return int(np.flatnonzero(dd == dd.min())[-1])
    return int(np.argmin(dd))


def realloc_slots(m, zone, keys, pos_xz, mem, out, wrong=None):
    """arrival_realloc_slots (arrival.c:391) on the zone dict (changed in place) and the member outputs `out`."""
    slots = np.asarray(zone["slots_xz"], F).reshape(-1, 2)
    M = len(slots)
    if M == 0 or zone["num_rows"] == 0:
        return
    keyset = set(int(k) for k in keys)
    fill = F(zone["fill_frac"])
    if fill < F(0.25) or (wrong == "freeze_le" and fill <= F(0.25)):
        zone["num_rows"], zone["slot_ring"] = geodesic_rings(m, zone, keys, pos_xz, mem, wrong)
        zone["active_row"] = 0
    R, ring = zone["num_rows"], np.asarray(zone["slot_ring"], np.int32)
    cap = np.bincount(ring, minlength=R)
    occupied = np.array([m.blocked(zone["layer"], s[0], s[1]) for s in slots], bool)
    for uid, settled in zip(mem["uid"], mem["settled"]):
        if not settled:
            continue
        best = _nearest(slots, pos_xz[uid][0], pos_xz[uid][1], ~occupied if wrong == "settled_neighbour" else None, wrong == "le_settled")
        if best >= 0:
            occupied[best] = True
    occ = np.bincount(ring[occupied], minlength=R)
    zone["fill_frac"] = F(F(int(occ.sum())) / F(M))
    inside = [(not s) and in_region(m, keyset, pos_xz[u][0], pos_xz[u][1]) for u, s in zip(mem["uid"], mem["settled"])]
    crowd = sum(inside)
    row = zone["active_row"]
    rising = occ[row] > zone["prev_occ"]
    advanced = False
    while row < R - 1 and F(occ[row]) >= F(1.0) * F(cap[row]):
        row += 1
        advanced = True
    if advanced or rising or crowd == 0:
        zone["stall_counter"] = 0
    else:
        zone["stall_counter"] += 1
        if zone["stall_counter"] >= STALL_REALLOCS and row < R - 1:
            row += 1
            zone["stall_counter"] = 0
    zone["active_row"] = row
    zone["prev_occ"] = int(occ[row])
    allowed = ~occupied & (ring <= row)
    for j, (uid, settled) in enumerate(zip(mem["uid"], mem["settled"])):
        if settled:
            continue
        if not inside[j]:
            out["sink_valid"][j] = 0
            continue
        if out["substate"][j] < 2:
            out["substate"][j] += 2                                          # unit_commit
        best = _nearest(slots, pos_xz[uid][0], pos_xz[uid][1], allowed, wrong == "le_sink")
        out["sink_valid"][j] = int(best >= 0)
        if best >= 0:
            out["sink_xz"][j] = slots[best]


def host_row(m, zone, keys, n_ents, mem):
    """What the device leaves to the host (NAVHIP_AF_HOST, include/navhip.h)."""
    uid = np.asarray(mem["uid"], np.int64)
    layer = int(zone["arg_layer"])
    return (zone["phase"] != FILLING or len(np.asarray(zone["slots_xz"]).reshape(-1, 2)) > MAX_SLOTS or len(keys) > MAX_SLOTS
            or layer not in m.blockers or bool(((uid < 0) | (uid >= n_ents)).any())
            or not 0 <= zone["num_rows"] <= MAX_SLOTS
            or (zone["num_rows"] > 0 and not 0 <= zone["active_row"] < zone["num_rows"]))


def update_flock(m, zone, keys, pos_xz, mem, wrong=None, decide_host=True):
    """One call for one zone: (the zone after the call -- a new dict --, the member outputs, status)."""
    pos_xz = np.asarray(pos_xz, F).reshape(-1, 2)
    z = dict(zone, slot_ring=np.array(zone["slot_ring"], np.int32))
    n = len(mem["uid"])
    out = {"substate": np.array(mem["substate"], np.uint8), "sink_valid": np.array(mem["sink_valid"], np.uint8),
           "sink_xz": np.array(mem["sink_xz"], F).reshape(n, 2)}
    if decide_host and host_row(m, zone, keys, len(pos_xz), mem):
        return z, out, AF_HOST
    if all(bool(s) for s in mem["settled"]):
        z["phase"] = DONE
        return z, out, 0
    z["layer"] = int(zone["arg_layer"])
    z["radius"] = zone_radius(int(zone["arg_total_members"]), zone["arg_unit_radius"])
    z["unit_radius"] = F(zone["arg_unit_radius"])
    z["phase"] = FILLING
    z["realloc_counter"] += 1
    if z["realloc_counter"] >= REALLOC_PERIOD:
        z["realloc_counter"] = 0
        realloc_slots(m, z, keys, pos_xz, mem, out, wrong)
    return z, out, 0


def update_flocks(m, zones, keys, pos_xz, members, wrong=None):
    """The batch: (zones after, member outputs, status [n_zones])"""
    res = [update_flock(m, z, k, pos_xz, mem, wrong) for z, k, mem in zip(zones, keys, members)]
    return [r[0] for r in res], [r[1] for r in res], np.array([r[2] for r in res], np.uint8)
