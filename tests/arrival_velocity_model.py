"""A plain Python / numpy model of G_Arrival_DesiredVelocity (arrival.c:862-944) for a unit whose zone is filling: the
control flow is written from that function alone; what it calls in the nav module is restated here -- M_Tile_DescForPoint2D
(tile.c:547), N_SegmentWithinRegion (nav.c:4326) over M_Tile_LineSupercoverTilesSorted (tile.c:430), N_PositionBlocked
(nav.c:4070), N_DesiredGroupArrivalVelocity (nav.c:3561), the cache-hit path of N_DesiredPointSeekVelocity
(n_interpolated_flow_dir, nav.c:3407) -- and tests/test_arrival_velocity_cpu.py holds every one of those ingredients
against the reference's own code.  Floats are np.float32 operation by operation, double where the reference is.

`arm` of every answer names the statement that produced it, so that a test can count the arms it covers:
    "host"  "beeline"  "nearest"  "none"  "zone"  "centre"  "com"  "com_miss"
"""
import numpy as np

F = np.float32
EPS = F(1.0 / 1024)
AV_COM_MISS, AV_HOST = 0x01, 0x80
ST_FIELD_MISS, ST_FIELD_NONE = 0x02, 0x04
FD_NONE = 0
LOS_HYST = 12
_D = F(0.70710678118654757)
# N_FlowDir (field.c:2428): NONE NW N NE W E SW S SE
FLOW = np.array([(0, 0), (_D, -_D), (0, -1), (-_D, -_D), (1, 0), (-1, 0), (_D, _D), (0, 1), (-_D, _D)], F)


class Map:
    """What the rule reads of the nav state: the map's size in chunks, the blockers plane per layer ([h][w][64][64] u16;
    a layer that is not a key has no plane) and the field tables (rows x chunks slots of `pool`, -1 = not cached)."""

    def __init__(self, w, h, blockers, region_field_slot=None, flock_field_slot=None, pool=None):
        self.w, self.h = w, h
        self.mx, self.mz = F(w * 128.0), F(-h * 128.0)
        self.blockers = {int(l): np.asarray(b).reshape(h, w, 64, 64) for l, b in blockers.items()}
        self.zone_tab = None if region_field_slot is None else np.asarray(region_field_slot, np.int32).reshape(-1, w * h)
        self.com_tab = None if flock_field_slot is None else np.asarray(flock_field_slot, np.int32).reshape(-1, w * h)
        self.pool = None if pool is None else np.asarray(pool, np.uint8).reshape(-1, 4096)

    # ---- M_Tile_DescForPoint2D: (chunk_r, chunk_c, tile_r, tile_c) or None
    def tile(self, x, z):
        x, z = F(x), F(z)
        if x > self.mx or x < self.mx - F(self.w * 256) or z < self.mz or z > self.mz + F(self.h * 256):
            return None
        if x != x or z != z:
            return None
        cr = min(max(int(abs(self.mz - z) / F(256)), 0), self.h - 1)
        cc = min(max(int(abs(self.mx - x) / F(256)), 0), self.w - 1)
        bx, bz = self.mx - F(cc * 256), self.mz + F(cr * 256)
        tr = min(max(int(abs(bz - z) / F(4)), 0), 63)
        tc = min(max(int(abs(bx - x) / F(4)), 0), 63)
        return cr, cc, tr, tc

    def blocked(self, layer, x, z):
        """N_PositionBlocked; a point off the map (the reference asserts) is not blocked."""
        t = self.tile(x, z)
        return t is not None and self.blockers[layer][t] > 0

    def bounds(self, t):
        """M_Tile_Bounds (tile.c:356): the tile's corner (x, z) of largest x and smallest z."""
        return F(F(self.mx - F(t[1] * 256)) - F(t[3] * 4)), F(F(self.mz + F(t[0] * 256)) + F(t[2] * 4))


def key_of(t):
    """td_key, nav.c:207"""
    return (t[0] << 48) | (t[1] << 32) | (t[2] << 16) | t[3]


def vlen(x, z):
    """PFM_Vec2_Len: sqrt in double of the float sum, as a float"""
    with np.errstate(all="ignore"):
        return F(np.sqrt(np.float64(F(F(x * x) + F(z * z)))))


def heading(x, z):
    """`if(PFM_Vec2_Len(&v) > EPSILON) PFM_Vec2_Normal(&v, &v)`"""
    with np.errstate(all="ignore"):
        l = vlen(x, z)
        return (F(x / l), F(z / l)) if l > EPS else (F(x), F(z))


def in_region(m, keys, x, z):
    """arrival_in_region (arrival.c:153): the walk from a point to itself is its tile"""
    t = m.tile(x, z)
    return len(keys) > 0 and t is not None and key_of(t) in keys


def near_region(m, keys, unit_radius, x, z):
    """arrival_near_region, arrival.c:158"""
    if in_region(m, keys, x, z):
        return True
    pad = max(1, int(np.ceil(F(F(unit_radius) / F(4)))))
    for dz in range(-pad, pad + 1):
        for dx in range(-pad, pad + 1):
            if (dx or dz) and in_region(m, keys, F(x + F(F(dx) * F(4))), F(z + F(F(dz) * F(4)))):
                return True
    return False


def segment_within(m, keys, ax, az, bx, bz):
    """N_SegmentWithinRegion (nav.c:4326): every tile of the supercover walk from a to b (both on the map) is a key."""
    if not len(keys):
        return False
    ta, tb = m.tile(ax, az), m.tile(bx, bz)
    if ta is None or tb is None:
        return False
    ar, ac, br, bc = ta[0] * 64 + ta[2], ta[1] * 64 + ta[3], tb[0] * 64 + tb[2], tb[1] * 64 + tb[3]
    maxout = abs(br - ar) + abs(bc - ac) + 2
    with np.errstate(all="ignore"):
        dx, dz = F(F(bx) - F(ax)), F(F(bz) - F(az))
        l = vlen(dx, dz)
        dx, dz = F(dx / l), F(dz / l)
        step_c, step_r = (1 if dx <= 0 else -1), (1 if dz >= 0 else -1)
        t_delta_x, t_delta_z = F(abs(F(F(4) / dx))), F(abs(F(F(4) / dz)))
        x0, z0 = m.bounds(ta)
        num_x = F(F(ax) - F(x0 - F(4))) if step_c > 0 else F(F(ax) - x0)
        num_z = F(F(az) - F(z0 + F(4))) if step_r > 0 else F(F(az) - z0)
        t_max_x = F(abs(np.float64(num_x)) / abs(np.float64(dx)))
        t_max_z = F(abs(np.float64(num_z)) / abs(np.float64(dz)))
        r, c = ar, ac
        for _ in range(maxout):
            if key_of((r >> 6, c >> 6, r & 63, c & 63)) not in keys:
                return False
            dc = dr = 0
            if t_max_x < t_max_z:
                t_max_x = F(t_max_x + t_delta_x)
                dc = step_c
            else:
                t_max_z = F(t_max_z + t_delta_z)
                dr = step_r
            if (r, c) == (br, bc):
                break
            r, c = r + dr, c + dc
            if r < 0 or r >= m.h * 64 or c < 0 or c >= m.w * 64:        # M_Tile_RelativeDesc
                break
    return True


def nearest_slot(m, zone, x, z, open_only):
    """arrival_nearest_slot (arrival.c:344) / arrival_nearest_open_slot (:304): index of the winner or -1; the strict `<`
    from best = INFINITY keeps the earliest of equal dd and never takes a dd that is not < INFINITY."""
    slots, ring = zone["slots_xz"], zone["slot_ring"]
    best, at = F(np.inf), -1
    with np.errstate(all="ignore"):
        for i in range(len(ring)):
            if ring[i] > zone["active_row"]:
                continue
            if open_only and m.blocked(zone["layer"], slots[i][0], slots[i][1]):
                continue
            dx, dz = F(slots[i][0] - x), F(slots[i][1] - z)
            dd = F(F(dx * dx) + F(dz * dz))
            if dd < best:
                best, at = dd, i
    return at


def zone_lookup(m, zone, row, x, z):
    """N_DesiredGroupArrivalVelocity (nav.c:3561): (returned true, velocity, at_slot)"""
    t, tc = m.tile(x, z), m.tile(zone["centre_xz"][0], zone["centre_xz"][1])
    if t is None or tc is None or row < 0 or m.zone_tab is None:
        return False, (F(0), F(0)), False
    slot = m.zone_tab[row, t[0] * m.w + t[1]]
    if slot < 0:
        return False, (F(0), F(0)), False
    d = int(m.pool[slot, t[2] * 64 + t[3]]) & 0xf
    at = False
    if d == FD_NONE:
        dr, dc = (t[0] * 64 + t[2]) - (tc[0] * 64 + tc[2]), (t[1] * 64 + t[3]) - (tc[1] * 64 + tc[3])
        at = dr * dr + dc * dc <= int(zone["radius"]) ** 2
    return True, (FLOW[d][0], FLOW[d][1]), at


def sample_flow(m, row, x, z):
    """The cache-hit path of N_DesiredPointSeekVelocity with n_interpolated_flow_dir (nav.c:3407): (velocity, status);
    status names what makes the reference leave that path (no field for the chunk, FD_NONE under the unit)."""
    t = m.tile(x, z)
    if row < 0 or m.com_tab is None or m.pool is None or t is None:
        return (F(0), F(0)), ST_FIELD_MISS
    slots = m.com_tab[row]
    slot = slots[t[0] * m.w + t[1]]
    if slot < 0:
        return (F(0), F(0)), ST_FIELD_MISS
    base = int(m.pool[slot, t[2] * 64 + t[3]]) & 0xf
    status = ST_FIELD_NONE if base == FD_NONE else 0
    bx, bz = m.bounds(t)
    cx, cz = F(bx - F(2)), F(bz + F(2))
    dx, dz = F(F(x) - cx), F(F(z) - cz)
    dc, dr = (1 if dx < 0 else -1), (1 if dz > 0 else -1)
    wc, wr = min(F(abs(dx) / F(4)), F(1)), min(F(abs(dz) / F(4)), F(1))
    sw = [F(F(F(1) - wc) * F(F(1) - wr)), F(wc * F(F(1) - wr)), F(F(F(1) - wc) * wr), F(wc * wr)]
    ax = az = wsum = F(0)
    for i, (sdc, sdr) in enumerate(((0, 0), (dc, 0), (0, dr), (dc, dr))):
        if not sw[i] > 0:
            continue
        r, c = t[0] * 64 + t[2] + sdr, t[1] * 64 + t[3] + sdc
        if r < 0 or r >= m.h * 64 or c < 0 or c >= m.w * 64:
            continue
        s = slots[(r >> 6) * m.w + (c >> 6)]
        if s < 0:
            continue
        d = int(m.pool[s, (r & 63) * 64 + (c & 63)]) & 0xf
        if d == FD_NONE:
            continue
        ax, az = F(ax + F(FLOW[d][0] * sw[i])), F(az + F(FLOW[d][1] * sw[i]))
        wsum = F(wsum + sw[i])
    if wsum < F(1e-6) or vlen(ax, az) < F(1e-6):
        return (FLOW[base][0], FLOW[base][1]), status
    l = vlen(ax, az)
    return (F(ax / l), F(az / l)), status


def desired_velocity(m, zones, keys, zone_row, com_row, pos_xz, units):
    """The rule for every row of `units` (uid, zone, has_dest_los, substate, sink_valid, sink_xz, los_latched, los_hyst);
    pos_xz: the world's positions; keys: per zone a sorted u64 array.  Returns the dict of outputs the device gives
    (vdes_xz, status, the unit state after the call) plus `arm`."""
    nq = len(units["uid"])
    keysets = [set(int(k) for k in kk) for kk in keys]
    out = {"vdes_xz": np.full((nq, 2), np.nan, F), "status": np.zeros(nq, np.uint8),
           "substate": np.array(units["substate"], np.uint8), "sink_valid": np.array(units["sink_valid"], np.uint8),
           "sink_xz": np.array(units["sink_xz"], F).reshape(nq, 2), "los_latched": np.array(units["los_latched"], np.uint8),
           "los_hyst": np.array(units["los_hyst"], np.int32), "arm": []}
    pos_xz = np.asarray(pos_xz, F).reshape(-1, 2)
    for q in range(nq):
        uid, zi, sub = int(units["uid"][q]), int(units["zone"][q]), int(units["substate"][q])
        host = not (0 <= uid < len(pos_xz)) or not (0 <= zi < len(zones)) or sub > 3
        if not host:
            Z, ks = zones[zi], keysets[zi]
            x, z = pos_xz[uid]
            host = m.tile(x, z) is None or int(Z["layer"]) not in m.blockers
        if host:
            out["status"][q] = AV_HOST
            out["arm"].append("host")
            continue
        layer = int(Z["layer"])
        if near_region(m, ks, Z["unit_radius"], x, z) and sub < 2:          # unit_commit
            sub += 2
        if sub >= 2:
            valid, sink = bool(units["sink_valid"][q]), out["sink_xz"][q].copy()
            if valid and m.blocked(layer, sink[0], sink[1]):
                k = nearest_slot(m, Z, x, z, True)
                valid = k >= 0
                if valid:
                    sink = np.array(Z["slots_xz"][k], F)
            if valid and segment_within(m, ks, x, z, sink[0], sink[1]):
                v, arm = heading(F(sink[0] - x), F(sink[1] - z)), "beeline"
            else:
                k = nearest_slot(m, Z, x, z, False)
                if k >= 0:
                    v, arm = heading(F(Z["slots_xz"][k][0] - x), F(Z["slots_xz"][k][1] - z)), "nearest"
                else:
                    v, arm = (F(0), F(0)), "none"
            out["sink_valid"][q], out["sink_xz"][q] = int(valid), sink
        else:
            ok, zvel, at_slot = zone_lookup(m, Z, int(zone_row[zi]), x, z)
            if ok and not at_slot and vlen(zvel[0], zvel[1]) > EPS:
                v, arm = zvel, "zone"
            else:
                los, latched, hyst = bool(units["has_dest_los"][q]), bool(units["los_latched"][q]), int(units["los_hyst"][q])
                if los == latched:
                    hyst = 0
                else:
                    hyst += 1
                    if hyst >= LOS_HYST:
                        latched, hyst = los, 0
                out["los_latched"][q], out["los_hyst"][q] = int(latched), hyst
                if latched:
                    v, arm = heading(F(F(Z["centre_xz"][0]) - x), F(F(Z["centre_xz"][1]) - z)), "centre"
                else:
                    v, st = sample_flow(m, int(com_row[zi]), x, z)
                    arm = "com"
                    if st:
                        v, arm = (F(np.nan), F(np.nan)), "com_miss"
                        out["status"][q] = AV_COM_MISS
        out["substate"][q] = sub
        out["vdes_xz"][q] = v
        out["arm"].append(arm)
    out["arm"] = np.array(out["arm"])
    return out
