"""A plain model of the two frontier functions behind the enemy-seek and surround fields, written from field.c and tile.c:
field_enemies_initial_frontier (field.c:1209) and field_entity_initial_frontier (:1317) with what they call --
field_chunk_bounds :863, bg_ent_inrange_rect's membership in fixed point (bitmap_grid.h:1236-1374), filter_garrisoned
(position.c:100), field_enemy_ent :963, M_Tile_AllUnderCircle (tile.c:687), M_Tile_Contour (:759), the tds[512] caps -- and the
rows navhip_build_seek_fields hands back (NAVHIP_SK_HOST).  `Rules` switches single statements to a wrong reading, so that a test
can show that its worlds tell the readings apart.  Test infrastructure only."""
import collections

import numpy as np

from tests import surround_model as sm

F = np.float32
COMBATABLE, BUILDING, GARRISONED = 1 << 4, 1 << 8, 1 << 18
SEEK_ENEMIES, SEEK_ENTITY, SK_HOST = 0, 1, 0x80
RDIM = 128
MAX_ENTS = 4096
POS_LIMIT = F(4194304.0)
NLAYERS = 12

Rules = collections.namedtuple("Rules", "union kind1_rule search_buffer fixed_point drop_garrisoned cap")
REFERENCE = Rules(union=True, kind1_rule=True, search_buffer=16.0, fixed_point=True, drop_garrisoned=True, cap=512)
WRONG = {
    "contour of the previous contour only": REFERENCE._replace(union=False),
    "kind 0's contour rule for kind 1": REFERENCE._replace(kind1_rule=False),
    "no SEARCH_BUFFER": REFERENCE._replace(search_buffer=0.0),
    "float compare": REFERENCE._replace(fixed_point=False),
    "garrisoned kept": REFERENCE._replace(drop_garrisoned=False),
    "cap 1024": REFERENCE._replace(cap=1024),
}


def bg_scale(v):
    """BG_SCALE_F: lrintf(v * 256.0f), round to nearest even."""
    return int(np.rint(F(F(v) * F(256.0))))


def contours(kind, layer, rules=REFERENCE):
    first = (layer >= 1) if (kind == SEEK_ENEMIES or not rules.kind1_rule) else (layer == 1)
    return int(first) + int(layer >= 2) + int(layer >= 3)


def base_of(chunk_r, chunk_c):
    """region.base and (roff, coff), field.c:1567-1572, :1596-1597."""
    return ((chunk_r - 1) * 64 + 32 if chunk_r > 0 else 0, (chunk_c - 1) * 64 + 32 if chunk_c > 0 else 0,
            32 if chunk_r > 0 else 0, 32 if chunk_c > 0 else 0)


def rect_of(w, h, chunk_r, chunk_c, rules=REFERENCE):
    """(min x, max x, min z, max z) of the query, in float as field.c:1222-1243 computes them."""
    mx, mz = sm.map_pos(w, h)
    x_max = F(mx + F(-(chunk_c * 256))); x_min = F(x_max - F(256))
    z_min = F(mz + F(chunk_r * 256));    z_max = F(z_min + F(256))
    xlen, zlen, sb = F(x_max - x_min), F(z_max - z_min), F(rules.search_buffer)
    return (F(F(x_min - F(xlen / F(2))) - sb), F(F(x_max + F(xlen / F(2))) + sb),
            F(F(z_min - F(zlen / F(2))) - sb), F(F(z_max + F(zlen / F(2))) + sb))


def members(w, h, pos, rect, rules=REFERENCE):
    """bool [n]: bg_ent_inrange_rect over a grid with the map's bounds (garrisoned entities still in)."""
    pos = np.asarray(pos, F).reshape(-1, 2)
    if len(pos) == 0:
        return np.zeros(0, bool)
    mnx, mxx, mny, mxy = rect
    if not rules.fixed_point:
        return (pos[:, 0] >= mnx) & (pos[:, 0] <= mxx) & (pos[:, 1] >= mny) & (pos[:, 1] <= mxy)
    ix = np.rint(pos[:, 0] * F(256)).astype(np.int64)
    iy = np.rint(pos[:, 1] * F(256)).astype(np.int64)
    imnx, imxx, imny, imxy = (bg_scale(v) for v in rect)
    # _bg_cell_extent: the grid of G_Pos_Init (position.c:276-283) is the map, centred on the origin
    ox, oy = bg_scale(-w * 128.0), bg_scale(-h * 128.0)
    gw, gh = (bg_scale(w * 128.0) - ox + 4095) >> 12, (bg_scale(h * 128.0) - oy + 4095) >> 12
    if imxx < ox or imxy < oy or imnx >= ox + (gw << 12) or imny >= oy + (gh << 12):
        return np.zeros(len(pos), bool)
    return (ix >= imnx) & (ix <= imxx) & (iy >= imny) & (iy <= imxy)


def contour(tiles, marked, w, h, room):
    """M_Tile_Contour of `marked` (bounding box of `tiles`... the reference passes the same list for both), row-major, at
    most `room` entries."""
    if not tiles or room <= 0:
        return []
    rs, cs = [t[0] for t in tiles], [t[1] for t in tiles]
    out = []
    for r in range(min(rs) - 1, max(rs) + 2):
        for c in range(min(cs) - 1, max(cs) + 2):
            if r < 0 or r >= h * 64 or c < 0 or c >= w * 64 or (r, c) in marked:
                continue
            if len(out) == room:
                return out
            if any((r + dr, c + dc) in marked for dr in (-1, 0, 1) for dc in (-1, 0, 1) if dr or dc):
                out.append((r, c))
    return out


_cache = {}


def circle_tiles(w, h, x, z, radius, ncont, rules=REFERENCE):
    """(tiles in the order of tds[], counts after the first call and after every contour) of one entity."""
    key = (w, h, float(x), float(z), float(radius), ncont, rules.union, rules.cap)
    if key in _cache:
        return _cache[key]
    cen = sm.tile_for_point(w, h, x, z)
    tds, counts = [], []
    if cen is not None:
        nt = int(np.ceil(float(F(radius) / F(4))))
        for dr in range(-nt, nt + 1):
            for dc in range(-nt, nt + 1):
                r, c = cen[0] + dr, cen[1] + dc
                if len(tds) == rules.cap or r < 0 or r >= h * 64 or c < 0 or c >= w * 64:
                    continue
                if sm.circle_hits_tile(w, h, x, z, radius, r, c):
                    tds.append((r, c))
    counts.append(len(tds))
    prev = list(tds)
    for _ in range(ncont):
        src = tds if rules.union else prev
        prev = contour(src, set(src), w, h, rules.cap - len(tds))
        if not rules.union:
            prev = [t for t in prev if t not in set(tds)]
        tds = tds + prev
        counts.append(len(tds))
    _cache[key] = (tds, counts)
    return _cache[key]


def window_fits(radius, ncont):
    """The 64 x 64 window holds ceil(radius / 4) + contours <= 31; a NaN radius does not fit."""
    q = F(radius) / F(4)
    if not (q <= 31):
        return False
    return (-1 if q < -1 else int(np.ceil(float(q)))) + ncont <= 31


def plain(p):
    return bool(abs(F(p[0])) < POS_LIMIT and abs(F(p[1])) < POS_LIMIT)


def seeds_of(world, req, rules=REFERENCE):
    """(status, bits [128, 128] bool) of one request of a world (tests/seek_worlds.py)."""
    w, h = world["w"], world["h"]
    pos, radius, flags, faction = world["pos"], world["radius"], world["flags"], world["faction"]
    exclude, masks, n = world["exclude"], world["enemy_mask"], len(world["pos"])
    kind, layer, cr, cc = int(req["kind"]), int(req["layer"]), int(req["chunk_r"]), int(req["chunk_c"])
    bits = np.zeros((RDIM, RDIM), bool)
    if kind > 1 or layer >= NLAYERS or not (world["layers"] >> layer) & 1 or w < 2 or h < 2 or not (0 <= cr < h and 0 <= cc < w):
        return SK_HOST, bits
    br, bc, _, _ = base_of(cr, cc)
    ncont = contours(kind, layer, rules)
    if kind == SEEK_ENTITY:
        t = int(req["target_uid"])
        if not 0 <= t < n or flags[t] & BUILDING or not plain(pos[t]) or not window_fits(radius[t], ncont):
            return SK_HOST, bits
        sources = [t]
    else:
        fid = int(req["faction_id"])
        if not 0 <= fid <= 15:
            return SK_HOST, bits
        ok = np.array([plain(p) for p in pos], bool) if n else np.zeros(0, bool)
        inside = np.zeros(n, bool)
        inside[ok] = members(w, h, pos[ok], rect_of(w, h, cr, cc, rules), rules)
        if inside.sum() > MAX_ENTS:
            return SK_HOST, bits
        sources = []
        for e in np.flatnonzero(inside | ~ok):
            if (rules.drop_garrisoned and flags[e] & GARRISONED) or faction[e] == fid or not flags[e] & COMBATABLE:
                continue
            if not 0 <= faction[e] <= 15 or not (masks[fid] >> int(faction[e])) & 1 or (exclude is not None and exclude[e]):
                continue
            if not ok[e] or flags[e] & BUILDING or not window_fits(radius[e], ncont):
                return SK_HOST, bits
            sources.append(int(e))
    for e in sources:
        for r, c in circle_tiles(w, h, pos[e][0], pos[e][1], radius[e], ncont, rules)[0]:
            if 0 <= r - br < RDIM and 0 <= c - bc < RDIM:
                bits[r - br, c - bc] = True
    return 0, bits


def pack_bits(bits):
    """[128, 128] bool -> the 2 048 bytes of an out_seed_bits row (bit r * 128 + c)."""
    return np.packbits(bits.reshape(-1), bitorder="little")


def region_req(req, n_seeds_before, n_seeds):
    """The navhip_region_req of a decided request, as N_HIP_RegionRequest fills it (a dict of its members)."""
    br, bc, roff, coff = base_of(int(req["chunk_r"]), int(req["chunk_c"]))
    return dict(layer=int(req["layer"]), out_mode=1, enemies=0, base_abs_r=br, base_abs_c=bc, rdim=RDIM, cdim=RDIM, roff=roff,
                coff=coff, seed_begin=n_seeds_before, seed_count=n_seeds, overlay_begin=0, overlay_count=0)
