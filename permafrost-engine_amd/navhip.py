"""Host-side mirror of the reference's navigation interface over the C ABI of libnavhip.so.

The product boundary is the C ABI (include/navhip.h); this module only loads it with ctypes
and gives the entry points the names / argument meaning of the reference functions they stand
in for (N_FlowFieldInit / N_FlowFieldUpdate / N_FlowFieldID, field.c:2020,2030,1952; the
packed plane uploads of nav.c:2408-2490), so parity tests read like calls into the reference.
PyTorch is used for device buffers / streams only (see `dev_ptr`).

There is NO CPU fallback: if libnavhip.so is missing or no GPU is visible, calls raise.

Read top to bottom: (1) the ABI mirror -- constants, records, signatures; (2) RECORDS, the C type name of every
record; (3) the loader; (4) the packing helpers and the module-level entry points; (5) NavContext, LosChain, Tick.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NAVHIP_LIB: load another build of the same library (A/B runs of kernel variants, scripts/ab_lib.py)
LIB_PATH = os.environ.get("NAVHIP_LIB") or os.path.join(_HERE, "libnavhip.so")

# ---------------------------------------------------------------------------------------------
# 1. the ABI mirror: constants
# ---------------------------------------------------------------------------------------------
OK = 0
ERR_INVALID, ERR_DEVICE, ERR_NOMEM, ERR_NOT_UPLOADED = -1, -2, -3, -4        # NAVHIP_ERR_*
ERR_ARG = ERR_INVALID
FIELD_RES = 64
FIELD_CELLS = 4096
COST_IMPASSABLE = 0xFF
ISLAND_NONE = 0xFFFF
FACTION_ID_NONE = 0xF
TARGET_PORTAL, TARGET_TILE, TARGET_NEAREST_PATHABLE = 0, 1, 2
PLANE_COST_BASE, PLANE_BLOCKERS, PLANE_LOCAL_ISLANDS, PLANE_FACTIONS, PLANE_ISLANDS = 0, 1, 2, 3, 4
REQ_INOUT, REQ_IF_CHANGED, REQ_LIVE_IIDS, REQ_ISLAND_NEAREST = 0x1, 0x2, 0x4, 0x8
FD_NONE, FD_NW, FD_N, FD_NE, FD_W, FD_E, FD_SW, FD_S, FD_SE = range(9)
FFID_ENEMIES, FFID_ENTITY, FFID_ZONE = 2, 4, 5
COMM_ID_BYTES = 128
POOL_RESIDENT = -1
ARRIVAL_PHASE_INACTIVE, ARRIVAL_PHASE_FILLING, ARRIVAL_PHASE_DONE = 0, 1, 2
ARRIVAL_MAX_SLOTS = 4096
AF_HOST = 0x80
LOS_REFRESH_DOWNSTREAM = 1

# per-agent movement step
STATE_MOVING, STATE_MOVING_IN_FORMATION, STATE_ARRIVED, STATE_SEEK_ENEMIES, STATE_WAITING, \
    STATE_SURROUND_ENTITY, STATE_ENTER_ENTITY_RANGE, STATE_TURNING, STATE_ARRIVING_TO_CELL = range(9)
ENTITY_FLAG_MOVABLE = 1 << 3
ENTITY_FLAG_WATER = 1 << 14
ENTITY_FLAG_AIR = 1 << 15
ENTITY_FLAG_GARRISONED = 1 << 18
ENTITY_FLAG_COMBAT_HELD = 1 << 21
ST_MOVED, ST_FIELD_MISS, ST_FIELD_NONE, ST_LOS_MISS, ST_UNSUPPORTED = 0x01, 0x02, 0x04, 0x08, 0x80
LOS_LOOKUP = 0xFF
PREFETCH_FRONT_INLINE, PREFETCH_SNAPSHOT_HELD, PREFETCH_FOLLOWS_STEP = 1, 2, 4
STAGE_NEIGHBOURS, STAGE_LISTS, STAGE_START, STAGE_END = 0, 1, 2, 3
STEP_PHASES = ("sp_build", "agent_nbr", "cohesion", "coh_regroup", "agent_finish")

# the state pass
SU_SET_STATE, SU_BLOCK, SU_HOST = 0x01, 0x02, 0x80
GATE_TURN, GATE_HOST = 0x01, 0x80
SU_SET_MOVING, SU_TARGET_DIR, SU_SET_DEST, SU_SURROUND_DEST, SU_SURROUND_PREV = 0x04, 0x08, 0x10, 0x20, 0x40
SQ_ADJACENT, SQ_HAS_DEST_0, SQ_HAS_DEST_1, SQ_HOST = 0x01, 0x02, 0x04, 0x80
FS_MEMBER, FS_READY, FS_ASSIGNED, FS_IN_RANGE, FS_ARRIVED = 0x01, 0x02, 0x04, 0x08, 0x10
DQ_NEAREST, DQ_TILES, DQ_HOST = 0x1, 0x2, 0x80
DQ_MAX_TILES = 256                                                           # per query: FIELD_RES_R * 2 + FIELD_RES_C * 2
OQ_IN_RANGE, OQ_REACHABLE = 0x1, 0x2                                         # navhip_order_query.flags
OQ_SAME_ISLAND, OQ_NO_TILE, OQ_HOST = 0x01, 0x02, 0x80                       # out_status of the order queries
RR_HOST = 0x80                                                               # out_status of the region-field repair
SEEK_ENEMIES, SEEK_ENTITY, SK_HOST = 0, 1, 0x80                              # navhip_seek_req.kind; out_status of the seek fields
ENTITY_FLAG_COMBATABLE, ENTITY_FLAG_BUILDING, ENTITY_FLAG_GARRISONED = 1 << 4, 1 << 8, 1 << 18   # entity.h, as the seed pass reads them
FACTION_NONE = 15                                                            # FACTION_ID_NONE: a dest id without a faction

# the whole tick behind one call
TICK_SERIAL, TICK_TIME_FIELDS, TICK_OWNS_SNAPSHOT = 0x2, 0x8, 0x10

# ---------------------------------------------------------------------------------------------
# 1. the ABI mirror: records (arrays of them cross the boundary as numpy dtypes, single ones as ctypes structures)
# ---------------------------------------------------------------------------------------------
# navhip_field_req, include/navhip.h (32 bytes)
FIELD_REQ_DTYPE = np.dtype([
    ("layer", np.uint8), ("type", np.uint8), ("faction_id", np.uint8), ("flags", np.uint8),
    ("enemies", np.uint16), ("chunk_r", np.uint16), ("chunk_c", np.uint16),
    ("tile_r", np.uint8), ("tile_c", np.uint8),
    ("port_r0", np.uint8), ("port_c0", np.uint8), ("port_r1", np.uint8), ("port_c1", np.uint8),
    ("next_r0", np.uint8), ("next_c0", np.uint8), ("next_r1", np.uint8), ("next_c1", np.uint8),
    ("next_chunk_r", np.uint16), ("next_chunk_c", np.uint16),
    ("port_iid", np.uint16), ("next_iid", np.uint16), ("aux_iid", np.uint16), ("_pad", np.uint16),
], align=False)
assert FIELD_REQ_DTYPE.itemsize == 32

# navhip_circle, include/navhip.h (24 bytes)
CIRCLE_DTYPE = np.dtype([("x", np.float32), ("z", np.float32), ("radius", np.float32),
                         ("faction_id", np.int32), ("flags", np.uint32), ("delta", np.int32)])
assert CIRCLE_DTYPE.itemsize == 24

# navhip_los_req, include/navhip.h (16 bytes)
LOS_REQ_DTYPE = np.dtype([("layer", np.uint8), ("faction_id", np.uint8), ("enemies", np.uint16),
                          ("chunk_r", np.uint16), ("chunk_c", np.uint16),
                          ("target_chunk_r", np.uint16), ("target_chunk_c", np.uint16),
                          ("target_tile_r", np.uint8), ("target_tile_c", np.uint8),
                          ("prev_dr", np.int8), ("prev_dc", np.int8)])
assert LOS_REQ_DTYPE.itemsize == 16

# navhip_region_req, include/navhip.h (32 bytes)
REGION_REQ_DTYPE = np.dtype([("layer", np.uint8), ("out_mode", np.uint8), ("enemies", np.uint16),
                             ("base_abs_r", np.int16), ("base_abs_c", np.int16),
                             ("rdim", np.uint16), ("cdim", np.uint16), ("roff", np.uint16),
                             ("coff", np.uint16), ("seed_begin", np.uint32), ("seed_count", np.uint32),
                             ("overlay_begin", np.uint32), ("overlay_count", np.uint32)])
assert REGION_REQ_DTYPE.itemsize == 32

# navhip_region_repair_req, include/navhip.h (20 bytes)
REGION_REPAIR_REQ_DTYPE = np.dtype([("layer", np.uint8), ("reserved", np.uint8), ("dim", np.uint16),
                                    ("centre_abs_r", np.int16), ("centre_abs_c", np.int16),
                                    ("start_abs_r", np.int16), ("start_abs_c", np.int16),
                                    ("overlay_begin", np.uint32), ("overlay_count", np.uint32)])
assert REGION_REPAIR_REQ_DTYPE.itemsize == 20

# navhip_seek_req, include/navhip.h (12 bytes)
SEEK_REQ_DTYPE = np.dtype([("kind", np.uint8), ("layer", np.uint8), ("chunk_r", np.int16), ("chunk_c", np.int16),
                           ("faction_id", np.int16), ("target_uid", np.int32)])
assert SEEK_REQ_DTYPE.itemsize == 12

# navhip_dest_query, include/navhip.h (16 bytes)
DEST_QUERY_DTYPE = np.dtype([("x", np.float32), ("z", np.float32), ("layer", np.int32), ("flags", np.uint32)])
assert DEST_QUERY_DTYPE.itemsize == 16

# navhip_order_query, include/navhip.h (32 bytes)
ORDER_QUERY_DTYPE = np.dtype([("src_x", np.float32), ("src_z", np.float32), ("dst_x", np.float32), ("dst_z", np.float32),
                              ("range", np.float32), ("layer", np.int32), ("faction", np.int32), ("flags", np.uint32)])
assert ORDER_QUERY_DTYPE.itemsize == 32


class World(C.Structure):
    """navhip_world, include/navhip.h"""
    _fields_ = [
        ("n_ents", C.c_int32), ("n_flocks", C.c_int32), ("hz", C.c_int32),
        ("n_field_slots", C.c_int32),
        ("pos_xz", C.c_void_p), ("vel_xz", C.c_void_p), ("radius", C.c_void_p),
        ("max_speed", C.c_void_p), ("speed", C.c_void_p), ("flags", C.c_void_p),
        ("state", C.c_void_p), ("has_dest_los", C.c_void_p), ("flock", C.c_void_p),
        ("vdes_xz", C.c_void_p), ("flock_target_xz", C.c_void_p), ("flock_offsets", C.c_void_p),
        ("flock_members", C.c_void_p), ("flock_field_slot", C.c_void_p), ("field_pool", C.c_void_p),
        ("map_pos_x", C.c_float), ("map_pos_z", C.c_float),
        ("grid_xmin", C.c_float), ("grid_xmax", C.c_float), ("grid_zmin", C.c_float),
        ("grid_zmax", C.c_float), ("work_begin", C.c_int32), ("work_end", C.c_int32),
        ("form_ready", C.c_void_p), ("cell_pos_xz", C.c_void_p), ("form_cohesion_xz", C.c_void_p),
        ("form_align_xz", C.c_void_p), ("form_drag_xz", C.c_void_p),
        ("arrival_sink_xz", C.c_void_p), ("arrival_flags", C.c_void_p),
        ("los_pool", C.c_void_p), ("flock_los_slot", C.c_void_p), ("los_pos_xz", C.c_void_p),
        ("n_los_slots", C.c_int32), ("static_epoch", C.c_uint32),
        ("region_row", C.c_void_p), ("region_field_slot", C.c_void_p), ("n_region_rows", C.c_int32)]


class SeekGame(C.Structure):
    """navhip_seek_game, include/navhip.h"""
    _fields_ = [("faction", C.c_void_p), ("exclude", C.c_void_p), ("enemy_mask", C.c_uint16 * 16)]


class StepOut(C.Structure):
    """navhip_step_out, include/navhip.h"""
    _fields_ = [("vel_xz", C.c_void_p), ("new_pos_xz", C.c_void_p), ("vdes_xz", C.c_void_p),
                ("vpref_xz", C.c_void_p), ("status", C.c_void_p)]


class StateIn(C.Structure):
    """navhip_state_in, include/navhip.h"""
    _fields_ = [("new_pos_xz", C.c_void_p), ("vdes_xz", C.c_void_p), ("skip", C.c_void_p),
                ("flock_layer", C.c_void_p), ("flock_nearest_xz", C.c_void_p), ("flock_tiles_off", C.c_void_p),
                ("flock_tiles", C.c_void_p)]


class StateAuxIn(C.Structure):
    """navhip_state_aux_in, include/navhip.h"""
    _fields_ = [("fstate", C.c_void_p), ("wait_ticks_left", C.c_void_p), ("wait_prev", C.c_void_p), ("new_pos_xz", C.c_void_p),
                ("ent_rot", C.c_void_p), ("target_dir", C.c_void_p), ("range_target", C.c_void_p), ("target_range", C.c_void_p),
                ("target_prev_xz", C.c_void_p), ("range_tiles_row", C.c_void_p), ("range_tiles_off", C.c_void_p),
                ("range_tiles", C.c_void_p), ("n_range_rows", C.c_int32),
                ("surround_target", C.c_void_p), ("surround_query", C.c_void_p), ("surround_target_prev_xz", C.c_void_p),
                ("surround_nearest_prev_xz", C.c_void_p), ("surround_dest_xz", C.c_void_p), ("vdes_xz", C.c_void_p),
                ("out_surround_dest_xz", C.c_void_p), ("sparse_units", C.c_void_p), ("n_sparse", C.c_int32)]


class GateIn(C.Structure):
    """navhip_gate_in, include/navhip.h"""
    _fields_ = [("next_rot", C.c_void_p), ("new_vel_xz", C.c_void_p), ("vdes_xz", C.c_void_p),
                ("interp_from_xz", C.c_void_p), ("interp_step", C.c_void_p)]


class StatePassIn(C.Structure):
    """navhip_state_pass_in, include/navhip.h"""
    _fields_ = [("gate", GateIn), ("state", StateIn), ("aux", StateAuxIn)]


class StatePassOut(C.Structure):
    """navhip_state_pass_out, include/navhip.h"""
    _fields_ = [("state", C.c_void_p), ("flags", C.c_void_p), ("gate", C.c_void_p), ("new_pos_xz", C.c_void_p),
                ("vel_xz", C.c_void_p), ("wait_ticks_left", C.c_void_p)]


class ArrivalZone(C.Structure):
    """navhip_arrival_zone, include/navhip.h"""
    _fields_ = [("centre_x", C.c_float), ("centre_z", C.c_float), ("unit_radius", C.c_float), ("fill_frac", C.c_float),
                ("radius", C.c_int32), ("layer", C.c_int32), ("active_row", C.c_int32), ("num_rows", C.c_int32),
                ("slot_begin", C.c_int32), ("slot_end", C.c_int32), ("key_begin", C.c_int32), ("key_end", C.c_int32)]


class SettleIn(C.Structure):
    """navhip_settle_in, include/navhip.h"""
    _fields_ = [("n_zones", C.c_int32), ("nq", C.c_int32), ("zones", C.c_void_p), ("slots_xz", C.c_void_p),
                ("slot_ring", C.c_void_p), ("region_keys", C.c_void_p), ("uid", C.c_void_p), ("zone", C.c_void_p),
                ("new_pos_xz", C.c_void_p), ("nsettled", C.c_void_p), ("substate", C.c_void_p),
                ("sink_valid", C.c_void_p), ("sink_xz", C.c_void_p), ("order_pos_xz", C.c_void_p),
                ("progress_anchor_xz", C.c_void_p), ("progress_anchored", C.c_void_p), ("stuck", C.c_void_p)]


class SettleOut(C.Structure):
    """navhip_settle_out, include/navhip.h"""
    _fields_ = [("settle", C.c_void_p), ("substate", C.c_void_p), ("progress_anchor_xz", C.c_void_p),
                ("progress_anchored", C.c_void_p), ("stuck", C.c_void_p), ("nsettled", C.c_void_p)]


class ArrivalVelIn(C.Structure):
    """navhip_arrival_vel_in, include/navhip.h"""
    _fields_ = [("n_zones", C.c_int32), ("nq", C.c_int32), ("n_slots", C.c_int32), ("n_keys", C.c_int32),
                ("zones", C.c_void_p), ("slots_xz", C.c_void_p), ("slot_ring", C.c_void_p), ("region_keys", C.c_void_p),
                ("zone_row", C.c_void_p), ("com_row", C.c_void_p), ("uid", C.c_void_p), ("zone", C.c_void_p),
                ("has_dest_los", C.c_void_p), ("substate", C.c_void_p), ("sink_valid", C.c_void_p), ("sink_xz", C.c_void_p),
                ("los_latched", C.c_void_p), ("los_hyst", C.c_void_p)]


class ArrivalVelOut(C.Structure):
    """navhip_arrival_vel_out, include/navhip.h"""
    _fields_ = [("vdes_xz", C.c_void_p), ("status", C.c_void_p), ("substate", C.c_void_p), ("sink_valid", C.c_void_p),
                ("sink_xz", C.c_void_p), ("los_latched", C.c_void_p), ("los_hyst", C.c_void_p), ("dense_vdes_xz", C.c_void_p)]


class ArrivalFlock(C.Structure):
    """navhip_arrival_flock, include/navhip.h"""
    _fields_ = [("phase", C.c_int32), ("realloc_counter", C.c_int32), ("stall_counter", C.c_int32), ("prev_occ", C.c_int32),
                ("row_height", C.c_float), ("unit_radius", C.c_float), ("total_members", C.c_int32), ("layer", C.c_int32),
                ("member_begin", C.c_int32), ("member_end", C.c_int32)]


class ArrivalFlockIn(C.Structure):
    """navhip_arrival_flock_in, include/navhip.h"""
    _fields_ = [("n_zones", C.c_int32), ("nm", C.c_int32), ("n_slots", C.c_int32), ("n_keys", C.c_int32),
                ("zones", C.c_void_p), ("flocks", C.c_void_p), ("slots_xz", C.c_void_p), ("slot_ring", C.c_void_p),
                ("region_keys", C.c_void_p), ("uid", C.c_void_p), ("settled", C.c_void_p), ("substate", C.c_void_p),
                ("sink_valid", C.c_void_p), ("sink_xz", C.c_void_p)]


class ArrivalFlockOut(C.Structure):
    """navhip_arrival_flock_out, include/navhip.h"""
    _fields_ = [("zones", C.c_void_p), ("flocks", C.c_void_p), ("slot_ring", C.c_void_p), ("substate", C.c_void_p),
                ("sink_valid", C.c_void_p), ("sink_xz", C.c_void_p), ("status", C.c_void_p)]


class ArrivalBuildIn(C.Structure):
    """navhip_arrival_build_in, include/navhip.h"""
    _fields_ = [("n_zones", C.c_int32), ("nm", C.c_int32), ("n_slots", C.c_int32), ("n_keys", C.c_int32),
                ("zones", C.c_void_p), ("flocks", C.c_void_p), ("target_xz", C.c_void_p), ("slots_xz", C.c_void_p),
                ("slot_ring", C.c_void_p), ("region_keys", C.c_void_p), ("uid", C.c_void_p), ("settled", C.c_void_p),
                ("substate", C.c_void_p), ("sink_valid", C.c_void_p), ("sink_xz", C.c_void_p)]


class ArrivalBuildOut(C.Structure):
    """navhip_arrival_build_out, include/navhip.h"""
    _fields_ = [("zones", C.c_void_p), ("flocks", C.c_void_p), ("slots_xz", C.c_void_p), ("slot_ring", C.c_void_p),
                ("region_keys", C.c_void_p), ("axis_xz", C.c_void_p), ("com_xz", C.c_void_p), ("com_dest_id", C.c_void_p),
                ("substate", C.c_void_p), ("sink_valid", C.c_void_p), ("sink_xz", C.c_void_p), ("status", C.c_void_p)]


class LosChainStats(C.Structure):
    """navhip_los_chain_stats, include/navhip.h"""
    _fields_ = [("slots", C.c_int32), ("levels", C.c_int32), ("stale", C.c_int32), ("rebuilt", C.c_int32),
                ("redone", C.c_int32)]


class TickDesc(C.Structure):
    """navhip_tick_desc, include/navhip.h"""
    _fields_ = [("world", World), ("pos_xz_1", C.c_void_p), ("vel_xz_1", C.c_void_p), ("status", C.c_void_p),
                ("vdes_xz", C.c_void_p), ("vpref_xz", C.c_void_p), ("dev_reqs", C.c_void_p), ("n_reqs", C.c_int32),
                ("req_slot0", C.c_int32), ("field_pool_1", C.c_void_p), ("field_cus", C.c_int32),
                ("fields_stage", C.c_int32), ("dev_moves", C.c_void_p), ("n_moves", C.c_int32),
                ("n_move_ticks", C.c_int32), ("move_tick0", C.c_int32), ("bounds", C.c_void_p), ("stream", C.c_void_p),
                ("field_stream", C.c_void_p), ("comm_stream", C.c_void_p), ("flags", C.c_uint32)]


class TickInfo(C.Structure):
    """navhip_tick_info, include/navhip.h"""
    _fields_ = [("ticks", C.c_int64),
                ("host_enqueue_ms", C.c_double), ("stream", C.c_void_p), ("field_stream", C.c_void_p),
                ("comm_stream", C.c_void_p), ("fields_ms", C.c_double), ("fields_samples", C.c_int32), ("_pad", C.c_int32)]


# the members of navhip_counters (uint64_t each), in order
COUNTER_NAMES = ("field_calls", "chunk_fields", "step_calls", "agent_steps", "los_fields", "region_fields",
                 "blocker_circles")

# the array members of navhip_world with their element types: what make_world packs
_WORLD_ARRAYS = (
    ("pos_xz", np.float32), ("vel_xz", np.float32), ("radius", np.float32),
    ("max_speed", np.float32), ("speed", np.float32), ("flags", np.uint32), ("state", np.uint8),
    ("has_dest_los", np.uint8), ("flock", np.int32), ("vdes_xz", np.float32),
    ("flock_target_xz", np.float32), ("flock_offsets", np.int32), ("flock_members", np.int32),
    ("flock_field_slot", np.int32), ("field_pool", np.uint8), ("form_ready", np.uint8),
    ("cell_pos_xz", np.float32), ("form_cohesion_xz", np.float32), ("form_align_xz", np.float32),
    ("form_drag_xz", np.float32), ("arrival_sink_xz", np.float32), ("arrival_flags", np.uint8),
    ("los_pool", np.uint8), ("flock_los_slot", np.int32), ("los_pos_xz", np.float32),
    ("region_row", np.int32), ("region_field_slot", np.int32))

# ---------------------------------------------------------------------------------------------
# 1. the ABI mirror: signatures (restype, argtypes) of every entry point include/navhip.h declares, by the unit of
# csrc/ that defines it; checked by the CPU test-suite against the header and the library's exports
# ---------------------------------------------------------------------------------------------
_P, _I, _F, _Z, _U32, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_uint32, C.c_uint64
_WORLD = C.POINTER(World)
_SIGS = {
    # navhip_api: the context, the planes, the blockers, the field builds
    "navhip_ctx_create": (_I, [C.POINTER(_P), _I, _I, _I]),
    "navhip_ctx_destroy": (None, [_P]),
    "navhip_last_error": (C.c_char_p, [_P]),
    "navhip_device": (_I, [_P]),
    "navhip_stream": (_P, [_P]),
    "navhip_sync": (_I, [_P]),
    "navhip_get_counters": (_I, [_P, _P, _I]),
    "navhip_upload_plane": (_I, [_P, _I, _I, _P, _Z]),
    "navhip_upload_chunk": (_I, [_P, _I, _I, _I, _I, _P, _Z]),
    "navhip_plane_dev": (_P, [_P, _I, _I]),
    "navhip_download_plane": (_I, [_P, _I, _I, _P, _Z]),
    "navhip_blockers_circles": (_I, [_P, _P, _I, _F, _F]),
    "navhip_blockers_circles_dev": (_I, [_P, _P, _I, _F, _F, _P]),
    "navhip_relabel_local_islands": (_I, [_P, _I]),
    "navhip_changed_chunks": (_I, [_P, _I, _P, _I]),
    "navhip_faction_changed_chunks": (_I, [_P, _I, _P, _I]),
    "navhip_clear_changed": (_I, [_P, _P]),
    "navhip_build_region_fields": (_I, [_P, _P, _I, _P, _Z, _P, _Z, _P, _Z]),
    "navhip_build_region_fields_dev": (_I, [_P, _P, _I, _I, _P, _P, _P, _Z, _P]),
    "navhip_build_los": (_I, [_P, _P, _I, _P, _P, _F, _F]),
    "navhip_build_los_dev": (_I, [_P, _P, _I, _P, _P, _F, _F, _P]),
    "navhip_build_fields": (_I, [_P, _P, _I, _P, _P]),
    "navhip_build_fields_dev": (_I, [_P, _P, _I, _P, _P, _P]),
    "navhip_flow_field_id": (_U64, [_P]),
    "navhip_region_field_id": (_U64, [_I, _I, _I, _I, _U32, _I, _I]),
    "navhip_set_field_kernel": (_I, [_P, _I]),
    "navhip_last_fields_split": (_I, [_P, C.POINTER(C.c_int32 * 2)]),
    # step_api: the agent step and the host-pointer utilities over its kernels
    "navhip_agent_step": (_I, [_P, _WORLD, C.POINTER(StepOut)]),
    "navhip_agent_step_dev": (_I, [_P, _WORLD, C.POINTER(StepOut), _P]),
    "navhip_agent_prefetch_dev": (_I, [_P, _WORLD, _P]),
    "navhip_agent_prefetch_dev_ex": (_I, [_P, _WORLD, _P, _U32]),
    "navhip_stream_wait_stage": (_I, [_P, _P, _I]),
    "navhip_set_profiling": (_I, [_P, _I]),
    "navhip_last_step_ms": (_I, [_P, C.POINTER(_F * 5)]),
    "navhip_last_step_lists": (_I, [_P, C.POINTER(C.c_int32 * 6)]),
    "navhip_step_lists_peek": (_I, [_P, C.POINTER(C.c_int32 * 6)]),
    "navhip_debug_cp_attempts": (_I, [_P, _I]),
    "navhip_spatial_query": (_I, [_P, _WORLD, _P, _I, _F, _I, _P, _P]),
    "navhip_region_lookup": (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _F, _F, _P, _P]),
    "navhip_clearpath": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "navhip_clearpath_rows": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "navhip_clearpath_team": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P]),
    # state_kernels: the state half of the tick
    "navhip_heading_gate": (_I, [_P, _WORLD, C.POINTER(GateIn), _P, _P, _P]),
    "navhip_heading_gate_dev": (_I, [_P, _WORLD, C.POINTER(GateIn), _P, _P, _P, _P]),
    "navhip_state_update": (_I, [_P, _WORLD, C.POINTER(StateIn), _P, _P]),
    "navhip_state_update_dev": (_I, [_P, _WORLD, C.POINTER(StateIn), _P, _P, _P]),
    "navhip_state_update_aux": (_I, [_P, _WORLD, C.POINTER(StateAuxIn), _P, _P, _P]),
    "navhip_state_update_aux_dev": (_I, [_P, _WORLD, C.POINTER(StateAuxIn), _P, _P, _P, _P]),
    "navhip_state_pass": (_I, [_P, _WORLD, C.POINTER(StatePassIn), C.POINTER(StatePassOut)]),
    "navhip_state_pass_resident": (_I, [_P, C.POINTER(StatePassIn), C.POINTER(StatePassOut)]),
    "navhip_settled_count": (_I, [_P, _WORLD, _I, _P, _P]),
    "navhip_settled_count_resident": (_I, [_P, _P, _I, _P, _P]),
    "navhip_arrival_settle": (_I, [_P, _WORLD, C.POINTER(SettleIn), C.POINTER(SettleOut)]),
    "navhip_arrival_settle_dev": (_I, [_P, _WORLD, C.POINTER(SettleIn), C.POINTER(SettleOut), _P]),
    "navhip_arrival_settle_resident": (_I, [_P, _P, _P, _P]),
    "navhip_arrival_velocity": (_I, [_P, _WORLD, C.POINTER(ArrivalVelIn), C.POINTER(ArrivalVelOut)]),
    "navhip_arrival_velocity_dev": (_I, [_P, _WORLD, C.POINTER(ArrivalVelIn), C.POINTER(ArrivalVelOut), _P]),
    # arrival_flock_kernels: the built-zone branch of G_Arrival_UpdateFlock
    "navhip_arrival_flock_update": (_I, [_P, _WORLD, C.POINTER(ArrivalFlockIn), C.POINTER(ArrivalFlockOut)]),
    "navhip_arrival_flock_update_dev": (_I, [_P, _WORLD, C.POINTER(ArrivalFlockIn), C.POINTER(ArrivalFlockOut), _P]),
    # arrival_build_kernels: the first build of a zone, the `!built` branch of G_Arrival_UpdateFlock
    "navhip_arrival_zone_build": (_I, [_P, _WORLD, C.POINTER(ArrivalBuildIn), C.POINTER(ArrivalBuildOut)]),
    "navhip_arrival_zone_build_dev": (_I, [_P, _WORLD, C.POINTER(ArrivalBuildIn), C.POINTER(ArrivalBuildOut), _P]),
    # dest_query_kernels: the destination queries of arrived()
    "navhip_dest_queries": (_I, [_P, _P, _I, _F, _F, _P, _P, _P, _I, _P]),
    "navhip_dest_queries_dev": (_I, [_P, _P, _I, _F, _F, _P, _P, _P, _I, _P, _P]),
    # surround_query_kernels: the two unit queries of the surround arm
    "navhip_surround_queries": (_I, [_P, _WORLD, _P, _P, _P, _I, _P, _P]),
    "navhip_surround_queries_dev": (_I, [_P, _WORLD, _P, _P, _P, _I, _P, _P, _P]),
    "navhip_static_targets_set": (_I, [_P, _I, _P, _P]),
    "navhip_surround_queries_ex": (_I, [_P, _WORLD, _P, _P, _P, _P, _I, _P, _P]),
    "navhip_surround_queries_ex_dev": (_I, [_P, _WORLD, _P, _P, _P, _P, _I, _P, _P, _P]),
    # order_query_kernels: the nav queries of an order
    "navhip_order_queries": (_I, [_P, _P, _I, _F, _F, _P, _P, _P]),
    "navhip_order_queries_dev": (_I, [_P, _P, _I, _F, _F, _P, _P, _P, _P]),
    # region_repair_kernels: the nearest-pathable repair of a region field
    "navhip_repair_region_fields": (_I, [_P, _P, _I, _P, _Z, _P, _Z, _P]),
    "navhip_repair_region_fields_dev": (_I, [_P, _P, _I, _I, _P, _P, _Z, _P, _P]),
    # seek_seed_kernels: enemy-seek and surround fields from the snapshot
    "navhip_build_seek_fields": (_I, [_P, _WORLD, C.POINTER(SeekGame), _P, _I, _P, _Z, _P, _P]),
    "navhip_build_seek_fields_dev": (_I, [_P, _WORLD, C.POINTER(SeekGame), _P, _I, _P, _Z, _P, _P, _P]),
    # pool_api: the resident field pool
    "navhip_pool_create": (_I, [_P, _I, _I]),
    "navhip_pool_destroy": (None, [_P]),
    "navhip_pool_clear": (_I, [_P]),
    "navhip_pool_contains": (_I, [_P, _U64]),
    "navhip_pool_put": (_I, [_P, _U64, _P]),
    "navhip_pool_get": (_I, [_P, _U64, _P]),
    "navhip_pool_invalidate": (_I, [_P, _U64]),
    "navhip_pool_build": (_I, [_P, _P, _P, _P, _I, _P]),
    "navhip_pool_map": (_I, [_P, _I, _P, _P, _P, _P]),
    # submit_api: the asynchronous host-buffer step, page-locked memory
    "navhip_host_alloc": (_P, [_Z]),
    "navhip_host_free": (None, [_P]),
    "navhip_agent_step_submit": (_I, [_P, _WORLD, C.POINTER(StepOut)]),
    "navhip_agent_step_poll": (_I, [_P]),
    "navhip_agent_step_wait": (_I, [_P]),
    # stream_set: the library's streams
    "navhip_stream_create_partial": (_I, [_P, _I, _I, C.POINTER(_P)]),
    "navhip_stream_beside": (_I, [_P, _P, _I, _I, C.POINTER(_P)]),
    "navhip_stream_main": (_I, [_P, C.POINTER(_P)]),
    # comm_api: the slab exchange between ranks
    "navhip_comm_unique_id": (_I, [_P]),
    "navhip_comm_init": (_I, [_P, _I, _I, _P]),
    "navhip_comm_init_mailbox": (_I, [_P, _I, _I, _P, _Z]),
    "navhip_comm_destroy": (None, [_P]),
    "navhip_comm_rank": (_I, [_P]),
    "navhip_comm_world": (_I, [_P]),
    "navhip_comm_allgather_step_dev": (_I, [_P, _P, _P, _P, _P]),
    "navhip_comm_allgather_rows_dev": (_I, [_P, _P, _Z, _P, _P]),
    # los_chain_api: resident LOS chains
    "navhip_los_chain_create": (_I, [_P, _P, _P, _I, _P, _F, _F, C.POINTER(_P)]),
    "navhip_los_chain_build": (_I, [_P, _P]),
    "navhip_los_chain_refresh": (_I, [_P, _U32, _P]),
    "navhip_los_chain_get_stats": (_I, [_P, C.POINTER(LosChainStats)]),
    "navhip_los_chain_destroy": (None, [_P]),
    # tick_api: the whole tick behind one call
    "navhip_tick_create": (_I, [_P, C.POINTER(TickDesc), C.POINTER(_P)]),
    "navhip_tick_run": (_I, [_P, _I]),
    "navhip_tick_compute": (_I, [_P]),
    "navhip_tick_advance": (_I, [_P]),
    "navhip_tick_set_los_chain": (_I, [_P, _P, _U32]),
    "navhip_tick_sync": (_I, [_P]),
    "navhip_tick_get_info": (_I, [_P, C.POINTER(TickInfo)]),
    "navhip_tick_destroy": (None, [_P]),
}

# ---------------------------------------------------------------------------------------------
# 2. the records table: the C type name of every record above (tests/test_abi_cpu.py compares each with the header)
# ---------------------------------------------------------------------------------------------
RECORDS = {
    "navhip_field_req": FIELD_REQ_DTYPE, "navhip_circle": CIRCLE_DTYPE, "navhip_los_req": LOS_REQ_DTYPE,
    "navhip_region_req": REGION_REQ_DTYPE, "navhip_region_repair_req": REGION_REPAIR_REQ_DTYPE,
    "navhip_dest_query": DEST_QUERY_DTYPE, "navhip_order_query": ORDER_QUERY_DTYPE,
    "navhip_seek_req": SEEK_REQ_DTYPE, "navhip_seek_game": SeekGame,
    "navhip_world": World, "navhip_step_out": StepOut,
    "navhip_state_in": StateIn, "navhip_state_aux_in": StateAuxIn, "navhip_gate_in": GateIn,
    "navhip_state_pass_in": StatePassIn, "navhip_state_pass_out": StatePassOut,
    "navhip_arrival_zone": ArrivalZone, "navhip_settle_in": SettleIn, "navhip_settle_out": SettleOut,
    "navhip_arrival_vel_in": ArrivalVelIn, "navhip_arrival_vel_out": ArrivalVelOut,
    "navhip_arrival_flock": ArrivalFlock, "navhip_arrival_flock_in": ArrivalFlockIn, "navhip_arrival_flock_out": ArrivalFlockOut,
    "navhip_arrival_build_in": ArrivalBuildIn, "navhip_arrival_build_out": ArrivalBuildOut,
    "navhip_los_chain_stats": LosChainStats, "navhip_tick_desc": TickDesc, "navhip_tick_info": TickInfo,
}

# ---------------------------------------------------------------------------------------------
# 3. the loader
# ---------------------------------------------------------------------------------------------
_lib = None


class NavHipError(RuntimeError):
    pass


def lib():
    """Load libnavhip.so (built in-tree by build.py).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NavHipError("libnavhip.so not built (run __graft_entry__.build()); "
                              "there is no CPU fallback")
        if os.environ.get("NAVHIP_LIB"):
            # never silent: a development / test build (an A/B variant, the host emulator of tests/hostsim) stands
            # in for the in-tree library -- bench.py names it in config.library
            import sys
            sys.stderr.write("navhip: NAVHIP_LIB=%s replaces the in-tree libnavhip.so\n" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (rt, at) in _SIGS.items():
            if os.environ.get("NAVHIP_LIB") and not hasattr(L, name):
                continue                 # (an A/B build of an older revision lacks the newer entry points)
            f = getattr(L, name)
            f.restype = rt
            f.argtypes = at
        _lib = L
    return _lib


# ---------------------------------------------------------------------------------------------
# 4. the packing helpers, and the entry points that need no context
# ---------------------------------------------------------------------------------------------
def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _opt(a, ptr=_hp):
    """An optional buffer: NULL for None, else ptr(a)."""
    return None if a is None else ptr(a)


def dev_ptr(t):
    """torch CUDA tensor -> void* for the *_dev entry points."""
    return C.c_void_p(t.data_ptr())


def _stream(stream):
    """A hipStream_t value -> the stream argument of an entry point (None / 0: the context's own)."""
    return C.c_void_p(stream) if stream else None


def _arr(a, dt=np.float32, *shape):
    """A contiguous host array of element type `dt`, reshaped when a shape is given; None (an optional array) stays None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dt)
    return a.reshape(shape) if shape else a


def _point(st, **arrays):
    """Point the members of the structure `st` at host arrays.  Returns the arrays: the caller keeps them alive."""
    for name, a in arrays.items():
        setattr(st, name, a.ctypes.data)
    return list(arrays.values())


# element type and per-chunk shape of every plane
_PLANES = {PLANE_COST_BASE: (np.uint8, (64, 64)), PLANE_BLOCKERS: (np.uint16, (64, 64)),
           PLANE_LOCAL_ISLANDS: (np.uint16, (64, 64)), PLANE_FACTIONS: (np.uint8, (15, 64, 64)),
           PLANE_ISLANDS: (np.uint16, (64, 64))}


def _plane(plane):
    return _PLANES.get(plane, _PLANES[PLANE_BLOCKERS])        # (a plane number out of range is the library's to reject)


def _tiles_csr(tile_lists):
    """list of [k, 2] int16 arrays (absolute (row, col) tiles) -> (CSR offsets [len + 1] int32, the tiles [.., 2] int16 with
    one spare row, so that the array is never empty)."""
    offs = np.zeros(len(tile_lists) + 1, np.int32)
    offs[1:] = np.cumsum([len(t) for t in tile_lists])
    tiles = np.concatenate([np.asarray(t, np.int16).reshape(-1, 2) for t in tile_lists] + [np.zeros((1, 2), np.int16)])
    return offs, np.ascontiguousarray(tiles)


def _step_out(n, want):
    """(StepOut, dict of its host arrays) for n entities: vel_xz always, the others when named in `want`."""
    out = {name: np.zeros((n, 2), np.float32) for name in ("vel_xz", "new_pos_xz", "vdes_xz", "vpref_xz")
           if name in want or name == "vel_xz"}
    if "status" in want:
        out["status"] = np.zeros(n, np.uint8)
    so = StepOut()
    _point(so, **out)
    return so, out


def _fill_gate(gi, n, next_rot, new_vel_xz, vdes_xz, interp=None):
    """The members of the GateIn `gi`.  interp: (movestate.next_pos xz [n][2], movestate.step [n]) at a rate below
    20 Hz.  Returns the arrays to keep alive."""
    keep = _point(gi, next_rot=_arr(next_rot, np.float32, n, 4), new_vel_xz=_arr(new_vel_xz, np.float32, n, 2),
                  vdes_xz=_arr(vdes_xz, np.float32, n, 2))
    if interp is not None:
        keep += _point(gi, interp_from_xz=_arr(interp[0], np.float32, n, 2), interp_step=_arr(interp[1]))
    return keep


def _fill_state(si, flock_layer, flock_nearest_xz, flock_tiles, skip=None):
    """The per-flock members and `skip` of the StateIn `si` (new_pos_xz / vdes_xz are the single pass's: the combined
    pass takes them from its gate).  flock_tiles: list of [k, 2] int16 arrays.  Returns the arrays to keep alive."""
    offs, tiles = _tiles_csr(flock_tiles)
    keep = _point(si, flock_layer=_arr(flock_layer, np.uint8), flock_nearest_xz=_arr(flock_nearest_xz, np.float32, -1, 2),
                  flock_tiles_off=offs, flock_tiles=tiles)
    if skip is not None:
        keep += _point(si, skip=_arr(skip, np.uint8))
    return keep


def _fill_aux(ai, n, fstate, wait_ticks_left, wait_prev, ent_rot=None, target_dir=None, range_in=None, surround=None):
    """The base members of the StateAuxIn `ai` and its turn / enter-range / surround arms.  range_in: dict(target [n]
    row or -1 / -2, range [n], prev_xz [n][2], tiles_row [n], tiles: list of [k, 2] int16); surround: dict(target [n]
    row or -1 / -2, query [n] SQ_*, target_prev_xz [n][2], nearest_prev_xz [n][2], dest_xz [n][2][2]).
    Returns (the arrays to keep alive, the surround output array or None)."""
    keep = _point(ai, fstate=_arr(fstate, np.uint8), wait_ticks_left=_arr(wait_ticks_left, np.int32),
                  wait_prev=_arr(wait_prev, np.uint8))
    su_out = None
    if ent_rot is not None:
        keep += _point(ai, ent_rot=_arr(ent_rot, np.float32, n, 4), target_dir=_arr(target_dir, np.float32, n, 4))
    if range_in is not None:
        offs, tiles = _tiles_csr(range_in["tiles"])
        keep += _point(ai, range_target=_arr(range_in["target"], np.int32), target_range=_arr(range_in["range"], np.float32, n),
                       target_prev_xz=_arr(range_in["prev_xz"], np.float32, n, 2),
                       range_tiles_row=_arr(range_in["tiles_row"], np.int32), range_tiles_off=offs, range_tiles=tiles)
        ai.n_range_rows = len(range_in["tiles"])
    if surround is not None:
        su_out = np.zeros((n, 2), np.float32)
        keep += _point(ai, surround_target=_arr(surround["target"], np.int32), surround_query=_arr(surround["query"], np.uint8),
                       surround_target_prev_xz=_arr(surround["target_prev_xz"], np.float32, n, 2),
                       surround_nearest_prev_xz=_arr(surround["nearest_prev_xz"], np.float32, n, 2),
                       surround_dest_xz=_arr(surround["dest_xz"], np.float32, n, 2, 2), out_surround_dest_xz=su_out)
    return keep, su_out


def _pack_zones(zones, region_keys):
    """Zones as dicts (layer, centre_xz, radius, unit_radius, fill_frac, active_row, num_rows, slots_xz, slot_ring) and
    their sorted u64 key arrays -> (ArrivalZone array, slots_xz, slot_ring, region_keys): the three shared arrays, each
    with one spare element so that none is empty."""
    zs = (ArrivalZone * max(1, len(zones)))()
    slots, rings, keys = [], [], []
    so = ko = 0
    for i, z in enumerate(zones):
        sl = np.asarray(z["slots_xz"], np.float32).reshape(-1, 2)
        kk = np.asarray(region_keys[i], np.uint64)
        zs[i] = ArrivalZone(float(z["centre_xz"][0]), float(z["centre_xz"][1]), float(z["unit_radius"]),
                            float(z["fill_frac"]), int(z["radius"]), int(z["layer"]), int(z["active_row"]),
                            int(z["num_rows"]), so, so + len(sl), ko, ko + len(kk))
        so += len(sl)
        ko += len(kk)
        slots.append(sl)
        rings.append(np.asarray(z["slot_ring"], np.int32))
        keys.append(kk)
    cat = lambda parts, dt, shape: np.ascontiguousarray(np.concatenate(parts + [np.zeros(shape, dt)]))      # noqa: E731
    return zs, cat(slots, np.float32, (1, 2)), cat(rings, np.int32, (1,)), cat(keys, np.uint64, (1,))


def pack_flocks(zones, members):
    """The per-zone companions of navhip_arrival_flock_update and the member arrays of every zone side by side (one
    spare row each, so that none is empty): (ArrivalFlock array, dict of arrays)."""
    fs = (ArrivalFlock * max(1, len(zones)))()
    parts = {name: [] for name, _, _ in NavContext._AF_IN}
    mo = 0
    for i, (z, mem) in enumerate(zip(zones, members)):
        n = len(mem["uid"])
        fs[i] = ArrivalFlock(int(z["phase"]), int(z["realloc_counter"]), int(z["stall_counter"]), int(z["prev_occ"]),
                             float(z["row_height"]), float(z["arg_unit_radius"]), int(z["arg_total_members"]), int(z["arg_layer"]),
                             mo, mo + n)
        mo += n
        for name, dt, width in NavContext._AF_IN:
            parts[name].append(np.asarray(mem[name], dt).reshape((n, width) if width > 1 else (n,)))
    cat = {name: np.ascontiguousarray(np.concatenate(parts[name] + [np.zeros((1, width) if width > 1 else (1,), dt)]))
           for name, dt, width in NavContext._AF_IN}
    return fs, cat


def unpack_flocks(zs, fs, res, nz):
    """What navhip_arrival_flock_update left: (per zone a dict of the zone's and the companion's members and its
    slot_ring, per zone a dict of the member outputs, status [nz])."""
    zones, members = [], []
    for i in range(nz):
        z, f = zs[i], fs[i]
        d = {name: getattr(z, name) for name in ("unit_radius", "fill_frac", "radius", "layer", "active_row", "num_rows")}
        d.update({name: getattr(f, name) for name in ("phase", "realloc_counter", "stall_counter", "prev_occ")})
        d["slot_ring"] = np.array(res["slot_ring"][z.slot_begin:z.slot_end])
        zones.append(d)
        members.append({name: np.array(res[name][f.member_begin:f.member_end]) for name, _, _ in NavContext._AF_OUT})
    return zones, members, np.array(res["status"][:nz])


def make_reqs(n):
    r = np.zeros(n, FIELD_REQ_DTYPE)
    r["faction_id"] = FACTION_ID_NONE
    return r


def flock_csr(flock, n_flocks, order=None):
    """CSR member lists from a per-entity flock index (members in ascending uid order unless
    `order` -- a list of per-flock uid arrays, e.g. the reference's kh_foreach order -- is given)."""
    flock = np.asarray(flock)
    lists = order if order is not None else [np.flatnonzero(flock == f) for f in range(n_flocks)]
    offs = np.zeros(n_flocks + 1, np.int32)
    offs[1:] = np.cumsum([len(l) for l in lists])
    members = np.concatenate(lists).astype(np.int32) if n_flocks else np.zeros(0, np.int32)
    return offs, members


def grid_bounds(chunk_w, chunk_h):
    """bg_ent_init bounds the engine uses (position.c:276-283): the map, centred on the origin."""
    hx, hz = chunk_w * 128.0, chunk_h * 128.0
    return (-hx, hx, -hz, hz)


def make_world(chunk_w, chunk_h, arrays, hz=20, xp=None):
    """Build a navhip_world from a dict of numpy arrays (host form) or torch CUDA tensors
    (device form).  Returns (World, keepalive)."""
    w = World()
    keep = {}
    n = len(arrays["pos_xz"])
    w.n_ents = n
    w.n_flocks = len(arrays["flock_target_xz"]) if arrays.get("flock_target_xz") is not None else 0
    w.hz = hz
    for name, dt in _WORLD_ARRAYS:
        a = arrays.get(name)
        if a is None:
            setattr(w, name, None)
            continue
        if hasattr(a, "data_ptr"):          # torch tensor on the GPU
            keep[name] = a
            setattr(w, name, a.data_ptr())
        else:
            a = np.ascontiguousarray(a, dtype=dt)
            keep[name] = a
            setattr(w, name, a.ctypes.data)
    fp = arrays.get("field_pool")
    w.n_field_slots = 0 if fp is None else int(fp.shape[0])
    lp = arrays.get("los_pool")
    w.n_los_slots = 0 if lp is None else int(lp.shape[0])
    rs = arrays.get("region_field_slot")
    w.n_region_rows = int(arrays.get("n_region_rows") or (0 if rs is None else int(rs.shape[0])))
    w.map_pos_x = chunk_w * 128.0
    w.map_pos_z = -chunk_h * 128.0
    w.grid_xmin, w.grid_xmax, w.grid_zmin, w.grid_zmax = grid_bounds(chunk_w, chunk_h)
    w.static_epoch = int(arrays.get("static_epoch") or 0)
    return w, keep


def make_seek_game(faction, enemy_mask, exclude=None):
    """A navhip_seek_game of numpy arrays (host form) or torch CUDA tensors (device form).  Returns (SeekGame, keepalive)."""
    g = SeekGame()
    keep = []
    for name, a, dt in (("faction", faction, np.int32), ("exclude", exclude, np.uint8)):
        if a is None:
            setattr(g, name, None)
        elif hasattr(a, "data_ptr"):
            keep.append(a)
            setattr(g, name, a.data_ptr())
        else:
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            setattr(g, name, a.ctypes.data)
    for f, m in enumerate(enemy_mask):
        g.enemy_mask[f] = int(m)
    return g, keep


def N_FlowFieldID(req):
    """N_FlowFieldID (field.c:1952) for one navhip_field_req record."""
    r = np.ascontiguousarray(np.asarray(req, dtype=FIELD_REQ_DTYPE).reshape(1))
    return int(lib().navhip_flow_field_id(_hp(r)))


def _ids_of(reqs):
    reqs = _arr(reqs, FIELD_REQ_DTYPE)
    return np.array([lib().navhip_flow_field_id(_hp(reqs[i:i + 1])) for i in range(len(reqs))], np.uint64)


def N_RegionFieldID(kind, layer, chunk_r, chunk_c, a, b=0, c=0):
    """N_FlowFieldID for an ENEMIES / ENTITY / ZONE target (field.c:1976-2003)."""
    return int(lib().navhip_region_field_id(kind, layer, chunk_r, chunk_c, a, b, c))


def comm_unique_id():
    """ncclGetUniqueId through the library (rank 0); 128 bytes to hand to the other ranks."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = lib().navhip_comm_unique_id(buf)
    if rc != 0:
        raise NavHipError("navhip_comm_unique_id failed (%d): is librccl present?" % rc)
    return bytes(buf)


def host_alloc(nbytes):
    """navhip_host_alloc: pinned host memory as a writable buffer (freed with host_free(buf))."""
    p = lib().navhip_host_alloc(nbytes)
    if not p:
        raise MemoryError("navhip_host_alloc(%d)" % nbytes)
    buf = (C.c_uint8 * nbytes).from_address(p)
    buf._navhip_ptr = p
    return buf


def host_free(buf):
    lib().navhip_host_free(C.c_void_p(buf._navhip_ptr))


# ---------------------------------------------------------------------------------------------
# 5. the classes
# ---------------------------------------------------------------------------------------------
class _Handle:
    """An object of the library behind `self._h`, freed once by the entry point `_destroy` names.  Errors are the
    context's: an object made from one (`self.ctx`) raises through it."""
    _destroy = None

    def _chk(self, rc, what):
        self.ctx._chk(rc, what)

    def _call(self, name, *args):
        """The entry point `name` on this handle; raises NavHipError, under that name, unless it returns NAVHIP_OK."""
        self._chk(getattr(lib(), name)(self._h, *args), name)

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NavContext(_Handle):
    """Device-resident navigation state of one map: the GPU counterpart of the planes of
    `struct nav_private` (nav_private.h:52) that the hot path reads."""
    _destroy = "navhip_ctx_destroy"

    def __init__(self, chunk_w, chunk_h, device=0):
        self._h = C.c_void_p()
        rc = lib().navhip_ctx_create(C.byref(self._h), chunk_w, chunk_h, device)
        if rc != OK:
            self._h = None
            raise NavHipError("navhip_ctx_create failed (%d): no MI355X visible?" % rc)
        self.w, self.h, self.device = chunk_w, chunk_h, device

    def _chk(self, rc, what):
        if rc != OK:
            raise NavHipError("%s failed (%d): %s" % (what, rc, self.last_error()))

    def _world(self, arrays, hz=20, work=None):
        """make_world for a host-buffer call of this map; work: (work_begin, work_end)."""
        w, keep = make_world(self.w, self.h, arrays, hz)
        if work is not None:
            w.work_begin, w.work_end = work
        return w, keep

    # -- navhip_api: the context -------------------------------------------------------------------
    def last_error(self):
        msg = lib().navhip_last_error(self._h)
        return msg.decode() if msg else ""

    @property
    def stream(self):
        return lib().navhip_stream(self._h)

    def sync(self):
        self._call("navhip_sync")

    def counters(self, reset=False):
        """navhip_get_counters: work counters of the context as a dict."""
        out = (C.c_uint64 * len(COUNTER_NAMES))()
        self._call("navhip_get_counters", out, int(bool(reset)))
        return dict(zip(COUNTER_NAMES, [int(x) for x in out]))

    # -- navhip_api: map state (N_CopyCostBasePacked / N_CopyBlockersPacked layouts, nav.c:2432,2470) ----------
    def upload_plane(self, layer, plane, array):
        a = _arr(array, _plane(plane)[0])
        self._call("navhip_upload_plane", layer, plane, _hp(a), a.nbytes)

    def upload_chunk(self, layer, plane, chunk_r, chunk_c, array):
        a = _arr(array, _plane(plane)[0])
        self._call("navhip_upload_chunk", layer, plane, chunk_r, chunk_c, _hp(a), a.nbytes)

    def download_plane(self, layer, plane):
        dt, chunk_shape = _plane(plane)
        out = np.zeros((self.h, self.w) + chunk_shape, dt)
        self._call("navhip_download_plane", layer, plane, _hp(out), out.nbytes)
        return out

    # -- navhip_api: dynamic obstacles (N_BlockersIncref / N_BlockersDecref, nav.c:4663,4685) ------------------
    def map_pos(self):
        return self.w * 128.0, -self.h * 128.0

    def N_BlockersUpdate(self, circles):
        """circles: CIRCLE_DTYPE records (delta +1 = N_BlockersIncref, -1 = N_BlockersDecref)."""
        c = _arr(circles, CIRCLE_DTYPE)
        self._call("navhip_blockers_circles", _hp(c), len(c), *self.map_pos())

    def blockers_circles_dev(self, d_circles, n, stream=None):
        self._call("navhip_blockers_circles_dev", dev_ptr(d_circles), n, *self.map_pos(), _stream(stream))

    def relabel_local_islands(self, layer=0):
        self._call("navhip_relabel_local_islands", layer)

    def changed_chunks(self, layer=0, clear=False):
        out = np.zeros(self.w * self.h, np.uint8)
        self._call("navhip_changed_chunks", layer, _hp(out), int(clear))
        return out.reshape(self.h, self.w)

    def faction_changed_chunks(self, layer=0, clear=False):
        """[h][w] u16: bit f = a blocker update changed which tiles of the chunk faction f holds."""
        out = np.zeros(self.w * self.h, np.uint16)
        self._call("navhip_faction_changed_chunks", layer, _hp(out), int(clear))
        return out.reshape(self.h, self.w)

    def clear_changed(self, stream=None):
        self._call("navhip_clear_changed", _stream(stream))

    # -- navhip_api: flow fields ---------------------------------------------------------------------
    def set_field_kernel(self, mode):
        self._call("navhip_set_field_kernel", mode)

    def last_fields_split(self):
        """(requests the bit-parallel BFS kernel kept, requests the generic kernel built) of the last chunk-field
        build of this context; waits for it."""
        out = (C.c_int32 * 2)()
        self._call("navhip_last_fields_split", C.byref(out))
        return int(out[0]), int(out[1])

    def N_FlowFieldUpdate(self, reqs, inout=None, want_integ=False):
        """Batched N_FlowFieldInit + N_FlowFieldUpdate (field.c:2020,2030) through host buffers.
        reqs: FIELD_REQ_DTYPE array.  inout: [n,64,64] u8 existing fields (rows used only for
        requests flagged REQ_INOUT).  Returns (dirs [n,64,64] u8, integ [n,64,64] f32 | None)."""
        reqs = _arr(reqs, FIELD_REQ_DTYPE)
        n = len(reqs)
        dirs = np.zeros((n, 64, 64), np.uint8)
        if inout is not None:
            dirs[...] = np.asarray(inout, np.uint8).reshape(n, 64, 64)
        integ = np.zeros((n, 64, 64), np.float32) if want_integ else None
        self._call("navhip_build_fields", _hp(reqs), n, _hp(dirs), _opt(integ))
        return dirs, integ

    def build_fields_dev(self, d_reqs, n, d_dirs, d_integ=None, stream=None):
        """Everything resident in HBM (torch tensors); asynchronous on `stream`."""
        self._call("navhip_build_fields_dev", dev_ptr(d_reqs), n, dev_ptr(d_dirs), _opt(d_integ, dev_ptr), _stream(stream))

    def build_region_fields(self, reqs, seeds, overlay=None, inout=None, out_stride=None):
        """Region flow fields (N_CellArrivalFieldCreate / N_GroupArrivalFieldCreate in mode 0, the
        padded-region builders behind TARGET_ENEMIES / ENTITY / ZONE in mode 1).  seeds / overlay:
        [k, 2] int16 absolute (row, col) tiles.  Returns [n, out_stride] u8."""
        reqs = _arr(reqs, REGION_REQ_DTYPE)
        n = len(reqs)
        seeds = _arr(seeds, np.int16, -1, 2)
        ov = np.zeros((0, 2), np.int16) if overlay is None else _arr(overlay, np.int16, -1, 2)
        if out_stride is None:
            out_stride = 8192
        buf = np.zeros((n, out_stride), np.uint8)
        if inout is not None:
            a = np.asarray(inout, np.uint8).reshape(n, -1)
            buf[:, :a.shape[1]] = a
        self._call("navhip_build_region_fields", _hp(reqs), n, _hp(seeds), len(seeds), _hp(ov), len(ov), _hp(buf), out_stride)
        return buf

    def build_region_fields_dev(self, d_reqs, n, max_dim, d_seeds, d_overlay, d_inout, out_stride, stream=None):
        """navhip_build_region_fields_dev: every buffer a torch CUDA tensor (d_overlay may be None), asynchronous on
        `stream`."""
        self._call("navhip_build_region_fields_dev", dev_ptr(d_reqs), int(n), int(max_dim), _opt(d_seeds, dev_ptr),
                   _opt(d_overlay, dev_ptr), dev_ptr(d_inout), int(out_stride), _stream(stream))

    def repair_region_fields(self, reqs, overlay=None, inout=None, stride=None):
        """Batched N_CellArrivalFieldUpdateToNearestPathable (field.c:2603) through host buffers.  reqs:
        REGION_REPAIR_REQ_DTYPE records; overlay: [k, 2] int16 absolute (row, col) tiles; inout: [n, >= dim * dim / 2] u8
        packed fields (two directions per byte), copied.  Returns (fields [n, stride] u8, status [n]: 0 or RR_HOST with
        the field as it came in)."""
        reqs = _arr(reqs, REGION_REPAIR_REQ_DTYPE)
        n = len(reqs)
        ov = np.zeros((0, 2), np.int16) if overlay is None else _arr(overlay, np.int16, -1, 2)
        a = np.asarray(inout, np.uint8).reshape(n, -1) if n else np.zeros((0, stride or 0), np.uint8)
        if stride is None:
            stride = a.shape[1]
        buf = np.zeros((n, stride), np.uint8)
        buf[:, :a.shape[1]] = a
        status = np.zeros(n, np.uint8)
        self._call("navhip_repair_region_fields", _hp(reqs), n, _hp(ov), len(ov), _hp(buf), stride, _hp(status))
        return buf, status

    def repair_region_fields_dev(self, d_reqs, n, max_dim, d_overlay, d_inout, stride, d_status, stream=None):
        """navhip_repair_region_fields_dev: every buffer a torch CUDA tensor (d_overlay may be None), one launch,
        asynchronous on `stream`; behind build_region_fields_dev on the same stream it is cell_field_fixup_task."""
        self._call("navhip_repair_region_fields_dev", dev_ptr(d_reqs), int(n), int(max_dim), _opt(d_overlay, dev_ptr),
                   dev_ptr(d_inout), int(stride), dev_ptr(d_status), _stream(stream))

    def build_seek_fields(self, world, faction, enemy_mask, reqs, inout, exclude=None, seed_bits=None):
        """Enemy-seek (kind SEEK_ENEMIES) and surround (SEEK_ENTITY) chunk fields, seeds taken from the snapshot on the
        device, through host buffers.  world: a host World (make_world) of which n_ents, pos_xz, radius, flags, map_pos_*
        and grid_* are read; faction: [n_ents] i32; enemy_mask: 16 u16 (bit g of [f]: f is at war with g); exclude:
        [n_ents] u8 or None; reqs: SEEK_REQ_DTYPE records; inout: [n, >= 4096] u8 chunk fields, copied; seed_bits:
        [n, 2048] u8 to start from (rows of SK_HOST requests keep it) or None for zeros.
        Returns (fields [n, stride] u8, status [n]: 0 or SK_HOST with the field as it came in, seed bits [n, 2048] u8)."""
        reqs = _arr(reqs, SEEK_REQ_DTYPE)
        n = len(reqs)
        buf = np.array(np.asarray(inout, np.uint8).reshape(n, -1) if n else np.zeros((0, 4096), np.uint8), order="C")
        status = np.zeros(n, np.uint8)
        bits = np.zeros((n, 2048), np.uint8) if seed_bits is None else np.array(np.asarray(seed_bits, np.uint8).reshape(n, 2048), order="C")
        g, keep = make_seek_game(faction, enemy_mask, exclude)
        self._call("navhip_build_seek_fields", C.byref(world), C.byref(g), _hp(reqs), n, _hp(buf), buf.shape[1] if n else 4096,
                   _hp(status), _hp(bits))
        return buf, status, bits

    def build_seek_fields_dev(self, dev_world, dev_game, d_reqs, n, d_inout, stride, d_status, d_seed_bits=None, stream=None):
        """navhip_build_seek_fields_dev: dev_world (make_world of CUDA tensors) and dev_game (make_seek_game of CUDA
        tensors) are host structures of device pointers; every other buffer a torch CUDA tensor; two launches,
        asynchronous on `stream`."""
        self._call("navhip_build_seek_fields_dev", C.byref(dev_world), C.byref(dev_game), dev_ptr(d_reqs), int(n), dev_ptr(d_inout),
                   int(stride), dev_ptr(d_status), _opt(d_seed_bits, dev_ptr), _stream(stream))

    def N_LOSFieldCreate(self, reqs, prev=None):
        """Batched N_LOSFieldCreate (field.c:2085).  reqs: LOS_REQ_DTYPE; prev: [n,64,64] u8 previous
        fields (bit0 visible, bit1 wavefront_blocked) or None.  Returns [n,64,64] u8."""
        reqs = _arr(reqs, LOS_REQ_DTYPE)
        n = len(reqs)
        out = np.zeros((n, 64, 64), np.uint8)
        self._call("navhip_build_los", _hp(reqs), n, _opt(_arr(prev, np.uint8, n, 64, 64)), _hp(out), *self.map_pos())
        return out

    def build_los_dev(self, d_reqs, n, d_prev, d_out, stream=None):
        """navhip_build_los_dev: n LOS fields, every buffer a torch CUDA tensor (d_prev may be None)."""
        self._call("navhip_build_los_dev", dev_ptr(d_reqs), int(n), _opt(d_prev, dev_ptr), dev_ptr(d_out), *self.map_pos(),
                   _stream(stream))

    # -- step_api: the per-agent movement step -----------------------------------------------------------
    def agent_step(self, arrays, hz=20, want=("vel_xz", "new_pos_xz", "vdes_xz", "vpref_xz", "status")):
        """Host-buffer velocity step: move_velocity_work (movement.c:3395) for every non-still entity.
        arrays: dict of numpy arrays named after navhip_world members.  Returns dict of outputs."""
        w, keep = self._world(arrays, hz)
        if arrays.get("field_pool") is None and arrays.get("use_resident_pool"):
            w.n_field_slots = POOL_RESIDENT
        so, out = _step_out(w.n_ents, want)
        self._call("navhip_agent_step", C.byref(w), C.byref(so))
        return out

    def agent_step_dev(self, world, stepout, stream=None):
        self._call("navhip_agent_step_dev", C.byref(world), C.byref(stepout), _stream(stream))

    def agent_prefetch_dev(self, world, stream=None, flags=0):
        self._call("navhip_agent_prefetch_dev_ex", C.byref(world), _stream(stream), flags)

    def stream_wait_stage(self, stream, stage, check=True):
        """Make `stream` (a hipStream_t value) wait for a stage of the agent step in flight.  check=False: return whether
        the library could do so instead of raising (NAVHIP_STAGE_END after a step that ran on one stream: it cannot)."""
        rc = lib().navhip_stream_wait_stage(self._h, C.c_void_p(stream), stage)
        if check:
            self._chk(rc, "navhip_stream_wait_stage")
        return rc == 0

    def set_profiling(self, on):
        self._call("navhip_set_profiling", int(bool(on)))

    def last_step_ms(self):
        """Milliseconds of the kernel groups STEP_PHASES of the last profiled agent step."""
        out = (C.c_float * 5)()
        self._call("navhip_last_step_ms", C.byref(out))
        return tuple(float(x) for x in out)

    def last_step_lists(self):
        """Agents per ClearPath work list of the last step: light 1..4 neighbours, wave, full-wave."""
        out = (C.c_int32 * 6)()
        self._call("navhip_last_step_lists", C.byref(out))
        return tuple(int(x) for x in out)

    def step_lists_peek(self):
        """Like last_step_lists, without waiting: the counts of the latest step whose copy has arrived."""
        out = (C.c_int32 * 6)()
        self._call("navhip_step_lists_peek", C.byref(out))
        return list(out)

    def spatial_query(self, pos_xz, query_xz, rng, maxout, bounds=None):
        """G_Pos_EntsInCircleFrom candidate lists (bitmap_grid.h:1376 order) for each query.
        bounds: (xmin, xmax, zmin, zmax) of the index instead of the map's (the C ABI takes any)."""
        w, keep = self._world({"pos_xz": pos_xz})
        if bounds is not None:
            w.grid_xmin, w.grid_xmax, w.grid_zmin, w.grid_zmax = (float(b) for b in bounds)
        q = _arr(query_xz, np.float32, -1, 2)
        counts = np.zeros(len(q), np.int32)
        ids = np.zeros((len(q), maxout), np.uint32)
        self._call("navhip_spatial_query", C.byref(w), _hp(q), len(q), rng, maxout, _hp(counts), _hp(ids))
        return counts, ids

    def region_lookup(self, pos_xz, rows, region_field_slot=None, field_pool=None, centre_abs=None, radius=None):
        """N_DesiredGroupArrivalVelocity for many points: (dir [nq] u8 with 0xff = no field, at_slot [nq] | None)."""
        p = _arr(pos_xz, np.float32, -1, 2)
        nq = len(p)
        r = _arr(rows, np.int32)
        tbl = _arr(region_field_slot, np.int32)
        fp = _arr(field_pool, np.uint8, -1, 4096)
        cen = _arr(centre_abs, np.int32, nq, 2)
        rad = _arr(radius, np.int32)
        out = np.zeros(nq, np.uint8)
        at = np.zeros(nq, np.uint8) if cen is not None else None
        self._call("navhip_region_lookup", nq, _hp(p), _hp(r), _opt(tbl), 0 if tbl is None else len(tbl),
                   _opt(fp), 0 if fp is None else len(fp), _opt(cen), _opt(rad), *self.map_pos(), _hp(out), _opt(at))
        return out, at

    def G_ClearPath_NewVelocity(self, ent, des_v, dyn, n_dyn, stat, n_stat, rows=False):
        """G_ClearPath_NewVelocity (clearpath.c:694) for a batch of independent problems, one wave per
        problem; rows=True: one row of 16 lanes per problem (<= 16 neighbours); rows="team": the waves of a
        workgroup per problem."""
        ent = _arr(ent, np.float32, -1, 5)
        nq = len(ent)
        args = (ent, _arr(des_v, np.float32, nq, 2), _arr(dyn, np.float32, nq, 32, 5), _arr(n_dyn, np.int32),
                _arr(stat, np.float32, nq, 32, 5), _arr(n_stat, np.int32), np.zeros((nq, 2), np.float32))
        name = "navhip_clearpath_team" if rows == "team" else "navhip_clearpath_rows" if rows else "navhip_clearpath"
        self._call(name, nq, *[_hp(a) for a in args])
        return args[-1]

    # -- state_kernels: the state half of the tick ------------------------------------------------------
    def heading_gate(self, arrays, next_rot, new_vel_xz, vdes_xz, work=None, hz=20, interp=None):
        """The heading gate of entity_compute_update (movement.c:2319-2336) for the units of the snapshot `arrays`
        (pos_xz, vel_xz, state).  Returns (velocity after the gate [n][2], new_pos [n][2], gate flags [n])."""
        w, keep = self._world(arrays, hz, work)
        n = w.n_ents
        gi = GateIn()
        k = _fill_gate(gi, n, next_rot, new_vel_xz, vdes_xz, interp)
        vel, pos, gate = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        self._call("navhip_heading_gate", C.byref(w), C.byref(gi), _hp(vel), _hp(pos), _hp(gate))
        return vel, pos, gate

    def state_update(self, arrays, new_pos_xz, vdes_xz, flock_layer, flock_nearest_xz, flock_tiles, skip=None,
                     hz=20, work=None):
        """The arrival arm of entity_compute_update (movement.c:2303) for every unit of the snapshot `arrays`.
        flock_tiles: list of [k, 2] int16 arrays (absolute (row, col) tiles per flock).  Returns (next_state, flags)."""
        w, keep = self._world(arrays, hz, work)
        n = w.n_ents
        si = StateIn()
        k = _fill_state(si, flock_layer, flock_nearest_xz, flock_tiles, skip)
        k += _point(si, new_pos_xz=_arr(new_pos_xz, np.float32, n, 2), vdes_xz=_arr(vdes_xz, np.float32, n, 2))
        st, fl = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self._call("navhip_state_update", C.byref(w), C.byref(si), _hp(st), _hp(fl))
        return st, fl

    # -- dest_query_kernels: the destination queries of arrived() ---------------------------------------
    def dest_queries(self, queries, tiles_cap=None):
        """N_ClosestPathable (nav.c:4126) and the closest island tiles of N_IsMaximallyClose (nav.c:4707) for the
        DEST_QUERY_DTYPE records `queries`.  Returns (nearest_xz [n][2] with x = NaN for "none", list of [k, 2] int16
        tile arrays, status [n]: 0 or DQ_HOST).  tiles_cap: rows of the tile buffer (default: 256 per query)."""
        q = _arr(queries, DEST_QUERY_DTYPE)
        n = len(q)
        cap = DQ_MAX_TILES * n if tiles_cap is None else int(tiles_cap)
        nearest, off = np.zeros((n, 2), np.float32), np.zeros(n + 1, np.int32)
        tiles, status = np.zeros((max(cap, 1), 2), np.int16), np.zeros(n, np.uint8)
        self._call("navhip_dest_queries", _hp(q), n, *self.map_pos(), _hp(nearest), _hp(off), _hp(tiles), cap, _hp(status))
        return nearest, [tiles[off[i]:off[i + 1]].copy() for i in range(n)], status

    def dest_queries_dev(self, d_queries, n, d_nearest_xz, d_tiles_off, d_tiles, tiles_cap, d_status, stream=None):
        """navhip_dest_queries_dev: every buffer a torch CUDA tensor, asynchronous on `stream`; the outputs are what
        navhip_state_in.flock_nearest_xz / .flock_tiles_off / .flock_tiles take."""
        self._call("navhip_dest_queries_dev", dev_ptr(d_queries), int(n), *self.map_pos(), dev_ptr(d_nearest_xz),
                   dev_ptr(d_tiles_off), dev_ptr(d_tiles), int(tiles_cap), dev_ptr(d_status), _stream(stream))

    # -- surround_query_kernels: the two unit queries of the surround arm -------------------------------
    def static_targets_set(self, tile_lists):
        """navhip_static_targets_set: the table of static targets' tile lists, replaced as a whole.  tile_lists: one [k, 2]
        int16 array of absolute (row, column) tiles per set, in M_Tile_AllUnderObj's order; an empty list clears the table."""
        offs, tiles = _tiles_csr(list(tile_lists))
        self._call("navhip_static_targets_set", len(offs) - 1, _hp(offs), _hp(tiles))

    def surround_queries(self, arrays, new_vel, target, units=None, target_set=None):
        """M_NavObjAdjacentFrom and M_NavClosestReachableAdjacentPosFrom (from pos + new_vel and from pos).  arrays: pos_xz,
        radius, flags of the snapshot; target [nq]: the target's row or < 0; units [nq]: the rows' units, None = the dense
        form (row i is unit i); target_set [nq]: the row of static_targets_set's table for a target without
        ENTITY_FLAG_MOVABLE, None = movable targets only.  Returns (query [nq] SQ_*, dest_xz [nq][2][2]): the shapes of
        `surround` in state_update_aux."""
        w, keep = self._world(arrays)
        vel = _arr(new_vel, np.float32, w.n_ents, 2)
        tgt = _arr(target, np.int32)
        un, ts = _arr(units, np.int32), _arr(target_set, np.int32)
        nq = len(tgt)
        query, dest = np.zeros(nq, np.uint8), np.zeros((nq, 2, 2), np.float32)
        if ts is None:
            self._call("navhip_surround_queries", C.byref(w), _hp(vel), _opt(un), _hp(tgt), nq, _hp(query), _hp(dest))
        else:
            self._call("navhip_surround_queries_ex", C.byref(w), _hp(vel), _opt(un), _hp(tgt), _hp(ts), nq, _hp(query), _hp(dest))
        return query, dest

    def surround_queries_dev(self, world, d_new_vel_xz, d_units, d_target, nq, d_query, d_dest_xz, stream=None, d_target_set=None):
        """navhip_surround_queries[_ex]_dev: `world` a World of device pointers (make_world of torch CUDA tensors), every
        buffer a torch CUDA tensor (d_units None: the dense form; d_target_set None: movable targets only), asynchronous on
        `stream`; the dense outputs are what navhip_state_aux_in.surround_query / .surround_dest_xz take."""
        if d_target_set is None:
            self._call("navhip_surround_queries_dev", C.byref(world), dev_ptr(d_new_vel_xz), _opt(d_units, dev_ptr),
                       dev_ptr(d_target), int(nq), dev_ptr(d_query), dev_ptr(d_dest_xz), _stream(stream))
        else:
            self._call("navhip_surround_queries_ex_dev", C.byref(world), dev_ptr(d_new_vel_xz), _opt(d_units, dev_ptr),
                       dev_ptr(d_target), dev_ptr(d_target_set), int(nq), dev_ptr(d_query), dev_ptr(d_dest_xz), _stream(stream))

    # -- order_query_kernels: the nav queries of an order ------------------------------------------------
    def order_queries(self, queries):
        """N_ClosestReachableInRange (nav.c:5067), N_ClosestReachableDest (nav.c:4085), N_LocationsReachable and
        N_DestIDForPos[Attacking] for the ORDER_QUERY_DTYPE records `queries` (flags OQ_IN_RANGE | OQ_REACHABLE).  Returns
        (dest_xz [n][2], dest_id [n] uint32, status [n]: OQ_SAME_ISLAND | OQ_NO_TILE, or OQ_HOST with (NaN, 0) and id 0)."""
        q = _arr(queries, ORDER_QUERY_DTYPE)
        n = len(q)
        dest, ids, status = np.zeros((n, 2), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._call("navhip_order_queries", _hp(q), n, *self.map_pos(), _hp(dest), _hp(ids), _hp(status))
        return dest, ids, status

    def order_queries_dev(self, d_queries, n, d_dest_xz, d_dest_id, d_status, stream=None):
        """navhip_order_queries_dev: every buffer a torch CUDA tensor, one launch, asynchronous on `stream`."""
        self._call("navhip_order_queries_dev", dev_ptr(d_queries), int(n), *self.map_pos(), dev_ptr(d_dest_xz),
                   dev_ptr(d_dest_id), dev_ptr(d_status), _stream(stream))

    def state_update_aux(self, arrays, fstate, wait_ticks_left, wait_prev, new_pos_xz, state, flags, work=None,
                         ent_rot=None, target_dir=None, range_in=None, surround=None, vdes_xz=None, hz=20):
        """The flag / counter arms of the state switch, after state_update on the same slab: returns (state, flags,
        wait_ticks_left) with the rows this pass decides overwritten -- and, with `surround` (see _fill_aux; needs
        vdes_xz), the positions of NAVHIP_SU_SURROUND_PREV rows as a fourth value."""
        w, keep = self._world(arrays, hz, work)
        n = w.n_ents
        ai = StateAuxIn()
        k, su_out = _fill_aux(ai, n, fstate, wait_ticks_left, wait_prev, ent_rot, target_dir, range_in, surround)
        k += _point(ai, new_pos_xz=_arr(new_pos_xz, np.float32, n, 2))
        if surround is not None:
            k += _point(ai, vdes_xz=_arr(vdes_xz, np.float32, n, 2))
        st, fl, ticks = np.array(state, np.uint8), np.array(flags, np.uint8), np.zeros(n, np.int32)
        self._call("navhip_state_update_aux", C.byref(w), C.byref(ai), _hp(st), _hp(fl), _hp(ticks))
        if surround is not None:
            return st, fl, ticks, su_out
        return st, fl, ticks

    def state_pass(self, arrays, next_rot, new_vel_xz, vdes_xz, flock_layer, flock_nearest_xz, flock_tiles, skip=None,
                   aux=None, work=None, hz=20, interp=None):
        """The state half of the tick in one call (navhip_state_pass): heading gate -> state update -> flag / counter arms.
        aux: dict(fstate, wait_ticks_left, wait_prev[, ent_rot, target_dir][, range_in]) or None.  Returns a dict of the
        outputs (state, flags, gate, new_pos_xz, vel_xz, wait_ticks_left[, surround_dest_xz with aux["surround"]]).
        interp: (movestate.next_pos xz, movestate.step) at a rate below 20 Hz."""
        w, keep = self._world(arrays, hz, work)
        n = w.n_ents
        pi = StatePassIn()
        k = _fill_gate(pi.gate, n, next_rot, new_vel_xz, vdes_xz, interp)
        k += _fill_state(pi.state, flock_layer, flock_nearest_xz, flock_tiles, skip)
        res = {"state": np.zeros(n, np.uint8), "flags": np.zeros(n, np.uint8), "gate": np.zeros(n, np.uint8),
               "new_pos_xz": np.zeros((n, 2), np.float32), "vel_xz": np.zeros((n, 2), np.float32),
               "wait_ticks_left": np.zeros(n, np.int32)}
        po = StatePassOut()
        _point(po, **res)
        if aux is not None:
            arms, su_out = _fill_aux(pi.aux, n, aux["fstate"], aux["wait_ticks_left"], aux["wait_prev"], aux.get("ent_rot"),
                                     aux.get("target_dir"), aux.get("range_in"), aux.get("surround"))
            k += arms
            if su_out is not None:
                res["surround_dest_xz"] = su_out
        self._call("navhip_state_pass", C.byref(w), C.byref(pi), C.byref(po))
        return res

    def settled_count(self, arrays, uids):
        """adjacent_settled_count (movement.c:982) for the units `uids` of the snapshot `arrays` (pos_xz, radius,
        flags, state); -1 = the host counts (radius > 12.5)."""
        w, keep = self._world(arrays)
        u = _arr(uids, np.int32)
        out = np.zeros(len(u), np.int32)
        self._call("navhip_settled_count", C.byref(w), len(u), _hp(u), _hp(out))
        return out

    def arrival_settle(self, arrays, zones, region_keys, units):
        """G_Arrival_ShouldSettle (arrival.c:946).  zones: list of dicts (layer, centre_xz, radius, unit_radius,
        fill_frac, active_row, num_rows, slots_xz, slot_ring), region_keys: list of sorted u64 arrays per zone;
        units: dict of nq-row arrays (uid, zone, new_pos_xz, nsettled, substate, sink_valid, sink_xz, order_pos_xz,
        progress_anchor_xz, progress_anchored, stuck).  Returns (settle [nq], dict of the unit state after)."""
        w, keep = self._world(arrays)
        zs, slots_cat, ring_cat, keys_cat = _pack_zones(zones, region_keys)
        nq = len(units["uid"])
        spec = (("uid", np.int32, 1), ("zone", np.int32, 1), ("new_pos_xz", np.float32, 2), ("nsettled", np.int32, 1),
                ("substate", np.uint8, 1), ("sink_valid", np.uint8, 1), ("sink_xz", np.float32, 2),
                ("order_pos_xz", np.float32, 2), ("progress_anchor_xz", np.float32, 2), ("progress_anchored", np.uint8, 1),
                ("stuck", np.int32, 1))
        si = SettleIn()
        si.n_zones, si.nq = len(zones), nq
        si.zones = C.addressof(zs)
        k = _point(si, slots_xz=slots_cat, slot_ring=ring_cat, region_keys=keys_cat)
        k += _point(si, **{name: _arr(units[name], dt, *((nq, width) if width > 1 else (nq,))) for name, dt, width in spec})
        res = {"settle": np.zeros(nq, np.uint8), "substate": np.zeros(nq, np.uint8),
               "progress_anchor_xz": np.zeros((nq, 2), np.float32), "progress_anchored": np.zeros(nq, np.uint8),
               "stuck": np.zeros(nq, np.int32)}
        so_ = SettleOut()
        _point(so_, **res)
        self._call("navhip_arrival_settle", C.byref(w), C.byref(si), C.byref(so_))
        settle = res.pop("settle")
        return settle, res

    # the per-unit members of navhip_arrival_vel_in / _out: (name, element type, width)
    _AV_IN = (("uid", np.int32, 1), ("zone", np.int32, 1), ("has_dest_los", np.uint8, 1), ("substate", np.uint8, 1),
              ("sink_valid", np.uint8, 1), ("sink_xz", np.float32, 2), ("los_latched", np.uint8, 1), ("los_hyst", np.int32, 1))
    _AV_OUT = (("vdes_xz", np.float32, 2), ("status", np.uint8, 1), ("substate", np.uint8, 1), ("sink_valid", np.uint8, 1),
               ("sink_xz", np.float32, 2), ("los_latched", np.uint8, 1), ("los_hyst", np.int32, 1))

    def arrival_velocity(self, arrays, zones, region_keys, units, zone_row=None, com_row=None, patch=None):
        """G_Arrival_DesiredVelocity (arrival.c:862) for units of filling zones, host buffers.  arrays: the world (pos_xz;
        flock_field_slot / region_field_slot / field_pool, or use_resident_pool); zones, region_keys: as for
        arrival_settle; zone_row / com_row: [n_zones] mapping rows (default: none); units: dict of nq-row arrays (uid, zone,
        has_dest_los, substate, sink_valid, sink_xz, los_latched, los_hyst).  patch: a function of (ArrivalVelIn,
        ArrivalVelOut, zones array) that may damage the call before it is made (argument-error tests).  Returns the dict
        of outputs (vdes_xz, status and the unit state after the call)."""
        w, keep = self._world(arrays)
        w.n_flocks = 0 if arrays.get("flock_field_slot") is None else len(arrays["flock_field_slot"])
        if arrays.get("field_pool") is None and arrays.get("use_resident_pool"):
            w.n_field_slots = POOL_RESIDENT
        zs, slots, ring, keys = _pack_zones(zones, region_keys)
        nz, nq = len(zones), len(units["uid"])
        none = np.full(max(nz, 1), -1, np.int32)
        vi = ArrivalVelIn()
        vi.n_zones, vi.nq, vi.n_slots, vi.n_keys = nz, nq, len(ring) - 1, len(keys) - 1
        vi.zones = C.addressof(zs)
        k = _point(vi, slots_xz=slots, slot_ring=ring, region_keys=keys,
                   zone_row=none if zone_row is None else _arr(zone_row, np.int32, nz),
                   com_row=none if com_row is None else _arr(com_row, np.int32, nz))
        k += _point(vi, **{name: _arr(units[name], dt, *((nq, width) if width > 1 else (nq,))) for name, dt, width in self._AV_IN})
        res = {name: np.zeros((nq, width) if width > 1 else (nq,), dt) for name, dt, width in self._AV_OUT}
        vo = ArrivalVelOut()
        _point(vo, **res)
        if patch is not None:
            patch(vi, vo, zs)
        self._call("navhip_arrival_velocity", C.byref(w), C.byref(vi), C.byref(vo))
        return res

    def arrival_velocity_dev(self, world, vel_in, vel_out, stream=None):
        """navhip_arrival_velocity_dev: a World, an ArrivalVelIn and an ArrivalVelOut of device pointers; asynchronous."""
        self._call("navhip_arrival_velocity_dev", C.byref(world), C.byref(vel_in), C.byref(vel_out), _stream(stream))

    # the members of navhip_arrival_flock a caller gives per zone, and the per-member arrays: (name, element type, width)
    _AF_FLOCK = ("phase", "realloc_counter", "stall_counter", "prev_occ", "row_height", "unit_radius", "total_members", "layer")
    _AF_IN = (("uid", np.int32, 1), ("settled", np.uint8, 1), ("substate", np.uint8, 1), ("sink_valid", np.uint8, 1),
              ("sink_xz", np.float32, 2))
    _AF_OUT = (("substate", np.uint8, 1), ("sink_valid", np.uint8, 1), ("sink_xz", np.float32, 2))

    def arrival_flock_update(self, arrays, zones, region_keys, members, patch=None):
        """The built-zone branch of G_Arrival_UpdateFlock (arrival.c:767) for a batch of zones, host buffers.  arrays: the
        world (pos_xz); zones: dicts as for arrival_settle plus phase, realloc_counter, stall_counter, prev_occ, row_height,
        and the call's arguments as arg_unit_radius, arg_total_members, arg_layer; region_keys: per zone a sorted u64
        array; members: per zone a dict of its member rows in the reference's order (uid, settled, substate, sink_valid,
        sink_xz).  patch: a function of (ArrivalFlockIn, ArrivalFlockOut, zones array, flocks array) that may damage the
        call before it is made.  Returns (zones after the call as dicts of the members that can change, per-zone lists of
        the member outputs, status [n_zones])."""
        w, keep = self._world(arrays)
        zs, slots, ring, keys = _pack_zones(zones, region_keys)
        fs, cat = pack_flocks(zones, members)
        nz, nm = len(zones), len(cat["uid"]) - 1
        fi = ArrivalFlockIn()
        fi.n_zones, fi.nm, fi.n_slots, fi.n_keys = nz, nm, len(ring) - 1, len(keys) - 1
        fi.zones, fi.flocks = C.addressof(zs), C.addressof(fs)
        k = _point(fi, slots_xz=slots, slot_ring=ring, region_keys=keys, **cat)
        zs_out, fs_out = (ArrivalZone * max(1, nz))(), (ArrivalFlock * max(1, nz))()
        res = {name: np.zeros((nm + 1, width) if width > 1 else (nm + 1,), dt) for name, dt, width in self._AF_OUT}
        res["slot_ring"], res["status"] = np.zeros(len(ring), np.int32), np.zeros(max(1, nz), np.uint8)
        fo = ArrivalFlockOut()
        fo.zones, fo.flocks = C.addressof(zs_out), C.addressof(fs_out)
        _point(fo, **res)
        if patch is not None:
            patch(fi, fo, zs, fs)
        self._call("navhip_arrival_flock_update", C.byref(w), C.byref(fi), C.byref(fo))
        return unpack_flocks(zs_out, fs_out, res, nz)

    def arrival_flock_update_dev(self, world, flock_in, flock_out, stream=None):
        """navhip_arrival_flock_update_dev: a World, an ArrivalFlockIn and an ArrivalFlockOut of device pointers; asynchronous."""
        self._call("navhip_arrival_flock_update_dev", C.byref(world), C.byref(flock_in), C.byref(flock_out), _stream(stream))

    def arrival_zone_build(self, arrays, zones, members, targets, patch=None):
        """The first build of G_Arrival_UpdateFlock (arrival.c:784-848) for a batch of INACTIVE zones, host buffers.
        arrays: the world (pos_xz); zones: dicts as for arrival_flock_update whose slots_xz / slot_ring and whose entry of
        `keys` (a u64 array under "room_keys") are the zone's ROOM and what it holds now; members: per zone a dict of its
        member rows; targets: [n_zones][2].  patch: as for arrival_flock_update.  Returns a dict: zs / fs (the two tables
        after the call), slots_xz, slot_ring, region_keys (the shared arrays), axis_xz, com_xz, com_dest_id, substate,
        sink_valid, sink_xz, status."""
        w, keep = self._world(arrays)
        zs, slots, ring, keys = _pack_zones(zones, [z["room_keys"] for z in zones])
        fs, cat = pack_flocks(zones, members)
        nz, nm = len(zones), len(cat["uid"]) - 1
        bi = ArrivalBuildIn()
        bi.n_zones, bi.nm, bi.n_slots, bi.n_keys = nz, nm, len(ring) - 1, len(keys) - 1
        bi.zones, bi.flocks = C.addressof(zs), C.addressof(fs)
        tgt = np.ascontiguousarray(np.concatenate([np.asarray(targets, np.float32).reshape(-1, 2), np.zeros((1, 2), np.float32)]))
        k = _point(bi, slots_xz=slots, slot_ring=ring, region_keys=keys, target_xz=tgt, **cat)
        zs_out, fs_out = (ArrivalZone * max(1, nz))(), (ArrivalFlock * max(1, nz))()
        res = {name: np.zeros((nm + 1, width) if width > 1 else (nm + 1,), dt) for name, dt, width in self._AF_OUT}
        res.update(slots_xz=np.full(slots.shape, -7.0, np.float32), slot_ring=np.full(ring.shape, -7, np.int32),
                   region_keys=np.full(keys.shape, 7, np.uint64), axis_xz=np.full((nz + 1, 2), -7.0, np.float32),
                   com_xz=np.full((nz + 1, 2), -7.0, np.float32), com_dest_id=np.full(nz + 1, 7, np.uint32),
                   status=np.full(max(1, nz), 0x55, np.uint8))
        bo = ArrivalBuildOut()
        bo.zones, bo.flocks = C.addressof(zs_out), C.addressof(fs_out)
        _point(bo, **res)
        if patch is not None:
            patch(bi, bo, zs, fs)
        self._call("navhip_arrival_zone_build", C.byref(w), C.byref(bi), C.byref(bo))
        return dict(res, zs=zs_out, fs=fs_out)

    def arrival_zone_build_dev(self, world, build_in, build_out, stream=None):
        """navhip_arrival_zone_build_dev: a World, an ArrivalBuildIn and an ArrivalBuildOut of device pointers; asynchronous."""
        self._call("navhip_arrival_zone_build_dev", C.byref(world), C.byref(build_in), C.byref(build_out), _stream(stream))

    # -- pool_api: the resident field pool --------------------------------------------------------------
    def pool_create(self, n_slots, n_dests):
        self._call("navhip_pool_create", n_slots, n_dests)

    def pool_build(self, reqs, ff_ids=None, base_ids=None, readback=True):
        """Batched N_FlowFieldInit + N_FlowFieldUpdate + N_FC_PutFlowField into the resident pool; ids
        default to N_FlowFieldID of every request.  Returns (ids, dirs [n,64,64] | None)."""
        reqs = _arr(reqs, FIELD_REQ_DTYPE)
        n = len(reqs)
        ids = _ids_of(reqs) if ff_ids is None else _arr(ff_ids, np.uint64)
        out = np.zeros((n, 64, 64), np.uint8) if readback else None
        self._call("navhip_pool_build", _hp(reqs), _hp(ids), _opt(_arr(base_ids, np.uint64)), n, _opt(out))
        return ids, out

    def pool_put(self, ff_id, dirs):
        self._call("navhip_pool_put", int(ff_id), _hp(_arr(dirs, np.uint8, 4096)))

    def pool_get(self, ff_id):
        d = np.zeros((64, 64), np.uint8)
        rc = lib().navhip_pool_get(self._h, int(ff_id), _hp(d))
        return None if rc != OK else d

    def pool_contains(self, ff_id):
        return bool(lib().navhip_pool_contains(self._h, int(ff_id)))

    def pool_invalidate(self, ff_id):
        self._call("navhip_pool_invalidate", int(ff_id))

    def pool_map(self, dest, chunk_r, chunk_c, ff_ids):
        d = _arr(dest, np.int32)
        self._call("navhip_pool_map", len(d), _hp(d), _hp(_arr(chunk_r, np.uint16)), _hp(_arr(chunk_c, np.uint16)),
                   _hp(_arr(ff_ids, np.uint64)))

    # -- submit_api: the asynchronous host-buffer step --------------------------------------------------
    def agent_step_async(self, arrays, hz=20, work=None, want=("vel_xz", "new_pos_xz", "status"), spin=None):
        """navhip_agent_step_submit + _poll: returns the outputs once the step has completed; `spin`
        is called while it is still running (what the nav task does between submit and join)."""
        w, keep = self._world(arrays, hz, work)
        if arrays.get("field_pool") is None and arrays.get("use_resident_pool"):
            w.n_field_slots = POOL_RESIDENT
        so, out = _step_out(w.n_ents, want)
        self._call("navhip_agent_step_submit", C.byref(w), C.byref(so))
        polls = 0
        while True:
            rc = lib().navhip_agent_step_poll(self._h)
            if rc == 0:
                break
            if rc < 0:
                self._chk(rc, "navhip_agent_step_poll")
            polls += 1
            if spin:
                spin()
        out["polls"] = polls
        return out

    # -- stream_set: the library's streams ----------------------------------------------------------------
    def stream_create_partial(self, cu_begin, cu_count):
        """A hipStream_t value restricted to the compute units [cu_begin, cu_begin + cu_count)."""
        out = C.c_void_p()
        self._call("navhip_stream_create_partial", cu_begin, cu_count, C.byref(out))
        return out.value

    def stream_beside(self, main_stream, cu_begin=0, cu_count=0):
        """navhip_stream_beside: the library's stream for wide work beside a step on `main_stream` (a hipStream_t value);
        cu_count > 0 restricts it to the compute units [cu_begin, cu_begin + cu_count)."""
        out = C.c_void_p()
        self._call("navhip_stream_beside", C.c_void_p(main_stream), cu_begin, cu_count, C.byref(out))
        return out.value

    def stream_main(self):
        """navhip_stream_main: the library's own stream for the agent chain (a hipStream_t value)."""
        out = C.c_void_p()
        self._call("navhip_stream_main", C.byref(out))
        return out.value

    # -- comm_api: the slab exchange between ranks ---------------------------------------------------------
    def comm_init(self, rank, world, uid):
        """navhip_comm_init: this context joins the RCCL communicator named by `uid` (comm_unique_id())."""
        self._call("navhip_comm_init", int(rank), int(world), (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid))

    def comm_init_mailbox(self, rank, world, d_mailbox):
        """navhip_comm_init_mailbox: the exchange step over a device buffer instead of RCCL (bring-up, tests)."""
        self._call("navhip_comm_init_mailbox", int(rank), int(world), dev_ptr(d_mailbox),
                   int(d_mailbox.numel() * d_mailbox.element_size()))

    def comm_destroy(self):
        return lib().navhip_comm_destroy(self._h)

    def comm_world(self):
        return int(lib().navhip_comm_world(self._h))

    def comm_allgather_step_dev(self, d_new_pos, d_vel, bounds, stream=None):
        self._call("navhip_comm_allgather_step_dev", dev_ptr(d_new_pos), dev_ptr(d_vel), _hp(_arr(bounds, np.int32)),
                   _stream(stream))

    def comm_allgather_rows_dev(self, d_rows, row_bytes, bounds, stream=None):
        self._call("navhip_comm_allgather_rows_dev", dev_ptr(d_rows), int(row_bytes), _hp(_arr(bounds, np.int32)),
                   _stream(stream))

    # -- los_chain_api: resident LOS chains (see LosChain) ---------------------------------------------
    def los_chain_create(self, reqs, prev_slot, d_pool):
        return LosChain(self, reqs, prev_slot, d_pool)

    def los_chain_build(self, chain, stream=None):
        return chain.build(stream)

    def los_chain_refresh(self, chain, flags=0, stream=None):
        return chain.refresh(flags, stream)

    def los_chain_stats(self, chain):
        return chain.stats()


class LosChain(_Handle):
    """One navhip_los_chain over `d_pool` (a [n][4096] u8 device tensor, the caller's: navhip_world.los_pool).  reqs:
    LOS_REQ_DTYPE in level order, prev_slot: the slot of every request's predecessor, -1 for a destination chunk."""
    _destroy = "navhip_los_chain_destroy"

    def __init__(self, ctx, reqs, prev_slot, d_pool):
        reqs = _arr(reqs, LOS_REQ_DTYPE)
        prev_slot = _arr(prev_slot, np.int32)
        assert len(prev_slot) == len(reqs) and int(d_pool.shape[0]) >= len(reqs)
        self.ctx, self._keep = ctx, d_pool
        self._h = C.c_void_p()
        ctx._call("navhip_los_chain_create", _hp(reqs), _hp(prev_slot), len(reqs), dev_ptr(d_pool), *ctx.map_pos(),
                  C.byref(self._h))

    def build(self, stream=None):
        self._call("navhip_los_chain_build", _stream(stream))

    def refresh(self, flags=0, stream=None):
        self._call("navhip_los_chain_refresh", flags, _stream(stream))

    def stats(self):
        out = LosChainStats()
        self._call("navhip_los_chain_get_stats", C.byref(out))
        return out


class Tick(_Handle):
    """One navhip_tick: the per-tick loop of a device-resident world inside the library (the reference's
    navigation_tick_task, movement.c:4263).  `desc` is a filled TickDesc; `keep` whatever owns the device arrays."""
    _destroy = "navhip_tick_destroy"

    def __init__(self, ctx, desc, keep=None):
        self.ctx, self._keep = ctx, (keep, desc)
        self._h = C.c_void_p()
        ctx._call("navhip_tick_create", C.byref(desc), C.byref(self._h))
        self._run = lib().navhip_tick_run

    def run(self, n=1):
        # (the one wrapper on the per-tick path of the default driver: a bound function, no helper unless it fails)
        rc = self._run(self._h, n)
        if rc != OK:
            self._chk(rc, "navhip_tick_run")

    def compute(self):
        self._call("navhip_tick_compute")

    def advance(self):
        self._call("navhip_tick_advance")

    def set_los_chain(self, chain, flags=0):
        """The LosChain every tick with a blocker batch refreshes behind it (None: none)."""
        self._chain = chain
        self._call("navhip_tick_set_los_chain", chain._h if chain is not None else None, flags)

    def sync(self):
        self._call("navhip_tick_sync")

    def info(self):
        out = TickInfo()
        self._call("navhip_tick_get_info", C.byref(out))
        return out
