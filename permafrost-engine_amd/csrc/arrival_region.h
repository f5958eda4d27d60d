// arrival_region.h -- what the arrival overlay's kernels share about a zone's footprint, device only: td_key, the binary
// searches over the sorted region_keys, N_SegmentWithinRegion over the supercover walk, arrival_in_region, and
// arrival_zone_radius.  Used by state_kernels.hip (k_arrival_settle, k_arrival_velocity), arrival_flock_kernels.hip
// (k_arrival_flock) and arrival_build_kernels.hip (k_arrival_build); every function here was moved from the first two
// unchanged.  Free of device variables, so any unit may include it.
#pragma once
#include "navhip_internal.h"
#include "agent_internal.h"
#include "agent_math.h"

__device__ __forceinline__ uint64_t sk_key(const tiledesc &t)              // td_key, nav.c:207
{
    return ((uint64_t)t.chunk_r << 48) | ((uint64_t)t.chunk_c << 32) | ((uint64_t)t.tile_r << 16) | (uint64_t)t.tile_c;
}

__device__ inline bool sk_keys_contain(const uint64_t *keys, int num, uint64_t k)   // region_keys_contain, nav.c:4283
{
    int lo = 0, hi = num;
    while(lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const uint64_t v = keys[mid];
        if(v == k) return true;
        if(v < k) lo = mid + 1; else hi = mid;
    }
    return false;
}

// N_SegmentWithinRegion (nav.c:4326): every tile of the supercover walk from a to b (tile.c:430, both ends
// inside the map, so the walk starts at a) is a key of the region.  The walk's floats are the reference's:
// PFM_Vec2_Normal of the direction, fabs() promoting the t_max quotients to double before they are stored in a
// float, M_Tile_Bounds as (map - chunk * 256) - tile * 4.  a == b gives NaN everywhere and one tile, as there.
__device__ inline bool sk_segment_within(const nh_step_params &P, v2 a, v2 b, const uint64_t *keys, int num)
{
    if(num == 0) return false;
    tiledesc ta, tb;
    if(!tile_for_point(P, a.x, a.z, ta) || !tile_for_point(P, b.x, b.z, tb)) return false;
    const int ar = ta.chunk_r * 64 + ta.tile_r, ac = ta.chunk_c * 64 + ta.tile_c;
    const int br = tb.chunk_r * 64 + tb.tile_r, bc = tb.chunk_c * 64 + tb.tile_c;
    const int maxout = abs(br - ar) + abs(bc - ac) + 2;
    v2 dir = mkv(b.x - a.x, b.z - a.z);
    const float len = vlen(dir);
    dir = mkv(dir.x / len, dir.z / len);
    const int step_c = dir.x <= 0.0f ? 1 : -1, step_r = dir.z >= 0.0f ? 1 : -1;
    const float t_delta_x = fabsf(4.0f / dir.x), t_delta_z = fabsf(4.0f / dir.z);
    const float bx = (P.map_x - (float)(ta.chunk_c * 256)) - (float)(ta.tile_c * 4);
    const float bz = (P.map_z + (float)(ta.chunk_r * 256)) + (float)(ta.tile_r * 4);
    float t_max_x = (float)((step_c > 0 ? fabs((double)(a.x - (bx - 4.0f))) : fabs((double)(a.x - bx))) / fabs((double)dir.x));
    float t_max_z = (float)((step_r > 0 ? fabs((double)(a.z - (bz + 4.0f))) : fabs((double)(a.z - bz))) / fabs((double)dir.z));
    int r = ar, c = ac;
    const int max_r = P.map.h * 64, max_c = P.map.w * 64;
    for(int n = 0; n < maxout; n++) {
        tiledesc t;
        t.chunk_r = r >> 6; t.chunk_c = c >> 6; t.tile_r = r & 63; t.tile_c = c & 63;
        if(!sk_keys_contain(keys, num, sk_key(t))) return false;
        int dc = 0, dr = 0;
        if(t_max_x < t_max_z) { t_max_x = t_max_x + t_delta_x; dc = step_c; }
        else                  { t_max_z = t_max_z + t_delta_z; dr = step_r; }
        if(r == br && c == bc) break;
        r += dr; c += dc;
        if(r < 0 || r >= max_r || c < 0 || c >= max_c) break;             // M_Tile_RelativeDesc
    }
    return true;
}

__device__ __forceinline__ bool sk_in_region(const nh_step_params &P, v2 p, const uint64_t *keys, int num)
{
    // arrival_in_region (arrival.c:153): the walk from p to p is the tile of p
    tiledesc t;
    if(num == 0 || !tile_for_point(P, p.x, p.z, t)) return false;
    return sk_keys_contain(keys, num, sk_key(t));
}

__device__ __forceinline__ uint64_t af_key(int chunk_r, int chunk_c, int tile_r, int tile_c)    // td_key, nav.c:207
{
    return ((uint64_t)chunk_r << 48) | ((uint64_t)chunk_c << 32) | ((uint64_t)tile_r << 16) | (uint64_t)tile_c;
}

__device__ inline int af_key_index(const uint64_t *keys, int num, uint64_t k)     // region_key_index, nav.c:4369
{
    int lo = 0, hi = num;
    while(lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        const uint64_t v = keys[mid];
        if(v == k) return mid;
        if(v < k) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// arrival_zone_radius, arrival.c:363: `ntiles / M_PI` is a double, narrowed for sqrtf.  Host and device: the host forms
// check a zone's room with it before they launch (sqrtf there, the IEEE square root here: both correctly rounded).
#ifdef NH_HOSTSIM
#define AR_HOST_DEVICE
#else
#define AR_HOST_DEVICE __host__ __device__
#endif
AR_HOST_DEVICE inline int af_zone_radius(int nunits, float unit_radius)
{
    float per_unit = (1.85f * unit_radius) / 4.0f;                           // ARRIVAL_SLOT_SPACING, tile_dim
    per_unit *= per_unit;
    if(per_unit < 1.0f) per_unit = 1.0f;
    const float ntiles = (float)nunits * per_unit;
    const float narrowed = (float)((double)ntiles / 3.14159265358979323846);
#if defined(__HIP_DEVICE_COMPILE__) || defined(NH_HOSTSIM)
    const float root = nh_sqrt_ieee(narrowed);
#else
    const float root = sqrtf(narrowed);
#endif
    return (int)(uint16_t)(int)(ceilf(root) + 3.0f);                         // ARRIVAL_ZONE_PAD
}

// arrival_region_area, arrival.c:147: M_PI * radius * radius + 0.5f is a double; the cap before the cast (the same
// number wherever the reference's cast is defined)
AR_HOST_DEVICE inline int af_region_area(int radius)
{
    const double area = 3.14159265358979323846 * (double)radius * (double)radius + (double)0.5f;
    return area < 4096.0 ? (int)area : 4096;                                 // ARRIVAL_MAX_SLOTS
}
