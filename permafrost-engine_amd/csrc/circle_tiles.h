// circle_tiles.h -- the tile-under-circle test of M_Tile_AllUnderCircle (tile.c:687), device only: C_CircleRectIntersection
// (collision.c:997; C_PointInsideRect2D :756, C_LineCircleIntersection :960) against M_Tile_Bounds (tile.c:356) of a nav
// tile, expression by expression.  Shared by the units that rebuild a circle's tile set: blocker_kernels.hip (the tiles a
// blocker covers) and surround_query_kernels.hip (the tiles of a surround target and of the unit that surrounds it).  Free
// of device variables, so any unit may include it.
#pragma once

#define BLK_EPS 0.0009765625f      /* collision.c:64 EPSILON 1/1024 */

// PFM_Vec2_Len (pf_math.c:82): sqrt in double of a float sum == correctly rounded float sqrt
__device__ __forceinline__ float len2f(float x, float z) { return __builtin_sqrtf(x * x + z * z); }

// C_LineCircleIntersection, collision.c:960 (pow(.,2) and sqrt are double in the reference)
__device__ inline bool line_circle(float ax, float az, float bx, float bz, float cx, float cz, float radius)
{
    float dx = bx - ax, dz = bz - az;
    float A = (float)((double)dx * (double)dx + (double)dz * (double)dz);
    float B = 2 * (dx * (ax - cx) + dz * (az - cz));
    float fx = ax - cx, fz = az - cz;
    float C = (float)((double)fx * (double)fx + (double)fz * (double)fz - (double)radius * (double)radius);
    float det = (float)((double)B * (double)B - (double)(4 * A * C));
    float t;
    if(det < 0.0f || A < BLK_EPS) {
        return false;
    }else if(det == 0.0f) {
        t = __fdiv_rn(-B, 2 * A);
    }else{
        double sq = __builtin_sqrt((double)det);
        float t1 = (float)(((double)(-B) + sq) / (double)(2 * A));
        float t2 = (float)(((double)(-B) - sq) / (double)(2 * A));
        t = t1 < t2 ? t1 : t2;
    }
    return !(t < 0.0f || t > 1.0f);
}

// C_CircleRectIntersection (collision.c:997) against M_Tile_Bounds (tile.c:356) of the nav tile
// (abs_r, abs_c): box {x, z, 4, 4} with x decreasing to the right.  P: anything with the map's origin in map_x / map_z
template <class MAP> __device__ inline bool circle_hits_tile(const MAP &P, float cx, float cz, float radius,
                                                              int abs_r, int abs_c)
{
    const int chunk_r = abs_r >> 6, chunk_c = abs_c >> 6, tile_r = abs_r & 63, tile_c = abs_c & 63;
    const float x = (P.map_x - (float)(chunk_c * 256)) - (float)(tile_c * 4);
    const float z = (P.map_z + (float)(chunk_r * 256)) + (float)(tile_r * 4);
    const float wdt = 4.0f, hgt = 4.0f;
    const float qx[4] = {x - wdt, x, x, x - wdt};
    const float qz[4] = {z, z, z + hgt, z + hgt};
    // C_PointInsideRect2D(center, a, b, c, d), collision.c:756
    {
        float apx = cx - qx[0], apz = cz - qz[0];
        float abx = qx[1] - qx[0], abz = qz[1] - qz[0];
        float adx = qx[3] - qx[0], adz = qz[3] - qz[0];
        float ap_ab = apx * abx + apz * abz, ap_ad = apx * adx + apz * adz;
        if((ap_ab >= 0.0f && ap_ab <= abx * abx + abz * abz)
        && (ap_ad >= 0.0f && ap_ad <= adx * adx + adz * adz))
            return true;
    }
    for(int i = 0; i < 4; i++)
        if(len2f(qx[i] - cx, qz[i] - cz) <= radius) return true;
    for(int i = 0; i < 4; i++) {
        int j = (i + 1) & 3;
        if(line_circle(qx[i], qz[i], qx[j], qz[j], cx, cz, radius)) return true;
    }
    return false;
}
