// raster.h -- the render contract's rasteriser (oracle/ro_render.c, operation by operation): pose -> float rotation, vertex
// projection, scan conversion of one projected triangle.  Shared by the outlier test (k_render.hip) and the scene renderer
// (k_scene.hip); every translation unit that includes it is built with -ffp-contract=off.
#pragma once

#include "roft_device.h"

namespace roft {

struct RenderPose {
    float R[9];
    float t[3];
};

__device__ __forceinline__ RenderPose make_pose(const double* x, const double* q)
{
    RenderPose p;
    const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
    p.R[0] = (float)(1.0 - 2.0 * (qy * qy + qz * qz)); p.R[1] = (float)(2.0 * (qx * qy - w * qz)); p.R[2] = (float)(2.0 * (qx * qz + w * qy));
    p.R[3] = (float)(2.0 * (qx * qy + w * qz)); p.R[4] = (float)(1.0 - 2.0 * (qx * qx + qz * qz)); p.R[5] = (float)(2.0 * (qy * qz - w * qx));
    p.R[6] = (float)(2.0 * (qx * qz - w * qy)); p.R[7] = (float)(2.0 * (qy * qz + w * qx)); p.R[8] = (float)(1.0 - 2.0 * (qx * qx + qy * qy));
    for (int i = 0; i < 3; ++i) p.t[i] = (float)x[i];
    return p;
}

__device__ __forceinline__ void project_vertex(const float* v, const RenderPose& P, float fx, float fy, float cx,
                                               float cy, float& sx, float& sy, float& z)
{
    const float X = ((P.R[0] * v[0] + P.R[1] * v[1]) + P.R[2] * v[2]) + P.t[0];
    const float Y = ((P.R[3] * v[0] + P.R[4] * v[1]) + P.R[5] * v[2]) + P.t[1];
    z = ((P.R[6] * v[0] + P.R[7] * v[1]) + P.R[8] * v[2]) + P.t[2];
    if (z > 0.001f) {
        const float iz = 1.0f / z;   // (one reciprocal per vertex: the contract of oracle/ro_render.c)
        sx = (fx * X) * iz + cx;
        sy = (fy * Y) * iz + cy;
    } else {
        sx = sy = 0.0f;
    }
}

// Scan conversion of one projected triangle on a w x h target: `store(i, j, z)` receives every covered pixel with its
// eye-space depth (the render contract of oracle/ro_render.c, operation by operation); rows outside [j_lo, j_hi] are
// skipped (a strip of the target).  cull: 0 = draw; 1 / 2 = the mesh is a closed surface (mesh_class.h) and this triangle is
// wound counter-clockwise (1) / clockwise (2) seen from outside: it is drawn only if it faces the camera -- a counter-clockwise
// triangle that does has NEGATIVE screen area under the contract's projection (x right, y down, z forward).
// (The candidate pixels as ONE loop of columns x rows iterations instead of two nested ones -- rounds of a wave = its largest box
// instead of tallest x widest -- was measured in rounds 5 and 6, with and without the back-face rule: 15.6 against 15.0 us for the
// triangle phase, the compiler hoists the row terms of the edge functions out of the inner loop.  Nested it stays.)
template <class Store>
__device__ __forceinline__ void raster_projected(float x0, float y0, float z0, float x1, float y1, float z1, float x2, float y2,
                                                 float z2, int w, int h, int j_lo, int j_hi, int cull, Store store)
{
    if (!(z0 > 0.001f && z1 > 0.001f && z2 > 0.001f)) return;
    const float area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
    if (area == 0.0f || !(area == area)) return;
    if (cull && ((area < 0.0f) == (cull == 2))) return;   // faces away
    const float minx = fminf(x0, fminf(x1, x2)), maxx = fmaxf(x0, fmaxf(x1, x2));
    const float miny = fminf(y0, fminf(y1, y2)), maxy = fmaxf(y0, fmaxf(y1, y2));
    float fi0 = ceilf(minx - 0.5f), fi1 = floorf(maxx - 0.5f);
    float fj0 = ceilf(miny - 0.5f), fj1 = floorf(maxy - 0.5f);
    if (fi0 < 0.0f) fi0 = 0.0f;
    if (fj0 < 0.0f) fj0 = 0.0f;
    if (fi1 > (float)(w - 1)) fi1 = (float)(w - 1);
    if (fj1 > (float)(h - 1)) fj1 = (float)(h - 1);
    if (!(fi0 <= fi1) || !(fj0 <= fj1)) return;
    const int ia = (int)fi0, ib = (int)fi1, ja = max((int)fj0, j_lo), jb = min((int)fj1, j_hi);
    if (jb < ja) return;
    // perspective-correct depth of a covered pixel as ONE quotient (oracle/ro_render.c):
    //   z = area z0 z1 z2 / (w0 z1 z2 + w1 z0 z2 + w2 z0 z1)
    // -- five multiplications per triangle, three multiply-adds and a division per pixel; no reciprocal of a vertex depth, no
    // normalised barycentric weights (an IEEE division is ~10 instructions and the kernel is bound by instruction issue)
    const float p12 = z1 * z2, p02 = z0 * z2, p01 = z0 * z1;
    const float num = area * (z0 * p12);
    for (int j = ja; j <= jb; ++j) {
        const float py = (float)j + 0.5f;
        for (int i = ia; i <= ib; ++i) {
            const float px = (float)i + 0.5f;
            const float w0 = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1);
            const float w1 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2);
            const float w2 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0);
            const bool inside = (area > 0.0f) ? (w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f)
                                              : (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);
            if (!inside) continue;
            const float den = (w0 * p12 + w1 * p02) + w2 * p01;
            const float z = num / den;
            if (!(z > 0.0f)) continue;
            store(i, j, z);
        }
    }
}

}  // namespace roft
