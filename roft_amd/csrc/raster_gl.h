// raster_gl.h -- the numerics of the reference's OpenGL pipeline, render mode ROFT_RENDER_GL (RO_RENDER_GL of oracle/ro_render.c,
// operation by operation): vertex projection with a division per vertex, window z of a vertex and of a pixel centre, the 24-bit
// depth buffer's quantisation, the top-left coverage rule and the fragment shader's linearisation.
// Every triangle is drawn (depth test LESS, no culling: SICAD.cpp:271-272), window z is interpolated linearly in screen space
// (plane equation in double), quantised to the 24-bit depth buffer, the first fragment in the caller's triangle order wins a tie,
// and the fragment shader linearises the winner's window z in float (shader_model.frag:33-51).  Coverage follows the top-left rule.
// Used by the GL mode of the outlier test (outlier_fused_kernel<true>, k_render.hip); RenderPose and the mesh walk around the
// triangles are raster.h's, and like every translation unit that includes raster.h its users are built with -ffp-contract=off.
#pragma once

#include "raster.h"

namespace roft {

constexpr float kGlNear = 0.001f, kGlFar = 1000.0f;
constexpr uint32_t kGlDepthClear = 0xFFFFFFu;                                  // glClear: depth 1.0 in 24 bits
constexpr uint64_t kGlKeyClear = ((uint64_t)kGlDepthClear << 32) | 0xFFFFFFFFu;  // (qz << 32 | triangle): nothing drawn

// u = (fx X) / Z + cx: a division per vertex (the contract multiplies by one reciprocal)
__device__ __forceinline__ void project_vertex_gl(const float* v, const RenderPose& P, float fx, float fy, float cx,
                                                  float cy, float& sx, float& sy, float& z)
{
    const float X = ((P.R[0] * v[0] + P.R[1] * v[1]) + P.R[2] * v[2]) + P.t[0];
    const float Y = ((P.R[3] * v[0] + P.R[4] * v[1]) + P.R[5] * v[2]) + P.t[1];
    z = ((P.R[6] * v[0] + P.R[7] * v[1]) + P.R[8] * v[2]) + P.t[2];
    if (z > 0.001f) {
        sx = (fx * X) / z + cx;
        sy = (fy * Y) / z + cy;
    } else {
        sx = sy = 0.0f;
    }
}

// window z of a vertex at eye depth Z > near: the third row of the projection (SICAD.cpp:1634-1637), the perspective divide and the
// depth range [0, 1]
__device__ __forceinline__ float gl_vertex_window_z(float Z)
{
    const float gl_a = (kGlFar + kGlNear) / (kGlFar - kGlNear), gl_b = (2.0f * (kGlFar * kGlNear)) / (kGlFar - kGlNear);
    const float z_ndc = (gl_a * Z - gl_b) / Z;
    return 0.5f * z_ndc + 0.5f;
}

// window z of the pixel centre (px, py) inside the triangle: its plane equation in double, handed on as a float gl_FragCoord.z
__device__ __forceinline__ float gl_pixel_window_z(float x0, float y0, float x1, float y1, float x2, float y2, float zw0, float zw1,
                                                   float zw2, float px, float py)
{
    const double dw0 = ((double)x2 - x1) * ((double)py - y1) - ((double)y2 - y1) * ((double)px - x1);
    const double dw1 = ((double)x0 - x2) * ((double)py - y2) - ((double)y0 - y2) * ((double)px - x2);
    const double dw2 = ((double)x1 - x0) * ((double)py - y0) - ((double)y1 - y0) * ((double)px - x0);
    return (float)((dw0 * zw0 + dw1 * zw1 + dw2 * zw2) / (dw0 + dw1 + dw2));
}

// the fragment shader's output: eye-space depth of window z
__device__ __forceinline__ float gl_linear_depth(float z_w)
{
    const float zn = z_w * 2.0f - 1.0f;
    return (2.0f * kGlNear * kGlFar) / (kGlFar + kGlNear - zn * (kGlFar - kGlNear));
}

// raster_projected under the GL numerics: `store(i, j, qz)` receives every fragment that survives the depth range and can pass
// GL_LESS against a cleared buffer, with its quantised window z.  The vertices are projected by project_vertex_gl.
template <class Store>
__device__ __forceinline__ void raster_projected_gl(float x0, float y0, float z0, float x1, float y1, float z1, float x2, float y2,
                                                    float z2, int w, int h, int j_lo, int j_hi, Store store)
{
    if (!(z0 > 0.001f && z1 > 0.001f && z2 > 0.001f)) return;
    const float area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0);
    if (area == 0.0f || !(area == area)) return;
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
    // top-left rule: with the weights oriented so that the interior is w > 0, edge k is w_k = a_k px + b_k py + c_k; a centre ON
    // the edge is covered iff a_k > 0 (left edge) or a_k == 0 and b_k > 0 (top edge, image rows grow downwards)
    const float sgn = (area > 0.0f) ? 1.0f : -1.0f;
    const float ea0 = -sgn * (y2 - y1), ea1 = -sgn * (y0 - y2), ea2 = -sgn * (y1 - y0);
    const float eb0 = sgn * (x2 - x1), eb1 = sgn * (x0 - x2), eb2 = sgn * (x1 - x0);
    const bool own0 = (ea0 > 0.0f) || (ea0 == 0.0f && eb0 > 0.0f);
    const bool own1 = (ea1 > 0.0f) || (ea1 == 0.0f && eb1 > 0.0f);
    const bool own2 = (ea2 > 0.0f) || (ea2 == 0.0f && eb2 > 0.0f);
    const float zw0 = gl_vertex_window_z(z0), zw1 = gl_vertex_window_z(z1), zw2 = gl_vertex_window_z(z2);
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
            if ((w0 == 0.0f && !own0) || (w1 == 0.0f && !own1) || (w2 == 0.0f && !own2)) continue;
            const float z_w = gl_pixel_window_z(x0, y0, x1, y1, x2, y2, zw0, zw1, zw2, px, py);
            if (!(z_w >= 0.0f && z_w <= 1.0f)) continue;   // clipped by the depth range
            const uint32_t qz = (uint32_t)floor((double)z_w * 16777215.0 + 0.5);
            if (qz >= kGlDepthClear) continue;             // never less than the cleared buffer
            store(i, j, qz);
        }
    }
}

}  // namespace roft
