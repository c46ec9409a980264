// raster.h -- the render contract's rasteriser (oracle/ro_render.c, operation by operation): pose -> float rotation, vertex
// projection, scan conversion of one projected triangle -- and the mesh walk around it: the vertex pass (project_mesh), the corner
// fetch (fetch_triangle), the back-face rule's guard (cull_table / cull_code) and the LDS arithmetic of a launcher.  Shared by the
// outlier test (k_render.hip), track quality (k_quality.hip), masks from poses (k_silhouette.hip) and the scene renderer
// (k_scene.hip); every translation unit that includes it is built with -ffp-contract=off.  The numerics of the outlier test's other
// render mode, ROFT_RENDER_GL, stand next to it in raster_gl.h.
#pragma once

#include "roft_device.h"

namespace roft {

constexpr uint32_t kDepthEmpty = 0x7F800000u;   // +inf: the pixel of a depth window nothing was drawn into

// Dynamic LDS of a workgroup that draws a mesh: [the projected vertices, when they are cached] | [its window].
constexpr size_t kRasterLdsBudget = 160 * 1024 - 4096;   // what such a kernel may ask for (the rest: its static LDS)
__host__ __device__ constexpr size_t vertex_cache_bytes(int verts) { return ((size_t)verts * 12 + 15) & ~(size_t)15; }   // = the window's offset

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
// (cull_code below makes the code of triangle t from a mesh's flip table.)
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

// The back-face rule's guard: the flip table to cull with, or nullptr = every triangle is drawn.  Triangles that face away are
// left out only while the mesh is closed (it has a flip table) and all of it is in front of the near plane (`behind`: project_mesh's
// flag): with a vertex behind, the camera may be inside the surface, and what it sees there are back faces.
__device__ __forceinline__ const uint8_t* cull_table(const uint8_t* tri_flip, int behind)
{
    return (tri_flip && !behind) ? tri_flip : nullptr;
}

// raster_projected's `cull` for triangle t: 1 + its flip bit
__device__ __forceinline__ int cull_code(const uint8_t* flips, int t) { return flips ? 1 + (int)flips[t] : 0; }

// The vertex pass of a workgroup of kThreads threads that draws a mesh on a w x h target: every vertex goes through
// `project(const float* v, float& sx, float& sy, float& z)` -- project_vertex with the caller's pose and intrinsics --, is kept in
// s_v (3 floats per vertex) when `cached`, and widens s_box = {i0, j0, i1, j1}, the pixel box of everything that can be drawn;
// *s_behind is set when some vertex is not in front of the near plane (cull_table).  kVB: vertices per thread whose coordinates are
// fetched together.  kRowsOnly: the caller uses the rows of the box only (s_box[1], s_box[3]); the columns are left as it set them.
// Contract: the caller sets s_box = {INT32_MAX, INT32_MAX, -1, -1} and *s_behind = 0 behind a barrier, and puts a barrier after
// the call.  It then reads i0 = min(s_box[0], w - 1), i1 = s_box[2], j0 = min(s_box[1], h - 1), j1 = s_box[3]; nothing can be drawn
// when i1 < i0 or j1 < j0 (every vertex on one side of the target, or none in front: the box is untouched).
// Why the box of the VERTICES covers every triangle: raster_projected clips a triangle to ceil(min - 0.5) .. floor(max - 0.5)
// of its corners' coordinates, clamped to the target; both bounds are monotone in the coordinates, so a triangle's range lies
// between the smallest lower bound and the largest upper bound of its vertices, and only triangles with all three corners in
// front are drawn.  A vertex left of or above the target contributes the lower bound 0, one right of or below it the upper bound
// w - 1 / h - 1; its other bound is the empty one, -1 or w / h (hence (float)w against w - 1; the caller's min takes that back).
// A coordinate far off the target clamps the same way before the conversion (which would saturate anyway).  A NaN coordinate is
// dropped by fminf / fmaxf, which return their other operand: the vertex counts as one left of and above the target, and the
// rasteriser draws nothing of its triangles (NaN fails every comparison there).
template <int kThreads, int kVB, bool kRowsOnly = false, class Project>
__device__ __forceinline__ void project_mesh(const float* verts, int nv, bool cached, float* s_v, int w, int h, int* s_box,
                                             int* s_behind, Project project)
{
    const int tid = threadIdx.x;
    int bi0 = INT32_MAX, bj0 = INT32_MAX, bi1 = -1, bj1 = -1;
    bool behind = false;
    for (int vb = tid; vb < nv; vb += kVB * kThreads) {
        float vc[kVB][3];
#pragma unroll
        for (int k = 0; k < kVB; ++k) {
            const int v = min(vb + k * kThreads, nv - 1);
#pragma unroll
            for (int q = 0; q < 3; ++q) vc[k][q] = verts[(size_t)3 * v + q];
        }
#pragma unroll
        for (int k = 0; k < kVB; ++k) {
            const int v = vb + k * kThreads;
            if (v >= nv) break;
            float sx, sy, z;
            project(vc[k], sx, sy, z);
            if (cached) { s_v[3 * v] = sx; s_v[3 * v + 1] = sy; s_v[3 * v + 2] = z; }
            if (z > 0.001f) {
                if constexpr (!kRowsOnly) {
                    const float lo_i = fminf(fmaxf(ceilf(sx - 0.5f), 0.0f), (float)w), hi_i = fminf(fmaxf(floorf(sx - 0.5f), -1.0f), (float)(w - 1));
                    bi0 = min(bi0, (int)lo_i); bi1 = max(bi1, (int)hi_i);
                }
                const float lo_j = fminf(fmaxf(ceilf(sy - 0.5f), 0.0f), (float)h), hi_j = fminf(fmaxf(floorf(sy - 0.5f), -1.0f), (float)(h - 1));
                bj0 = min(bj0, (int)lo_j); bj1 = max(bj1, (int)hi_j);
            } else {
                behind = true;
            }
        }
    }
    if (__any(behind) && (tid & 63) == 0) atomicOr(s_behind, 1);
    for (int off = 32; off > 0; off >>= 1) {
        if constexpr (!kRowsOnly) { bi0 = min(bi0, __shfl_xor(bi0, off, 64)); bi1 = max(bi1, __shfl_xor(bi1, off, 64)); }
        bj0 = min(bj0, __shfl_xor(bj0, off, 64)); bj1 = max(bj1, __shfl_xor(bj1, off, 64));
    }
    if ((tid & 63) == 0) {
        if constexpr (!kRowsOnly) { atomicMin(&s_box[0], bi0); atomicMax(&s_box[2], bi1); }
        atomicMin(&s_box[1], bj0); atomicMax(&s_box[3], bj1);
    }
}

// project_mesh's two results -- the box and `behind` -- from the eight corners of the mesh's axis-aligned box instead of all its
// vertices.  Called by a whole wave; every lane holds corner (lane & 7) in `corner`.  True: no vertex of the mesh is behind the
// near plane (the caller leaves *s_behind 0) and box = {i0, j0, i1, j1}, in project_mesh's format, CONTAINS the box project_mesh
// would have found: the same triangles then leave the same depths at the same pixels, and the pixels this box adds stay empty.
// False: the corners do not settle it, the caller runs project_mesh.
// Why.  A vertex is a convex combination of the corners.  Its exact depth is affine in it, so at least the smallest exact corner
// depth; with all depths positive its exact screen coordinates lie between the corners' extremes (a perspective projection maps
// the box onto the convex hull of its projected corners).  The float values differ from the exact ones by rounding: the three-term
// sums of project_vertex err by less than 4e-7 x the sum of their terms' magnitudes, which for a vertex is at most the largest
// such sum `mag` among the corners (a sum of absolute values of affine functions is convex).  Hence
//   * behind: every float corner depth > 0.01 -- ten times the near plane -- and above 0.001 by more than 1e-6 mag (2 x 4e-7, rounded
//     up; far beyond 0.009 only for coordinates of tens of kilometres) => every float vertex depth > 0.001;
//   * box: a screen coordinate s = (f X) (1 / z) + c errs by less than px_err = 1e-6 (f (mag / z) (1 + mag / z) + |c|) (seven roundings,
//     each relative 6e-8, on X, z, the reciprocal, two products and the sum).  While px_err < 1/4 a vertex' float coordinate is no more
//     than half a pixel outside the float corners' range, and ceil(s - 1/2) / floor(s - 1/2) move by at most one: the corners'
//     bounds widened by one pixel, then clamped to the target as project_mesh clamps.
__device__ __forceinline__ bool corner_box_settles(const float* corner, const RenderPose& P, float fx, float fy, float cx, float cy, int w,
                                                   int h, int* box)
{
    float sx, sy, z;
    project_vertex(corner, P, fx, fy, cx, cy, sx, sy, z);
    float mag = 0.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
        mag = fmaxf(mag, ((fabsf(P.R[3 * r] * corner[0]) + fabsf(P.R[3 * r + 1] * corner[1])) + fabsf(P.R[3 * r + 2] * corner[2])) + fabsf(P.t[r]));
    float mag_max = mag, z_min = z;   // (fminf / fmaxf drop a NaN: the lane that holds it fails its own test below)
    for (int off = 1; off < 8; off <<= 1) {
        mag_max = fmaxf(mag_max, __shfl_xor(mag_max, off, 64));
        z_min = fminf(z_min, __shfl_xor(z_min, off, 64));
    }
    const float q = mag_max / z_min;
    const float px_err = 1e-6f * (fmaxf(fabsf(fx), fabsf(fy)) * q * (1.0f + q) + (fabsf(cx) + fabsf(cy)));
    const bool good = z > 0.01f && (z - 0.001f) > 1e-6f * mag_max && px_err < 0.25f && (mag == mag);
    if (!__all(good)) return false;
    int bi0 = (int)fminf(fmaxf(ceilf(sx - 0.5f) - 1.0f, 0.0f), (float)w), bi1 = (int)fminf(fmaxf(floorf(sx - 0.5f) + 1.0f, -1.0f), (float)(w - 1));
    int bj0 = (int)fminf(fmaxf(ceilf(sy - 0.5f) - 1.0f, 0.0f), (float)h), bj1 = (int)fminf(fmaxf(floorf(sy - 0.5f) + 1.0f, -1.0f), (float)(h - 1));
    for (int off = 1; off < 8; off <<= 1) {
        bi0 = min(bi0, __shfl_xor(bi0, off, 64)); bi1 = max(bi1, __shfl_xor(bi1, off, 64));
        bj0 = min(bj0, __shfl_xor(bj0, off, 64)); bj1 = max(bj1, __shfl_xor(bj1, off, 64));
    }
    box[0] = bi0; box[1] = bj0; box[2] = bi1; box[3] = bj1;
    return true;
}

// The projected corners of a triangle: from the cache project_mesh filled, else through `project` again.
// (Callers read cull_code BEFORE the fetch, so that the flip table's load is in flight with the corners': read behind the fetch it
//  cost quality_kernel and pose_silhouette_kernel 3 us of 135 per launch, docs/notebook.md.)
template <class Project>
__device__ __forceinline__ void fetch_triangle(const float* s_v, bool cached, const float* verts, int v0, int v1, int v2, Project project,
                                               float& x0, float& y0, float& z0, float& x1, float& y1, float& z1, float& x2, float& y2,
                                               float& z2)
{
    if (cached) {
        x0 = s_v[3 * v0]; y0 = s_v[3 * v0 + 1]; z0 = s_v[3 * v0 + 2];
        x1 = s_v[3 * v1]; y1 = s_v[3 * v1 + 1]; z1 = s_v[3 * v1 + 2];
        x2 = s_v[3 * v2]; y2 = s_v[3 * v2 + 1]; z2 = s_v[3 * v2 + 2];
    } else {
        project(verts + (size_t)3 * v0, x0, y0, z0);
        project(verts + (size_t)3 * v1, x1, y1, z1);
        project(verts + (size_t)3 * v2, x2, y2, z2);
    }
}

}  // namespace roft
