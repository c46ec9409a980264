// raster.h -- the render contract's rasteriser (oracle/ro_render.c, operation by operation) and the stage that draws a mesh with it
// into an LDS window, in pieces.  Shared by the outlier test (k_render.hip), track quality and pose hypotheses (quality_body.h), VSD
// (k_vsd.hip), masks from poses (k_silhouette.hip) and the scene renderer (k_scene.hip); every translation unit that includes it is
// built with -ffp-contract=off.  The numerics of the outlier test's other render mode, ROFT_RENDER_GL, stand next to it in
// raster_gl.h; the LDS arithmetic of a launcher in raster_shape.h.
// THE DRAW CONTRACT, for a workgroup of kThreads threads whose threads all take every step:
//   1. box_reset(sh); barrier.
//   2. `project` = project_vertex with the pose and the intrinsics; project_mesh(.., sh.box, &sh.behind, project); barrier.
//      (Several boxes may be reset behind one barrier and filled behind one more.)
//   3. box = box_read(sh, w, h).  Nothing can be drawn unless box.drawable(): every vertex on one side of the target, or none in
//      front of the near plane -- the box is then as box_reset left it.  flips = cull_table(mesh.flip, sh.behind).
//   4. Per strip of the box's rows (strip_rows: as many as the window holds, at least one; the launcher refuses a target whose row
//      does not fit): clear the window; barrier; draw_triangles(.., strip.js, strip.je, store); barrier; read the window; barrier
//      before the next strip clears it.  The stores are order-free atomics, so a window's bits depend on the pose and the mesh only.
#pragma once

#include "raster_shape.h"
#include "roft_device.h"

namespace roft {

constexpr uint32_t kDepthEmpty = 0x7F800000u;   // +inf: the pixel of a depth window nothing was drawn into

// The mesh a kernel draws: `tris` in the order the caller wants triangle indices in, `flip` the bits of a closed mesh (mesh_class.h:
// 1 = wound clockwise seen from outside) or nullptr: every triangle is drawn.
struct MeshView {
    const float* verts;
    const int32_t* tris;
    const uint8_t* flip;
    int n_verts, n_tris;
};
__host__ __device__ inline MeshView mesh_view(const ObjParams& p) { return MeshView{p.verts, p.tris, p.tri_flip, p.n_verts, p.n_tris}; }

// x y z, w x y z: false = the pose draws nothing (its triangles would fail raster_projected's own tests one by one)
__device__ __forceinline__ bool pose_is_finite(const double* pose7)
{
    bool finite = true;
    for (int i = 0; i < 7; ++i) finite = finite && (fabs(pose7[i]) < INFINITY);
    return finite;
}

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
// s_box / s_behind: a MeshBoxShared's fields, reset and read as the draw contract above says (box_reset, box_read below).
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
// (draw_triangles reads cull_code BEFORE the fetch, so that the flip table's load is in flight with the corners': read behind the fetch it
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

// ---- the box: what project_mesh leaves in LDS (the caller declares it __shared__), reset before and read behind the pass
struct MeshBoxShared { int box[4], behind; };   // box = {i0, j0, i1, j1}
__device__ __forceinline__ void box_reset(MeshBoxShared& sh)   // (the caller owes a barrier before project_mesh)
{
    if (threadIdx.x < 4) sh.box[threadIdx.x] = (threadIdx.x < 2) ? INT32_MAX : -1;
    if (threadIdx.x == 0) sh.behind = 0;
}
// The pixel box of everything that can be drawn: columns i0 .. i1, rows j0 .. j1 of the target.
struct MeshBox {
    int i0, j0, i1, j1;
    __device__ __forceinline__ int width() const { return i1 - i0 + 1; }
    __device__ __forceinline__ bool drawable() const { return i1 >= i0 && j1 >= j0 && i0 >= 0 && j0 >= 0; }
};
// (behind the barrier after project_mesh; the min takes back the empty lower bound w / h of a vertex right of or below the target)
__device__ __forceinline__ MeshBox box_read(const MeshBoxShared& sh, int w, int h)
{
    return MeshBox{min(sh.box[0], w - 1), min(sh.box[1], h - 1), sh.box[2], sh.box[3]};
}

// ---- the window.  One strip of a box: columns i0 .. i1 (win_w of them), rows js .. je, npx pixels, row-major: pixel i of the
// strip is (i0 + i % win_w, js + i / win_w).
struct Strip { int i0, i1, js, je, win_w, npx; };
// rows of a strip when the window holds win_cap pixels and the box is win_w wide (win_cap >= win_w: the launcher's refusal)
__device__ __forceinline__ int strip_rows(int win_cap, int win_w) { return max(1, win_cap / win_w); }
// the strip of `rows` rows that begins at row js of the box
__device__ __forceinline__ Strip strip_from(const MeshBox& b, int js, int rows)
{
    const int je = min(b.j1, js + rows - 1), win_w = b.width();
    return Strip{b.i0, b.i1, js, je, win_w, win_w * (je - js + 1)};
}
// strip k of a box cut into runs of cw columns x strips of `rows` rows, n_cols runs side by side (a row wider than the window)
__device__ __forceinline__ Strip strip_at(const MeshBox& b, int cw, int rows, int n_cols, int k)
{
    const int is = b.i0 + (k % n_cols) * cw, js = b.j0 + (k / n_cols) * rows;
    return strip_from(MeshBox{is, js, min(b.i1, is + cw - 1), b.j1}, js, rows);
}
// The contract's window, in dynamic LDS: a pixel is the IEEE bits of its (positive) eye-space depth -- positive floats order like
// their bits --, kDepthEmpty where nothing was drawn.  clear / the stores / the reads each need a barrier between them.
struct DepthWindow {
    uint32_t* z;   // [win_cap]
    __device__ __forceinline__ void clear(int npx, int threads) const { for (int i = threadIdx.x; i < npx; i += threads) z[i] = kDepthEmpty; }
    // order-free minimum of the depth bits: raster_projected's `store(i, j, z)` and, the index unused, draw_triangles' `store(i, j, z, t)`
    __device__ __forceinline__ auto store(const Strip& s) const
    {
        ROFT_LDS uint32_t* const zw = pin_lds(z);
        const int i0 = s.i0, js = s.js, win_w = s.win_w;
        return [zw, i0, js, win_w](int i, int j, float depth, int /*t*/ = 0) {
            (void)__hip_atomic_fetch_min(zw + ((j - js) * win_w + (i - i0)), __float_as_uint(depth), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
    }
    __device__ __forceinline__ bool covered(int i) const { return z[i] != kDepthEmpty; }
    __device__ __forceinline__ float depth(int i, int, int) const { return __uint_as_float(z[i]); }
};

// ---- the triangles.  Every triangle of the mesh, thread-strided, onto rows j_lo .. j_hi of a w x h target: `store(i, j, z, t)`
// receives every covered pixel with its eye-space depth and the triangle's index.  s_v / cached / project: as project_mesh left and took them; flips:
// cull_table's.  Behind the barrier after the clear; the caller owes a barrier before anything reads what the stores wrote.
template <int kThreads, class Project, class Store>
__device__ __forceinline__ void draw_triangles(const MeshView& mesh, const float* s_v, bool cached, const uint8_t* flips, Project project,
                                               int w, int h, int j_lo, int j_hi, Store store)
{
    for (int t = threadIdx.x; t < mesh.n_tris; t += kThreads) {
        const int32_t* tri = mesh.tris + (size_t)3 * t;
        const int v0 = tri[0], v1 = tri[1], v2 = tri[2];
        const int cull = cull_code(flips, t);   // (before the fetch: see fetch_triangle)
        float x0, y0, z0, x1, y1, z1, x2, y2, z2;
        fetch_triangle(s_v, cached, mesh.verts, v0, v1, v2, project, x0, y0, z0, x1, y1, z1, x2, y2, z2);
        raster_projected(x0, y0, z0, x1, y1, z1, x2, y2, z2, w, h, j_lo, j_hi, cull, [&store, t](int i, int j, float z) { store(i, j, z, t); });
    }
}

// ---- the counts.  Integer counts of a workgroup's threads -> one LDS row per wave; behind a barrier of the caller's, rows_total
// adds the rows of count k (exact, so no figure depends on threads or waves).
template <int N>
__device__ __forceinline__ void wave_sums_to_rows(int (&cnt)[N], int (*s_rows)[N])
{
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) cnt[k] += __shfl_down(cnt[k], off, 64);
    }
#pragma unroll
    for (int k = 0; k < N; ++k)
        if ((threadIdx.x & 63) == 0) s_rows[threadIdx.x >> 6][k] = cnt[k];
}
template <int kThreads, int N>
__device__ __forceinline__ int rows_total(const int (*s_rows)[N], int k)
{
    int tot = 0;
    for (int w = 0; w < kThreads / 64; ++w) tot += s_rows[w][k];
    return tot;
}

}  // namespace roft
