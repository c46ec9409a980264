// k_vsd.hip -- BOP's Visible Surface Discrepancy of pose pairs against depth images (gfx950; include/roft_engine.h, section 3i).
//
// One workgroup per (pose pair, part).  It projects the mesh at both poses for their pixel boxes, takes the boxes' union -- outside
// it both visibility masks are empty -- and cuts the union into strips of rows that fit two LDS depth windows.  Per strip it draws the
// estimated pose into one window and the reference pose into the other exactly as quality_kernel draws its one: raster_projected of
// raster.h, the back-face rule for closed meshes, atomicMin on the float bits -- so the windows hold, bit for bit, what
// roft_render_depth(.., divider 1) returns under the strip.  The rendered depths never leave the CU.  The projected vertices are kept
// in ONE LDS cache where the mesh fits: a strip draws first the pose the cache holds, then refills it for the other one (one vertex
// pass per strip), else every triangle projects its own corners.  Then the strip's pixels are walked row by row (consecutive lanes,
// consecutive pixels: the reads of the depth image are coalesced), only where something was drawn: distance images, the two masks
// and the 4 + n_taus counts in registers, reduced wave -> workgroup -> one integer atomic add per count into the pair's row.
// vsd_finish_kernel divides.  Every figure is a sum of integers: no row depends on strips, parts, threads or the launch.
// Built with -ffp-contract=off like every user of raster.h; the distance images are specified operation by operation in double.
#include <algorithm>

#include "raster.h"
#include "vsd.h"

namespace roft {

constexpr int kVsdThreads = 1024;

// BOP's depth_im_to_dist_im_fast for one pixel: a = (i - cx) / fx, b = (j - cy) / fy
__device__ __forceinline__ double vsd_dist(double a, double b, float depth)
{
    const double d = (double)depth, ad = a * d, bd = b * d;
    return sqrt((ad * ad + bd * bd) + d * d);
}

// BOP's visibility test (bop19) of a model distance m > 0 against the measured distance t
__device__ __forceinline__ bool vsd_visible(double m, double t, float delta)
{
    const float diff = (float)m - (float)t;
    return (t > 0.0 && diff <= delta) || t == 0.0;
}

__global__ __launch_bounds__(kVsdThreads) void vsd_kernel(VsdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_cnt[kVsdThreads / 64][kVsdCounts];
    __shared__ int s_box[2][4];
    __shared__ int s_behind[2];
    const int tid = threadIdx.x;
    const int part = (int)(blockIdx.x % (unsigned)a.parts), pair = (int)(blockIdx.x / (unsigned)a.parts);
    const int W = a.W, H = a.H, nv = a.mesh.n_verts, nt = a.mesh.n_tris;
    const bool cached = nv <= a.vcache_cap;
    float* s_v = reinterpret_cast<float*>(smem);
    uint32_t* const s_ze = reinterpret_cast<uint32_t*>(smem + vertex_cache_bytes(a.vcache_cap));   // the estimate's window
    uint32_t* const s_zg = s_ze + a.win_alloc;                                                     // the reference's
    const double* const pose_e = a.est + (size_t)pair * 7;
    const double* const pose_g = a.ref + (size_t)pair * 7;
    bool finite_e = true, finite_g = true;   // (uniform over the workgroup) a pose with a non-finite component draws nothing, as in the scene renderer
    for (int i = 0; i < 7; ++i) {
        finite_e = finite_e && (fabs(pose_e[i]) < INFINITY);
        finite_g = finite_g && (fabs(pose_g[i]) < INFINITY);
    }
    const RenderPose Pe = make_pose(pose_e, pose_e + 3), Pg = make_pose(pose_g, pose_g + 3);   // (not used when not finite)
    if (tid < 8) s_box[tid >> 2][tid & 3] = ((tid & 3) < 2) ? INT32_MAX : -1;
    if (tid < 2) s_behind[tid] = 0;
    __syncthreads();

    // vertices -> screen: the pixel box of everything either pose can draw; the cache is left with the estimate's vertices
    auto project_e = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, Pe, a.fx, a.fy, a.cx, a.cy, sx, sy, z); };
    auto project_g = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, Pg, a.fx, a.fy, a.cx, a.cy, sx, sy, z); };
    if (finite_g) project_mesh<kVsdThreads, 1>(a.mesh.verts, nv, false, s_v, W, H, s_box[1], &s_behind[1], project_g);
    if (finite_e) project_mesh<kVsdThreads, 1>(a.mesh.verts, nv, cached, s_v, W, H, s_box[0], &s_behind[0], project_e);
    __syncthreads();
    int holds = finite_e ? 0 : -1;   // the pose whose vertices the cache holds: 0 the estimate, 1 the reference
    int i0 = INT32_MAX, j0 = INT32_MAX, i1 = -1, j1 = -1;
    bool drawn_e, drawn_g;   // the pose can draw something on the target
    {
        const int bi0 = min(s_box[0][0], W - 1), bi1 = s_box[0][2], bj0 = min(s_box[0][1], H - 1), bj1 = s_box[0][3];
        drawn_e = finite_e && bi1 >= bi0 && bj1 >= bj0 && bi0 >= 0 && bj0 >= 0;
        if (drawn_e) { i0 = bi0; i1 = bi1; j0 = bj0; j1 = bj1; }
    }
    {
        const int bi0 = min(s_box[1][0], W - 1), bi1 = s_box[1][2], bj0 = min(s_box[1][1], H - 1), bj1 = s_box[1][3];
        drawn_g = finite_g && bi1 >= bi0 && bj1 >= bj0 && bi0 >= 0 && bj0 >= 0;
        if (drawn_g) { i0 = min(i0, bi0); i1 = max(i1, bi1); j0 = min(j0, bj0); j1 = max(j1, bj1); }
    }
    const uint8_t* const flips_e = cull_table(a.mesh.flip, s_behind[0]);
    const uint8_t* const flips_g = cull_table(a.mesh.flip, s_behind[1]);

    int cnt[kVsdCounts];
#pragma unroll
    for (int k = 0; k < kVsdCounts; ++k) cnt[k] = 0;

    if (drawn_e || drawn_g) {
        // (the launcher refuses targets wider than a window: a strip holds at least one row of any union)
        const int win_w = i1 - i0 + 1, rows = max(1, a.win_cap / win_w), n_strips = (j1 - j0 + rows) / rows;
        const float* depth = a.depth + (size_t)pair * a.depth_stride;
        for (int strip = part; strip < n_strips; strip += a.parts) {
            const int js = j0 + strip * rows, je = min(j1, js + rows - 1), npx = win_w * (je - js + 1);
            for (int i = tid; i < npx; i += kVsdThreads) { s_ze[i] = kDepthEmpty; s_zg[i] = kDepthEmpty; }
            __syncthreads();
            const int first = (cached && holds == 1) ? 1 : 0;
            for (int pass = 0; pass < 2; ++pass) {
                const int w = pass == 0 ? first : 1 - first;
                if (!(w ? drawn_g : drawn_e)) continue;   // (uniform)
                const RenderPose Pw = w ? Pg : Pe;
                if (cached && holds != w) {
                    __syncthreads();   // the other pose's triangles have read the cache
                    for (int v = tid; v < nv; v += kVsdThreads) {
                        float sx, sy, z;
                        project_vertex(a.mesh.verts + (size_t)3 * v, Pw, a.fx, a.fy, a.cx, a.cy, sx, sy, z);
                        s_v[3 * v] = sx; s_v[3 * v + 1] = sy; s_v[3 * v + 2] = z;
                    }
                    holds = w;
                    __syncthreads();
                }
                ROFT_LDS uint32_t* const zw = pin_lds(w ? s_zg : s_ze);
                auto store = [zw, i0, js, win_w](int i, int j, float z) {
                    (void)__hip_atomic_fetch_min(zw + ((j - js) * win_w + (i - i0)), __float_as_uint(z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                };
                auto project = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, Pw, a.fx, a.fy, a.cx, a.cy, sx, sy, z); };
                const uint8_t* const fl = w ? flips_g : flips_e;
                for (int t = tid; t < nt; t += kVsdThreads) {
                    const int32_t* tri = a.mesh.tris + (size_t)3 * t;
                    const int v0 = tri[0], v1 = tri[1], v2 = tri[2];
                    const int cull = cull_code(fl, t);
                    float x0, y0, z0, x1, y1, z1, x2, y2, z2;
                    fetch_triangle(s_v, cached, a.mesh.verts, v0, v1, v2, project, x0, y0, z0, x1, y1, z1, x2, y2, z2);
                    raster_projected(x0, y0, z0, x1, y1, z1, x2, y2, z2, W, H, js, je, cull, store);
                }
            }
            __syncthreads();
            // the strip's pixels, row by row; a pixel neither pose drew is in neither mask
            for (int idx = tid; idx < npx; idx += kVsdThreads) {
                const uint32_t be = s_ze[idx], bg = s_zg[idx];
                if (be == kDepthEmpty && bg == kDepthEmpty) continue;
                const int jj = idx / win_w, i = i0 + (idx - jj * win_w), j = js + jj;
                const double ca = ((double)i - a.dcx) / a.dfx, cb = ((double)j - a.dcy) / a.dfy;   // once per pixel, for T, G and E
                const double T = vsd_dist(ca, cb, depth[(size_t)j * W + i]);
                const double G = bg == kDepthEmpty ? 0.0 : vsd_dist(ca, cb, __uint_as_float(bg));
                const double E = be == kDepthEmpty ? 0.0 : vsd_dist(ca, cb, __uint_as_float(be));
                const bool vg = G > 0.0 && vsd_visible(G, T, a.delta);
                const bool ve = E > 0.0 && (vsd_visible(E, T, a.delta) || vg);
                if (!(vg || ve)) continue;
                cnt[0] += 1;
                cnt[2] += vg ? 1 : 0;
                cnt[3] += ve ? 1 : 0;
                if (vg && ve) {
                    cnt[1] += 1;
                    const double gap = fabs(G - E), c = a.diameter > 0.0 ? gap / a.diameter : gap;
#pragma unroll
                    for (int k = 0; k < kVsdMaxTaus; ++k)
                        if (k < a.n_taus && c >= a.taus[k]) cnt[4 + k] += 1;
                }
            }
            __syncthreads();   // the next strip clears the windows
        }
    }

    // wave -> workgroup -> the pair's row
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kVsdCounts; ++k) cnt[k] += __shfl_down(cnt[k], off, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kVsdCounts; ++k) s_cnt[tid >> 6][k] = cnt[k];
    }
    __syncthreads();
    if (tid < kVsdCounts) {
        int tot = 0;
        for (int w = 0; w < kVsdThreads / 64; ++w) tot += s_cnt[w][tid];
        if (tot) atomicAdd(&a.counts[(size_t)pair * kVsdCounts + tid], tot);
    }
}

// one thread per pair: the step cost over the pair's counts
__global__ void vsd_finish_kernel(const int32_t* counts, int n, int n_taus, double* errors, int32_t* rows)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int32_t* c = counts + (size_t)f * kVsdCounts;
    const int n_union = c[0], n_inter = c[1];
    int32_t* row = rows + (size_t)f * (4 + n_taus);
    for (int k = 0; k < 4; ++k) row[k] = c[k];
    for (int k = 0; k < n_taus; ++k) {
        row[4 + k] = c[4 + k];
        errors[(size_t)f * n_taus + k] = n_union > 0 ? (double)(c[4 + k] + n_union - n_inter) / (double)n_union : 1.0;
    }
}

// LDS of a workgroup: the projected vertices where they leave room for two windows of 4 k pixels, and two windows of at most 16 k
// pixels (an object of a tracked sequence covers a few tens of thousands of pixels at 640 x 480: a handful of strips).
bool vsd_shape(int n_verts, int width, int window_pixels, int& vcache_cap, int& win_alloc, int& win_cap, size_t& lds)
{
    const size_t budget = kRasterLdsBudget, vbytes = vertex_cache_bytes(n_verts);
    const bool cache = vbytes + 8 * (size_t)std::max(4096, width) <= budget;
    vcache_cap = cache ? n_verts : 0;
    const size_t room = (budget - (cache ? vbytes : 0)) / 8;   // pixels per window
    if ((size_t)width > room) return false;                    // not even one row of the target
    win_cap = (int)std::min<size_t>(room, (size_t)std::max(16384, width));
    lds = (cache ? vbytes : 0) + 8 * (size_t)win_cap;
    // (a smaller cap uses less of the same allocation: a strip of one row is at most `width` <= the allocation wide)
    win_alloc = win_cap;
    if (window_pixels > 0) win_cap = std::min(win_cap, window_pixels);
    return true;
}

void launch_vsd(const VsdArgs& a, int n, size_t lds, hipStream_t s)
{
    (void)set_max_dynamic_lds(reinterpret_cast<const void*>(vsd_kernel), (int)kRasterLdsBudget);
    hipLaunchKernelGGL(vsd_kernel, dim3((unsigned)n * (unsigned)a.parts), dim3(kVsdThreads), (uint32_t)lds, s, a);
}

void launch_vsd_finish(const int32_t* counts, int n, int n_taus, double* errors, int32_t* rows, hipStream_t s)
{
    hipLaunchKernelGGL(vsd_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, s, counts, n, n_taus, errors, rows);
}

}  // namespace roft
