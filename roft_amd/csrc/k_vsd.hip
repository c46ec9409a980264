// k_vsd.hip -- BOP's Visible Surface Discrepancy of pose pairs against depth images (gfx950; include/roft_engine.h, section 3i).
//
// One workgroup per (pose pair, part).  It projects the mesh at both poses, takes the union of their pixel boxes -- outside it both
// visibility masks are empty -- and per strip of the union draws the estimate into one LDS DepthWindow and the reference into another
// by raster.h's draw contract: the windows hold, bit for bit, what roft_render_depth(.., divider 1) returns, and never leave the CU.
// ONE LDS cache holds the projected vertices where the mesh fits: a strip draws first the pose the cache holds, then refills it for
// the other (one vertex pass per strip).  Then the strip's pixels are walked row by row (coalesced reads of the depth image), only
// where something was drawn: distance images, the two masks and the 4 + n_taus counts in registers, reduced wave -> workgroup -> one
// integer atomic add per count into the pair's row.  vsd_finish_kernel divides.  Every figure is a sum of integers: no row depends on
// strips, parts, threads or the launch.  Built with -ffp-contract=off; the distance images are specified in double.
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
    __shared__ MeshBoxShared s_mb[2];   // 0: the estimate, 1: the reference
    const int tid = threadIdx.x;
    const int part = (int)(blockIdx.x % (unsigned)a.parts), pair = (int)(blockIdx.x / (unsigned)a.parts);
    const MeshView& mesh = a.mesh;
    const int W = a.W, H = a.H, nv = mesh.n_verts;
    const bool cached = nv <= a.vcache_cap;
    float* s_v = reinterpret_cast<float*>(smem);
    const DepthWindow win_e{reinterpret_cast<uint32_t*>(smem + vertex_cache_bytes(a.vcache_cap))}, win_g{win_e.z + a.win_alloc};
    const double* const pose_e = a.est + (size_t)pair * 7;
    const double* const pose_g = a.ref + (size_t)pair * 7;
    const bool finite_e = pose_is_finite(pose_e), finite_g = pose_is_finite(pose_g);   // (uniform over the workgroup)
    const RenderPose Pe = make_pose(pose_e, pose_e + 3), Pg = make_pose(pose_g, pose_g + 3);   // (not used when not finite)
    box_reset(s_mb[0]);
    box_reset(s_mb[1]);
    __syncthreads();

    // vertices -> screen: the pixel box of everything either pose can draw; the cache is left with the estimate's vertices
    auto project_e = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, Pe, a.fx, a.fy, a.cx, a.cy, sx, sy, z); };
    auto project_g = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, Pg, a.fx, a.fy, a.cx, a.cy, sx, sy, z); };
    if (finite_g) project_mesh<kVsdThreads, 1>(mesh.verts, nv, false, s_v, W, H, s_mb[1].box, &s_mb[1].behind, project_g);
    if (finite_e) project_mesh<kVsdThreads, 1>(mesh.verts, nv, cached, s_v, W, H, s_mb[0].box, &s_mb[0].behind, project_e);
    __syncthreads();
    int holds = finite_e ? 0 : -1;   // the pose whose vertices the cache holds: 0 the estimate, 1 the reference
    const MeshBox box_e = box_read(s_mb[0], W, H), box_g = box_read(s_mb[1], W, H);
    const bool drawn_e = finite_e && box_e.drawable(), drawn_g = finite_g && box_g.drawable();   // the pose can draw something on the target
    MeshBox box = {INT32_MAX, INT32_MAX, -1, -1};   // the union
    if (drawn_e) box = box_e;
    if (drawn_g) box = MeshBox{min(box.i0, box_g.i0), min(box.j0, box_g.j0), max(box.i1, box_g.i1), max(box.j1, box_g.j1)};
    const uint8_t* const flips_e = cull_table(mesh.flip, s_mb[0].behind);
    const uint8_t* const flips_g = cull_table(mesh.flip, s_mb[1].behind);

    int cnt[kVsdCounts];
#pragma unroll
    for (int k = 0; k < kVsdCounts; ++k) cnt[k] = 0;

    if (drawn_e || drawn_g) {
        const int rows = strip_rows(a.win_cap, box.width()), n_strips = (box.j1 - box.j0 + rows) / rows;
        const float* depth = a.depth + (size_t)pair * a.depth_stride;
        for (int strip = part; strip < n_strips; strip += a.parts) {
            const Strip s = strip_from(box, box.j0 + strip * rows, rows);
            win_e.clear(s.npx, kVsdThreads);
            win_g.clear(s.npx, kVsdThreads);
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
                        project_vertex(mesh.verts + (size_t)3 * v, Pw, a.fx, a.fy, a.cx, a.cy, sx, sy, z);
                        s_v[3 * v] = sx; s_v[3 * v + 1] = sy; s_v[3 * v + 2] = z;
                    }
                    holds = w;
                    __syncthreads();
                }
                auto project = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, Pw, a.fx, a.fy, a.cx, a.cy, sx, sy, z); };
                draw_triangles<kVsdThreads>(mesh, s_v, cached, w ? flips_g : flips_e, project, W, H, s.js, s.je, (w ? win_g : win_e).store(s));
            }
            __syncthreads();
            // the strip's pixels, row by row; a pixel neither pose drew is in neither mask
            for (int idx = tid; idx < s.npx; idx += kVsdThreads) {
                const bool has_e = win_e.covered(idx), has_g = win_g.covered(idx);
                if (!has_e && !has_g) continue;
                const int jj = idx / s.win_w, i = s.i0 + (idx - jj * s.win_w), j = s.js + jj;
                const double ca = ((double)i - a.dcx) / a.dfx, cb = ((double)j - a.dcy) / a.dfy;   // once per pixel, for T, G and E
                const double T = vsd_dist(ca, cb, depth[(size_t)j * W + i]);
                const double G = has_g ? vsd_dist(ca, cb, win_g.depth(idx, i, j)) : 0.0;
                const double E = has_e ? vsd_dist(ca, cb, win_e.depth(idx, i, j)) : 0.0;
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
    wave_sums_to_rows(cnt, s_cnt);
    __syncthreads();
    if (tid < kVsdCounts) {
        const int tot = rows_total<kVsdThreads>(s_cnt, tid);
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
