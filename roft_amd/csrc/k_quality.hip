// k_quality.hip -- track quality (gfx950): silhouette overlap and depth residual of a frame's final estimate against the frame's
// own mask and depth (include/roft_engine.h, section 3d).
//
// One workgroup per (object, frame) pair that gets a record.  It counts the bits of the whole object plane, projects the mesh at
// the pose the step left in the log row and draws it into an LDS depth window exactly as the outlier test does -- the vertices
// projected once into LDS where they fit, else per triangle; raster_projected of raster.h, the back-face rule for closed meshes;
// strips when the window exceeds its LDS share -- so the window holds, bit for bit, the tile roft_render_depth returns.  Then it
// walks the image pixels under the strip row by row (consecutive threads, consecutive pixels: the plane words and the depth
// gathers are row-coalesced), reads the depth only where mask and render meet, and adds the counts as integers and |e| as a
// LikelihoodSum: every figure is a sum of integers, so no record depends on strips, threads or waves.
// Built with -ffp-contract=off like every user of raster.h.
#include <algorithm>

#include "quality.h"
#include "raster.h"

namespace roft {

constexpr int kQualityThreads = 1024;
constexpr int kQualityCounts = 6;   // n_mask, n_render, n_both, n_depth, n_front, n_behind

__global__ __launch_bounds__(kQualityThreads) void quality_kernel(EngineArrays a, QualityArgs qa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ long long s_hi[kQualityThreads / 64], s_lo[kQualityThreads / 64];
    __shared__ int s_cnt[kQualityThreads / 64][kQualityCounts];
    __shared__ int s_box[4];
    __shared__ int s_behind;
    const int obj = blockIdx.x, tid = threadIdx.x;
    const FrameCtrl& c = frame_ctrl(a, (int)((qa.frames_packed >> (4 * blockIdx.y)) & 15u), obj);
    const float* depth = c.depth_cur;
    const int slot_cur = c.slot_cur, frame_idx = c.frame_idx;
    const ObjParams& prm = a.params[obj];
    const double* est = a.out_log[(size_t)(frame_idx % a.log_cap) * a.n_obj + obj].pose;
    const RenderPose P = make_pose(est + 6, est + 9);
    const int d = a.cam.divider, tw = a.tile_w, th = a.tile_h, W = a.cam.W, wpr = a.cam.wpr;
    const float fx = (float)(a.cam.fx / d), fy = (float)(a.cam.fy / d), cx = (float)(a.cam.cx / d), cy = (float)(a.cam.cy / d);
    const int nv = prm.n_verts, nt = prm.n_tris;
    const bool cached = nv <= qa.vcache_cap;
    float* s_v = reinterpret_cast<float*>(smem);
    uint32_t* s_z = reinterpret_cast<uint32_t*>(smem + vertex_cache_bytes(qa.vcache_cap));
    if (tid < 4) s_box[tid] = (tid < 2) ? INT32_MAX : -1;
    if (tid == 0) s_behind = 0;
    __syncthreads();

    // the whole object plane: n_mask
    const uint32_t* plane = a.planes + plane_offset(a, obj, slot_cur, 1);
    int n_mask = 0, n_render = 0, n_both = 0, n_depth = 0, n_front = 0, n_behind = 0;
    {
        const size_t n4 = a.plane_words / 4;
        for (size_t i = tid; i < n4; i += kQualityThreads) {
            const uint4 w = reinterpret_cast<const uint4*>(plane)[i];
            n_mask += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
        }
        for (size_t i = n4 * 4 + tid; i < a.plane_words; i += kQualityThreads) n_mask += __popc(plane[i]);
    }

    // vertices -> screen and the pixel box of everything that can be drawn (raster.h)
    auto project = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, P, fx, fy, cx, cy, sx, sy, z); };
    project_mesh<kQualityThreads, 1>(prm.verts, nv, cached, s_v, tw, th, s_box, &s_behind, project);
    __syncthreads();
    const int i0 = min(s_box[0], tw - 1), i1 = s_box[2], j0 = min(s_box[1], th - 1), j1 = s_box[3];
    const int win_w = i1 - i0 + 1;
    LikelihoodSum err;
    // (the launcher refuses targets wider than the window's capacity: a strip holds at least one row of any window)
    if (win_w > 0 && win_w <= qa.win_cap && j1 >= j0 && i0 >= 0 && j0 >= 0) {
        const int rows = max(1, qa.win_cap / win_w);
        const uint8_t* const flips = cull_table(prm.tri_flip, s_behind);
        for (int js = j0; js <= j1; js += rows) {
            const int je = min(j1, js + rows - 1), npx = win_w * (je - js + 1);
            for (int i = tid; i < npx; i += kQualityThreads) s_z[i] = kDepthEmpty;
            __syncthreads();
            ROFT_LDS uint32_t* const zw = pin_lds(s_z);
            auto store = [zw, i0, js, win_w](int i, int j, float z) {
                (void)__hip_atomic_fetch_min(zw + ((j - js) * win_w + (i - i0)), __float_as_uint(z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            for (int t = tid; t < nt; t += kQualityThreads) {
                const int32_t* tri = prm.tris + (size_t)3 * t;
                const int v0 = tri[0], v1 = tri[1], v2 = tri[2];
                const int cull = cull_code(flips, t);
                float x0, y0, z0, x1, y1, z1, x2, y2, z2;
                fetch_triangle(s_v, cached, prm.verts, v0, v1, v2, project, x0, y0, z0, x1, y1, z1, x2, y2, z2);
                raster_projected(x0, y0, z0, x1, y1, z1, x2, y2, z2, tw, th, js, je, cull, store);
            }
            __syncthreads();
            // the image pixels under the strip: (u, v) with u / d in [i0, i1], v / d in [js, je] -- all inside the image, since
            // tw d <= W and th d <= H
            const int rw = win_w * d, n_img = rw * (je - js + 1) * d;
            for (int idx = tid; idx < n_img; idx += kQualityThreads) {
                const int vv = idx / rw, uu = idx - vv * rw;
                const uint32_t b = s_z[(vv / d) * win_w + uu / d];
                if (b == kDepthEmpty) continue;
                n_render += 1;
                const int u = i0 * d + uu, v = js * d + vv;
                if (!((plane[(size_t)v * wpr + (u >> 5)] >> (u & 31)) & 1u)) continue;
                n_both += 1;
                const float D = depth[(size_t)v * W + u];
                if (!(D > 0.0f && (double)D < qa.depth_maximum)) continue;   // (NaN fails both)
                n_depth += 1;
                const float e = D - __uint_as_float(b);
                if (e < -qa.depth_tolerance) n_front += 1;
                if (e > qa.depth_tolerance) n_behind += 1;
                err.add(fabsf(e));
            }
            __syncthreads();   // the next strip clears the window
        }
    }
    int cnt[kQualityCounts] = {n_mask, n_render, n_both, n_depth, n_front, n_behind};
    for (int off = 32; off > 0; off >>= 1) {
        err.hi += __shfl_down(err.hi, off, 64);
        err.lo += __shfl_down(err.lo, off, 64);
#pragma unroll
        for (int k = 0; k < kQualityCounts; ++k) cnt[k] += __shfl_down(cnt[k], off, 64);
    }
    if ((tid & 63) == 0) {
        s_hi[tid >> 6] = err.hi; s_lo[tid >> 6] = err.lo;
#pragma unroll
        for (int k = 0; k < kQualityCounts; ++k) s_cnt[tid >> 6][k] = cnt[k];
    }
    __syncthreads();
    if (tid == 0) {
        long long hi = 0, lo = 0;
        int tot[kQualityCounts] = {0, 0, 0, 0, 0, 0};
        for (int w = 0; w < kQualityThreads / 64; ++w) {
            hi += s_hi[w]; lo += s_lo[w];
            for (int k = 0; k < kQualityCounts; ++k) tot[k] += s_cnt[w][k];
        }
        QualityRaw& out = qa.ring[(size_t)(frame_idx % qa.cap) * a.n_obj + obj];
        out.frame = frame_idx;
        out.n_mask = tot[0]; out.n_render = tot[1]; out.n_both = tot[2];
        out.n_depth = tot[3]; out.n_front = tot[4]; out.n_behind = tot[5];
        out.reserved = 0;
        out.hi = hi; out.lo = lo;
    }
}

// LDS of a workgroup: the projected vertices of the largest mesh where they leave room for a window, and a window of 16 k pixels
// (an object's window is about 70 x 90 of 320 x 240 at the metric shape; a larger one is drawn in strips) -- not the whole LDS, so
// that workgroups of the chains the launch runs next to still find a place on the CU.
static bool quality_shape(const EngineArrays& a, int window_pixels, int& vcache_cap, int& win_cap, size_t& lds)
{
    const size_t lds_total = kRasterLdsBudget;
    const size_t vbytes = vertex_cache_bytes(a.max_verts);
    const size_t min_win = 4 * (size_t)std::max(8192, a.tile_w);
    const bool cache = vbytes + min_win <= lds_total;
    vcache_cap = cache ? a.max_verts : 0;
    const size_t room = (lds_total - (cache ? vbytes : 0)) / 4;
    if ((size_t)a.tile_w > room) return false;   // not even one row of the target
    win_cap = (int)std::min<size_t>(room, (size_t)std::max(16384, a.tile_w));
    lds = (cache ? vbytes : 0) + 4 * (size_t)win_cap;
    if (window_pixels > 0) win_cap = std::max(a.tile_w, std::min(win_cap, window_pixels));
    return true;
}

bool quality_fits(const EngineArrays& a)
{
    int vc, wc;
    size_t lds;
    return quality_shape(a, 0, vc, wc, lds);
}

void launch_quality(const EngineArrays& a, QualityRaw* ring, int cap, unsigned frames_packed, int n_frames, float depth_tolerance,
                    double depth_maximum, int window_pixels, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    QualityArgs qa;
    qa.ring = ring;
    qa.cap = cap;
    qa.frames_packed = frames_packed;
    qa.depth_tolerance = depth_tolerance;
    qa.depth_maximum = depth_maximum;
    size_t lds = 0;
    if (!quality_shape(a, window_pixels, qa.vcache_cap, qa.win_cap, lds)) return;   // (callers ask quality_fits first)
    (void)set_max_dynamic_lds(reinterpret_cast<const void*>(quality_kernel), (int)kRasterLdsBudget);
    hipExtLaunchKernelGGL(quality_kernel, dim3(a.n_obj, n_frames), dim3(kQualityThreads), (uint32_t)lds, s, start, stop, 0, a, qa);
}

}  // namespace roft
