// quality_body.h -- the body of a track-quality record (include/roft_engine.h, section 3d), between "project the mesh" and "the
// record": ONE pose of one mesh against one object plane and one depth image, by one workgroup.  It draws the mesh into an LDS
// DepthWindow by raster.h's draw contract, so the window holds, bit for bit, the tile roft_render_depth returns.  Then it walks the
// image pixels under the strip row by row (consecutive threads, consecutive pixels: the plane words and the depth gathers are
// row-coalesced), reads the depth only where mask and render meet, and adds the counts as integers and |e| as a LikelihoodSum:
// every figure is a sum of integers, so no record depends on strips, threads or waves.
// Two kernels include it: quality_kernel (k_quality.hip: the engine's estimate of a frame) and hypotheses_kernel (k_hypotheses.hip:
// n candidate poses against one frame, section 3j).  Both are built with -ffp-contract=off like every user of raster.h.
#pragma once

#include "raster.h"

namespace roft {

constexpr int kQualityCounts = 6;   // n_mask, n_render, n_both, n_depth, n_front, n_behind

// What the body reads besides the pose: plain pointers and numbers, no engine structure.
struct QualityScene {
    const uint32_t* plane;   // the object plane M: wpr words per image row
    const float* depth;      // D, W floats per row
    MeshView mesh;           // as ObjParams describes it (walk order and flip bits of a closed mesh)
    int d, tw, th, W, wpr;   // divider, render target, image width, plane words per row
    float fx, fy, cx, cy;    // the camera over the divider, as the render contract rounds it
    float depth_tolerance;
    double depth_maximum;
    int vcache_cap;          // vertices the LDS cache holds (0: every triangle projects its own)
    int win_cap;             // pixels of the LDS depth window (a larger window is drawn in strips)
};

// The sums of one record; thread 0 holds them when quality_body returns.
struct QualitySums {
    int cnt[kQualityCounts];
    long long hi, lo;
};

// Called by all kThreads threads of a workgroup.  smem: the dynamic LDS, [vertex_cache_bytes(vcache_cap)] | [4 win_cap].  n_mask: the
// calling thread's share of the plane's bit count (it is summed with the other counts; a caller that knows the plane's count passes 0
// and ignores cnt[0]).  The launcher refuses targets wider than win_cap: a strip holds at least one row of any window.
// May be called again by the same workgroup (another pose): it ends behind a barrier, and thread 0 has read the sums by then.
template <int kThreads>
__device__ __forceinline__ void quality_body(const QualityScene& sc, const RenderPose& P, int n_mask, unsigned char* smem, QualitySums& sums)
{
    __shared__ long long s_hi[kThreads / 64], s_lo[kThreads / 64];
    __shared__ int s_cnt[kThreads / 64][kQualityCounts];
    __shared__ MeshBoxShared s_mb;
    const int tid = threadIdx.x;
    const float* depth = sc.depth;
    const uint32_t* plane = sc.plane;
    const MeshView& mesh = sc.mesh;
    const int d = sc.d, tw = sc.tw, th = sc.th, W = sc.W, wpr = sc.wpr;
    const float fx = sc.fx, fy = sc.fy, cx = sc.cx, cy = sc.cy;
    const bool cached = mesh.n_verts <= sc.vcache_cap;
    float* s_v = reinterpret_cast<float*>(smem);
    const DepthWindow win{reinterpret_cast<uint32_t*>(smem + vertex_cache_bytes(sc.vcache_cap))};
    box_reset(s_mb);
    __syncthreads();
    int n_render = 0, n_both = 0, n_depth = 0, n_front = 0, n_behind = 0;

    auto project = [&](const float* v, float& sx, float& sy, float& z) { project_vertex(v, P, fx, fy, cx, cy, sx, sy, z); };
    project_mesh<kThreads, 1>(mesh.verts, mesh.n_verts, cached, s_v, tw, th, s_mb.box, &s_mb.behind, project);
    __syncthreads();
    const MeshBox box = box_read(s_mb, tw, th);
    LikelihoodSum err;
    if (box.drawable() && box.width() <= sc.win_cap) {
        const int rows = strip_rows(sc.win_cap, box.width());
        const uint8_t* const flips = cull_table(mesh.flip, s_mb.behind);
        for (int js = box.j0; js <= box.j1; js += rows) {
            const Strip s = strip_from(box, js, rows);
            win.clear(s.npx, kThreads);
            __syncthreads();
            draw_triangles<kThreads>(mesh, s_v, cached, flips, project, tw, th, s.js, s.je, win.store(s));
            __syncthreads();
            // the image pixels under the strip: (u, v) with u / d in [i0, i1], v / d in [js, je] -- all inside the image, since
            // tw d <= W and th d <= H
            const int rw = s.win_w * d, n_img = rw * (s.je - s.js + 1) * d;
            for (int idx = tid; idx < n_img; idx += kThreads) {
                const int vv = idx / rw, uu = idx - vv * rw;
                const int px = (vv / d) * s.win_w + uu / d;
                if (!win.covered(px)) continue;
                n_render += 1;
                const int u = s.i0 * d + uu, v = s.js * d + vv;
                if (!((plane[(size_t)v * wpr + (u >> 5)] >> (u & 31)) & 1u)) continue;
                n_both += 1;
                const float D = depth[(size_t)v * W + u];
                if (!(D > 0.0f && (double)D < sc.depth_maximum)) continue;   // (NaN fails both)
                n_depth += 1;
                const float e = D - win.depth(px, u / d, v / d);
                if (e < -sc.depth_tolerance) n_front += 1;
                if (e > sc.depth_tolerance) n_behind += 1;
                err.add(fabsf(e));
            }
            __syncthreads();   // the next strip clears the window
        }
    }
    int cnt[kQualityCounts] = {n_mask, n_render, n_both, n_depth, n_front, n_behind};
    // (raster.h's wave_sums_to_rows / rows_total, kept fused with the LikelihoodSum's reduction: one shuffle loop, one serial add)
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
        sums.hi = sums.lo = 0;
        for (int k = 0; k < kQualityCounts; ++k) sums.cnt[k] = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            sums.hi += s_hi[w]; sums.lo += s_lo[w];
            for (int k = 0; k < kQualityCounts; ++k) sums.cnt[k] += s_cnt[w][k];
        }
    }
}

// The plane's bit count, a thread's share: thread `tid` of `threads` reads every threads-th 16-byte group (n_mask of section 3d).
__device__ __forceinline__ int plane_bits_share(const uint32_t* plane, size_t plane_words, int tid, int threads)
{
    int n = 0;
    const size_t n4 = plane_words / 4;
    for (size_t i = tid; i < n4; i += threads) {
        const uint4 w = reinterpret_cast<const uint4*>(plane)[i];
        n += __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);
    }
    for (size_t i = n4 * 4 + tid; i < plane_words; i += threads) n += __popc(plane[i]);
    return n;
}

}  // namespace roft
