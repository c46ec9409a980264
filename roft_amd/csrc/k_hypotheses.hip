// k_hypotheses.hip -- pose hypotheses (gfx950): n candidate poses of one mesh scored against one frame's mask and depth in one launch
// (include/roft_engine.h, section 3j).
//
// A record of section 3d is a set of integer sums, so a batch of hypotheses is embarrassingly parallel and bit-reproducible: one
// workgroup per hypothesis runs quality_body.h -- the body quality_kernel runs for the engine's estimate -- on its own pose, against
// the plane, the depth and the mesh all hypotheses share.  n_mask is the same for every pose: plane_count_kernel counts the plane's
// bits once, ahead of the hypotheses on the same stream, and every record copies the word.  A pose with a non-finite component
// draws nothing (pose_is_finite).  The kernel takes a plain argument block (hypotheses.h), no engine structure: the operator (on the one-object
// context) and the engine entry (on the idle engine's own stream) use the same launcher.
//
// Workgroup shape: 1024 threads with quality_kernel's LDS (the vertex cache and a 16 k-pixel window), one workgroup per CU.  256-thread
// workgroups with a quarter of the LDS -- four hypotheses per CU, a large mesh projected per triangle -- were measured and lost
// (docs/notebook.md); no bit would depend on the shape.
// Built with -ffp-contract=off like every user of raster.h.
#include "hypotheses.h"
#include "quality_body.h"

namespace roft {

constexpr int kHypothesesThreads = 1024;

__global__ __launch_bounds__(1024) void plane_count_kernel(const uint32_t* plane, size_t plane_words, int* n_mask)
{
    __shared__ int s_n[1024 / 64][1];
    int n[1] = {plane_bits_share(plane, plane_words, threadIdx.x, 1024)};
    wave_sums_to_rows(n, s_n);
    __syncthreads();
    if (threadIdx.x == 0) *n_mask = rows_total<1024>(s_n, 0);
}

__global__ __launch_bounds__(kHypothesesThreads) void hypotheses_kernel(HypothesesArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int h = blockIdx.x, tid = threadIdx.x;
    const double* pose = a.poses + (size_t)7 * h;
    QualitySums tot;
    if (pose_is_finite(pose)) {   // (uniform over the workgroup: the body's barriers are met by all or by none)
        const int d = a.cam.divider;
        QualityScene sc;
        sc.plane = a.plane;
        sc.depth = a.depth;
        sc.mesh = a.mesh;
        sc.d = d; sc.tw = a.tile_w; sc.th = a.tile_h; sc.W = a.cam.W; sc.wpr = a.cam.wpr;
        sc.fx = (float)(a.cam.fx / d); sc.fy = (float)(a.cam.fy / d); sc.cx = (float)(a.cam.cx / d); sc.cy = (float)(a.cam.cy / d);
        sc.depth_tolerance = a.depth_tolerance;
        sc.depth_maximum = a.depth_maximum;
        sc.vcache_cap = a.vcache_cap;
        sc.win_cap = a.win_cap;
        const RenderPose P = make_pose(pose, pose + 3);
        quality_body<kHypothesesThreads>(sc, P, 0, smem, tot);
    } else {
        tot.hi = tot.lo = 0;
        for (int k = 0; k < kQualityCounts; ++k) tot.cnt[k] = 0;
    }
    if (tid == 0) {
        QualityRaw& out = a.out[h];
        out.frame = a.frame;
        out.n_mask = *a.n_mask;
        out.n_render = tot.cnt[1]; out.n_both = tot.cnt[2];
        out.n_depth = tot.cnt[3]; out.n_front = tot.cnt[4]; out.n_behind = tot.cnt[5];
        out.reserved = 0;
        out.hi = tot.hi; out.lo = tot.lo;
    }
}

void launch_hypotheses(const HypothesesArgs& a, int n, size_t lds, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(plane_count_kernel, dim3(1), dim3(1024), 0, s, a.plane, a.plane_words, a.n_mask);
    (void)set_max_dynamic_lds(reinterpret_cast<const void*>(hypotheses_kernel), (int)kRasterLdsBudget);
    hipLaunchKernelGGL(hypotheses_kernel, dim3(n), dim3(kHypothesesThreads), (uint32_t)lds, s, a);
}

}  // namespace roft
