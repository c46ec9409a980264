// k_quality.hip -- track quality (gfx950): silhouette overlap and depth residual of a frame's final estimate against the frame's
// own mask and depth (include/roft_engine.h, section 3d).
//
// One workgroup per (object, frame) pair that gets a record.  It counts the bits of the whole object plane and hands the pose the
// step left in the log row to quality_body.h, which draws the mesh and makes the record's sums.  (The same body scores pose
// hypotheses: k_hypotheses.hip.)  Built with -ffp-contract=off like every user of raster.h.
#include "quality.h"
#include "quality_body.h"

namespace roft {

constexpr int kQualityThreads = 1024;

__global__ __launch_bounds__(kQualityThreads) void quality_kernel(EngineArrays a, QualityArgs qa)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int obj = blockIdx.x, tid = threadIdx.x;
    const FrameCtrl& c = frame_ctrl(a, (int)((qa.frames_packed >> (4 * blockIdx.y)) & 15u), obj);
    const int frame_idx = c.frame_idx;
    const ObjParams& prm = a.params[obj];
    const double* est = a.out_log[(size_t)(frame_idx % a.log_cap) * a.n_obj + obj].pose;
    const RenderPose P = make_pose(est + 6, est + 9);
    const int d = a.cam.divider;
    QualityScene sc;
    sc.plane = a.planes + plane_offset(a, obj, c.slot_cur, 1);
    sc.depth = c.depth_cur;
    sc.mesh = mesh_view(prm);
    sc.d = d; sc.tw = a.tile_w; sc.th = a.tile_h; sc.W = a.cam.W; sc.wpr = a.cam.wpr;
    sc.fx = (float)(a.cam.fx / d); sc.fy = (float)(a.cam.fy / d); sc.cx = (float)(a.cam.cx / d); sc.cy = (float)(a.cam.cy / d);
    sc.depth_tolerance = qa.depth_tolerance;
    sc.depth_maximum = qa.depth_maximum;
    sc.vcache_cap = qa.vcache_cap;
    sc.win_cap = qa.win_cap;

    // the whole object plane: n_mask; then the pose's render against plane and depth (quality_body.h)
    const int n_mask = plane_bits_share(sc.plane, a.plane_words, tid, kQualityThreads);
    QualitySums tot;
    quality_body<kQualityThreads>(sc, P, n_mask, smem, tot);
    if (tid == 0) {
        QualityRaw& out = qa.ring[(size_t)(frame_idx % qa.cap) * a.n_obj + obj];
        out.frame = frame_idx;
        out.n_mask = tot.cnt[0]; out.n_render = tot.cnt[1]; out.n_both = tot.cnt[2];
        out.n_depth = tot.cnt[3]; out.n_front = tot.cnt[4]; out.n_behind = tot.cnt[5];
        out.reserved = 0;
        out.hi = tot.hi; out.lo = tot.lo;
    }
}

bool quality_fits(const EngineArrays& a) { return quality_window_shape(a.max_verts, a.tile_w, 0).ok; }

void launch_quality(const EngineArrays& a, QualityRaw* ring, int cap, unsigned frames_packed, int n_frames, float depth_tolerance,
                    double depth_maximum, int window_pixels, hipStream_t s, hipEvent_t start, hipEvent_t stop)
{
    QualityArgs qa;
    qa.ring = ring;
    qa.cap = cap;
    qa.frames_packed = frames_packed;
    qa.depth_tolerance = depth_tolerance;
    qa.depth_maximum = depth_maximum;
    const RasterShape sh = quality_window_shape(a.max_verts, a.tile_w, window_pixels);
    if (!sh.ok) return;   // (callers ask quality_fits first)
    qa.vcache_cap = sh.vcache_cap;
    qa.win_cap = sh.win_cap;
    (void)set_max_dynamic_lds(reinterpret_cast<const void*>(quality_kernel), (int)kRasterLdsBudget);
    hipExtLaunchKernelGGL(quality_kernel, dim3(a.n_obj, n_frames), dim3(kQualityThreads), (uint32_t)sh.lds, s, start, stop, 0, a, qa);
}

}  // namespace roft
