// k_quality.hip -- track quality (gfx950): silhouette overlap and depth residual of a frame's final estimate against the frame's
// own mask and depth (include/roft_engine.h, section 3d).
//
// One workgroup per (object, frame) pair that gets a record.  It counts the bits of the whole object plane and hands the pose the
// step left in the log row to quality_body.h, which projects the mesh, draws it into an LDS depth window exactly as the outlier
// test does, walks the image pixels under it and adds the counts as integers and |e| as a LikelihoodSum: every figure is a sum of
// integers, so no record depends on strips, threads or waves.  (The same body scores pose hypotheses: k_hypotheses.hip.)
// Built with -ffp-contract=off like every user of raster.h.
#include <algorithm>

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
    sc.verts = prm.verts; sc.tris = prm.tris; sc.tri_flip = prm.tri_flip;
    sc.n_verts = prm.n_verts; sc.n_tris = prm.n_tris;
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

// LDS of a workgroup: the projected vertices of the largest mesh where they leave room for a window, and a window of 16 k pixels
// (an object's window is about 70 x 90 of 320 x 240 at the metric shape; a larger one is drawn in strips) -- not the whole LDS, so
// that workgroups of the chains the launch runs next to still find a place on the CU.
bool quality_window_shape(int max_verts, int tile_w, int window_pixels, int& vcache_cap, int& win_cap, size_t& lds)
{
    const size_t lds_total = kRasterLdsBudget;
    const size_t vbytes = vertex_cache_bytes(max_verts);
    const size_t min_win = 4 * (size_t)std::max(8192, tile_w);
    const bool cache = vbytes + min_win <= lds_total;
    vcache_cap = cache ? max_verts : 0;
    const size_t room = (lds_total - (cache ? vbytes : 0)) / 4;
    if ((size_t)tile_w > room) return false;   // not even one row of the target
    win_cap = (int)std::min<size_t>(room, (size_t)std::max(16384, tile_w));
    lds = (cache ? vbytes : 0) + 4 * (size_t)win_cap;
    if (window_pixels > 0) win_cap = std::max(tile_w, std::min(win_cap, window_pixels));
    return true;
}

static bool quality_shape(const EngineArrays& a, int window_pixels, int& vcache_cap, int& win_cap, size_t& lds)
{
    return quality_window_shape(a.max_verts, a.tile_w, window_pixels, vcache_cap, win_cap, lds);
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
