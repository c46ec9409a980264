// engine_hypotheses.hip -- pose hypotheses (include/roft_engine.h, section 3j): n candidate poses of one object scored against one
// frame's mask and depth.  Two entry points over one launcher (hypotheses.h): roft_pose_hypotheses_score on host buffers, on the
// one-object context (op_context.h), and roft_engine_score_hypotheses on what an idle engine holds of its last stepped frame, on the
// engine's own stream.  Both upload the poses in chunks of kHypothesesChunk and write only the call's own buffers.
#include "op_context.h"

// the argument checks both entry points make, before a device is looked for
static int check_hypotheses_args(const double* poses, int n, float depth_tolerance, const roft_quality_record* out)
{
    if (n < 0 || n > kHypothesesMax) return fail(ROFT_ERR_INVALID, "n must be in 0 .. " + std::to_string(kHypothesesMax));
    if (!(depth_tolerance >= 0.0f)) return fail(ROFT_ERR_INVALID, "depth_tolerance must be >= 0");
    if (n > 0 && (!poses || !out)) return fail(ROFT_ERR_INVALID, "null argument");
    return ROFT_OK;
}

// n poses through the launcher, a chunk at a time: poses up, one launch, records down.  a: everything but poses / out / n_mask.
static int score_in_chunks(HypothesesArgs a, HypothesesScratch& hs, size_t lds, const double* poses, int n, hipStream_t s,
                           roft_quality_record* out)
{
    const int chunk = std::min(n, kHypothesesChunk);
    HIP_TRY(hs.poses.ensure((size_t)7 * chunk));
    HIP_TRY(hs.records.ensure((size_t)chunk));
    HIP_TRY(hs.n_mask.ensure(1));
    a.poses = hs.poses.p;
    a.out = hs.records.p;
    a.n_mask = hs.n_mask.p;
    std::vector<QualityRaw> raw((size_t)chunk);
    for (int first = 0; first < n; first += chunk) {
        const int m = std::min(chunk, n - first);
        HIP_TRY(hipMemcpyAsync(hs.poses.p, poses + (size_t)7 * first, sizeof(double) * 7 * m, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(hs.records.p, 0xFF, sizeof(QualityRaw) * m, s));   // frame = -1: no record
        launch_hypotheses(a, m, lds, s);
        HIP_TRY(hipMemcpyAsync(raw.data(), hs.records.p, sizeof(QualityRaw) * m, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipGetLastError());
        for (int i = 0; i < m; ++i) {
            if (raw[i].frame != a.frame) return fail(ROFT_ERR_DEVICE, "pose hypotheses: the kernel left no record");
            out[first + i] = quality_record(raw[i]);
        }
    }
    return ROFT_OK;
}

extern "C" int roft_pose_hypotheses_score(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask,
                                          const roft_mesh* mesh, const double* poses, int n, float depth_tolerance,
                                          double depth_maximum, int window_pixels, roft_quality_record* out)
{
    TRY(check_hypotheses_args(poses, n, depth_tolerance, out));
    if (divider <= 0) return fail(ROFT_ERR_INVALID, "divider must be > 0");
    if (window_pixels < 0) return fail(ROFT_ERR_INVALID, "window_pixels must be >= 0");
    if (n == 0) return ROFT_OK;
    if (!cam || !depth || !mask || !mesh) return fail(ROFT_ERR_INVALID, "null argument");
    TRY(check_mesh(*mesh, "mesh", true));   // (no mesh: nothing is rendered, the records count the mask alone)
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    EngineArrays a;
    TRY(c.one_object(*cam, nullptr, 35, divider, &a));
    if (a.tile_w <= 0 || a.tile_h <= 0) return fail(ROFT_ERR_INVALID, "divider larger than the image");
    HypothesesArgs ha;
    std::memset(&ha, 0, sizeof(ha));
    const RasterShape sh = quality_window_shape(has_mesh(*mesh) ? mesh->n_verts : 0, a.tile_w, window_pixels);
    if (!sh.ok)
        return fail(ROFT_ERR_INVALID, "track quality: the render target is too wide for the kernel's depth window");
    const size_t npix = (size_t)cam->width * cam->height;
    hipStream_t s = c.stream;
    TRY(c.mesh.upload(*mesh, MeshLayout::kWalkOrder, s));
    uint8_t* d_mask;
    float* d_depth;
    TRY(c.upload(0, mask, npix, &d_mask));
    TRY(c.upload(1, depth, npix, &d_depth));
    // the object plane of the byte mask, by the engine's ingest (as roft_track_quality makes it)
    FrameCtrl fc;
    clear_ctrl(fc);
    fc.has_new_mask = 1;
    fc.new_mask = d_mask;
    fc.slot_cur = kSlotNew;
    fc.depth_cur = d_depth;
    fc.frame_idx = 0;
    init_state(c.st);
    TRY(c.begin_object(a, nullptr, fc));
    launch_mask_reset(a, s);
    launch_mask_ingest(a, 0, s);
    ha.plane = a.planes + plane_offset(a, 0, kSlotNew, 1);
    ha.plane_words = a.plane_words;
    ha.depth = d_depth;
    ha.mesh = c.mesh.view();
    ha.vcache_cap = sh.vcache_cap;
    ha.win_cap = sh.win_cap;
    ha.cam = a.cam;
    ha.tile_w = a.tile_w;
    ha.tile_h = a.tile_h;
    ha.frame = 0;
    ha.depth_tolerance = depth_tolerance;
    ha.depth_maximum = depth_maximum;
    return score_in_chunks(ha, c.hypotheses, sh.lds, poses, n, s, out);
}

extern "C" int roft_engine_score_hypotheses(roft_engine* e, int obj_id, const double* poses, int n, float depth_tolerance,
                                            roft_quality_record* out)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    if (obj_id < 0 || obj_id >= (int)e->objs.size()) return fail(ROFT_ERR_INVALID, "bad obj_id");
    TRY(check_hypotheses_args(poses, n, depth_tolerance, out));
    if (e->cfg.render_mode == ROFT_RENDER_GL)
        return fail(ROFT_ERR_INVALID, "pose hypotheses render under ROFT_RENDER_CONTRACT: an engine with render_mode ROFT_RENDER_GL keeps its meshes "
                                      "unsorted and without the flip bits of the back-face rule, so that render does not exist there");
    const HostObject& ho = *e->objs[obj_id];
    const Sched& o = ho.s;
    if (o.track_frames == 0 || e->submitted || !ho.stepped_depth) return fail(ROFT_ERR_STATE, "no stepped frame to score hypotheses against");
    const EngineArrays& a = e->arr.a;
    if (!quality_fits(a)) return fail(ROFT_ERR_INVALID, "track quality: the render target is too wide for the kernel's depth window");
    if (n == 0) return ROFT_OK;
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (int rc = roft_sync(e)) return rc;
    const ObjParams& prm = e->h_params[obj_id];
    const bool mesh = has_mesh(prm);
    HypothesesArgs ha;
    std::memset(&ha, 0, sizeof(ha));
    const RasterShape sh = quality_window_shape(mesh ? prm.n_verts : 0, a.tile_w, 0);
    if (!sh.ok)
        return fail(ROFT_ERR_INVALID, "track quality: the render target is too wide for the kernel's depth window");
    ha.plane = a.planes + plane_offset(a, obj_id, (o.frame_idx - 1) % kPlaneSlots, 1);   // (the slot roft_get_mask reads)
    ha.plane_words = a.plane_words;
    ha.depth = ho.stepped_depth;
    if (mesh) ha.mesh = mesh_view(prm);
    ha.vcache_cap = sh.vcache_cap;
    ha.win_cap = sh.win_cap;
    ha.cam = a.cam;
    ha.tile_w = a.tile_w;
    ha.tile_h = a.tile_h;
    ha.frame = o.frame_idx - 1;
    ha.depth_tolerance = depth_tolerance;
    ha.depth_maximum = e->cfg.depth_maximum;
    return score_in_chunks(ha, e->hypotheses, sh.lds, poses, n, e->stream, out);
}
