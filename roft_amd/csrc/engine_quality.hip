// engine_quality.hip -- track quality (include/roft_engine.h, section 3d): enabling it on an engine, reading the records, the
// operator-level entry point on host buffers, the kernel's time.  The launch itself is part of a batch's plan: engine_step.hip.
#include "op_context.h"

static_assert(roft_engine::kBatchRing == 8, "EngineQuality keeps one event pair per slot of the batch ring");
static_assert(sizeof(roft_quality_record) == 40, "roft_quality_record is 40 bytes");

// the frames of the submitted batch that get a record: four bits per frame index, lowest first
unsigned quality_frames_of_batch(const roft_engine* e, int* n_out)
{
    unsigned packed = 0;
    int n = 0;
    const int every = std::max(e->quality.prm.every, 1);
    for (int t = 0; t < e->pending.facts.T && t < 8; ++t)
        if ((e->frame_counter + t) % every == 0) packed |= (unsigned)t << (4 * n++);
    if (n_out) *n_out = n;
    return packed;
}

extern "C" {

int roft_default_quality_params(roft_quality_params* p)
{
    if (!p) return fail(ROFT_ERR_INVALID, "null argument");
    p->every = 1;
    p->depth_tolerance = 0.01f;
    return ROFT_OK;
}

int roft_engine_enable_quality(roft_engine* e, const roft_quality_params* p)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    roft_quality_params prm;
    (void)roft_default_quality_params(&prm);
    if (p) prm = *p;
    if (prm.every < 1) return fail(ROFT_ERR_INVALID, "quality: every must be >= 1");
    if (!(prm.depth_tolerance >= 0.0f) || !std::isfinite(prm.depth_tolerance)) return fail(ROFT_ERR_INVALID, "quality: depth_tolerance must be finite and >= 0");
    if (e->cfg.render_mode == ROFT_RENDER_GL)
        return fail(ROFT_ERR_INVALID, "track quality renders under ROFT_RENDER_CONTRACT: an engine with render_mode ROFT_RENDER_GL keeps its meshes "
                                      "unsorted and without the flip bits of the back-face rule, so that render does not exist there");
    if (e->frame_counter > 0 || e->submitted) return fail(ROFT_ERR_STATE, "track quality must be enabled before the first frame");
    if (!e->arr.a.out_log) return fail(ROFT_ERR_STATE, "track quality reads the estimates from the output log: call roft_engine_enable_log first");
    // frames that can be in flight: the submit of batch b returns only when batch b - lead has ended, so at most `lead` batches of
    // at most T_max frames are open -- a log row (and a record) must not be rewritten under a launch that has not run yet
    const int least = e->lead * e->T_max;
    if (e->arr.a.log_cap < least)
        return fail(ROFT_ERR_INVALID, "track quality needs a log of at least " + std::to_string(least) + " frames (" + std::to_string(e->lead) +
                                          " batches in flight x max_batch_frames " + std::to_string(e->T_max) + "); the log holds " +
                                          std::to_string(e->arr.a.log_cap));
    if (!quality_fits(e->arr.a)) return fail(ROFT_ERR_INVALID, "track quality: the render target is too wide for the kernel's depth window");
    HIP_TRY(hipSetDevice(e->cfg.device));
    EngineQuality& q = e->quality;
    q.cap = e->arr.a.log_cap;
    HIP_TRY(q.ring.ensure((size_t)q.cap * e->cfg.max_objects));
    HIP_TRY(hipMemset(q.ring.p, 0xFF, sizeof(QualityRaw) * (size_t)q.cap * e->cfg.max_objects));   // frame = -1: no record
    // nothing of the launch may happen for the first time inside a caller's timed region (engine_setup): each event pair has
    // completed one dispatch on the stream that will carry it
    for (int i = 0; i < roft_engine::kBatchRing; ++i) {
        HIP_TRY(q.ev_start[i].create());
        HIP_TRY(q.ev_done[i].create());
        hipExtLaunchKernelGGL(probe_tiny_kernel, dim3(1), dim3(64), 0, e->pose_stream[kNumLin - 1], q.ev_start[i], q.ev_done[i], 0,
                              reinterpret_cast<int*>(q.ring.p));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->pose_stream[kNumLin - 1]));
    HIP_TRY(hipMemset(q.ring.p, 0xFF, sizeof(int)));
    q.prm = prm;
    q.last_slot = -1;
    q.enabled = true;
    return ROFT_OK;
}

int roft_engine_get_quality(roft_engine* e, int first_frame, int n_frames, roft_quality_record* out)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    if (!e->quality.enabled) return fail(ROFT_ERR_INVALID, "track quality not enabled");
    if (!out) return fail(ROFT_ERR_INVALID, "null argument");
    if (n_frames < 0 || first_frame < 0) return fail(ROFT_ERR_INVALID, "bad frame range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (int rc = roft_sync(e)) return rc;
    const EngineQuality& q = e->quality;
    const int cap = q.cap, stepped = e->frame_counter, n_obj = e->arr.a.n_obj;
    if (n_frames > cap || (long)first_frame + n_frames > stepped || first_frame < stepped - cap)
        return fail(ROFT_ERR_INVALID, "frame range is not (or no longer) in the quality ring");
    if (n_frames == 0 || n_obj == 0) return ROFT_OK;
    std::vector<QualityRaw> raw((size_t)n_frames * n_obj);
    for (int f = 0; f < n_frames;) {   // one copy per contiguous run of ring rows
        const int slot = (first_frame + f) % cap;
        const int run = std::min(n_frames - f, cap - slot);
        HIP_TRY(hipMemcpy(raw.data() + (size_t)f * n_obj, q.ring.p + (size_t)slot * n_obj, sizeof(QualityRaw) * n_obj * run, hipMemcpyDeviceToHost));
        f += run;
    }
    for (int f = 0; f < n_frames; ++f)
        for (int o = 0; o < n_obj; ++o) {
            const QualityRaw& r = raw[(size_t)f * n_obj + o];
            roft_quality_record& dst = out[(size_t)f * n_obj + o];
            if ((first_frame + f) % q.prm.every == 0 && r.frame == first_frame + f) {
                dst = quality_record(r);
            } else {   // no record for this (frame, object)
                std::memset(&dst, 0, sizeof(dst));
                dst.frame = -1;
            }
        }
    return ROFT_OK;
}

int roft_debug_quality_kernel_ms(roft_engine* e, double* ms_out)
{
    if (!e || !ms_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (!e->quality.enabled || e->quality.last_slot < 0) return fail(ROFT_ERR_STATE, "no quality launch so far");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const int s = e->quality.last_slot;
    HIP_TRY(hipEventSynchronize(e->quality.ev_done[s]));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, e->quality.ev_start[s], e->quality.ev_done[s]));
    *ms_out = (double)ms;
    return ROFT_OK;
}

}  // extern "C"

// ---- operator level: the engine's kernel on host buffers, on the one-object context (op_context.h) ---------------------------------
extern "C" int roft_track_quality(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                                  const double x[3], const double q[4], float depth_tolerance, double depth_maximum, int window_pixels,
                                  roft_quality_record* out)
{
    if (!cam || !depth || !mask || !mesh || !x || !q || !out) return fail(ROFT_ERR_INVALID, "null argument");
    if (divider <= 0) return fail(ROFT_ERR_INVALID, "divider must be > 0");
    if (!(depth_tolerance >= 0.0f)) return fail(ROFT_ERR_INVALID, "depth_tolerance must be >= 0");
    if (window_pixels < 0) return fail(ROFT_ERR_INVALID, "window_pixels must be >= 0");
    TRY(check_mesh(*mesh, "mesh", true));   // (no mesh: nothing is rendered, the record counts the mask alone)
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    EngineArrays a;
    TRY(c.one_object(*cam, nullptr, 35, divider, &a));
    if (a.tile_w <= 0 || a.tile_h <= 0) return fail(ROFT_ERR_INVALID, "divider larger than the image");
    a.out_log = c.arr.log.p;
    a.log_cap = 1;
    a.max_verts = has_mesh(*mesh) ? mesh->n_verts : 0;
    a.max_tris = has_mesh(*mesh) ? mesh->n_tris : 0;
    if (!quality_fits(a)) return fail(ROFT_ERR_INVALID, "track quality: the render target is too wide for the kernel's depth window");
    const size_t npix = (size_t)cam->width * cam->height;
    hipStream_t s = c.stream;
    ObjParams prm;
    std::memset(&prm, 0, sizeof(prm));
    TRY(c.mesh.upload(*mesh, MeshLayout::kWalkOrder, s));
    c.mesh.describe(prm);
    uint8_t* d_mask;
    float* d_depth;
    TRY(c.upload(0, mask, npix, &d_mask));
    TRY(c.upload(1, depth, npix, &d_depth));
    FrameCtrl fc;
    clear_ctrl(fc);
    fc.has_new_mask = 1;
    fc.new_mask = d_mask;
    fc.slot_cur = kSlotNew;   // (the ingest leaves the planes of the delivered mask in the slot the kernel is told to read)
    fc.depth_cur = d_depth;
    fc.frame_idx = 0;
    roft_object_output row;
    std::memset(&row, 0, sizeof(row));
    for (int i = 0; i < 3; ++i) row.pose[6 + i] = x[i];
    for (int i = 0; i < 4; ++i) row.pose[9 + i] = q[i];
    HIP_TRY(hipMemcpyAsync(a.out_log, &row, sizeof(row), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c.quality.p, 0xFF, sizeof(QualityRaw), s));
    init_state(c.st);
    TRY(c.begin_object(a, &prm, fc));   // (row lives on this stack as well)
    launch_mask_reset(a, s);   // (the ingest adds its pixel counts to the context's mask table)
    launch_mask_ingest(a, 0, s);
    launch_quality(a, c.quality.p, 1, 0u, 1, depth_tolerance, depth_maximum, window_pixels, s);
    QualityRaw raw;
    HIP_TRY(hipMemcpyAsync(&raw, c.quality.p, sizeof(raw), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    if (raw.frame != 0) return fail(ROFT_ERR_DEVICE, "track quality: the kernel left no record");
    *out = quality_record(raw);
    return ROFT_OK;
}
