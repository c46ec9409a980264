// engine_step.hip -- roft_step / roft_sync: step_batch gathers the counters a batch's plan depends on, has plan_batch
// (batch_plan.h) decide the launch graph, enqueues it on the engine's four HIP streams chain by chain (preparation, mask frames +
// features, velocity chain, two pose lanes) and copies the plan into the batch trace.  No decision is taken
// between two launches.  Also here: the timing marks around the launch groups.
//
// ORDERING -- why no wait between streams, or of the host, can hang.  (Waits INSIDE kernels: PROGRESS, on plan_batch.)
//
//  (1) Every cross-stream dependency of a batch is an EVENT recorded behind the producer (the stop event of its last kernel) and
//      waited for by the consumer's stream before the consumer's first kernel: ev_up (HOST copies) -> mask / velocity stream;
//      ev_prep (control blocks + ingest prepared on the upload stream) -> mask stream; ev_mask / ev_part (mask frames) -> velocity
//      stream and the features kernel; ev_skf (velocity filter) | ev_vel (+ the features behind it) -> pose lanes; ev_feat (a feature
//      kernel that ran on the MASK stream: one-frame submits, engines with few objects) -> the lanes whose tests read this batch's
//      sets, the preparation ahead two batches on (it rewrites the control blocks that kernel reads), the host; ev_done[lane] -> host
//      (in-flight bound, roft_sync).  Events only point from work enqueued EARLIER to work enqueued later, batch by batch and chain by chain in the
//      fixed order of step_batch: the wait-for graph is acyclic by construction.
//      Camera images (roft_frames_submit_images): the submit call enqueues the flow production -- pyramids, Lucas-Kanade levels, the
//      clones of aged-out flows -- on the UPLOAD stream behind its copies and records ev_up behind the production, so ev_up -> mask /
//      velocity stream covers the produced flows exactly as it covers a copied flow; it is recorded, and waited for, also when every
//      input was DEVICE memory and nothing was copied (SubmitFacts::produced_flows).  With the preparation on the upload stream the
//      control blocks follow the production in stream order and ev_prep carries it.  The velocity stream reads flows only behind an
//      event of this batch's mask stream (ev_ctrl / ev_part / ev_mask), which has waited.  The HOST waits for ev_host, recorded
//      behind the copies and BEFORE the production: no kernel is waited for, and no kernel waits in memory.
//  (2) The pose lanes' waits inside their kernels, and the three ways a lane is released: batch_plan.h.
//  (3) The outlier test's workgroups that share an alternative (k_render.hip) never wait for each other: each writes its slab,
//      counts itself in and EXITS unless it is the last to arrive; the last one merges.  No co-residency is needed.
//  (4) The mask frames hand over through kernel boundaries only (one launch per frame): no barrier among workgroups in memory.
//  (5) The host blocks in exactly two places: roft_frames_submit on ev_done / ev_vel / ev_feat / ev_quality of batch b - lead (the in-flight
//      bound that sizes every ring), and roft_sync.  Both wait for events of work already enqueued.
//  (6) Track quality (roft_engine_enable_quality; a batch without records enqueues none of this).  The launch of batch b is the LAST
//      thing the batch enqueues: on the stream of the last pose lane behind that lane's last segment, behind ev_done of the other
//      lane (its log rows) and ev_mask of the batch (its planes; the mask stream waited for the uploads, so its depth too) -- both
//      recorded earlier in this very step_batch, so (1) holds.  No fifth stream: a stream of its own would share a hardware queue
//      with one of the four chains and its event wait would block that chain.  It ends with ev_quality, which joins the events
//      wait_batch and roft_sync wait for.  Two lifetimes hang on that host wait.  (a) What the kernel reads outlives it: plane ring
//      slots, staged HOST depth and the caller's DEVICE buffers are re-used only by a batch whose submit has waited for batch
//      b (the in-flight bound); log rows and quality records lie in rings of at least lead x max_batch_frames rows -- the frames
//      that can be in flight --, which roft_engine_enable_quality enforces.  (b) The control blocks it reads are those of the batch's
//      own slot of the batch ring (BatchSlot::dctrl, kBatchRing slots > lead): rewritten by batch b + kBatchRing, whose submit has
//      waited for batch b + kBatchRing - lead > b.  It reads NOTHING from the two mask tables that alternate by batch parity
//      (EngineArrays::mrec), which the preparation of batch b + 2 resets -- the reason for prep_waits_feat.
#include "engine_internal.h"

// Control blocks of a batch: pinned (device-visible) host staging -> device by a kernel, so that they travel in-order on the
// compute queue instead of through an SDMA copy with its cross-engine signalling; and the reset of what the batch's mask chain
// accumulates into (ingest counters, the bits of the frames left to mask_general_kernel) on the way.  (a.ctrl, a.mrec: this batch's.)
__global__ void ctrl_upload_kernel(const uint4* __restrict__ src, EngineArrays a, size_t n16, int reset)
{
    uint4* dst = reinterpret_cast<uint4*>(a.ctrl);
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = i0; i < n16; i += stride) dst[i] = src[i];
    if (reset)
        for (size_t i = i0; i < (size_t)a.T * a.n_obj; i += stride) roft::mask_reset_tables(a, i);
}


// Timing marks accumulate over any number of steps until roft_engine_get_timing() collects them:
// mark i closes the interval (event i-1, event i] and attributes it to kernel id tmark[i]
// (-1 = step start, attributes nothing).
// appends a mark for `name` (null: -1) on stream `which` and returns its event
static hipEvent_t push_mark(roft_engine* e, const char* name, int which)
{
    const size_t idx = e->tmark.size();
    while (e->tev.size() <= idx) {
        e->tev.emplace_back();
        (void)e->tev.back().create();   // (a creation that fails leaves a null event: the mark is not recorded and roft_engine_get_timing reports it)
    }
    int id = -1;
    if (name) {
        for (size_t i = 0; i < e->tnames_s.size(); ++i)
            if (e->tnames_s[i] == name) id = (int)i;
        if (id < 0) { e->tnames_s.push_back(name); id = (int)e->tnames_s.size() - 1; }
    }
    e->tmark.push_back(id);
    e->tstream.push_back(which);
    return e->tev[idx];
}

static void tmark(roft_engine* e, const char* name, int which = 0)
{
    if (!e->timing) return;
    if (e->timing_level == 1) return;   // only the roofline kernel is timed (tmark_kernel)
    (void)hipEventRecord(push_mark(e, name, which), which == 1 ? e->pose_stream[0] : (which == 3 ? e->pose_stream[1] : (which == 2 ? e->vel_stream : (which == 4 ? e->up_stream : e->stream))));
}

// Timing of ONE kernel by a start / stop event pair bound to its dispatch (two consecutive marks: the first opens the
// interval, the second closes it and attributes it to `name`).  Leaves the events null when timing is off.
static void tmark_kernel(roft_engine* e, const char* name, int which, hipEvent_t* start, hipEvent_t* stop)
{
    if (!e->timing) return;
    *start = push_mark(e, nullptr, which);
    *stop = push_mark(e, name, which);
}

#define CHECK_LAUNCH(what)                                                                              \
    do {                                                                                                \
        hipError_t _e = hipGetLastError();                                                              \
        if (_e != hipSuccess) return fail(ROFT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(_e)); \
    } while (0)

// The batch being enqueued: its plan, its ring slot, the arrays its kernels see.
struct Enqueue {
    roft_engine* e;
    const BatchPlan& p;
    BatchSlot& cur;
    EngineArrays a;
    long long& launches;
    long long& evops;
    int wait(hipStream_t s, hipEvent_t ev)
    {
        HIP_TRY(hipStreamWaitEvent(s, ev, 0));
        ++evops;
        return ROFT_OK;
    }
    // resident-workgroup gate: the stream goes on when every velocity-filter workgroup launched so far has counted itself in
    int wait_gate(hipStream_t s)
    {
        HIP_TRY(hipStreamWaitValue64(s, e->arr.skf_started.p, e->skf_total, hipStreamWaitValueGte, ~0ull));
        ++evops;
        return ROFT_OK;
    }
    // "This span ends with `ev`": the span's last launch takes stop(how, ev); signalled(how, ev, s) follows the span's mark.
    static hipEvent_t stop(Signal how, hipEvent_t ev) { return how == Signal::stop ? ev : nullptr; }
    int signalled(Signal how, hipEvent_t ev, hipStream_t s)
    {
        if (how != Signal::record) return ROFT_OK;
        HIP_TRY(hipEventRecord(ev, s));
        ++evops;
        return ROFT_OK;
    }
};

// Control blocks of the batch -> device (+ reset of the mask chain's counters), ingest of the masks delivered with the batch
// (tables and ingest slots of this batch's parity: the carry of the chain before stays readable).
static int enqueue_preparation(Enqueue& q)
{
    roft_engine* e = q.e;
    const PendingBatch& pb = e->pending;
    const BatchPlan& p = q.p;
    const EngineArrays& a = q.a;
    hipStream_t s = e->stream, sp = p.prep ? e->up_stream : s;
    if (p.wait_up) TRY(q.wait(s, q.cur.ev_up));
    if (p.prep_waits_mask) {
        BatchSlot& two_back = e->slot_of(e->batch_counter - 2);
        TRY(q.wait(sp, two_back.ev_mask));
        if (p.prep_waits_feat) TRY(q.wait(sp, two_back.ev_feat));
    }
    tmark(e, nullptr, p.prep ? 4 : 0);
    static_assert(sizeof(FrameCtrl) % 16 == 0, "FrameCtrl is copied in 16-byte units");
    // (the label table of the batch lies behind its control blocks and is copied with them)
    const size_t n16 = (sizeof(FrameCtrl) * (size_t)a.n_obj * a.T + (p.label_ingest ? pb.label_table_bytes : 0)) / 16;
    const hipEvent_t ctrl_stop = Enqueue::stop(p.ev_ctrl, q.cur.ev_ctrl);
    const PrepLaunch last_launch = prep_last_launch(p, pb.facts.plain_mask_frames);
    // masks delivered as label images: one launch behind the per-object ingest (it ends with ev_prep where the plan has one and no
    // silhouette launch follows)
    auto label_ingest = [&]() -> int {
        LabelIngestArgs la;
        la.sets = reinterpret_cast<const LabelSet*>(a.ctrl + (size_t)a.n_obj * a.T);
        la.members = reinterpret_cast<const LabelMember*>(la.sets + pb.label_sets.size());
        la.planes = a.planes;
        la.plane_words = a.plane_words;
        la.obj_stride = (size_t)kPlaneSlotsTotal * 2 * a.plane_words;
        la.slot0 = a.slot_new;
        la.mrec = a.mrec;
        la.n_obj = a.n_obj;
        la.n_grp = a.cam.W * a.cam.H / 64;
        launch_label_ingest(la, (int)pb.label_sets.size(), sp, last_launch == PrepLaunch::label_ingest ? Enqueue::stop(p.ev_prep, q.cur.ev_prep) : nullptr);
        ++q.launches;
        CHECK_LAUNCH("label image ingest");
        return ROFT_OK;
    };
    // masks from poses: one launch for every silhouette of the batch, the preparation's last -- with silhouettes to resolve, the
    // clear of this parity's z-buffers, the draw and the resolve.  The stage ends with ev_prep where the plan has one bound to a
    // launch, else with an event of its own, which takes time stamps (roft_debug_pose_mask_kernel_ms: draw to resolve).
    auto pose_silhouettes = [&]() -> int {
        EnginePoseMasks& pm = e->pose_masks;
        SilhouetteArgs sa{};
        sa.ctrl = a.ctrl;
        sa.params = a.params;
        sa.planes = a.planes;
        sa.plane_words = a.plane_words;
        sa.obj_stride = (size_t)kPlaneSlotsTotal * 2 * a.plane_words;
        sa.slot0 = a.slot_new;
        sa.mrec = a.mrec;
        sa.n_obj = a.n_obj;
        sa.W = a.cam.W; sa.H = a.cam.H; sa.wpr = a.cam.wpr;
        sa.fx = (float)a.cam.fx; sa.fy = (float)a.cam.fy; sa.cx = (float)a.cam.cx; sa.cy = (float)a.cam.cy;   // (divider 1: the camera as it is)
        int n_frames = 0;
        for (int t = 0; t < a.T && t < 8; ++t)
            if (pb.pose_mask_frames & (1u << t)) sa.frames_packed |= (unsigned)t << (4 * n_frames++);
        if (p.pose_resolve) {
            const int par = e->batch_counter & 1;
            sa.n_zscenes = pm.n_zscenes;
            sa.zbuf = pm.zbuf.p + (size_t)par * kMaxBatch * pm.n_zscenes * a.cam.W * a.cam.H;
            sa.zpairs = pm.zpairs.p + (size_t)par * kMaxBatch * e->cfg.max_objects;
            sa.zstats = pm.zstats.p;
        }
        if (pm.gate) {
            // the depth gate: same launches, every drawn pair compared with FrameCtrl::gate_depth.  The gate images are resident when
            // the launch runs -- on the upload stream it follows the batch's copies and production in stream order; on the mask stream
            // that stream has waited for ev_up of every batch with copies or production, this one included (BatchPlan::wait_up), and
            // with one stream everything is in order anyway.  No wait is added.
            sa.gate = 1;
            sa.gate_tf = pm.gate_prm.front_tolerance;
            sa.gate_tb = pm.gate_prm.behind_tolerance;
            sa.gstats = pm.gstats.p;
            sa.zpairs = pm.zpairs.p + (size_t)(e->batch_counter & 1) * kMaxBatch * e->cfg.max_objects;
        }
        const int slot = e->batch_counter % roft_engine::kBatchRing;
        const hipEvent_t plan_stop = Enqueue::stop(p.ev_prep, q.cur.ev_prep);
        if (!p.prep) tmark(e, nullptr, 0);   // (timing runs: a mark of its own on the mask stream; ahead on the upload stream it is part of mask_prepare)
        const int launched = launch_pose_silhouette(sa, n_frames, a.max_verts, 0, 1, sp, pm.ev_start[slot], plan_stop ? plan_stop : pm.ev_stop[slot]);
        if (launched != pose_silhouette_launches(p))
            return fail(ROFT_ERR_INVALID, "pose masks: the image does not fit the kernel's bit window");
        pm.last_slot = slot;
        pm.last_timed = plan_stop == nullptr;
        q.launches += launched;
        CHECK_LAUNCH(p.pose_resolve ? "pose silhouettes: clear, draw and resolve" : "pose silhouettes");
        if (!p.prep) tmark(e, "pose_silhouettes", 0);
        return ROFT_OK;
    };
    if (p.try_fused && launch_ctrl_ingest(q.cur.stage.p, a, n16, pb.facts.plain_mask_frames, sp, ctrl_stop)) {
        ++q.launches;
        CHECK_LAUNCH("FrameCtrl upload + mask ingest");
        if (p.label_ingest) TRY(label_ingest());
        return p.pose_silhouettes ? pose_silhouettes() : ROFT_OK;
    }
    hipExtLaunchKernelGGL(ctrl_upload_kernel, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 64)), dim3(256), 0, sp, nullptr, ctrl_stop, 0,
                          reinterpret_cast<const uint4*>(q.cur.stage.p), a, n16, 1);
    ++q.launches;
    CHECK_LAUNCH("FrameCtrl upload");
    int last = -1;
    for (int t = 0; t < a.T; ++t)
        if (pb.facts.plain_mask_frames & (1u << t)) last = t;
    for (int t = 0; t <= last; ++t)
        if (pb.facts.plain_mask_frames & (1u << t)) {
            launch_mask_ingest(a, t, sp, (t == last && last_launch == PrepLaunch::mask_ingest) ? Enqueue::stop(p.ev_prep, q.cur.ev_prep) : nullptr);
            ++q.launches;
        }
    CHECK_LAUNCH("mask ingest");
    if (p.label_ingest) TRY(label_ingest());
    if (p.pose_silhouettes) TRY(pose_silhouettes());
    if (p.prep) {
        TRY(q.signalled(p.ev_prep, q.cur.ev_prep, sp));
        tmark(e, "mask_prepare", 4);
        TRY(q.wait(s, q.cur.ev_prep));
    }
    return ROFT_OK;
}

// Mask chain: every object's masks frame after frame; the outlier-rejection features of the batch's pose frames behind it where
// the plan runs them on this stream.
static int enqueue_mask_frames(Enqueue& q)
{
    roft_engine* e = q.e;
    const BatchPlan& p = q.p;
    hipStream_t s = e->stream;
    tmark(e, nullptr, 0);
    q.launches += launch_mask_chain(q.a, e->cfg.mask_frames_between, e->cfg.flow_aided_segmentation, e->pending.new_mask_frames, s,
                                    Enqueue::stop(p.ev_mask, q.cur.ev_mask), p.part_gate ? q.cur.ev_part : nullptr);
    CHECK_LAUNCH("mask chain");
    tmark(e, "mask_chain", 0);
    TRY(q.signalled(p.ev_mask, q.cur.ev_mask, s));
    q.cur.feat_used = p.ev_feat != Signal::none;   // (for wait_batch, like vel_used and done_used below)
    if (p.feat == FeatRun::mask_stream) {
        launch_features(q.a, s, Enqueue::stop(p.ev_feat, q.cur.ev_feat), e->pending.feat_frames);
        ++q.launches;
        CHECK_LAUNCH("features");
        tmark(e, "features", 0);
        TRY(q.signalled(p.ev_feat, q.cur.ev_feat, s));
    }
    return ROFT_OK;
}

// Velocity chain: flow measurement, velocity filter, and the features where the plan runs them behind the filter.
static int enqueue_velocity(Enqueue& q)
{
    roft_engine* e = q.e;
    const BatchPlan& p = q.p;
    const EngineArrays& a = q.a;
    hipStream_t sv = e->vel_stream;
    if (p.vel_waits != VelWait::none)
        TRY(q.wait(sv, p.vel_waits == VelWait::ev_ctrl ? q.cur.ev_ctrl : p.vel_waits == VelWait::ev_part ? q.cur.ev_part : q.cur.ev_mask));
    {
        // the roofline kernel is timed by a start / stop event pair on its own dispatch: its duration as rocprofv3
        // reports it, with no marker packets around it
        hipEvent_t k1_start = nullptr, k1_stop = nullptr;
        tmark_kernel(e, "flow_measure", 2, &k1_start, &k1_stop);
        // ... and, next to it, on the device's own clock: every workgroup leaves its start and end (first one in to last one
        // out = the launch as the kernel trace of a profiler sees it, without the packets the event pair brings along)
        EngineArrays ak = a;
        if (e->timing && (int)e->span_wgs.size() < roft_engine::kSpanLaunches && e->k1_span.p) {   // (allocated by roft_engine_enable_timing)
            ak.k1_span = e->k1_span.p + (size_t)2 * kMaxBatch * e->cfg.max_objects * e->span_wgs.size();
            e->span_wgs.push_back(a.T * a.n_obj);
        }
        launch_flow_measure(ak, e->cfg.depth_maximum, (int)(size_t)e->cfg.subsampling_radius, sv, k1_start, k1_stop);
        ++q.launches;
        CHECK_LAUNCH("flow measurement");
    }
    const bool feat_behind = p.feat == FeatRun::behind_skf;
    const Signal skf_how = feat_behind ? p.ev_skf : p.ev_vel;
    const hipEvent_t skf_ev = feat_behind ? q.cur.ev_skf : q.cur.ev_vel;
    q.cur.vel_used = p.ev_vel != Signal::none;
    launch_skf_chain(a, e->cfg.flow_weighting, sv, Enqueue::stop(skf_how, skf_ev));
    ++q.launches;
    if (hipError_t le = hipGetLastError()) {
        // the filter's workgroups will never count themselves in: no lane may ever wait for them (a stream-wait on a value has
        // no timeout) -- the hand-over is off for the rest of this engine's life
        e->knobs.handoff_mode = 0;
        return fail(ROFT_ERR_DEVICE, std::string("velocity filter chain: ") + hipGetErrorString(le));
    }
    e->skf_total += (unsigned long long)a.n_obj;   // (only once the launch is known to be enqueued: the lanes' gates wait for this count)
    tmark(e, "skf_chain", 2);
    TRY(q.signalled(skf_how, skf_ev, sv));
    if (feat_behind) {
        if (p.feat_waits_mask) TRY(q.wait(sv, q.cur.ev_mask));
        launch_features(a, sv, Enqueue::stop(p.ev_vel, q.cur.ev_vel), e->pending.feat_frames);
        ++q.launches;
        CHECK_LAUNCH("features");
        tmark(e, "features", 2);
        TRY(q.signalled(p.ev_vel, q.cur.ev_vel, sv));
    }
    return ROFT_OK;
}

// Pose chain of one lane (needs the twists of the batch; the next batches' image chains do not wait for it), on the lane's own
// stream: the frames before a pose arrival and the frames from it on belong to different belief lineages and do not depend on
// each other (BeliefSlot in roft_device.h), so the re-sync replay of this batch runs next to the ordinary steps of the other
// lineage -- of this batch and of the neighbouring ones.
static int enqueue_lane(Enqueue& q, int lin)
{
    roft_engine* e = q.e;
    const LanePlan& lp = q.p.lane[lin];
    hipStream_t sp = e->pose_stream[lin];
    q.cur.done_used[lin] = lp.ev_done != Signal::none;
    // slots handed over to this lane (submit_frames): behind the other lane's last launch that touched them
    const SubmitFacts& facts = e->pending.facts;
    if (lp.wait_relabel) TRY(q.wait(sp, e->slot_of(facts.relabel_wait[lin]).ev_done[1 - lin]));
    if (!facts.lin_any[lin]) return ROFT_OK;
    const int which = lin == 0 ? 1 : 3;
    switch (lp.release) {
    case Release::none: break;
    case Release::ctrl_only: TRY(q.wait(sp, q.cur.ev_ctrl)); break;
    case Release::gate: TRY(q.wait_gate(sp)); break;
    case Release::ev_skf: TRY(q.wait(sp, q.cur.ev_skf)); break;
    case Release::ev_vel: TRY(q.wait(sp, q.cur.ev_vel)); break;
    }
    if (lp.wait_feat) TRY(q.wait(sp, q.cur.ev_feat));
    tmark(e, nullptr, which);
    OutlierLaunchOpts oo;
    oo.render_mode = e->cfg.render_mode;
    if (q.p.outlier_div > 1) oo.parts = -q.p.outlier_div;   // (-d: the automatic count / d)
    const int n_seg = facts.n_segments[lin];
    for (int seg = 0; seg < n_seg; ++seg) {
        const bool last = seg == n_seg - 1;
        if (seg == 1 && lp.gate_second) TRY(q.wait_gate(sp));
        launch_ukf_chain(q.a, e->cfg.ut, seg == 0, lin, sp, last ? Enqueue::stop(lp.ev_done, q.cur.ev_done[lin]) : nullptr);
        ++q.launches;
        CHECK_LAUNCH("pose chain segment");
        tmark(e, "ukf_chain", which);
        if (last) break;
        if (seg == 0 && lp.wait_prev_vel) TRY(q.wait(sp, e->slot_of(e->batch_counter - 1).ev_vel));
        TRY(launch_outlier(q.a, lin, sp, nullptr, &oo));
        ++q.launches;
        CHECK_LAUNCH("outlier rejection");
        tmark(e, "outlier_render_likelihood", which);
    }
    return q.signalled(lp.ev_done, q.cur.ev_done[lin], sp);
}

// Track quality: every (frame, object) of the batch that gets a record in one launch, behind both lanes.
static int enqueue_quality(Enqueue& q)
{
    roft_engine* e = q.e;
    const BatchPlan& p = q.p;
    q.cur.quality_used = p.ev_quality != Signal::none;
    if (!p.quality) return ROFT_OK;
    const int slot = e->batch_counter % roft_engine::kBatchRing;
    hipStream_t sp = e->pose_stream[kNumLin - 1];
    if (p.quality_waits_mask) TRY(q.wait(sp, q.cur.ev_mask));
    if (p.quality_waits_lane) TRY(q.wait(sp, q.cur.ev_done[0]));
    int n_frames = 0;
    const unsigned packed = quality_frames_of_batch(e, &n_frames);
    EngineQuality& eq = e->quality;
    launch_quality(q.a, eq.ring.p, eq.cap, packed, n_frames, eq.prm.depth_tolerance, e->cfg.depth_maximum, 0, sp, eq.ev_start[slot],
                   Enqueue::stop(p.ev_quality, eq.ev_done[slot]));
    ++q.launches;
    CHECK_LAUNCH("track quality");
    tmark(e, "track_quality", 3);
    eq.last_slot = slot;
    return q.signalled(p.ev_quality, eq.ev_done[slot], sp);
}

// everything plan_batch may read, from the engine as the submit left it
static PlanInputs plan_inputs(roft_engine* e)
{
    PlanInputs in;
    static_cast<SubmitFacts&>(in) = e->pending.facts;
    in.knobs = e->knobs;
    in.multi = e->multi();
    in.timing = e->timing;
    in.timing_level = e->timing_level;
    in.wait_value_ok = e->wait_value_ok;
    in.have_skf_started = e->arr.skf_started.p != nullptr;
    in.n_obj = e->arr.a.n_obj;
    in.cus = device_cu_count();
    in.batch_counter = e->batch_counter; in.idle_mark = e->idle_mark; in.lead = e->lead; in.completed_batches = e->completed_batches;
    in.outlier_bands_per_alternative = e->cfg.outlier_bands_per_alternative;
    in.conflict_free = e->streams && e->streams->conflicts == 0;
    in.up_stream_distinct = e->up_stream != e->stream;
    if (e->quality.enabled) (void)quality_frames_of_batch(e, &in.quality_frames);
    in.feat_used_two_back = e->batch_counter >= 2 && e->slot_of(e->batch_counter - 2).feat_used;
    in.vel_used_prev = e->batch_counter >= 1 && e->slot_of(e->batch_counter - 1).vel_used;
    for (int l = 0; l < kNumLin; ++l) in.done_used_relabel[l] = in.relabel_wait[l] >= 0 && e->slot_of(in.relabel_wait[l]).done_used[1 - l];
    return in;
}

int step_batch(roft_engine* e)
{
    const PendingBatch& pb = e->pending;
    const int T = pb.facts.T;
    double hp_t = e->knobs.host_prof ? host_now_us() : 0.0;
    (void)hipGetLastError();   // a stale error of another library on this thread is not this step's
    const BatchPlan p = plan_batch(plan_inputs(e), [e] { return e->alone_on_device = alone_on_device(e->streams); });
    BatchSlot& cur = e->slot_of(e->batch_counter);
    Enqueue q{e, p, cur, e->arr.a, e->stats.launches, e->stats.event_ops};
    EngineArrays& a = q.a;
    a.T = T;
    a.ctrl = cur.dctrl.p;
    {
        // this batch's mask tables (parity) and the row of the other table that carries the state in
        const size_t table = (size_t)(kMaxBatch + 1) * a.n_obj;
        const int par = e->batch_counter & 1;
        MaskRec* base = e->arr.mrec.p;
        a.mrec = base + par * table;
        a.mrec_carry = e->prev_T > 0 ? base + (1 - par) * table + (size_t)e->prev_T * a.n_obj : a.mrec;
        a.slot_new = kSlotNew + par * kMaxBatch;
        a.slot_prev0 = (e->frame_counter + kPlaneSlots - 1) % kPlaneSlots;   // (submit_frames: slot_prev of every object)
    }
    a.handoff = p.handoff ? 1 : 0;
    a.skf_started = e->arr.skf_started.p;
    const long long launches0 = e->stats.launches, evops0 = e->stats.event_ops;

    TRY(enqueue_preparation(q));
    HP_MARK(e, 3, hp_t);
    TRY(enqueue_mask_frames(q));
    HP_MARK(e, 4, hp_t);
    TRY(enqueue_velocity(q));
    HP_MARK(e, 5, hp_t);
    for (int lin = 0; lin < kNumLin; ++lin) TRY(enqueue_lane(q, lin));
    TRY(enqueue_quality(q));
    HP_MARK(e, 6, hp_t);
    if (e->knobs.host_prof) {
        e->hp_batches++;
        if (e->knobs.host_prof_per_batch)   // (a burst's first batches are not its later ones)
            std::fprintf(stderr, "[roft host batch %d T=%d] ctrl %.1f mask %.1f vel %.1f lanes %.1f us (cumulative)\n", e->batch_counter, T,
                         e->hp_acc[3], e->hp_acc[4], e->hp_acc[5], e->hp_acc[6]);
    }
    {
        roft_batch_trace& tr = e->trace[e->batch_counter % roft_engine::kTraceRing];
        tr = roft_batch_trace{};
        tr.batch = e->batch_counter;
        tr.frames = T;
        tr.steady = p.steady; tr.throttled = pb.throttled; tr.handoff = p.handoff;
        tr.early_lanes = (p.early_lanes ? 4 : 0) | (p.lane[0].early ? 1 : 0) | (p.lane[1].early ? 2 : 0);
        tr.outlier_parts_halved = p.outlier_div > 1 ? 1 : 0;
        tr.launches = (int)(e->stats.launches - launches0);
        tr.event_ops = (int)(e->stats.event_ops - evops0);
        tr.t_submit_us = pb.submit_t0; tr.submit_us = pb.submit_us; tr.wait_us = pb.wait_us;
    }
    HIP_TRY(hipGetLastError());
    return ROFT_OK;
}

int roft_step(roft_engine* e)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    if (!e->submitted) return fail(ROFT_ERR_STATE, "roft_frame_submit must precede roft_step");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const double t_step0 = host_now_us();
    const int rc = step_batch(e);
    if (rc != ROFT_OK && e->arr.mask_general.p) {
        // A step that failed between the mask frames and mask_general_kernel (its only reader, which clears the bits it has
        // served) leaves bits of THIS batch's frames behind; the next batch's general kernel would replay those frame indices
        // against its own tables.  Clear them behind whatever the mask stream still carries (best effort: the device may be gone).
        (void)hipMemsetAsync(e->arr.mask_general.p, 0, sizeof(unsigned) * (size_t)std::max(e->arr.a.n_obj, 1), e->stream);
        // ... and the ingest counters of both mask tables: the chain's last kernel, which leaves them zeroed for the batch that
        // uses a table next (ctrl_ingest_kernel adds to them without a reset of its own), may not have run
        if (e->arr.mrec.p) {
            EngineArrays a2 = e->arr.a;
            a2.T = kMaxBatch;
            for (int par = 0; par < 2; ++par) {
                a2.mrec = e->arr.mrec.p + (size_t)par * (kMaxBatch + 1) * a2.n_obj;
                launch_mask_reset(a2, e->stream);
            }
        }
        (void)hipGetLastError();
    }
    {
        roft_batch_trace& tr = e->trace[e->batch_counter % roft_engine::kTraceRing];
        if (tr.batch == e->batch_counter) tr.step_us = host_now_us() - t_step0;
    }
    for (const auto& ho : e->objs) { ho->stepped_slot = ho->s.cur_slot; ho->stepped_lane = ho->s.own[ho->s.cur_slot]; ho->stepped_flow = ho->s.flow_made; ho->stepped_depth = ho->s.depth_prev; ho->last_out_valid = false; }
    // (a failed step leaves the engine consistent as far as the host can tell: the batch counts as enqueued)
    const int T = e->pending.facts.T;
    e->frame_counter += T;
    e->prev_T = T;
    e->slot_of(e->batch_counter).end_frame = e->frame_counter;
    e->batch_counter++;
    e->stats.frames += T;
    e->stats.batches++;
    e->submitted = false;
    return rc;
}

int roft_sync(roft_engine* e)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    HIP_TRY(hipSetDevice(e->cfg.device));
    // the batches in flight one by one, in order (their completion times go into the batch trace), then whatever else the
    // streams carry (uploads, timing marks, reads of results)
    // (only with several batches in flight: a tracker used live -- one frame submitted, stepped and read back at a time -- goes
    //  straight to the stream synchronisations, whose wake-up is faster than an event's)
    const int first_open = e->completed_batches, n_open = e->batch_counter - e->completed_batches;
    if (e->multi() && n_open > 1)
        for (int b = first_open; b < e->batch_counter; ++b)
            if (int rc = wait_batch(e, b)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->multi()) {
        HIP_TRY(hipStreamSynchronize(e->vel_stream));
        for (int l = 0; l < kNumLin; ++l) HIP_TRY(hipStreamSynchronize(e->pose_stream[l]));
        HIP_TRY(hipStreamSynchronize(e->up_stream));
    }
    for (int b = std::max(first_open, e->batch_counter - roft_engine::kTraceRing); b < e->batch_counter; ++b) {
        roft_batch_trace& tr = e->trace[b % roft_engine::kTraceRing];
        if (tr.batch == b && tr.t_done_us == 0.0) tr.t_done_us = host_now_us();
    }
    e->completed_batches = e->batch_counter;
    e->completed_frames = e->frame_counter;
    e->idle_mark = e->batch_counter;   // the device is idle: the next batches are a burst again (roft_engine::steady)
    return check_dev_error(e);
}
