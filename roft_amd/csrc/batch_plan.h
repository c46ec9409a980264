// batch_plan.h -- what the engine decides for a batch before it enqueues anything: a pure function from counters to decisions
// (plan_batch), and the engine-level switches it obeys (SchedKnobs).  Host-only, plain C++17, no HIP: tests/cpp/batch_plan_check.cpp
// sweeps it without a GPU.  engine_step.hip gathers the PlanInputs, enqueues the BatchPlan and copies it into the batch trace.
#pragma once

#include <cstdlib>

namespace roft {
namespace host {

constexpr int kPlanLanes = 2;   // pose lanes (kNumLin of roft_device.h)

// The debugging / experiment switches of an engine, read ONCE when it is created.  Modes: 0 never, 1 the default rule (a function
// of batch index and object count), 2 whenever structurally possible, 3 (where it exists) by the batch index whatever the object
// count.  No setting changes a result.
struct SchedKnobs {
    int handoff_mode = 1;        // ROFT_HANDOFF: frame-granular hand-over velocity filter -> pose lanes
    int prep_mode = 1;           // ROFT_PREP_AHEAD: control blocks + mask ingest of a batch on the upload stream
    int part_mode = 1;           // ROFT_MASK_PART_GATE: velocity chain released one mask frame before the mask chain ends
    int feat_mask_mode = 1;      // ROFT_FEAT_ON_MASK: feature kernel of a batch on the mask stream (1: at most one object per sixteen CUs)
    int lanes_wait_skf = 1;      // ROFT_LANES_WAIT_SKF=0: lanes behind an event wait for the features behind the filter too
    int early_lanes = 1;         // ROFT_EARLY_LANES=0: no lane is released behind the control blocks alone (several PROCESSES on one GPU)
    int ctrl_ingest = 1;         // ROFT_CTRL_INGEST=0: control blocks and mask ingest always in two launches
    int gather_copy = 1;         // ROFT_GATHER_COPY=0: one copy per small pinned HOST image instead of one gather launch
    int outlier_steady_div = 2;  // ROFT_OUTLIER_STEADY_DIV: divisor of the automatic outlier band count in steady batches (<= 1: none)
    bool host_prof = false;            // ROFT_HOST_PROF=1: host time of the sections of submit / step, printed at destroy
    bool host_prof_per_batch = false;  // ROFT_HOST_PROF=1+: ... and after every batch
    bool one_stream = false;           // ROFT_ONE_STREAM=1: every chain on one stream
};

inline SchedKnobs knobs_from_env()
{
    SchedKnobs k;
    auto num = [](const char* name, int& v) { const char* s = getenv(name); if (s) v = atoi(s); return s != nullptr; };
    num("ROFT_HANDOFF", k.handoff_mode);
    num("ROFT_PREP_AHEAD", k.prep_mode);
    num("ROFT_MASK_PART_GATE", k.part_mode);
    num("ROFT_FEAT_ON_MASK", k.feat_mask_mode);
    // A tool that lets only ONE kernel run at a time (rocprofv3 --pmc: counter collection serialises the dispatches) cannot run a
    // lane next to the velocity filter it waits for -- the runtime's stream-wait itself is a kernel that spins: off under it.
    // (The rule yields to an explicit ROFT_LANES_WAIT_SKF, not to ROFT_HANDOFF.)
    if (!num("ROFT_LANES_WAIT_SKF", k.lanes_wait_skf) && getenv("ROCPROF_COUNTER_COLLECTION")) k.handoff_mode = 0;
    num("ROFT_EARLY_LANES", k.early_lanes);
    num("ROFT_CTRL_INGEST", k.ctrl_ingest);
    num("ROFT_GATHER_COPY", k.gather_copy);
    num("ROFT_OUTLIER_STEADY_DIV", k.outlier_steady_div);
    const char* hp = getenv("ROFT_HOST_PROF");
    k.host_prof = hp && hp[0] == '1';
    k.host_prof_per_batch = k.host_prof && hp[1] == '+';
    const char* one = getenv("ROFT_ONE_STREAM");
    k.one_stream = one && one[0] == '1';
    return k;
}

// What a submit call leaves behind for the plan of its batch: declared once, kept by the engine (PendingBatch in engine_internal.h)
// and read by plan_batch as part of its PlanInputs.
struct SubmitFacts {
    int T = 1;                      // frames of the batch
    bool had_uploads = false;       // HOST inputs were copied
    // camera images / raw depth: the submit enqueued production (pyramids, flows, deferred flow clones; depth products) on the upload
    // stream behind its copies (ev_up is recorded behind it, uploads or not)
    bool produced_flows = false;
    unsigned plain_mask_frames = 0; // bit t: frame t delivers a per-object byte mask (what the ingest of the control-block launch converts)
    int label_sets = 0;             // distinct (frame, label image) pairs of the batch: masks delivered as label images
    int pose_masks = 0;             // (frame, object) pairs of the batch whose mask is the silhouette of a delivered pose (masks from poses)
    int pose_resolve = 0;           // ... of those, the pairs drawn against at least one other object of their scene on their frame
    bool any_feat = false, any_feat_now = false;
    bool feat_dep_in_batch = false; // an outlier test of the batch reads features buffered by a frame of the same batch
    int n_segments[kPlanLanes] = {1, 1};          // pose chain segments per lane (1 + outlier tests of the busiest object)
    bool lin_any[kPlanLanes] = {false, false};    // some object has a frame on the lane in the batch
    // per lane: objects with a frame on the lane, and how many of them START with a step whose twist was published by an EARLIER batch
    // (the first step of a re-sync replay reads the twist of pose_frames_between frames ago): such a lane can run its first segment --
    // and the outlier test behind it -- before this batch's velocity filter exists
    int lane_objs[kPlanLanes] = {0, 0}, lane_old_first[kPlanLanes] = {0, 0};
    int relabel_wait[kPlanLanes] = {-1, -1};      // batch of the OTHER lane this lane's launches must follow (slots that changed lanes)
};

// Everything a batch's plan depends on.  Counters and counts only -- never a timing (the launch graph of a run is reproducible).
struct PlanInputs : SubmitFacts {
    SchedKnobs knobs;
    bool multi = true;              // the chains have streams of their own (!knobs.one_stream)
    bool timing = false;            // roft_engine_enable_timing
    int timing_level = 2;           // 2: markers between the launch groups
    bool wait_value_ok = true;      // the device can make a stream wait for a value in memory
    bool have_skf_started = true;   // the counter the resident-workgroup gate waits on exists
    int n_obj = 0, cus = 256;
    int batch_counter = 0, idle_mark = 0, lead = 6, completed_batches = 0;
    int outlier_bands_per_alternative = 0;
    // the stream set
    bool conflict_free = false;         // probed: no two of its busy streams share a hardware queue
    bool up_stream_distinct = true;     // the upload stream is not the mask stream
    // the batch ring
    bool feat_used_two_back = false;    // batch b - 2 ran a feature kernel on the mask stream
    bool vel_used_prev = false;         // batch b - 1 ended its velocity chain with ev_vel
    bool done_used_relabel[kPlanLanes] = {false, false};   // the other lane had work in batch relabel_wait[lane]
    // track quality (roft_engine_enable_quality): frames of the batch that get a record (0: quality off, or no frame of the batch is due)
    int quality_frames = 0;
};

// how a span (a launch group on one stream) signals its event
enum class Signal {
    none,     // it does not
    stop,     // the stop event of its last kernel: costs neither the barrier packet nor the host call of a record behind it
    record,   // recorded behind it (full timing: the markers between the launches carry the events' roles as well)
};
enum class FeatRun { none, mask_stream, behind_skf };
enum class VelWait { none, ev_ctrl, ev_part, ev_mask };
enum class Release {
    none,      // one stream, or no work
    ev_vel,    // (a) the batch's velocity chain has ended
    ev_skf,    // (a) the batch's velocity filter has ended
    gate,      // (b) every workgroup of the batch's velocity filter is resident
    ctrl_only, // (c) the batch's control blocks are on the device
};

struct LanePlan {
    bool early = false;           // (c) holds for the lane, with work or without (the trace's bit)
    bool wait_relabel = false;    // slots handed over to this lane: behind ev_done of the other lane in batch relabel_wait
    Release release = Release::none;
    bool wait_feat = false;       // ... and ev_feat: a test of the lane reads a set this batch's mask-stream feature kernel buffers
    bool wait_prev_vel = false;   // the first outlier test waits for ev_vel of the batch before
    bool gate_second = false;     // the second segment is held at the resident-workgroup gate
    Signal ev_done = Signal::none;
};

struct BatchPlan {
    bool steady = false, handoff = false;
    bool early_lanes = false;   // both lanes are early because the device has CUs to spare
    // preparation: control blocks + mask ingest
    bool prep = false;          // on the upload stream, ahead of the mask chain
    bool prep_waits_mask = false, prep_waits_feat = false;   // ... behind ev_mask (and ev_feat) of batch b - 2
    bool wait_up = false;       // the mask stream waits for ev_up
    bool try_fused = false;     // control blocks + ingest in one launch, if the launcher accepts
    bool label_ingest = false;  // one more launch behind them: every label image of the batch, all of its objects
    bool pose_silhouettes = false;   // one more launch behind those: every silhouette of the batch (the preparation's last launch is the last of these that exists)
    bool pose_resolve = false;       // silhouettes to resolve: the silhouette launch draws them against z-buffers, and a resolve launch follows it
    Signal ev_ctrl = Signal::none, ev_prep = Signal::none;
    // mask frames and features
    bool part_gate = false;     // the mask chain signals ev_part with the masks of frames 0 .. T - 2
    Signal ev_mask = Signal::none;
    FeatRun feat = FeatRun::none;
    Signal ev_feat = Signal::none;
    // velocity chain (FeatRun::behind_skf: the feature kernel carries ev_vel, else the filter does)
    VelWait vel_waits = VelWait::none;
    bool feat_waits_mask = false;   // the feature kernel behind the filter waits for ev_mask (the filter only waited for ev_part)
    Signal ev_skf = Signal::none, ev_vel = Signal::none;
    LanePlan lane[kPlanLanes];
    int outlier_div = 1;        // the automatic band count of an outlier test is divided by this
    // track quality: ONE launch for every (frame, object) of the batch that gets a record, behind the last segment of the LAST pose
    // lane on that lane's stream (frames of one batch belong to either lineage: it reads the log rows of both lanes)
    bool quality = false;
    bool quality_waits_mask = false;    // ... behind ev_mask of the batch (a lane released early may run before the batch's last mask)
    bool quality_waits_lane = false;    // ... and behind ev_done of the other lane, where that lane had work
    Signal ev_quality = Signal::none;   // what the host waits for (in-flight bound, roft_sync)
};

// PROGRESS -- why no wait INSIDE a kernel can hang.  (Ordering, i.e. the waits between streams: engine_step.hip.)
//
// The only waits inside kernels are the frame-granular hand-over (a pose lane's step waits for the tag of the twist it needs,
// k_ukf.hip ukf_one_step; the velocity filter publishes value then tag, k_skf.hip).  A lane kernel is released in one of three
// ways (Release), each of which guarantees that what it waits for RUNS:
//   (a) behind ev_skf / ev_vel: the velocity filter of the batch has ended -- nothing is waited for in the kernel;
//   (b) `handoff`: behind a stream-wait on skf_started >= (all velocity-filter workgroups of the batch): every producer
//       workgroup is RESIDENT on a CU when the lane starts, so the lane only waits for workgroups that run;
//   (c) an early lane: behind the batch's control blocks only, while the producer may not even be enqueued (it sits behind the
//       mask chain on another stream).  Progress then needs (i) a hardware queue of its own for each of the four chains -- the
//       stream set was PROBED free of conflicts, else (c) is off --, (ii) CUs the spinning lanes do not hold: at most one
//       waiting object per eight CUs, all of the lane's workgroups together at most half the device, counted over THIS engine,
//       which is only meaningful while it is the only engine of the process on the device (`alone`: a count of stream sets in
//       use, taken at the submit -- never a timing); several PROCESSES on one GPU set ROFT_EARLY_LANES=0.
// Every in-kernel wait is bounded (two seconds on the device clock): it then raises ROFT_DEV_ERROR_TWIST_WAIT, the step is NOT
// applied, and the next synchronisation returns ROFT_ERR_DEVICE -- a wrong assumption above costs a batch, not a hang.
//
// `alone` is asked (it takes a lock) only when every cheaper condition of (c) holds.
template <class AloneFn>
BatchPlan plan_batch(const PlanInputs& in, AloneFn&& alone)
{
    const SchedKnobs& k = in.knobs;
    BatchPlan p;
    const bool multi = in.multi;
    const bool batch = multi && in.T > 1;
    const bool full = in.timing && in.timing_level > 1;
    auto ends = [full](bool signalled) { return !signalled ? Signal::none : full ? Signal::record : Signal::stop; };
    auto by_mode = [](int mode, bool by_index, bool by_count) { return mode == 2 || (mode == 3 && by_index) || (mode == 1 && by_index && by_count); };
    const bool cus_to_spare = 8 * in.n_obj <= in.cus;
    const bool own_sets = in.feat_dep_in_batch || in.any_feat_now;   // an outlier test of the batch reads features this very batch buffers

    // A function of the batch INDEX alone: at least `lead` batches have been stepped since the engine was last idle, i.e. the
    // submit call may have to wait for the in-flight bound.  Bursts favour latency, steady batches occupancy.
    p.steady = in.batch_counter - in.idle_mark >= in.lead;

    // Hand-over: not when a test reads features of this very batch (they are extracted behind the filter), not on one stream,
    // and -- by default -- only in bursts: a lane that waits inside its kernel holds the CU it waits on, which a full pipeline
    // cannot spare ... unless the device has CUs to spare anyway (at most one object per eight CUs: 32 on an MI355X -- always
    // handing over is worth +4 - 6 % at 8 and 32 objects in 60-step runs, +1 - 2 % in the steady state at 32, -1 % at 64).
    p.handoff = batch && k.handoff_mode > 0 && in.wait_value_ok && !(k.handoff_mode == 1 && p.steady && !cus_to_spare) && !own_sets &&
                in.have_skf_started;
    // (c).  In the steady state a lane is behind anyway, and at 1280x720 the early tests cost 3 %.
    const bool early_ok = p.handoff && !p.steady && k.early_lanes != 0 && in.conflict_free && alone();
    p.early_lanes = early_ok && cus_to_spare;
    bool any_early = false;
    for (int l = 0; l < kPlanLanes; ++l) {
        // ... and, whatever the number of objects: a lane whose objects START the batch with the first step of a re-sync replay.
        // That step reads the twist of pose_frames_between frames ago -- published by an earlier batch -- and ends the lane's
        // first segment (the outlier test follows it): segment and test need nothing of this batch but its control blocks, so in
        // a burst they run next to the batch's mask frames instead of behind its velocity filter, and only the SECOND segment
        // (the rest of the replay: this batch's twists) is held at the gate.  The few objects of the lane that are out of phase
        // (a dropped pose: they start with an ordinary step) wait for their twist inside the kernel, on CUs nobody needs -- at
        // most one per eight CUs.  The replay-first objects wait too -- for a twist of the batch BEFORE, whose velocity filter is
        // enqueued and may still be publishing: all of the lane's workgroups together leave it half the device.
        p.lane[l].early = p.early_lanes || (early_ok && in.n_segments[l] > 1 && in.lane_old_first[l] > 0 &&
                                            8 * (in.lane_objs[l] - in.lane_old_first[l]) <= in.cus && 2 * in.lane_objs[l] <= in.cus);
        any_early = any_early || p.lane[l].early;
    }

    // Preparation ahead: on the UPLOAD stream, so that it happens while the mask chain of the batch before is still walking --
    // the mask stream is the longest serial chain of the steady state (14 + 38 + 200 us of a 252 us period, and the 38 us were
    // this preparation).  What it writes was last read by the mask chain TWO batches back (tables and ingest slots of its
    // parity; the chain in between reads one row of them as its carry, but none of the counters that are reset), and by the
    // feature kernel behind that chain, where there was one (it reads the control blocks of its batch): it waits for both.
    // Only in the steady state: in a burst the mask stream is not behind, and the event between the two streams is one more
    // hop on the first batches' critical path (one box: 120 steps +1.5 %; 20 steps -5 % and 8 objects -5 % if bursts did the
    // same).  And only when the device is full: with fewer objects a batch is a chain of latencies at every load and the mask
    // stream is never the longest one (60 steps, 16 / 32 objects: 5.2e5 / 9.4e5 with it in steady batches, 5.8e5 / 1.02e6 without).
    p.prep = batch && in.up_stream_distinct && by_mode(k.prep_mode, p.steady, !cus_to_spare);
    p.prep_waits_mask = p.prep && in.batch_counter >= 2;
    p.prep_waits_feat = p.prep_waits_mask && in.feat_used_two_back;
    p.wait_up = multi && (in.had_uploads || in.produced_flows) && !p.prep;   // (prep: same stream as the uploads and the flow production)
    // Otherwise control blocks and the ingest of the delivered masks in ONE launch -- on the mask stream they and the first mask
    // frame were three dependent launches (27 - 35 us in front of the frame).  Not under timing: the marks name the two kernels.
    p.try_fused = k.ctrl_ingest != 0 && !p.prep && in.plain_mask_frames != 0 && !in.timing;
    p.ev_ctrl = (multi && (in.T == 1 || any_early)) ? Signal::stop : Signal::none;
    // Masks that arrive as label images: ONE launch for all of them, whatever the number of objects, frames and images, behind the
    // control blocks (it reads the table that travels with them) and whatever ingest there is of per-object masks; a batch
    // without label images enqueues what it always did.
    p.label_ingest = in.label_sets > 0;
    // Masks from poses: ONE launch for every silhouette of the batch, in the same place and by the same rule -- it reads the control
    // blocks (the poses travel in them) and the resident meshes, nothing the batch computes: on the upload stream when the
    // preparation runs ahead.  A batch without silhouettes enqueues what it always did.
    p.pose_silhouettes = in.pose_masks > 0;
    // Silhouettes of one scene that hide each other: the same launch draws them against z-buffers (cleared in front of it) and ONE
    // resolve launch follows, the preparation's last by the same rule.  A batch with nothing to resolve launches nothing new.
    p.pose_resolve = p.pose_silhouettes && in.pose_resolve > 0;
    p.ev_prep = !p.prep ? Signal::none
                : (full || (in.plain_mask_frames == 0 && !p.label_ingest && !p.pose_silhouettes)) ? Signal::record : Signal::stop;   // (no ingest: no kernel to end with it)

    // In a burst the velocity chain is released when the masks its flow measurements read are complete -- frames 0 .. T - 2: the
    // measurement of frame t is taken inside the mask of frame t - 1 --, one mask frame (the one that chases a delivered mask
    // through six flows, the longest) before the chain ends.  Not in the steady state: latency buys nothing there, and the event
    // costs the mask stream one more small launch.  And only with CUs to spare: with 64 objects the flow measurement then runs
    // NEXT to the longest mask frame instead of behind it and takes 48 us instead of 30 for no gain in the window
    // (1.084 / 1.072e6), while 16 objects gain 5 - 9 %.
    p.part_gate = batch && by_mode(k.part_mode, !p.steady, cus_to_spare);
    p.ev_mask = ends(multi);

    // Features of the batch's pose frames (they read the planes the mask chain just wrote).  Batches: behind the velocity filter
    // -- that stream has waited for this mask chain, has time to spare, and the pose lanes wait for its end anyway, so the
    // features cost the mask chain nothing and need no event of their own.  One-frame submits: on the mask stream ... and so do
    // batches of an engine with MANY CUs to spare (at most one object per sixteen CUs): there a batch is a chain of latencies on
    // every stream and the velocity stream's is the longest (120 steps: 8 objects 3.46e5 -> 3.64e5, 16 objects 6.46e5 -> 6.62e5;
    // 32 objects -4 %, 64 objects -7.5 %).  On the mask stream the kernel always ends with ev_feat -- a stop event costs nothing
    // --: the host waits for it, and so does a preparation ahead that rewrites the control blocks it reads.
    const bool feat_behind_skf = batch && !(k.feat_mask_mode == 2 || (k.feat_mask_mode == 1 && 16 * in.n_obj <= in.cus));
    p.feat = !in.any_feat ? FeatRun::none : feat_behind_skf ? FeatRun::behind_skf : FeatRun::mask_stream;
    p.ev_feat = ends(multi && p.feat == FeatRun::mask_stream);

    // Velocity chain: the measurement of frame k needs the control blocks and the mask planes of frame k - 1 -- the previous
    // batch's for a one-frame batch (ordered by the upload, which follows that batch's mask chain), this batch's otherwise.
    p.vel_waits = !multi ? VelWait::none : in.T == 1 ? VelWait::ev_ctrl : p.part_gate ? VelWait::ev_part : VelWait::ev_mask;
    p.feat_waits_mask = p.feat == FeatRun::behind_skf && p.part_gate;   // (the planes of the batch's last frame)
    // With the feature kernel behind it the filter's own event is ev_skf: a lane that waits for the batch's twists does not wait
    // for the features as well -- 39 us at 64 objects --, which its tests read from sets buffered by EARLIER batches.
    const bool lanes_wait_skf = p.feat == FeatRun::behind_skf && k.lanes_wait_skf != 0 && !own_sets;
    p.ev_skf = ends(lanes_wait_skf);
    p.ev_vel = ends(multi);

    // The lanes wait for ev_feat only when they need this batch's sets: with one-frame batches the set a test reads was buffered
    // by an earlier batch -- covered by ev_vel, since the velocity chain waited for the mask chain of the batch before -- unless
    // it is this very frame's.
    const bool lanes_wait_feat = p.ev_feat != Signal::none && (in.T > 1 || in.any_feat_now);
    for (int l = 0; l < kPlanLanes; ++l) {
        LanePlan& lp = p.lane[l];
        const int wb = in.relabel_wait[l];
        lp.wait_relabel = multi && wb >= in.completed_batches && wb < in.batch_counter && in.done_used_relabel[l];
        if (!in.lin_any[l]) continue;
        lp.ev_done = ends(true);   // (on one stream too: the in-flight bound waits for it)
        if (!multi) continue;
        const bool tests = in.n_segments[l] > 1;
        if (lp.early) {
            lp.release = Release::ctrl_only;
            // (its OUTLIER TEST waits for the velocity chain of the batch before -- its features kernel, ~35 us behind the
            //  filter's last twist: the sets this batch's tests read were buffered there or earlier)
            lp.wait_prev_vel = tests && in.batch_counter - 1 >= in.completed_batches && in.batch_counter >= 1 && in.vel_used_prev;
            lp.gate_second = !p.early_lanes;   // (released for its replay's first step: what follows needs this batch's twists)
        } else if (p.handoff) {
            lp.release = Release::gate;
        } else {
            lp.release = lanes_wait_skf ? Release::ev_skf : Release::ev_vel;
            lp.wait_feat = lanes_wait_feat && tests;
        }
    }

    // Track quality.  Nothing of this exists in the plan of a batch without records -- no launch, no event, no wait.  The launch
    // reads the batch's log rows (both lanes: it follows the last lane's last segment in stream order and waits for the other
    // lane's ev_done), the batch's mask planes and, through the planes' producer, its depth (ev_mask: the mask stream waited for the
    // uploads; a lane released at the gate or behind the control blocks alone does not imply the batch's last mask frame).
    p.quality = in.quality_frames > 0;
    p.quality_waits_mask = p.quality && multi;
    p.quality_waits_lane = p.quality && multi && in.lin_any[0];
    p.ev_quality = ends(p.quality);   // (on one stream too: the in-flight bound waits for it)

    // Bands per alternative of an outlier test: the caller's number, else by the CUs to spare -- and a fraction of that in the
    // steady state (fewer, longer workgroups leave more CUs to the chains; 64 objects: +5 %, and -2.5 % if a 20-frame burst did
    // the same).  The likelihood sums are exact, so the band count changes no result.
    p.outlier_div = (in.outlier_bands_per_alternative == 0 && p.steady && k.outlier_steady_div > 1) ? k.outlier_steady_div : 1;
    return p;
}

// The launches of a batch's preparation behind its control blocks, in the order they are enqueued.  The last of those that exist
// ends with ev_prep where the plan binds the event to a launch (Signal::stop).
enum class PrepLaunch { none, mask_ingest, label_ingest, pose_silhouettes, pose_resolve };
inline PrepLaunch prep_last_launch(const BatchPlan& p, unsigned plain_mask_frames)
{
    return p.pose_resolve ? PrepLaunch::pose_resolve
           : p.pose_silhouettes ? PrepLaunch::pose_silhouettes
           : p.label_ingest ? PrepLaunch::label_ingest
           : plain_mask_frames ? PrepLaunch::mask_ingest : PrepLaunch::none;
}
// kernel launches of the silhouette stage: none, the one-pass launch, or draw + resolve
inline int pose_silhouette_launches(const BatchPlan& p) { return p.pose_resolve ? 2 : p.pose_silhouettes ? 1 : 0; }

}  // namespace host
}  // namespace roft
