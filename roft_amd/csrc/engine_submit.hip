// engine_submit.hip -- roft_frames_submit / roft_frame_submit: what depends only on the delivery schedule is resolved here, on the
// host, into one FrameCtrl block per object and frame (the frame program: build_pose_program), HOST inputs are staged, the
// lanes are balanced.  Reference: ROFTFilter::filtering_step (src/roft-lib/src/ROFTFilter.cpp:255-452),
// CartesianQuaternionMeasurement::freeze (src/roft-lib/src/CartesianQuaternionMeasurement.cpp:92-348),
// ImageSegmentationOFAidedSource::step_frame (include/ROFT/ImageSegmentationOFAidedSource.hpp:127-231).
#include "engine_internal.h"

// The UKF steps of one frame (ROFTFilter.cpp:327-367 over CartesianQuaternionMeasurement::freeze, cpp:92-348).
// Returns false when the frame needs more than kMaxSteps steps.
bool build_pose_program(const roft_config& cfg, Sched& o, const roft_frame_input& in, FrameCtrl& c)
{
    const int slot = o.frame_idx % kTwistRing;
    c.twist_slot = slot;
    int n = 0;
    bool overflow = false;
    auto add = [&](StepDesc sd) { if (n < kMaxSteps) c.steps[n++] = sd; else overflow = true; };
    auto vel_pop_front = [&]() { std::memmove(o.vel_buf, o.vel_buf + 1, sizeof(int) * (size_t)(--o.n_vel)); };

    // CartesianQuaternionMeasurement::freeze(Standard)  (cpp:176-347)
    const bool has_vel = cfg.use_velocity != 0;
    const bool is_pose = cfg.use_pose && in.pose_valid;
    int type = ROFT_MEAS_NONE;
    if (has_vel && is_pose) type = ROFT_MEAS_POSE_VELOCITY;
    else if (has_vel) type = ROFT_MEAS_VELOCITY;
    else if (is_pose) type = ROFT_MEAS_POSE;
    if (has_vel) {
        // (only the last pose_frames_between + 1 entries are ever replayed; the ring bounds the rest)
        if (o.n_vel == kTwistRing) vel_pop_front();
        o.vel_buf[o.n_vel++] = slot;
        while (o.n_vel > kMaxSteps + 2) vel_pop_front();
        o.last_meas_slot = slot;
    }
    for (int i = 0; i < 3; ++i) c.pose_x[i] = in.pose_x[i];
    for (int i = 0; i < 4; ++i) c.pose_q[i] = in.pose_q[i];

    if (type == ROFT_MEAS_POSE_VELOCITY && cfg.use_pose_resync) {
        // ROFTFilter.cpp:333-340: buffered_belief_ <- p_corr_belief_, p_corr_belief_ <- the old buffered_belief_.
        // The two Gaussians swap roles; nothing is copied (see BeliefSlot in roft_device.h).
        o.cur_slot ^= 1;
    }
    const int cur = B_LIN0 + o.cur_slot;
    const int lin = o.own[o.cur_slot];
    c.lane = lin;
    c.cur_slot = cur;
    StepDesc sd{};
    sd.op = 1;
    sd.src = cur;
    sd.do_predict = 1;
    sd.twist_slot = slot;
    if (type == ROFT_MEAS_POSE_VELOCITY) {
        if (cfg.use_pose_resync) {
            // ROFTFilter.cpp:331-354: continue from the belief buffered at the previous pose arrival and
            // replay the buffered velocities (PopBufferedMeasurement, cpp:97-154)
            bool pose_pending = true;
            for (;;) {
                if (cfg.pose_frames_between > 0)
                    while (o.n_vel > cfg.pose_frames_between + 1) vel_pop_front();
                if (o.n_vel == 0) { o.vel_buf[o.n_vel++] = o.last_meas_slot; break; }
                const int ts = o.vel_buf[0];
                vel_pop_front();
                o.last_meas_slot = ts;
                StepDesc r{};
                r.op = 1;
                r.do_predict = 1;
                r.twist_slot = ts;
                r.src = cur;
                if (pose_pending) {
                    pose_pending = false;
                    if (cfg.outlier_rejection) {
                        r.n_corr = 2;
                        r.type[0] = ROFT_MEAS_POSE_VELOCITY; r.dst[0] = b_alt(lin, 0);
                        r.type[1] = ROFT_MEAS_VELOCITY;      r.dst[1] = b_alt(lin, 1);
                        c.outlier_step = n;
                    } else {
                        r.n_corr = 1;
                        r.type[0] = ROFT_MEAS_POSE_VELOCITY; r.dst[0] = cur;
                    }
                } else {
                    r.n_corr = 1;
                    r.type[0] = ROFT_MEAS_VELOCITY; r.dst[0] = cur;
                }
                add(r);
            }
            // the test reads the features buffered at the previous pose arrival; this frame's are buffered for
            // the next one (ROFTFilter.cpp:353)
            c.feat_read = o.feat_slot;
            if (c.feat_write < 0) { c.feat_write = o.feat_next; o.feat_next = (o.feat_next + 1) % kFeatRing; }
            o.feat_slot = c.feat_write;
        } else {
            if (cfg.outlier_rejection) {
                sd.n_corr = 2;
                sd.type[0] = ROFT_MEAS_POSE_VELOCITY; sd.dst[0] = b_alt(lin, 0);
                sd.type[1] = ROFT_MEAS_VELOCITY;      sd.dst[1] = b_alt(lin, 1);
                c.outlier_step = n;
                // without re-sync the test uses the current frame's depth and mask
                if (c.feat_write < 0) { c.feat_write = o.feat_next; o.feat_next = (o.feat_next + 1) % kFeatRing; }
                c.feat_read = c.feat_write;
                o.feat_slot = c.feat_write;
            } else {
                sd.n_corr = 1;
                sd.type[0] = ROFT_MEAS_POSE_VELOCITY; sd.dst[0] = cur;
            }
            add(sd);
        }
    } else if (type != ROFT_MEAS_NONE) {
        sd.n_corr = 1;
        sd.type[0] = type; sd.dst[0] = cur;
        add(sd);
    } else {
        sd.n_corr = 0;  // p_corr = p_pred (ROFTFilter.cpp:366-367)
        sd.dst[0] = cur;
        add(sd);
    }
    c.n_steps = n;
    return !overflow;
}

// `bytes` of the staging memory that is recycled with `frame`'s slot (bump allocation in 32 MB chunks)
static int stage_alloc(roft_engine* e, int frame, size_t bytes, unsigned char** out)
{
    StageFrame& sf = e->staging[frame % e->retain];
    const size_t need = (bytes + 255) & ~(size_t)255;
    while (sf.cur < sf.chunks.size() && sf.used + need > sf.chunks[sf.cur]->n) { ++sf.cur; sf.used = 0; }
    if (sf.cur == sf.chunks.size()) {
        auto* c = new DevBuf<unsigned char>();
        const hipError_t err = c->ensure(std::max(need, kStageChunk));
        if (err != hipSuccess) { delete c; return fail(ROFT_ERR_DEVICE, std::string("HOST staging memory: ") + hipGetErrorString(err)); }
        sf.chunks.push_back(c);
        sf.used = 0;
    }
    *out = sf.chunks[sf.cur]->p + sf.used;
    sf.used += need;
    return ROFT_OK;
}

// Many small HOST images -> their staging copies in ONE launch: workgroup (x, y) copies 16-byte units x, x + gridDim.x, ... of item y.
// The sources are PINNED host buffers the device can address (stage_host checks); a 300 KB hipMemcpyAsync costs ~11 us of
// which 6 are the transfer, and a delivery brings one mask per object: 64 copies = 0.7 ms per six frames in the shared-scene leg
// of bench.py (28 GB/s), against one kernel that keeps the link busy.
__global__ __launch_bounds__(256) void gather_copy_kernel(const GatherItem* __restrict__ tab)
{
    const GatherItem it = tab[blockIdx.y];
    const uint4* src = reinterpret_cast<const uint4*>(it.src);
    uint4* dst = reinterpret_cast<uint4*>(it.dst);
    const size_t n16 = it.bytes / 16;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// the items collected by stage_host during this submit -> one launch on the upload stream (before the submit waits for its uploads)
static int flush_gather(roft_engine* e)
{
    if (e->gather.empty()) return ROFT_OK;
    GatherItem*& tab = e->slot_of(e->batch_counter).gather_tab;
    if (!tab) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&tab), sizeof(GatherItem) * kGatherCap, hipHostMallocMapped));
    const size_t n = e->gather.size();
    std::memcpy(tab, e->gather.data(), sizeof(GatherItem) * n);
    size_t largest = 0;
    for (const GatherItem& g : e->gather) largest = std::max(largest, g.bytes);
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>(32, (largest / 16 + 2047) / 2048));   // ~8 units per thread
    hipLaunchKernelGGL(gather_copy_kernel, dim3(gx, (unsigned)n), dim3(256), 0, e->up_stream, tab);
    e->gather.clear();
    if (hipError_t le = hipGetLastError()) return fail(ROFT_ERR_DEVICE, std::string("gather copy of HOST inputs: ") + hipGetErrorString(le));
    e->stats.h2d_copies++;
    return ROFT_OK;
}

// the device address of a PINNED host buffer the GPU can read in place, or null (pageable memory, or not identity-mapped)
static const void* pinned_device_pointer(const void* host)
{
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (attr.type != hipMemoryTypeHost) return nullptr;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, const_cast<void*>(host), 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return dp;
}

// device copy of one HOST image of `frame` (uploads once per distinct host pointer and frame)
static int stage_host(roft_engine* e, int frame, const void* host, size_t bytes, const void** dev)
{
    StageFrame& sf = e->staging[frame % e->retain];
    for (auto& pr : sf.seen)
        if (pr.first == host) { *dev = pr.second; return ROFT_OK; }
    unsigned char* d = nullptr;
    if (int rc = stage_alloc(e, frame, bytes, &d)) return rc;
    const void* dp = nullptr;
    if (e->knobs.gather_copy && bytes <= kGatherMaxBytes && (bytes & 15) == 0 && (reinterpret_cast<uintptr_t>(host) & 15) == 0 &&
        (int)e->gather.size() < kGatherCap && (dp = pinned_device_pointer(host)) != nullptr) {
        e->gather.push_back(GatherItem{dp, d, bytes});   // fetched by flush_gather's one launch
        e->stats.h2d_bytes += (long long)bytes;
        e->had_uploads = true;
        sf.seen.emplace_back(host, d);
        *dev = d;
        return ROFT_OK;
    }
    HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, e->up_stream));
    e->stats.h2d_bytes += (long long)bytes;
    e->stats.h2d_copies++;
    e->had_uploads = true;
    sf.seen.emplace_back(host, d);
    *dev = d;
    return ROFT_OK;
}

// HOST images of consecutive frames of a batch that are CONSECUTIVE IN HOST MEMORY (a recorded sequence held as one
// [frames, H, W] array: frame t + 1 starts where frame t ends) are uploaded with ONE copy per run instead of one per frame --
// a 1.2 MB copy does not reach the link's rate, a batch's worth does (round 6: the shared-scene leg of bench.py moved 26 GB/s
// in per-frame copies against 43 GB/s in the per-object leg, whose 128 copies per frame keep the link busy by their number).
// The run lives in the staging slot of its LAST frame (recycled after every earlier one); each frame's slot learns where its
// image is, so that stage_host below finds it -- for every object that shows the same host pointer, too.
static int stage_host_runs(roft_engine* e, const roft_frame_input* inputs, int n_obj, int T, size_t depth_bytes, size_t flow_bytes_)
{
    if (T < 2) return ROFT_OK;
    const int frame0 = e->frame_counter;
    for (int kind = 0; kind < 2; ++kind) {
        const size_t bytes = kind == 0 ? depth_bytes : flow_bytes_;
        if (bytes == 0 || (bytes & 255)) continue;   // (the pieces of a run must keep the alignment a single image gets)
        for (int id = 0; id < n_obj; ++id) {
            auto ptr = [&](int t) -> const unsigned char* {
                const roft_frame_input& in = inputs[(size_t)t * n_obj + id];
                if (in.mem_kind != ROFT_MEM_HOST) return nullptr;
                return static_cast<const unsigned char*>(kind == 0 ? static_cast<const void*>(in.depth) : in.flow);
            };
            int t0 = 0;
            while (t0 < T) {
                int t1 = t0;
                const unsigned char* p0 = ptr(t0);
                if (p0)
                    while (t1 + 1 < T && ptr(t1 + 1) == p0 + (size_t)(t1 + 1 - t0) * bytes) ++t1;
                if (p0 && t1 > t0) {
                    bool known = false;   // (a shared scene: an object before this one brought the run)
                    for (auto& pr : e->staging[(frame0 + t0) % e->retain].seen)
                        if (pr.first == p0) { known = true; break; }
                    if (!known) {
                        const int len = t1 - t0 + 1;
                        unsigned char* d = nullptr;
                        if (int rc = stage_alloc(e, frame0 + t1, (size_t)len * bytes, &d)) return rc;
                        HIP_TRY(hipMemcpyAsync(d, p0, (size_t)len * bytes, hipMemcpyHostToDevice, e->up_stream));
                        e->stats.h2d_bytes += (long long)((size_t)len * bytes);
                        e->stats.h2d_copies++;
                        e->had_uploads = true;
                        if (kind == 0 && e->depth.enabled) e->depth.stats.image_bytes += (long long)((size_t)len * bytes);   // (raw frames)
                        for (int t = t0; t <= t1; ++t)
                            e->staging[(frame0 + t) % e->retain].seen.emplace_back(p0 + (size_t)(t - t0) * bytes, d + (size_t)(t - t0) * bytes);
                    }
                }
                t0 = t1 + 1;
            }
        }
    }
    return ROFT_OK;
}

namespace roft { int of_check_params(int W, int H, const roft_of_params* p); }   // flow_producer.hip

static size_t image_bytes(int type, size_t npix) { return type == ROFT_IMAGE_GRAY8 ? npix : 3 * npix; }

// The flow production of the accepted batch -> upload stream: a pyramid for each distinct image of each of its frames, then a flow
// for each distinct pair, then the clones of flows that aged out in the batch (they may read its products) -- the images and the
// pairs of ALL its frames in chunks of kOfChunk, whose pointers travel in the kernel arguments and whose workspace the next chunk
// reuses in stream order.  A batch of eight frames of a shared scene is one chunk of each: seven launches, not seven per frame.
static int enqueue_flow_production(roft_engine* e, int T)
{
    EngineFlow& f = e->flow;
    const size_t fbytes = flow_bytes(e->arr.a.ffmt);
    const size_t field_floats = (size_t)2 * e->cfg.cam.width * e->cfg.cam.height;
    const bool s16 = e->cfg.flow_type == ROFT_FLOW_S16C2;
    const int G = (int)f.pyr.size();
    OfImages im{};
    for (int t = 0; t < T; ++t) {
        const int gen = (e->frame_counter + t) % G;
        for (size_t i = 0; i < f.jobs[t].images.size(); ++i) {
            const int k = im.n++;
            im.type[k] = f.jobs[t].images[i].type; im.src[k] = f.jobs[t].images[i].dev; im.pyr[k] = f.pyr[gen][i]->p;
            if (im.n == kOfChunk) { launch_of_pyramids(f.geom, im, e->up_stream); im.n = 0; }
        }
    }
    if (im.n) launch_of_pyramids(f.geom, im, e->up_stream);
    OfPairs pr{};
    for (int t = 0; t < T; ++t) {
        const int gen = (e->frame_counter + t) % G, gen_prev = (e->frame_counter + t + G - 1) % G;
        for (const FlowPairJob& pj : f.jobs[t].pairs) {
            const int k = pr.n++;
            pr.pyr0[k] = f.pyr[gen_prev][pj.pyr0]->p;
            pr.pyr1[k] = f.pyr[gen][pj.pyr1]->p;
            pr.coarse[k] = f.coarse.p + (size_t)k * f.geom.flow_stride;
            pr.field[k] = s16 ? f.field.p + (size_t)k * field_floats : reinterpret_cast<float*>(pj.out);
            pr.out_s16[k] = s16 ? reinterpret_cast<int16_t*>(pj.out) : nullptr;
            if (pr.n == kOfChunk) { launch_of_pairs(f.geom, pr, e->up_stream); pr.n = 0; }
        }
    }
    if (pr.n) launch_of_pairs(f.geom, pr, e->up_stream);
    if (hipError_t le = hipGetLastError()) return fail(ROFT_ERR_DEVICE, std::string("flow production: ") + hipGetErrorString(le));
    for (int t = 0; t < T; ++t)
        for (const FlowCloneJob& c : f.jobs[t].clones) HIP_TRY(hipMemcpyAsync(c.dst, c.src, fbytes, hipMemcpyDeviceToDevice, e->up_stream));
    return ROFT_OK;
}

// The depth products of the accepted batch -> upload stream, behind the copies: all distinct raw images of the batch in one launch
// per phase (one for a conversion, three for an alignment), their pointers in the kernel arguments in chunks of kDepthChunk.
static int enqueue_depth_production(roft_engine* e)
{
    EngineDepth& d = e->depth;
    const size_t npix = (size_t)e->cfg.cam.width * e->cfg.cam.height;
    if (!d.ev0) { HIP_TRY(hipEventCreate(&d.ev0)); HIP_TRY(hipEventCreate(&d.ev1)); }
    HIP_TRY(hipEventRecord(d.ev0, e->up_stream));
    DepthJobs jobs{};
    auto launch = [&]() {
        if (d.src.align) launch_depth_align(jobs, d.geom, e->up_stream);
        else launch_depth_convert(jobs, npix, d.src.scale, e->up_stream);
        jobs.n = 0;
    };
    for (const DepthJob& j : d.jobs) {
        jobs.raw[jobs.n] = j.raw; jobs.out[jobs.n] = j.out;
        if (++jobs.n == kDepthChunk) launch();
    }
    if (jobs.n) launch();
    if (hipError_t le = hipGetLastError()) return fail(ROFT_ERR_DEVICE, std::string("depth production: ") + hipGetErrorString(le));
    HIP_TRY(hipEventRecord(d.ev1, e->up_stream));
    d.timed = true;
    return ROFT_OK;
}

static int submit_frames(roft_engine* e, const roft_frame_input* inputs, const roft_label_mask* labels, const roft_frame_image* images, int n_obj, int T)
{
    const roft_config& cfg = e->cfg;
    const size_t npix = (size_t)cfg.cam.width * cfg.cam.height;
    const size_t fbytes = flow_bytes(e->arr.a.ffmt);
    // what inputs[].depth carries: H x W floats, or on a raw-depth engine the sensor's 16-bit frame of the depth source's size
    const bool raw_depth = e->depth.enabled;
    const size_t depth_bytes = raw_depth ? e->depth.raw_pixels * sizeof(uint16_t) : npix * sizeof(float);
    const int b = e->batch_counter;
    FrameCtrl* blk = e->slot_of(b).stage;
    int max_outliers[kNumLin] = {0, 0};
    std::vector<int> n_outliers((size_t)n_obj * kNumLin, 0);
    e->lin_any[0] = e->lin_any[1] = false;
    e->lane_objs[0] = e->lane_objs[1] = e->lane_old_first[0] = e->lane_old_first[1] = 0;
    std::vector<unsigned char> lane_seen((size_t)n_obj * kNumLin, 0);
    {
        // Balance of the two pose chain lanes.  A lane's launch lasts as long as its busiest object, so the lanes only
        // overlap if, in every batch, the re-sync replays of all objects are on ONE lane and the ordinary steps in
        // front of them on the other.  An object that missed a pose (or received an extra one) has its lineages on the
        // opposite lanes from then on: hand its two slots over to the other lanes at the batch boundary.  The new lane
        // of a slot must run behind the last batch in which the old lane touched it (relabel_wait; in the steady state
        // that launch was a short one of the previous batch and has long ended).
        int cnt[kNumLin] = {0, 0};
        for (int id = 0; id < n_obj; ++id) cnt[e->objs[id]->s.own[e->objs[id]->s.cur_slot]]++;
        const int c = cnt[1] > cnt[0] ? 1 : 0;
        e->relabel_wait[0] = e->relabel_wait[1] = -1;
        for (int id = 0; id < n_obj; ++id) {
            Sched& o = e->objs[id]->s;
            if (o.own[o.cur_slot] == c) continue;
            e->relabel_wait[c] = std::max(e->relabel_wait[c], o.last_touch[o.cur_slot]);
            e->relabel_wait[1 - c] = std::max(e->relabel_wait[1 - c], o.last_touch[1 - o.cur_slot]);
            std::swap(o.own[0], o.own[1]);
        }
    }

    for (int t = 0; t < T; ++t) {   // the staging slots of the batch's frames are free again: every frame that could read them has ended (in-flight bound)
        StageFrame& sf = e->staging[(e->frame_counter + t) % e->retain];
        sf.cur = 0;
        sf.used = 0;
        sf.seen.clear();
    }
    if (int rc = stage_host_runs(e, inputs, n_obj, T, depth_bytes, fbytes)) return rc;
    for (int t = 0; t < T; ++t) {
        const int frame = e->frame_counter + t;
        for (int id = 0; id < n_obj; ++id) {
            HostObject& ho = *e->objs[id];
            Sched& o = ho.s;
            const roft_frame_input& in = inputs[(size_t)t * n_obj + id];
            FrameCtrl& c = blk[(size_t)t * n_obj + id];
            clear_ctrl(c);
            if (!in.depth) return fail(ROFT_ERR_INVALID, "cannot continue without a continuous depth stream (ROFTFilter.cpp:261-266)");
            c.dt = (in.dt > 0.0) ? in.dt : cfg.sample_time;

            // ---- inputs to device memory
            const float* d_depth;
            const void* d_flow = nullptr;
            const uint8_t* d_mask = nullptr;
            // the mask as the pixels of a label image equal to a value (roft_frames_submit_labels)
            const roft_label_mask* lm = (labels && labels[(size_t)t * n_obj + id].labels) ? &labels[(size_t)t * n_obj + id] : nullptr;
            const void* d_labels = nullptr;
            if (lm) {
                if (in.mask) return fail(ROFT_ERR_INVALID, "object " + std::to_string(id) + ": a label image AND a mask for one frame (one of the two)");
                if (lm->label_type != ROFT_LABEL_U8 && lm->label_type != ROFT_LABEL_U16)
                    return fail(ROFT_ERR_INVALID, "object " + std::to_string(id) + ": label_type must be ROFT_LABEL_U8 or ROFT_LABEL_U16");
                if (lm->label == 0) return fail(ROFT_ERR_INVALID, "object " + std::to_string(id) + ": label 0 is the background");
                if (lm->label < 0 || lm->label > (lm->label_type == ROFT_LABEL_U8 ? 255 : 65535))
                    return fail(ROFT_ERR_INVALID, "object " + std::to_string(id) + ": label " + std::to_string(lm->label) + " is outside the range of the label type");
            }
            // a camera image instead of a flow frame (roft_frames_submit_images)
            const roft_frame_image* fim = (images && images[(size_t)t * n_obj + id].image) ? &images[(size_t)t * n_obj + id] : nullptr;
            const void* d_image = nullptr;
            if (fim) {
                if (!e->flow.enabled) return fail(ROFT_ERR_STATE, "camera images need roft_engine_enable_flow before the first frame");
                if (in.flow) return fail(ROFT_ERR_INVALID, "object " + std::to_string(id) + ": a camera image AND a flow for one frame (one of the two)");
                if (fim->image_type != ROFT_IMAGE_GRAY8 && fim->image_type != ROFT_IMAGE_BGR8 && fim->image_type != ROFT_IMAGE_RGB8)
                    return fail(ROFT_ERR_INVALID, "object " + std::to_string(id) + ": image_type must be ROFT_IMAGE_GRAY8, ROFT_IMAGE_BGR8 or ROFT_IMAGE_RGB8");
            }
            if (in.mem_kind == ROFT_MEM_DEVICE) {
                d_depth = in.depth;
                if (fim) d_image = fim->image;
                d_flow = in.flow;
                d_mask = in.mask;
                if (lm) d_labels = lm->labels;
                // the first call of an engine only: a host pointer declared as device memory is a GPU page fault that takes
                // the process down at the first kernel -- the commonest mistake of a new binding is refused here instead
                if (!e->device_pointers_checked) {
                    const void* ptrs[5] = {in.depth, in.flow, in.mask, d_labels, d_image};
                    static const char* const what[5] = {"depth", "flow", "mask", "label image", "camera image"};
                    for (int q = 0; q < 5; ++q) {
                        if (!ptrs[q]) continue;
                        // device or managed memory, or host memory the GPU can address as it is (hipHostMalloc / hipHostRegister:
                        // pinned and mapped -- zero-copy over the bus); unregistered pageable memory is what is refused
                        hipPointerAttribute_t attr{};
                        const hipError_t pe = hipPointerGetAttributes(&attr, ptrs[q]);
                        if (pe != hipSuccess) (void)hipGetLastError();
                        bool usable = pe == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
                        if (!usable && pe == hipSuccess && attr.type == hipMemoryTypeHost) {
                            void* dp = nullptr;
                            usable = hipHostGetDevicePointer(&dp, const_cast<void*>(ptrs[q]), 0) == hipSuccess && dp == ptrs[q];
                            if (!usable) (void)hipGetLastError();
                        }
                        if (!usable)
                            return fail(ROFT_ERR_INVALID, std::string("mem_kind is ROFT_MEM_DEVICE but the ") + what[q] + " pointer of object " +
                                                              std::to_string(id) + " is neither device memory nor pinned, mapped host memory "
                                                              "(pass ROFT_MEM_HOST for ordinary host buffers)");
                    }
                }
                if ((reinterpret_cast<uintptr_t>(d_mask) & 15) || (reinterpret_cast<uintptr_t>(d_flow) & 7) ||
                    (reinterpret_cast<uintptr_t>(d_depth) & 3))
                    return fail(ROFT_ERR_INVALID, "device buffers must be aligned: mask 16 B, flow 8 B, depth 4 B");
                if (reinterpret_cast<uintptr_t>(d_labels) & 15) return fail(ROFT_ERR_INVALID, "device buffers must be aligned: label image 16 B");
                if (reinterpret_cast<uintptr_t>(d_image) & 3) return fail(ROFT_ERR_INVALID, "device buffers must be aligned: camera image 4 B");
            } else if (in.mem_kind == ROFT_MEM_HOST) {
                const void* p = nullptr;
                const long long before_depth = e->stats.h2d_bytes;
                if (int rc = stage_host(e, frame, in.depth, depth_bytes, &p)) return rc;
                if (raw_depth) e->depth.stats.image_bytes += e->stats.h2d_bytes - before_depth;   // (uploaded, and counted, once per distinct pointer)
                d_depth = static_cast<const float*>(p);
                if (in.flow) { if (int rc = stage_host(e, frame, in.flow, fbytes, &d_flow)) return rc; }
                if (in.mask) {
                    if (int rc = stage_host(e, frame, in.mask, npix, &p)) return rc;
                    d_mask = static_cast<const uint8_t*>(p);
                }
                if (lm) { if (int rc = stage_host(e, frame, lm->labels, npix * (lm->label_type == ROFT_LABEL_U8 ? 1 : 2), &d_labels)) return rc; }
                if (fim) {
                    const long long before = e->stats.h2d_bytes;   // (the objects of a shared scene name one image: uploaded, and counted, once)
                    if (int rc = stage_host(e, frame, fim->image, image_bytes(fim->image_type, npix), &d_image)) return rc;
                    e->flow.stats.image_bytes += e->stats.h2d_bytes - before;
                }
            } else {
                return fail(ROFT_ERR_INVALID, "mem_kind must be ROFT_MEM_HOST or ROFT_MEM_DEVICE");
            }

            // ---- raw depth: d_depth is the device address of the 16-bit frame so far.  Its float product goes where a staged HOST depth
            // of the frame would have been copied, one per distinct raw image and frame however many objects name it.
            if (raw_depth) {
                const uint16_t* d_raw = reinterpret_cast<const uint16_t*>(d_depth);
                float* made = nullptr;
                for (size_t i = e->depth.jobs.size(); i-- > 0 && e->depth.jobs[i].t == t;)
                    if (e->depth.jobs[i].raw == d_raw) { made = e->depth.jobs[i].out; break; }
                if (!made) {
                    unsigned char* out = nullptr;
                    if (int rc = stage_alloc(e, frame, npix * sizeof(float), &out)) return rc;
                    made = reinterpret_cast<float*>(out);
                    e->depth.jobs.push_back(DepthJob{t, d_raw, made});
                    e->depth.stats.images++;
                    e->depth.stats.products++;
                    e->produced_flows = true;   // (production behind the copies: ev_up is recorded behind it)
                }
                d_depth = made;
            }

            // ---- the flow of a camera image: produced where a staged HOST flow of the frame would have been copied, one pyramid per
            // distinct image and one flow per distinct (previous, current) pair of the frame; none without an image the frame before
            int pyr_cur = -1;
            if (fim) {
                EngineFlow& f = e->flow;
                FlowFrameJobs& fj = f.jobs[t];
                for (size_t i = 0; i < fj.images.size() && pyr_cur < 0; ++i)
                    if (fj.images[i].dev == d_image && fj.images[i].type == fim->image_type) pyr_cur = (int)i;
                if (pyr_cur < 0) {
                    pyr_cur = (int)fj.images.size();
                    fj.images.push_back(FlowImageJob{d_image, fim->image_type});
                    std::vector<DevBuf<float>*>& gen = f.pyr[(size_t)frame % f.pyr.size()];
                    if ((int)gen.size() <= pyr_cur) {
                        auto* pb = new DevBuf<float>();
                        gen.push_back(pb);
                        HIP_TRY(pb->ensure(f.geom.pyr_stride));
                    }
                    f.stats.images++;
                    f.stats.pyramids++;
                    e->produced_flows = true;   // (a pyramid to build, also where no pair follows in this batch)
                }
                if (o.pyr_prev >= 0) {
                    for (const FlowPairJob& pj : fj.pairs)
                        if (pj.pyr0 == o.pyr_prev && pj.pyr1 == pyr_cur) { d_flow = pj.out; break; }
                    if (!d_flow) {
                        unsigned char* out = nullptr;
                        if (int rc = stage_alloc(e, frame, fbytes, &out)) return rc;
                        fj.pairs.push_back(FlowPairJob{o.pyr_prev, pyr_cur, out});
                        f.stats.pairs++;
                        d_flow = out;
                        e->produced_flows = true;
                    }
                }
            }
            o.pyr_prev = pyr_cur;
            o.flow_made = fim ? d_flow : nullptr;

            // ---- ImageSegmentationOFAidedSource::step_frame (hpp:127-231), schedule part
            c.slot_prev = (o.frame_idx + kPlaneSlots - 1) % kPlaneSlots;
            c.slot_cur = o.frame_idx % kPlaneSlots;
            const bool has_mask = d_mask || d_labels;
            c.has_new_mask = has_mask ? 1 : 0;
            c.new_mask = d_mask;
            if (has_mask) e->new_mask_frames |= 1u << t;
            if (d_mask) e->plain_mask_frames |= 1u << t;
            if (d_labels) {
                c.label = lm->label;
                c.label_type = lm->label_type;
                // the set of this frame's objects that name this image (few distinct images per frame: a linear search)
                int si = -1;
                for (size_t i = e->label_sets.size(); i-- > 0 && e->label_sets[i].t == t;)
                    if (e->label_sets[i].img == d_labels && e->label_sets[i].type == lm->label_type) { si = (int)i; break; }
                if (si < 0) {
                    LabelSet ls{};
                    ls.img = d_labels; ls.type = lm->label_type; ls.t = t;
                    e->label_sets.push_back(ls);
                    e->label_members.emplace_back();
                    si = (int)e->label_sets.size() - 1;
                }
                e->label_members[si].push_back(LabelMember{id, lm->label});
            }
            c.first_mask = 0;
            if (has_mask && !o.seg_available) { o.seg_available = true; c.first_mask = 1; }
            if (!o.seg_available)
                return fail(ROFT_ERR_STATE, "no segmentation mask delivered yet: the first frame must carry one");
            const bool valid_flow = d_flow && !o.of_first_frame;
            o.of_first_frame = false;
            if (valid_flow) {
                const int keep = std::min(o.n_hist, e->hist_cap - 1);
                std::memmove(o.hist + 1, o.hist, sizeof(FlowEntry) * (size_t)keep);
                o.hist[0] = FlowEntry{d_flow, o.frame_idx, -1};
                o.n_hist = keep + 1;
                o.flows_since_mask++;
            }
            // Flows that later flows did not push out of the history in time (dropped flow frames): the caller may
            // recycle the buffer once the retention window closes, the reference keeps a clone -- so does the engine.
            for (int j = 0; j < o.n_hist; ++j) {
                FlowEntry& fe = o.hist[j];
                if (fe.owned >= 0 || o.frame_idx - fe.frame < e->hist_cap) continue;
                int k = -1;
                for (size_t q = 0; q < ho.owned.size(); ++q) {
                    bool referenced = ho.owned[q]->last_ref_frame >= e->completed_frames;
                    for (int j2 = 0; j2 < o.n_hist && !referenced; ++j2) referenced = o.hist[j2].owned == (int)q;
                    if (!referenced) { k = (int)q; break; }
                }
                if (k < 0) { ho.owned.push_back(new OwnedFlow()); k = (int)ho.owned.size() - 1; }
                HIP_TRY(ho.owned[k]->buf.ensure(fbytes));
                if (e->flow.enabled) {
                    // (the flow may be one this very submit produces: the copy goes behind that production, in stream order)
                    e->flow.jobs[t].clones.push_back(FlowCloneJob{ho.owned[k]->buf.p, fe.ptr});
                    e->produced_flows = true;
                } else {
                    HIP_TRY(hipMemcpyAsync(ho.owned[k]->buf.p, fe.ptr, fbytes, hipMemcpyDeviceToDevice, e->up_stream));
                    e->had_uploads = true;
                }
                fe.ptr = ho.owned[k]->buf.p;
                fe.owned = k;
            }
            c.flow_valid = valid_flow ? 1 : 0;
            if (cfg.stamped_masks) {
                // OpticalFlowQueueHandler: window of 30 stamped flows; get_buffer_region(mask stamp) = the flows stored
                // after the first entry within 1 ms of it (OpticalFlowQueueHandler.cpp:18-58)
                c.stamped = 1;
                if (valid_flow) {
                    if (o.n_stamps == 30) std::memmove(o.stamps, o.stamps + 1, sizeof(double) * (size_t)(--o.n_stamps));
                    o.stamps[o.n_stamps++] = in.stamp;
                }
                c.n_region = 0;
                if (has_mask)
                    for (int i = 0; i < o.n_stamps; ++i)
                        if (std::fabs(o.stamps[i] - in.mask_stamp) < 1e-3) { c.n_region = o.n_stamps - (i + 1); break; }
            } else if (has_mask && !c.first_mask) {
                // a delivered mask consumes (or, when empty and the number of frames between masks is unknown, drops)
                // the buffered flows; with that number unknown ALL of them are chased (hpp:239-245)
                if (cfg.mask_frames_between <= 0 && o.flows_since_mask > kMaxFlowHist)
                    return fail(ROFT_ERR_CAPACITY, "more than ROFT_MAX_FLOW_CHASE flows buffered since the last mask");
                o.flows_since_mask = valid_flow ? 1 : 0;   // upper bound: 0 after a consumed mask, 1 after an empty one
            }
            c.n_hist = o.n_hist;
            for (int j = 0; j < o.n_hist; ++j) {
                c.flow[j] = o.hist[j].ptr;
                if (o.hist[j].owned >= 0) ho.owned[o.hist[j].owned]->last_ref_frame = frame;
            }

            // ---- ImageOpticalFlowMeasurement::freeze state machine (hpp:217-229)
            bool data_in = true;  // segmentation is available at this point
            if (!d_flow || o.flow_first_frame) {
                o.flow_first_frame = false;
                data_in = false;
            }
            c.vel_stage = data_in ? 1 : 0;
            c.depth_prev = o.depth_prev;
            c.depth_cur = d_depth;
            // (data_in implies valid_flow, so c.flow[0] is this frame's flow whenever the velocity stage runs)
            o.depth_prev = d_depth;

            // ---- outlier-rejection features on the first frame (ROFTFilter.cpp:313-322)
            if (cfg.use_pose_resync && !o.features_initialized) {
                c.feat_write = o.feat_next;
                o.feat_next = (o.feat_next + 1) % kFeatRing;
                o.feat_slot = c.feat_write;
                o.features_initialized = true;
            }
            c.frame_idx = frame;
            if (!build_pose_program(cfg, o, in, c))
                return fail(ROFT_ERR_CAPACITY, "more buffered velocities to replay than one frame's program holds (kMaxSteps)");
            e->lin_any[c.lane] = true;
            if (!lane_seen[(size_t)id * kNumLin + c.lane]) {
                // the object's first frame on this lane in the batch: is its first step's twist older than the batch?
                lane_seen[(size_t)id * kNumLin + c.lane] = 1;
                e->lane_objs[c.lane]++;
                const int age = (c.n_steps > 0 && c.steps[0].op) ? ((o.frame_idx - c.steps[0].twist_slot) & (kTwistRing - 1)) : 0;
                if (age > t && c.outlier_step == 0) e->lane_old_first[c.lane]++;   // (a replay whose first step is the one the outlier test follows)
            }
            o.last_touch[o.cur_slot] = b;
            if (c.outlier_step >= 0)
                max_outliers[c.lane] = std::max(max_outliers[c.lane], ++n_outliers[(size_t)id * kNumLin + c.lane]);
            if (c.outlier_step >= 0 && c.feat_read >= 0 && c.feat_read != c.feat_write &&
                e->feat_batch[(size_t)id * kFeatRing + c.feat_read] == b) e->feat_dep_in_batch = true;
            if (c.feat_write >= 0) {
                e->feat_batch[(size_t)id * kFeatRing + c.feat_write] = b;
                e->any_feat = true;
                e->feat_frames |= 1u << t;
                // a feature set is re-used only when the batch that read or wrote it last has ended
                const int last = o.feat_use[c.feat_write];
                if (last >= 0 && last < b) { if (int rc = wait_batch(e, last)) return rc; }
                o.feat_use[c.feat_write] = b;
            }
            if (c.feat_read >= 0 && c.outlier_step >= 0) o.feat_use[c.feat_read] = b;
            if (c.outlier_step >= 0 && c.feat_read == c.feat_write) e->any_feat_now = true;
            o.frame_idx++;
        }
    }
    for (int l = 0; l < kNumLin; ++l) e->n_segments[l] = 1 + max_outliers[l];
    // the label table behind the batch's control blocks: the sets, then (16-byte aligned) the members set by set
    e->label_table_bytes = 0;
    if (!e->label_sets.empty()) {
        unsigned char* tab = reinterpret_cast<unsigned char*>(blk + (size_t)T * n_obj);
        const size_t sets_bytes = sizeof(LabelSet) * e->label_sets.size();
        LabelMember* mem = reinterpret_cast<LabelMember*>(tab + sets_bytes);
        int first = 0;
        for (size_t i = 0; i < e->label_sets.size(); ++i) {
            e->label_sets[i].first = first;
            e->label_sets[i].n = (int)e->label_members[i].size();
            std::memcpy(mem + first, e->label_members[i].data(), sizeof(LabelMember) * e->label_members[i].size());
            first += e->label_sets[i].n;
        }
        std::memcpy(tab, e->label_sets.data(), sets_bytes);
        e->label_table_bytes = (sets_bytes + sizeof(LabelMember) * (size_t)first + 15) & ~(size_t)15;
    }
    return ROFT_OK;
}

int roft_frames_submit(roft_engine* e, const roft_frame_input* inputs, int n_objects, int n_frames)
{
    return roft_frames_submit_labels(e, inputs, nullptr, n_objects, n_frames);
}

int roft_frames_submit_labels(roft_engine* e, const roft_frame_input* inputs, const roft_label_mask* labels, int n_objects, int n_frames)
{
    return roft_frames_submit_images(e, inputs, labels, nullptr, n_objects, n_frames);
}

int roft_frames_submit_images(roft_engine* e, const roft_frame_input* inputs, const roft_label_mask* labels, const roft_frame_image* images,
                              int n_objects, int n_frames)
{
    if (!e || !inputs) return fail(ROFT_ERR_INVALID, "null argument");
    if (n_objects != (int)e->objs.size() || n_objects <= 0) return fail(ROFT_ERR_INVALID, "one input per object and frame required");
    if (n_frames < 1 || n_frames > e->T_max) return fail(ROFT_ERR_INVALID, "n_frames must be 1 .. roft_config::max_batch_frames");
    if (e->submitted) return fail(ROFT_ERR_STATE, "previous batch not stepped yet");
    HIP_TRY(hipSetDevice(e->cfg.device));
    double hp_t = e->knobs.host_prof ? host_now_us() : 0.0;
    e->cur_submit_t0 = host_now_us();
    // bound the batches in flight (see roft_engine::lead); this also frees the batch ring slot
    if (int rc = wait_batch(e, e->batch_counter - e->lead, &e->throttled)) return rc;
    e->cur_wait_us = host_now_us() - e->cur_submit_t0;
    HP_MARK(e, 0, hp_t);   // time blocked on the GPU
    e->backup.resize(e->objs.size());
    for (size_t i = 0; i < e->objs.size(); ++i) e->backup[i] = e->objs[i]->s;
    e->any_feat = e->any_feat_now = e->had_uploads = e->produced_flows = false;
    if (e->flow.enabled) {
        e->flow.jobs.assign((size_t)n_frames, FlowFrameJobs{});
        e->flow.stats_backup = e->flow.stats;
    }
    if (e->depth.enabled) {
        e->depth.jobs.clear();
        e->depth.stats_backup = e->depth.stats;
        e->depth.timed = false;
    }
    e->feat_frames = 0;
    e->feat_dep_in_batch = false;
    e->new_mask_frames = e->plain_mask_frames = 0;
    e->label_sets.clear();
    e->label_members.clear();
    e->label_table_bytes = 0;
    e->gather.clear();
    int rc = submit_frames(e, inputs, labels, images, n_objects, n_frames);
    if (rc == ROFT_OK) rc = flush_gather(e);
    e->gather.clear();
    HP_MARK(e, 1, hp_t);
    int rc2 = ROFT_OK;
    BatchSlot& bs = e->slot_of(e->batch_counter);
    hipEvent_t ev_wait = nullptr;   // what the host waits for: the copies
    if (rc == ROFT_OK && e->produced_flows) {
        // Camera images and raw depth: the production follows the copies on the upload stream.  The streams wait for ev_up, recorded behind the
        // production; the host for ev_host, recorded behind the copies alone -- and for nothing when nothing was copied.
        hipError_t err = hipSuccess;
        if (e->had_uploads) { err = hipEventRecord(bs.ev_host, e->up_stream); ev_wait = bs.ev_host; }
        if (err == hipSuccess && !e->depth.jobs.empty()) rc = enqueue_depth_production(e);
        if (err == hipSuccess && rc == ROFT_OK && e->flow.enabled) rc = enqueue_flow_production(e, n_frames);
        if (err == hipSuccess && rc == ROFT_OK) err = hipEventRecord(bs.ev_up, e->up_stream);
        if (err != hipSuccess) rc2 = fail(ROFT_ERR_DEVICE, std::string("flow production: ") + hipGetErrorString(err));
    } else if (e->had_uploads) {
        hipError_t err = hipEventRecord(bs.ev_up, e->up_stream);
        if (err != hipSuccess) rc2 = fail(ROFT_ERR_DEVICE, std::string("input upload: ") + hipGetErrorString(err));
        ev_wait = bs.ev_up;
    }
    if (ev_wait && rc2 == ROFT_OK) {
        // HOST buffers belong to the caller again when this call returns
        const hipError_t err = hipEventSynchronize(ev_wait);
        if (err != hipSuccess) rc2 = fail(ROFT_ERR_DEVICE, std::string("input upload: ") + hipGetErrorString(err));
    }
    HP_MARK(e, 2, hp_t);
    if (rc != ROFT_OK || rc2 != ROFT_OK) {
        const std::string msg = last_error();
        for (size_t i = 0; i < e->objs.size(); ++i) e->objs[i]->s = e->backup[i];
        if (e->flow.enabled) e->flow.stats = e->flow.stats_backup;
        if (e->depth.enabled) { e->depth.stats = e->depth.stats_backup; e->depth.jobs.clear(); }
        return fail(rc != ROFT_OK ? rc : rc2, msg);
    }
    e->cur_T = n_frames;
    e->submitted = true;
    e->device_pointers_checked = true;
    e->cur_submit_us = host_now_us() - e->cur_submit_t0;
    return ROFT_OK;
}

int roft_frame_submit(roft_engine* e, const roft_frame_input* inputs, int n_inputs)
{
    return roft_frames_submit(e, inputs, n_inputs, 1);
}

// The configurations the producer serves are the two products of the reference's flow source: CV_32FC2 on the pixel grid, CV_16SC2
// S10.5 on a grid of 4 (ImageOpticalFlowNVOF.cpp:19-80).
int roft_engine_enable_flow(roft_engine* e, const roft_of_params* p)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    if (e->frame_counter > 0 || e->submitted) return fail(ROFT_ERR_STATE, "roft_engine_enable_flow must precede the first frame");
    roft_of_params prm;
    if (p) prm = *p; else (void)roft_default_of_params(&prm);
    const roft_config& cfg = e->cfg;
    if (cfg.flow_type == ROFT_FLOW_F32C2 && (cfg.flow_grid != 1 || cfg.flow_scale != 1.0f))
        return fail(ROFT_ERR_INVALID, "the producer's CV_32FC2 flow has flow_grid 1 and flow_scale 1");
    if (cfg.flow_type == ROFT_FLOW_S16C2 && (cfg.flow_grid != 4 || cfg.flow_scale != 32.0f))
        return fail(ROFT_ERR_INVALID, "the producer's CV_16SC2 flow has flow_grid 4 and flow_scale 32");
    if (int rc = roft::of_check_params(cfg.cam.width, cfg.cam.height, &prm)) return rc;
    HIP_TRY(hipSetDevice(cfg.device));
    EngineFlow& f = e->flow;
    of_geometry(f.geom, cfg.cam.width, cfg.cam.height, prm.levels, prm.radius, prm.iterations, prm.det_min);
    HIP_TRY(f.coarse.ensure((size_t)kOfChunk * f.geom.flow_stride));
    if (cfg.flow_type == ROFT_FLOW_S16C2) HIP_TRY(f.field.ensure((size_t)kOfChunk * 2 * cfg.cam.width * cfg.cam.height));
    for (auto& g : f.pyr) for (auto* b : g) delete b;   // (enabled again with other levels: another pyramid size)
    f.pyr.assign((size_t)e->T_max + 1, std::vector<DevBuf<float>*>());
    f.prm = prm;
    f.enabled = true;
    return ROFT_OK;
}

int roft_engine_get_flow(roft_engine* e, int obj_id, void* flow_out)
{
    if (!e || !flow_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (obj_id < 0 || obj_id >= (int)e->objs.size()) return fail(ROFT_ERR_INVALID, "bad obj_id");
    const void* src = e->objs[obj_id]->stepped_flow;
    if (!src) return fail(ROFT_ERR_STATE, "the engine produced no flow for the object's last stepped frame");
    if (int rc = roft_sync(e)) return rc;
    HIP_TRY(hipMemcpy(flow_out, src, flow_bytes(e->arr.a.ffmt), hipMemcpyDeviceToHost));
    return ROFT_OK;
}

int roft_engine_get_flow_stats(roft_engine* e, roft_engine_flow_stats* out)
{
    if (!e || !out) return fail(ROFT_ERR_INVALID, "null argument");
    *out = e->flow.stats;
    return ROFT_OK;
}

// ---- raw sensor depth (include/roft_engine.h section 3c) -------------------------------------------------------------------------
int roft_engine_enable_raw_depth(roft_engine* e, const roft_depth_source* src)
{
    if (!e || !src) return fail(ROFT_ERR_INVALID, "null argument");
    if (e->frame_counter > 0 || e->submitted) return fail(ROFT_ERR_STATE, "roft_engine_enable_raw_depth must precede the first frame");
    if (src->type != ROFT_DEPTH_Z16) return fail(ROFT_ERR_INVALID, "the depth source's type must be ROFT_DEPTH_Z16");
    if (int rc = depth_check_scale(src->scale)) return rc;
    const roft_camera& cam = e->cfg.cam;
    EngineDepth& d = e->depth;
    if (src->align) {
        if (int rc = depth_check_camera(src->cam, "depth")) return rc;
        if (int rc = depth_check_transform(*src)) return rc;
        depth_align_geometry(d.geom, *src, cam);
        d.raw_pixels = (size_t)src->cam.width * src->cam.height;
    } else {
        if (src->cam.width != cam.width || src->cam.height != cam.height)
            return fail(ROFT_ERR_INVALID, "a depth source that is not aligned on the device (align 0) must have the size of roft_config::cam");
        d.raw_pixels = (size_t)cam.width * cam.height;
    }
    d.src = *src;
    d.enabled = true;
    return ROFT_OK;
}

int roft_engine_get_depth(roft_engine* e, int obj_id, float* depth_out)
{
    if (!e || !depth_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (obj_id < 0 || obj_id >= (int)e->objs.size()) return fail(ROFT_ERR_INVALID, "bad obj_id");
    if (!e->depth.enabled) return fail(ROFT_ERR_STATE, "the engine makes no depth: roft_engine_enable_raw_depth was not called");
    const float* src = e->objs[obj_id]->stepped_depth;
    if (!src) return fail(ROFT_ERR_STATE, "no frame stepped yet");
    if (int rc = roft_sync(e)) return rc;
    HIP_TRY(hipMemcpy(depth_out, src, (size_t)e->cfg.cam.width * e->cfg.cam.height * sizeof(float), hipMemcpyDeviceToHost));
    return ROFT_OK;
}

int roft_engine_get_depth_stats(roft_engine* e, roft_engine_depth_stats* out)
{
    if (!e || !out) return fail(ROFT_ERR_INVALID, "null argument");
    *out = e->depth.stats;
    return ROFT_OK;
}

int roft_debug_depth_kernel_ms(roft_engine* e, double* ms_out)
{
    if (!e || !ms_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (!e->depth.timed) return fail(ROFT_ERR_STATE, "the engine's last submit call made no depth product");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipEventSynchronize(e->depth.ev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, e->depth.ev0, e->depth.ev1));
    *ms_out = (double)ms;
    return ROFT_OK;
}
