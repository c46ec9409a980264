// engine_submit.hip -- roft_frames_submit / roft_frame_submit: what depends only on the delivery schedule is resolved here, on the
// host, into one FrameCtrl block per object and frame (the frame program: build_pose_program), HOST inputs are staged, the
// lanes are balanced.  Reference: ROFTFilter::filtering_step (src/roft-lib/src/ROFTFilter.cpp:255-452),
// CartesianQuaternionMeasurement::freeze (src/roft-lib/src/CartesianQuaternionMeasurement.cpp:92-348),
// ImageSegmentationOFAidedSource::step_frame (include/ROFT/ImageSegmentationOFAidedSource.hpp:127-231).
#include "engine_internal.h"

// The UKF steps of one frame (ROFTFilter.cpp:327-367 over CartesianQuaternionMeasurement::freeze, cpp:92-348).
// Returns false when the frame needs more than kMaxSteps steps.
// the frame writes the next slot of the object's feature ring, if it does not write one yet: the buffered features are there from now on
static void take_feat_slot(Sched& o, FrameCtrl& c)
{
    if (c.feat_write < 0) { c.feat_write = o.feat_next; o.feat_next = (o.feat_next + 1) % kFeatRing; }
    o.feat_slot = c.feat_write;
}

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
    // the corrections of the step a pose arrives with: under outlier rejection both alternatives, with and without the pose (the test
    // behind the step chooses), else the pose into the current belief
    auto pose_corrections = [&](StepDesc& s) {
        if (cfg.outlier_rejection) {
            s.n_corr = 2;
            s.type[0] = ROFT_MEAS_POSE_VELOCITY; s.dst[0] = b_alt(lin, 0);
            s.type[1] = ROFT_MEAS_VELOCITY;      s.dst[1] = b_alt(lin, 1);
            c.outlier_step = n;
        } else {
            s.n_corr = 1;
            s.type[0] = ROFT_MEAS_POSE_VELOCITY; s.dst[0] = cur;
        }
    };
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
                    pose_corrections(r);
                } else {
                    r.n_corr = 1;
                    r.type[0] = ROFT_MEAS_VELOCITY; r.dst[0] = cur;
                }
                add(r);
            }
            // the test reads the features buffered at the previous pose arrival; this frame's are buffered for
            // the next one (ROFTFilter.cpp:353)
            c.feat_read = o.feat_slot;
            take_feat_slot(o, c);
        } else {
            pose_corrections(sd);
            if (cfg.outlier_rejection) {
                // without re-sync the test uses the current frame's depth and mask
                take_feat_slot(o, c);
                c.feat_read = c.feat_write;
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
    while (sf.cur < sf.chunks.size() && sf.used + need > sf.chunks[sf.cur].n) { ++sf.cur; sf.used = 0; }
    if (sf.cur == sf.chunks.size()) {
        DevBuf<unsigned char> c;
        const hipError_t err = c.ensure(std::max(need, kStageChunk));
        if (err != hipSuccess) return fail(ROFT_ERR_DEVICE, std::string("HOST staging memory: ") + hipGetErrorString(err));
        sf.chunks.push_back(std::move(c));
        sf.used = 0;
    }
    *out = sf.chunks[sf.cur].p + sf.used;
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
    std::vector<GatherItem>& gather = e->pending.gather;
    if (gather.empty()) return ROFT_OK;
    PinnedBuf<GatherItem>& tab = e->slot_of(e->batch_counter).gather_tab;
    HIP_TRY(tab.ensure(kGatherCap, hipHostMallocMapped));   // (allocated on the slot's first use)
    const size_t n = gather.size();
    std::memcpy(tab.p, gather.data(), sizeof(GatherItem) * n);
    size_t largest = 0;
    for (const GatherItem& g : gather) largest = std::max(largest, g.bytes);
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>(32, (largest / 16 + 2047) / 2048));   // ~8 units per thread
    hipLaunchKernelGGL(gather_copy_kernel, dim3(gx, (unsigned)n), dim3(256), 0, e->up_stream, tab.p);
    gather.clear();
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

// `bytes` of HOST inputs cross the bus for this submit, in `copies` copies of their own (0: fetched by the gather launch)
static void count_upload(roft_engine* e, size_t bytes, int copies)
{
    e->stats.h2d_bytes += (long long)bytes;
    e->stats.h2d_copies += copies;
    e->pending.facts.had_uploads = true;
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
    const bool gathered = e->knobs.gather_copy && bytes <= kGatherMaxBytes && (bytes & 15) == 0 && (reinterpret_cast<uintptr_t>(host) & 15) == 0 &&
                          (int)e->pending.gather.size() < kGatherCap && (dp = pinned_device_pointer(host)) != nullptr;
    if (gathered) e->pending.gather.push_back(GatherItem{dp, d, bytes});   // fetched by flush_gather's one launch
    else HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, e->up_stream));
    count_upload(e, bytes, gathered ? 0 : 1);
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
                        count_upload(e, (size_t)len * bytes, 1);
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

namespace roft {   // flow_producer.hip
int of_check_params(int W, int H, const roft_of_params* p);
int of_check_consistency(const roft_of_consistency* c);
}

static size_t image_bytes(int type, size_t npix) { return type == ROFT_IMAGE_GRAY8 ? npix : 3 * npix; }

// The flow production of the accepted batch -> upload stream: a pyramid for each distinct image of each of its frames, then a flow
// for each distinct pair, then the clones of flows that aged out in the batch (they may read its products) -- the images and the
// pairs of ALL its frames in chunks of kOfChunk, whose pointers travel in the kernel arguments and whose workspace the next chunk
// reuses in stream order.  A batch of eight frames of a shared scene is one chunk of each: seven launches, not seven per frame.
static int enqueue_flow_production(roft_engine* e, int T)
{
    EngineFlow& f = e->flow;
    const std::vector<FlowFrameJobs>& jobs = e->pending.flow_jobs;
    const size_t fbytes = flow_bytes(e->arr.a.ffmt);
    const size_t field_floats = (size_t)2 * e->cfg.cam.width * e->cfg.cam.height;
    const bool s16 = e->cfg.flow_type == ROFT_FLOW_S16C2;
    const int G = (int)f.pyr.size();
    OfImages im{};
    for (int t = 0; t < T; ++t) {
        const int gen = (e->frame_counter + t) % G;
        for (size_t i = 0; i < jobs[t].images.size(); ++i) {
            const int k = im.n++;
            im.type[k] = jobs[t].images[i].type; im.src[k] = jobs[t].images[i].dev; im.pyr[k] = f.pyr[gen][i].p;
            if (im.n == kOfChunk) { launch_of_pyramids(f.geom, im, e->up_stream); im.n = 0; }
        }
    }
    if (im.n) launch_of_pyramids(f.geom, im, e->up_stream);
    OfPairs pr{};
    OfCheck ck{};
    ck.tol_abs = f.tol.tolerance_abs; ck.tol_rel = f.tol.tolerance_rel;
    auto launch_checked = [&]() {
        of_check_close(pr);
        launch_of_pairs(f.geom, pr, e->up_stream);
        launch_of_check(f.geom, ck, e->up_stream);
        pr.n = ck.n = 0;
    };
    for (int t = 0; t < T; ++t) {
        const int gen = (e->frame_counter + t) % G, gen_prev = (e->frame_counter + t + G - 1) % G;
        for (const FlowPairJob& pj : jobs[t].pairs) {
            if (f.check) {   // (CV_32FC2 only: the product's place is the forward field)
                const int k = pr.n;
                of_check_put(pr, ck, f.pyr[gen_prev][pj.pyr0].p, f.pyr[gen][pj.pyr1].p, reinterpret_cast<float*>(pj.out),
                             f.coarse.p + (size_t)k * f.geom.flow_stride, f.coarse.p + (size_t)(kOfCheckChunk + k) * f.geom.flow_stride,
                             f.back.p + (size_t)k * field_floats);
                if (pr.n == kOfCheckChunk) launch_checked();
                continue;
            }
            const int k = pr.n++;
            pr.pyr0[k] = f.pyr[gen_prev][pj.pyr0].p;
            pr.pyr1[k] = f.pyr[gen][pj.pyr1].p;
            pr.coarse[k] = f.coarse.p + (size_t)k * f.geom.flow_stride;
            pr.field[k] = s16 ? f.field.p + (size_t)k * field_floats : reinterpret_cast<float*>(pj.out);
            pr.out_s16[k] = s16 ? reinterpret_cast<int16_t*>(pj.out) : nullptr;
            if (pr.n == kOfChunk) { launch_of_pairs(f.geom, pr, e->up_stream); pr.n = 0; }
        }
    }
    if (pr.n && f.check) launch_checked();
    if (pr.n) launch_of_pairs(f.geom, pr, e->up_stream);
    if (hipError_t le = hipGetLastError()) return fail(ROFT_ERR_DEVICE, std::string("flow production: ") + hipGetErrorString(le));
    for (int t = 0; t < T; ++t)
        for (const FlowCloneJob& c : jobs[t].clones) HIP_TRY(hipMemcpyAsync(c.dst, c.src, fbytes, hipMemcpyDeviceToDevice, e->up_stream));
    return ROFT_OK;
}

// The depth products of the accepted batch -> upload stream, behind the copies: all distinct raw images of the batch in one launch
// per phase (one for a conversion, three for an alignment), their pointers in the kernel arguments in chunks of kDepthChunk.
static int enqueue_depth_production(roft_engine* e)
{
    EngineDepth& d = e->depth;
    const size_t npix = (size_t)e->cfg.cam.width * e->cfg.cam.height;
    if (!d.ev0) { HIP_TRY(d.ev0.create()); HIP_TRY(d.ev1.create()); }
    HIP_TRY(hipEventRecord(d.ev0, e->up_stream));
    DepthJobs jobs{};
    auto launch = [&]() {
        if (d.src.align) launch_depth_align(jobs, d.geom, e->up_stream);
        else launch_depth_convert(jobs, npix, d.src.scale, e->up_stream);
        jobs.n = 0;
    };
    for (const DepthJob& j : e->pending.depth_jobs) {
        jobs.raw[jobs.n] = j.raw; jobs.out[jobs.n] = j.out;
        if (++jobs.n == kDepthChunk) launch();
    }
    if (jobs.n) launch();
    if (hipError_t le = hipGetLastError()) return fail(ROFT_ERR_DEVICE, std::string("depth production: ") + hipGetErrorString(le));
    HIP_TRY(hipEventRecord(d.ev1, e->up_stream));
    d.timed = true;
    return ROFT_OK;
}

// The rectified products of the accepted batch -> upload stream, behind the copies and in front of the depth and the flow production
// (both read them): all distinct (image, kind) pairs of the batch in one launch per chunk of kRectChunk, pointers in the kernel arguments.
static int enqueue_rectification(roft_engine* e)
{
    EngineRectify& r = e->rectify;
    if (!r.ev0) { HIP_TRY(r.ev0.create()); HIP_TRY(r.ev1.create()); }
    HIP_TRY(hipEventRecord(r.ev0, e->up_stream));
    RectJobs jobs{};
    for (const RectJob& j : e->pending.rect_jobs) {
        jobs.src[jobs.n] = j.src; jobs.dst[jobs.n] = j.out; jobs.kind[jobs.n] = (unsigned char)j.kind;
        if (++jobs.n == kRectChunk) { launch_rectify(jobs, r.geom, e->up_stream); jobs.n = 0; }
    }
    if (jobs.n) launch_rectify(jobs, r.geom, e->up_stream);
    if (hipError_t le = hipGetLastError()) return fail(ROFT_ERR_DEVICE, std::string("rectification: ") + hipGetErrorString(le));
    HIP_TRY(hipEventRecord(r.ev1, e->up_stream));
    r.timed = true;
    return ROFT_OK;
}

// ---- submit_frames: one object's frame of the batch at a time, through the stages below in their order --------------------------------

struct ImageSizes {
    size_t npix, flow;   // pixels of the camera; bytes of a flow frame
    size_t depth;        // bytes of what inputs[].depth carries: H x W floats, or on a raw-depth engine the sensor's 16-bit frame of the depth source's size
    explicit ImageSizes(const roft_engine* e)
        : npix((size_t)e->cfg.cam.width * e->cfg.cam.height), flow(flow_bytes(e->arr.a.ffmt)),
          depth(e->depth.enabled ? e->depth.raw_pixels * sizeof(uint16_t) : npix * sizeof(float)) {}
};

struct FrameJob {
    int t, id, frame;              // frame of the batch, object, the engine's count of that frame
    const roft_frame_input& in;
    const roft_label_mask* lm;     // the mask as the pixels of a label image equal to a value (roft_frames_submit_labels), or null
    const roft_frame_image* fim;   // a camera image instead of a flow frame (roft_frames_submit_images), or null
    HostObject& ho;
    FrameCtrl& c;
};

// the frame's inputs in device memory (depth: floats, or on a raw-depth engine the 16-bit frame until plan_depth_product; mask: bytes)
// (image_type: the camera image's as the flow producer will see it -- GRAY8 once plan_rectified_products has replaced the image)
struct DevInputs { const void *depth = nullptr, *flow = nullptr, *mask = nullptr, *labels = nullptr, *image = nullptr; int image_type = 0; };

// device or managed memory, or host memory the GPU can address as it is (hipHostMalloc / hipHostRegister: pinned and mapped --
// zero-copy over the bus); unregistered pageable memory is what is refused
static bool device_can_read(const void* p)
{
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged || pinned_device_pointer(p) == p;
}

static int check_frame_forms(const roft_engine* e, const FrameJob& j)
{
    auto obj = [&] { return "object " + std::to_string(j.id); };
    if (!j.in.depth) return fail(ROFT_ERR_INVALID, "cannot continue without a continuous depth stream (ROFTFilter.cpp:261-266)");
    if (e->rectify.enabled && j.in.flow)
        return fail(ROFT_ERR_INVALID, obj() + ": a flow on an engine with roft_engine_enable_rectification (a flow computed between distorted "
                                              "images cannot be rectified: hand the camera image instead)");
    if (const roft_label_mask* lm = j.lm) {
        if (j.in.mask) return fail(ROFT_ERR_INVALID, obj() + ": a label image AND a mask for one frame (one of the two)");
        if (lm->label_type != ROFT_LABEL_U8 && lm->label_type != ROFT_LABEL_U16)
            return fail(ROFT_ERR_INVALID, obj() + ": label_type must be ROFT_LABEL_U8 or ROFT_LABEL_U16");
        if (lm->label == 0) return fail(ROFT_ERR_INVALID, obj() + ": label 0 is the background");
        if (lm->label < 0 || lm->label > (lm->label_type == ROFT_LABEL_U8 ? 255 : 65535))
            return fail(ROFT_ERR_INVALID, obj() + ": label " + std::to_string(lm->label) + " is outside the range of the label type");
    }
    if (const roft_frame_image* fim = j.fim) {
        if (!e->flow.enabled) return fail(ROFT_ERR_STATE, "camera images need roft_engine_enable_flow before the first frame");
        if (j.in.flow) return fail(ROFT_ERR_INVALID, obj() + ": a camera image AND a flow for one frame (one of the two)");
        if (fim->image_type != ROFT_IMAGE_GRAY8 && fim->image_type != ROFT_IMAGE_BGR8 && fim->image_type != ROFT_IMAGE_RGB8)
            return fail(ROFT_ERR_INVALID, obj() + ": image_type must be ROFT_IMAGE_GRAY8, ROFT_IMAGE_BGR8 or ROFT_IMAGE_RGB8");
    }
    return ROFT_OK;
}

// The inputs to device memory: DEVICE pointers as they are (looked up on the engine's first call, and aligned), HOST images staged --
// depth, flow, mask, labels, image: the order decides their places in the frame's staging slot.
static int resolve_inputs(roft_engine* e, const FrameJob& j, const ImageSizes& sz, DevInputs& d)
{
    const roft_frame_input& in = j.in;
    if (in.mem_kind == ROFT_MEM_DEVICE) {
        d.depth = in.depth;
        d.flow = in.flow;
        d.mask = in.mask;
        if (j.lm) d.labels = j.lm->labels;
        if (j.fim) d.image = j.fim->image;
        // the first call of an engine only: a host pointer declared as device memory is a GPU page fault that takes
        // the process down at the first kernel -- the commonest mistake of a new binding is refused here instead
        if (!e->device_pointers_checked) {
            const void* ptrs[5] = {d.depth, d.flow, d.mask, d.labels, d.image};
            static const char* const what[5] = {"depth", "flow", "mask", "label image", "camera image"};
            for (int q = 0; q < 5; ++q) {
                if (ptrs[q] && !device_can_read(ptrs[q]))
                    return fail(ROFT_ERR_INVALID, std::string("mem_kind is ROFT_MEM_DEVICE but the ") + what[q] + " pointer of object " +
                                                      std::to_string(j.id) + " is neither device memory nor pinned, mapped host memory "
                                                      "(pass ROFT_MEM_HOST for ordinary host buffers)");
            }
        }
        if ((reinterpret_cast<uintptr_t>(d.mask) & 15) || (reinterpret_cast<uintptr_t>(d.flow) & 7) || (reinterpret_cast<uintptr_t>(d.depth) & 3))
            return fail(ROFT_ERR_INVALID, "device buffers must be aligned: mask 16 B, flow 8 B, depth 4 B");
        if (reinterpret_cast<uintptr_t>(d.labels) & 15) return fail(ROFT_ERR_INVALID, "device buffers must be aligned: label image 16 B");
        if (reinterpret_cast<uintptr_t>(d.image) & 3) return fail(ROFT_ERR_INVALID, "device buffers must be aligned: camera image 4 B");
        return ROFT_OK;
    }
    if (in.mem_kind != ROFT_MEM_HOST) return fail(ROFT_ERR_INVALID, "mem_kind must be ROFT_MEM_HOST or ROFT_MEM_DEVICE");
    const long long before_depth = e->stats.h2d_bytes;
    TRY(stage_host(e, j.frame, in.depth, sz.depth, &d.depth));
    if (e->depth.enabled) e->depth.stats.image_bytes += e->stats.h2d_bytes - before_depth;   // (uploaded, and counted, once per distinct pointer)
    if (in.flow) TRY(stage_host(e, j.frame, in.flow, sz.flow, &d.flow));
    if (in.mask) TRY(stage_host(e, j.frame, in.mask, sz.npix, &d.mask));
    if (j.lm) TRY(stage_host(e, j.frame, j.lm->labels, sz.npix * (j.lm->label_type == ROFT_LABEL_U8 ? 1 : 2), &d.labels));
    if (j.fim) {
        const long long before = e->stats.h2d_bytes;   // (the objects of a shared scene name one image: uploaded, and counted, once)
        TRY(stage_host(e, j.frame, j.fim->image, image_bytes(j.fim->image_type, sz.npix), &d.image));
        e->flow.stats.image_bytes += e->stats.h2d_bytes - before;
    }
    return ROFT_OK;
}

// Lens distortion: every image of the frame is the sensor's distorted one so far.  Each is replaced by its rectified product, which
// goes where a staged HOST image of the frame would have been copied, one per distinct (image, kind) and frame however many objects
// name it.  The depth of a raw-depth engine that aligns on the device is not touched: the alignment lands in the pinhole camera.
static int plan_rectified_products(roft_engine* e, const FrameJob& j, const ImageSizes& sz, DevInputs& d)
{
    std::vector<RectJob>& jobs = e->pending.rect_jobs;
    auto product = [&](const void*& img, int kind) -> int {
        bool source_known = false;
        for (size_t i = jobs.size(); i-- > 0 && jobs[i].t == j.t;) {
            if (jobs[i].src != img) continue;
            if (jobs[i].kind == kind) { img = jobs[i].out; return ROFT_OK; }
            source_known = true;
        }
        unsigned char* out = nullptr;
        TRY(stage_alloc(e, j.frame, sz.npix * rect_dst_pixel_bytes(kind), &out));
        jobs.push_back(RectJob{j.t, img, kind, out});
        roft_engine_rectify_stats& st = e->rectify.stats;
        if (!source_known) st.sources++;
        st.products++;
        st.bytes += (long long)(sz.npix * (rect_src_pixel_bytes(kind) + rect_dst_pixel_bytes(kind)));
        e->pending.facts.produced_flows = true;   // (production behind the copies: ev_up is recorded behind it)
        img = out;
        return ROFT_OK;
    };
    if (!(e->depth.enabled && e->depth.src.align)) TRY(product(d.depth, e->depth.enabled ? ROFT_RECTIFY_U16 : ROFT_RECTIFY_F32));
    if (d.mask) TRY(product(d.mask, ROFT_RECTIFY_U8));
    if (d.labels) TRY(product(d.labels, j.lm->label_type == ROFT_LABEL_U8 ? ROFT_RECTIFY_U8 : ROFT_RECTIFY_U16));
    if (d.image) {
        TRY(product(d.image, d.image_type == ROFT_IMAGE_GRAY8 ? ROFT_RECTIFY_GRAY8 : d.image_type == ROFT_IMAGE_BGR8 ? kRectGrayOfBgr8 : kRectGrayOfRgb8));
        d.image_type = ROFT_IMAGE_GRAY8;
    }
    return ROFT_OK;
}

// Raw depth: d.depth is the device address of the 16-bit frame so far.  Its float product goes where a staged HOST depth of the frame
// would have been copied, one per distinct raw image and frame however many objects name it.
static int plan_depth_product(roft_engine* e, const FrameJob& j, const ImageSizes& sz, DevInputs& d)
{
    std::vector<DepthJob>& jobs = e->pending.depth_jobs;
    const uint16_t* d_raw = static_cast<const uint16_t*>(d.depth);
    float* made = nullptr;
    for (size_t i = jobs.size(); i-- > 0 && jobs[i].t == j.t;)
        if (jobs[i].raw == d_raw) { made = jobs[i].out; break; }
    if (!made) {
        unsigned char* out = nullptr;
        TRY(stage_alloc(e, j.frame, sz.npix * sizeof(float), &out));
        made = reinterpret_cast<float*>(out);
        jobs.push_back(DepthJob{j.t, d_raw, made});
        e->depth.stats.images++;
        e->depth.stats.products++;
        e->pending.facts.produced_flows = true;   // (production behind the copies: ev_up is recorded behind it)
    }
    d.depth = made;
    return ROFT_OK;
}

// The flow of a camera image: produced where a staged HOST flow of the frame would have been copied, one pyramid per distinct image
// and one flow per distinct (previous, current) pair of the frame; none without an image the frame before.
static int plan_flow_product(roft_engine* e, const FrameJob& j, const ImageSizes& sz, DevInputs& d)
{
    Sched& o = j.ho.s;
    int pyr_cur = -1;
    if (j.fim) {
        EngineFlow& f = e->flow;
        FlowFrameJobs& fj = e->pending.flow_jobs[j.t];
        for (size_t i = 0; i < fj.images.size() && pyr_cur < 0; ++i)
            if (fj.images[i].dev == d.image && fj.images[i].type == d.image_type) pyr_cur = (int)i;
        if (pyr_cur < 0) {
            pyr_cur = (int)fj.images.size();
            fj.images.push_back(FlowImageJob{d.image, d.image_type});
            std::vector<DevBuf<float>>& gen = f.pyr[(size_t)j.frame % f.pyr.size()];
            if ((int)gen.size() <= pyr_cur) {
                DevBuf<float> pb;
                HIP_TRY(pb.ensure(f.geom.pyr_stride));
                gen.push_back(std::move(pb));
            }
            f.stats.images++;
            f.stats.pyramids++;
            e->pending.facts.produced_flows = true;   // (a pyramid to build, also where no pair follows in this batch)
        }
        if (o.pyr_prev >= 0) {
            for (const FlowPairJob& pj : fj.pairs)
                if (pj.pyr0 == o.pyr_prev && pj.pyr1 == pyr_cur) { d.flow = pj.out; break; }
            if (!d.flow) {
                unsigned char* out = nullptr;
                TRY(stage_alloc(e, j.frame, sz.flow, &out));
                fj.pairs.push_back(FlowPairJob{o.pyr_prev, pyr_cur, out});
                f.stats.pairs++;
                d.flow = out;
                e->pending.facts.produced_flows = true;
            }
        }
    }
    o.pyr_prev = pyr_cur;
    o.flow_made = j.fim ? d.flow : nullptr;
    return ROFT_OK;
}

// ImageSegmentationOFAidedSource::step_frame (hpp:127-231), schedule part: the delivered mask (its label set), the history of valid
// flows with the clones of those that aged out, the stamped window.
static int schedule_mask_source(roft_engine* e, const FrameJob& j, const ImageSizes& sz, const DevInputs& d)
{
    PendingBatch& pb = e->pending;
    HostObject& ho = j.ho;
    Sched& o = ho.s;
    FrameCtrl& c = j.c;
    c.slot_prev = (o.frame_idx + kPlaneSlots - 1) % kPlaneSlots;
    c.slot_cur = o.frame_idx % kPlaneSlots;
    // masks from poses (roft_engine_enable_pose_masks): an enrolled object whose frame brings neither a mask nor a label image takes
    // the silhouette of the delivered pose -- on the first frame of its track (Sched::track_frames), without one, of the pose it was
    // added or restarted with
    const EnginePoseMasks& pm = e->pose_masks;
    const bool enrolled = pm.enabled && (ho.pose_masks || (pm.all && has_mesh(e->h_params[j.id])));
    const bool from_pose = enrolled && !d.mask && !d.labels && (j.in.pose_valid || o.track_frames == 0);
    const bool has_mask = d.mask || d.labels || from_pose;
    c.has_new_mask = has_mask ? 1 : 0;
    c.new_mask = static_cast<const uint8_t*>(d.mask);
    if (has_mask) pb.new_mask_frames |= 1u << j.t;
    if (d.mask) pb.facts.plain_mask_frames |= 1u << j.t;
    if (d.labels) {
        c.label = j.lm->label;
        c.label_type = j.lm->label_type;
        // the set of this frame's objects that name this image (few distinct images per frame: a linear search)
        int si = -1;
        for (size_t i = pb.label_sets.size(); i-- > 0 && pb.label_sets[i].t == j.t;)
            if (pb.label_sets[i].img == d.labels && pb.label_sets[i].type == j.lm->label_type) { si = (int)i; break; }
        if (si < 0) {
            LabelSet ls{};
            ls.img = d.labels; ls.type = j.lm->label_type; ls.t = j.t;
            pb.label_sets.push_back(ls);
            pb.label_members.emplace_back();
            si = pb.facts.label_sets++;
        }
        pb.label_members[si].push_back(LabelMember{j.id, j.lm->label});
    }
    if (from_pose) {
        c.label_type = kMaskFromPose;   // (pose_silhouette_kernel draws the planes; the ordinary ingest skips the object)
        pb.pose_mask_frames |= 1u << j.t;
        pb.facts.pose_masks++;
    }
    if (has_mask && !o.seg_available) { o.seg_available = true; c.first_mask = 1; }
    if (!o.seg_available)
        return fail(ROFT_ERR_STATE, "no segmentation mask delivered yet: the first frame must carry one (or the object be enrolled with roft_engine_enable_pose_masks)");
    const bool valid_flow = d.flow && !o.of_first_frame;
    o.of_first_frame = false;
    if (valid_flow) {
        const int keep = std::min(o.n_hist, e->hist_cap - 1);
        std::memmove(o.hist + 1, o.hist, sizeof(FlowEntry) * (size_t)keep);
        o.hist[0] = FlowEntry{d.flow, o.frame_idx, -1, o.depth_prev};   // (depth_prev: still the frame before, schedule_flow_measurement moves it on)
        o.n_hist = keep + 1;
        o.flows_since_mask++;
        o.flows_buffered = std::min(o.flows_buffered + 1, kMaxFlowHist);
    }
    // Flows that later flows did not push out of the history in time (dropped flow frames): the caller may
    // recycle the buffer once the retention window closes, the reference keeps a clone -- so does the engine.
    for (int k0 = 0; k0 < o.n_hist; ++k0) {
        FlowEntry& fe = o.hist[k0];
        if (fe.owned >= 0 || o.frame_idx - fe.frame < e->hist_cap) continue;
        int k = -1;
        for (size_t q = 0; q < ho.owned.size(); ++q) {
            bool referenced = ho.owned[q].last_ref_frame >= e->completed_frames;
            for (int j2 = 0; j2 < o.n_hist && !referenced; ++j2) referenced = o.hist[j2].owned == (int)q;
            if (!referenced) { k = (int)q; break; }
        }
        if (k < 0) { ho.owned.emplace_back(); k = (int)ho.owned.size() - 1; }
        HIP_TRY(ho.owned[k].buf.ensure(sz.flow));
        if (pm.gate && fe.depth_before) {
            // the depth gate: the image the chase from this flow starts on ages out one frame BEFORE its flow; it is older than
            // anything this submit uploads or produces, so the copy needs no place behind the batch's production
            HIP_TRY(ho.owned[k].depth.ensure(sz.npix));   // (the float image, also where the caller's frames are the sensor's)
            HIP_TRY(hipMemcpyAsync(ho.owned[k].depth.p, fe.depth_before, sz.npix * sizeof(float), hipMemcpyDeviceToDevice, e->up_stream));
            fe.depth_before = ho.owned[k].depth.p;
        }
        if (e->flow.enabled) {
            // (the flow may be one this very submit produces: the copy goes behind that production, in stream order)
            pb.flow_jobs[j.t].clones.push_back(FlowCloneJob{ho.owned[k].buf.p, fe.ptr});
            pb.facts.produced_flows = true;
        } else {
            HIP_TRY(hipMemcpyAsync(ho.owned[k].buf.p, fe.ptr, sz.flow, hipMemcpyDeviceToDevice, e->up_stream));
            pb.facts.had_uploads = true;
        }
        fe.ptr = ho.owned[k].buf.p;
        fe.owned = k;
    }
    c.flow_valid = valid_flow ? 1 : 0;
    if (e->cfg.stamped_masks) {
        // OpticalFlowQueueHandler: window of 30 stamped flows; get_buffer_region(mask stamp) = the flows stored
        // after the first entry within 1 ms of it (OpticalFlowQueueHandler.cpp:18-58)
        c.stamped = 1;
        if (valid_flow) {
            if (o.n_stamps == 30) std::memmove(o.stamps, o.stamps + 1, sizeof(double) * (size_t)(--o.n_stamps));
            o.stamps[o.n_stamps++] = j.in.stamp;
        }
        if (has_mask)
            for (int i = 0; i < o.n_stamps; ++i)
                if (std::fabs(o.stamps[i] - j.in.mask_stamp) < 1e-3) { c.n_region = o.n_stamps - (i + 1); break; }
    } else if (has_mask && !c.first_mask) {
        // a delivered mask consumes (or, when empty and the number of frames between masks is unknown, drops)
        // the buffered flows; with that number unknown ALL of them are chased (hpp:239-245)
        if (e->cfg.mask_frames_between <= 0 && o.flows_since_mask > kMaxFlowHist)
            return fail(ROFT_ERR_CAPACITY, "more than ROFT_MAX_FLOW_CHASE flows buffered since the last mask");
        o.flows_since_mask = valid_flow ? 1 : 0;   // upper bound: 0 after a consumed mask, 1 after an empty one
    }
    if (from_pose && pm.gate) {
        // the gate image of the silhouette: the frame its chase starts on, or -- nothing to chase -- this frame's own depth
        const int k = pose_mask_gate_entry(o.n_hist, e->cfg.mask_frames_between, o.flows_buffered, c.first_mask != 0);
        c.gate_depth = k < 0 ? static_cast<const float*>(d.depth) : o.hist[k].depth_before;
        pb.gated_pairs++;
    }
    if (has_mask && !c.first_mask && !e->cfg.stamped_masks) o.flows_buffered = 0;   // (consumed: flow_buffer_.clear(), hpp:218)
    c.n_hist = o.n_hist;
    for (int k = 0; k < o.n_hist; ++k) {
        c.flow[k] = o.hist[k].ptr;
        if (o.hist[k].owned >= 0) ho.owned[o.hist[k].owned].last_ref_frame = j.frame;
    }
    return ROFT_OK;
}

// ImageOpticalFlowMeasurement::freeze state machine (hpp:217-229)
static void schedule_flow_measurement(const FrameJob& j, const DevInputs& d)
{
    Sched& o = j.ho.s;
    const bool data_in = d.flow && !o.flow_first_frame;   // (segmentation is available at this point)
    o.flow_first_frame = false;
    j.c.vel_stage = data_in ? 1 : 0;
    j.c.depth_prev = o.depth_prev;
    // (data_in implies valid_flow, so c.flow[0] is this frame's flow whenever the velocity stage runs)
    j.c.depth_cur = o.depth_prev = static_cast<const float*>(d.depth);
}

// What the frame's pose program means for the batch: its lane, the lane's segments, the feature slots it reads and writes.
static int account_lanes_and_features(roft_engine* e, const FrameJob& j)
{
    PendingBatch& pb = e->pending;
    SubmitFacts& facts = pb.facts;
    Sched& o = j.ho.s;
    const FrameCtrl& c = j.c;
    const int b = e->batch_counter;
    const size_t on_lane = (size_t)j.id * kNumLin + c.lane;
    facts.lin_any[c.lane] = true;
    if (pb.lane_tests[on_lane] < 0) {
        // the object's first frame on this lane in the batch: is its first step's twist older than the batch?
        pb.lane_tests[on_lane] = 0;
        facts.lane_objs[c.lane]++;
        const int age = (c.n_steps > 0 && c.steps[0].op) ? ((o.frame_idx - c.steps[0].twist_slot) & (kTwistRing - 1)) : 0;
        if (age > j.t && c.outlier_step == 0) facts.lane_old_first[c.lane]++;   // (a replay whose first step is the one the outlier test follows)
    }
    o.last_touch[o.cur_slot] = b;
    if (c.outlier_step >= 0) facts.n_segments[c.lane] = std::max(facts.n_segments[c.lane], 1 + ++pb.lane_tests[on_lane]);
    if (c.outlier_step >= 0 && c.feat_read >= 0 && c.feat_read != c.feat_write && o.feat_batch[c.feat_read] == b) facts.feat_dep_in_batch = true;
    if (c.feat_write >= 0) {
        o.feat_batch[c.feat_write] = b;
        facts.any_feat = true;
        pb.feat_frames |= 1u << j.t;
        // a feature set is re-used only when the batch that read or wrote it last has ended
        const int last = o.feat_use[c.feat_write];
        if (last >= 0 && last < b) TRY(wait_batch(e, last));
        o.feat_use[c.feat_write] = b;
    }
    if (c.feat_read >= 0 && c.outlier_step >= 0) o.feat_use[c.feat_read] = b;
    if (c.outlier_step >= 0 && c.feat_read == c.feat_write) facts.any_feat_now = true;
    return ROFT_OK;
}

static int submit_frames(roft_engine* e, const roft_frame_input* inputs, const roft_label_mask* labels, const roft_frame_image* images, int n_obj, int T)
{
    const roft_config& cfg = e->cfg;
    const ImageSizes sz(e);
    PendingBatch& pb = e->pending;
    FrameCtrl* blk = e->slot_of(e->batch_counter).stage.p;
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
        int* relabel_wait = pb.facts.relabel_wait;
        for (int id = 0; id < n_obj; ++id) {
            Sched& o = e->objs[id]->s;
            if (o.own[o.cur_slot] == c) continue;
            relabel_wait[c] = std::max(relabel_wait[c], o.last_touch[o.cur_slot]);
            relabel_wait[1 - c] = std::max(relabel_wait[1 - c], o.last_touch[1 - o.cur_slot]);
            std::swap(o.own[0], o.own[1]);
        }
    }

    for (int t = 0; t < T; ++t) {   // the staging slots of the batch's frames are free again: every frame that could read them has ended (in-flight bound)
        StageFrame& sf = e->staging[(e->frame_counter + t) % e->retain];
        sf.cur = sf.used = 0;
        sf.seen.clear();
    }
    TRY(stage_host_runs(e, inputs, n_obj, T, sz.depth, sz.flow));
    for (int t = 0; t < T; ++t) {
        for (int id = 0; id < n_obj; ++id) {
            const size_t k = (size_t)t * n_obj + id;
            const FrameJob j{t, id, e->frame_counter + t, inputs[k], (labels && labels[k].labels) ? &labels[k] : nullptr,
                             (images && images[k].image) ? &images[k] : nullptr, *e->objs[id], blk[k]};
            Sched& o = j.ho.s;
            DevInputs d;
            clear_ctrl(j.c);
            TRY(check_frame_forms(e, j));
            j.c.dt = (j.in.dt > 0.0) ? j.in.dt : cfg.sample_time;
            TRY(resolve_inputs(e, j, sz, d));
            if (j.fim) d.image_type = j.fim->image_type;
            if (e->rectify.enabled) TRY(plan_rectified_products(e, j, sz, d));
            if (e->depth.enabled) TRY(plan_depth_product(e, j, sz, d));
            TRY(plan_flow_product(e, j, sz, d));
            TRY(schedule_mask_source(e, j, sz, d));
            schedule_flow_measurement(j, d);
            // outlier-rejection features on the first frame (ROFTFilter.cpp:313-322)
            if (cfg.use_pose_resync && !o.features_initialized) {
                take_feat_slot(o, j.c);
                o.features_initialized = true;
            }
            j.c.frame_idx = j.frame;
            if (!build_pose_program(cfg, o, j.in, j.c))
                return fail(ROFT_ERR_CAPACITY, "more buffered velocities to replay than one frame's program holds (kMaxSteps)");
            if (j.c.label_type == kMaskFromPose && !j.in.pose_valid) {
                // the silhouette of a first frame without a pose: the initial pose, in the fields no step of the frame reads
                for (int i = 0; i < 3; ++i) j.c.pose_x[i] = j.ho.pose0[i];
                for (int i = 0; i < 4; ++i) j.c.pose_q[i] = j.ho.pose0[3 + i];
            }
            TRY(account_lanes_and_features(e, j));
            o.frame_idx++;
            o.track_frames++;
        }
    }
    // silhouettes of one scene hide each other: a pair that shares its frame with another drawn member of its scene is drawn against
    // the scene's z-buffer (FrameCtrl::label = 1 + z-buffer); a member drawn alone on its frame stays a plain silhouette
    if (e->pose_masks.occlusion && e->pose_masks.n_zscenes > 0 && pb.pose_mask_frames) {
        std::vector<int> drawn((size_t)e->pose_masks.n_zscenes);
        for (int t = 0; t < T; ++t) {
            if (!(pb.pose_mask_frames & (1u << t))) continue;
            std::fill(drawn.begin(), drawn.end(), 0);
            for (int id = 0; id < n_obj; ++id)
                if (blk[(size_t)t * n_obj + id].label_type == kMaskFromPose && e->objs[id]->pose_zscene >= 0) drawn[e->objs[id]->pose_zscene]++;
            for (int id = 0; id < n_obj; ++id) {
                FrameCtrl& c = blk[(size_t)t * n_obj + id];
                const int z = e->objs[id]->pose_zscene;
                if (c.label_type == kMaskFromPose && z >= 0 && drawn[z] >= 2) { c.label = 1 + z; pb.facts.pose_resolve++; }
            }
        }
    }
    // the label table behind the batch's control blocks: the sets, then (16-byte aligned) the members set by set
    if (!pb.label_sets.empty()) {
        unsigned char* tab = reinterpret_cast<unsigned char*>(blk + (size_t)T * n_obj);
        const size_t sets_bytes = sizeof(LabelSet) * pb.label_sets.size();
        LabelMember* mem = reinterpret_cast<LabelMember*>(tab + sets_bytes);
        int first = 0;
        for (size_t i = 0; i < pb.label_sets.size(); ++i) {
            pb.label_sets[i].first = first;
            pb.label_sets[i].n = (int)pb.label_members[i].size();
            std::memcpy(mem + first, pb.label_members[i].data(), sizeof(LabelMember) * pb.label_members[i].size());
            first += pb.label_sets[i].n;
        }
        std::memcpy(tab, pb.label_sets.data(), sets_bytes);
        pb.label_table_bytes = (sets_bytes + sizeof(LabelMember) * (size_t)first + 15) & ~(size_t)15;
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
    PendingBatch& pb = e->pending;
    double hp_t = e->knobs.host_prof ? host_now_us() : 0.0;
    pb.submit_t0 = host_now_us();
    // bound the batches in flight (see roft_engine::lead); this also frees the batch ring slot
    TRY(wait_batch(e, e->batch_counter - e->lead, &pb.throttled));
    pb.wait_us = host_now_us() - pb.submit_t0;
    HP_MARK(e, 0, hp_t);   // time blocked on the GPU
    // what a refused call puts back (SubmitSnapshot: not the h2d counters of roft_engine_stats, which count what crossed the bus)
    SubmitSnapshot& snap = e->snapshot;
    snap.sched.resize(e->objs.size());
    for (size_t i = 0; i < e->objs.size(); ++i) snap.sched[i] = e->objs[i]->s;
    snap.flow = e->flow.stats;
    snap.depth = e->depth.stats;
    snap.rectify = e->rectify.stats;
    pb.reset(n_objects, n_frames);
    e->depth.timed = false;
    e->rectify.timed = false;
    int rc = submit_frames(e, inputs, labels, images, n_objects, n_frames);
    if (rc == ROFT_OK) rc = flush_gather(e);
    HP_MARK(e, 1, hp_t);
    int rc2 = ROFT_OK;
    BatchSlot& bs = e->slot_of(e->batch_counter);
    hipEvent_t ev_wait = nullptr;   // what the host waits for: the copies
    if (rc == ROFT_OK && pb.facts.produced_flows) {
        // Camera images and raw depth: the production follows the copies on the upload stream.  The streams wait for ev_up, recorded behind the
        // production; the host for ev_host, recorded behind the copies alone -- and for nothing when nothing was copied.
        hipError_t err = hipSuccess;
        if (pb.facts.had_uploads) { err = hipEventRecord(bs.ev_host, e->up_stream); ev_wait = bs.ev_host; }
        if (err == hipSuccess && !pb.rect_jobs.empty()) rc = enqueue_rectification(e);
        if (err == hipSuccess && rc == ROFT_OK && !pb.depth_jobs.empty()) rc = enqueue_depth_production(e);
        if (err == hipSuccess && rc == ROFT_OK && e->flow.enabled) rc = enqueue_flow_production(e, n_frames);
        if (err == hipSuccess && rc == ROFT_OK) err = hipEventRecord(bs.ev_up, e->up_stream);
        if (err != hipSuccess) rc2 = fail(ROFT_ERR_DEVICE, std::string("flow production: ") + hipGetErrorString(err));
    } else if (pb.facts.had_uploads) {
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
        for (size_t i = 0; i < e->objs.size(); ++i) e->objs[i]->s = snap.sched[i];
        e->flow.stats = snap.flow;
        e->depth.stats = snap.depth;
        e->rectify.stats = snap.rectify;
        return fail(rc != ROFT_OK ? rc : rc2, msg);
    }
    e->submitted = true;
    e->device_pointers_checked = true;
    e->pose_masks.stats.silhouettes += pb.facts.pose_masks;
    e->pose_masks.stats.frames += __builtin_popcount(pb.pose_mask_frames);
    e->pose_masks.occl_stats.resolved += pb.facts.pose_resolve;
    e->pose_masks.gate_stats.gated += pb.gated_pairs;
    pb.submit_us = host_now_us() - pb.submit_t0;
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
    f.pyr.clear();   // (enabled again with other levels: another pyramid size)
    f.pyr.resize((size_t)e->T_max + 1);
    f.prm = prm;
    f.enabled = true;
    f.check = false;   // (enabled again: the check is asked for again, behind this call)
    return ROFT_OK;
}

// include/roft_engine.h section 3f
int roft_engine_enable_flow_consistency(roft_engine* e, const roft_of_consistency* c)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    if (!e->flow.enabled) return fail(ROFT_ERR_STATE, "roft_engine_enable_flow_consistency follows roft_engine_enable_flow");
    if (e->frame_counter > 0 || e->submitted) return fail(ROFT_ERR_STATE, "roft_engine_enable_flow_consistency must precede the first frame");
    if (e->cfg.flow_type != ROFT_FLOW_F32C2)
        return fail(ROFT_ERR_INVALID, "flow consistency: CV_16SC2 has no representation of an invalid vector, the check serves a CV_32FC2 engine only");
    roft_of_consistency tol;
    if (c) tol = *c; else (void)roft_default_of_consistency(&tol);
    if (int rc = roft::of_check_consistency(&tol)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    EngineFlow& f = e->flow;
    HIP_TRY(f.back.ensure((size_t)kOfCheckChunk * 2 * e->cfg.cam.width * e->cfg.cam.height));
    f.tol = tol;
    f.check = true;
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

// ---- masks from poses (include/roft_engine.h section 3e) -------------------------------------------------------------------------
int roft_engine_enable_pose_masks(roft_engine* e, const int* obj_ids, int n_ids)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    if (n_ids < 0 || (n_ids > 0 && !obj_ids)) return fail(ROFT_ERR_INVALID, "pose masks: n_ids object ids required (n_ids 0: every object)");
    if (e->frame_counter > 0 || e->submitted) return fail(ROFT_ERR_STATE, "roft_engine_enable_pose_masks must precede the first frame");
    if (e->cfg.stamped_masks) return fail(ROFT_ERR_INVALID, "pose masks: a pose carries no stamp, an engine with stamped_masks cannot place its silhouette in the flow queue");
    if (e->cfg.render_mode == ROFT_RENDER_GL)
        return fail(ROFT_ERR_INVALID, "pose masks are drawn under ROFT_RENDER_CONTRACT: an engine with render_mode ROFT_RENDER_GL keeps its meshes "
                                      "unsorted and without the flip bits of the back-face rule, so the defining render does not exist there");
    for (int i = 0; i < n_ids; ++i) {
        const int id = obj_ids[i];
        if (id < 0 || id >= (int)e->objs.size()) return fail(ROFT_ERR_INVALID, "pose masks: " + std::to_string(id) + " is not an object of the engine");
        if (!has_mesh(e->h_params[id]))
            return fail(ROFT_ERR_INVALID, "pose masks: object " + std::to_string(id) + " was added without a mesh");
    }
    if (e->cfg.cam.width / 32 > kSilhouetteWindowWords) return fail(ROFT_ERR_INVALID, "pose masks: an image row is wider than the kernel's bit window");
    HIP_TRY(hipSetDevice(e->cfg.device));
    EnginePoseMasks& pm = e->pose_masks;
    // nothing of the launch may happen for the first time inside a caller's timed region (engine_setup): each event pair has completed
    // one dispatch on the streams that will carry it
    for (int i = 0; i < roft_engine::kBatchRing; ++i) {
        HIP_TRY(pm.ev_start[i].create());
        HIP_TRY(pm.ev_stop[i].create());
        hipExtLaunchKernelGGL(probe_tiny_kernel, dim3(1), dim3(64), 0, (i & 1) ? e->up_stream : e->stream, pm.ev_start[i], pm.ev_stop[i], 0,
                              reinterpret_cast<int*>(e->arr.a.mask_general));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(e->up_stream));
    HIP_TRY(hipMemset(e->arr.a.mask_general, 0, sizeof(unsigned)));   // (what the probe touched)
    if (n_ids == 0) pm.all = true;
    for (int i = 0; i < n_ids; ++i) e->objs[obj_ids[i]]->pose_masks = true;
    pm.enabled = true;
    return ROFT_OK;
}

int roft_engine_get_pose_mask_stats(roft_engine* e, roft_engine_pose_mask_stats* out)
{
    if (!e || !out) return fail(ROFT_ERR_INVALID, "null argument");
    *out = e->pose_masks.stats;
    return ROFT_OK;
}

// Objects of one scene hide each other.  Scenes with at least two members get a z-buffer each; everything the hot path touches is
// allocated here.
int roft_engine_enable_pose_mask_occlusion(roft_engine* e, const int* obj_ids, const int* scene_ids, int n_ids)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    if (n_ids < 0 || (n_ids > 0 && (!obj_ids || !scene_ids)))
        return fail(ROFT_ERR_INVALID, "pose mask occlusion: n_ids object ids and scene ids required (n_ids 0: every enrolled object in scene 0)");
    if (e->frame_counter > 0 || e->submitted) return fail(ROFT_ERR_STATE, "roft_engine_enable_pose_mask_occlusion must precede the first frame");
    EnginePoseMasks& pm = e->pose_masks;
    if (!pm.enabled) return fail(ROFT_ERR_STATE, "pose mask occlusion: roft_engine_enable_pose_masks comes first");
    auto enrolled = [&](int id) { return e->objs[id]->pose_masks || (pm.all && has_mesh(e->h_params[id])); };
    for (int i = 0; i < n_ids; ++i) {
        const int id = obj_ids[i];
        if (id < 0 || id >= (int)e->objs.size()) return fail(ROFT_ERR_INVALID, "pose mask occlusion: " + std::to_string(id) + " is not an object of the engine");
        if (!enrolled(id)) return fail(ROFT_ERR_INVALID, "pose mask occlusion: object " + std::to_string(id) + " is not enrolled with roft_engine_enable_pose_masks");
        if (scene_ids[i] < 0) return fail(ROFT_ERR_INVALID, "pose mask occlusion: scene ids are >= 0");
    }
    // the scenes as they will be, and a z-buffer for each that has at least two members
    const int n = (int)e->objs.size();
    std::vector<int> scene((size_t)n), zscene((size_t)n, -1);
    for (int id = 0; id < n; ++id) scene[id] = (n_ids == 0 && enrolled(id)) ? 0 : e->objs[id]->pose_scene;
    for (int i = 0; i < n_ids; ++i) scene[obj_ids[i]] = scene_ids[i];
    int n_z = 0;
    for (int id = 0; id < n; ++id) {
        if (scene[id] < 0 || zscene[id] >= 0) continue;
        int members = 0;
        for (int k = id; k < n; ++k) members += scene[k] == scene[id];
        if (members < 2) continue;
        for (int k = id; k < n; ++k)
            if (scene[k] == scene[id]) zscene[k] = n_z;
        ++n_z;
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (n_z > 0) {
        HIP_TRY(pm.zbuf.ensure((size_t)2 * kMaxBatch * n_z * e->cfg.cam.width * e->cfg.cam.height));
        HIP_TRY(pm.zpairs.ensure((size_t)2 * kMaxBatch * e->cfg.max_objects));
        HIP_TRY(hipMemset(pm.zpairs.p, 0, sizeof(SilhouettePair) * pm.zpairs.n));
    }
    HIP_TRY(pm.zstats.ensure(2, true));
    for (int id = 0; id < n; ++id) { e->objs[id]->pose_scene = scene[id]; e->objs[id]->pose_zscene = zscene[id]; }
    pm.n_zscenes = n_z;
    pm.occlusion = true;
    return ROFT_OK;
}

// (hidden and pixels_removed are counted by the resolve on the device: the call waits for the batches stepped so far)
int roft_engine_get_pose_mask_occlusion_stats(roft_engine* e, roft_engine_pose_mask_occlusion_stats* out)
{
    if (!e || !out) return fail(ROFT_ERR_INVALID, "null argument");
    EnginePoseMasks& pm = e->pose_masks;
    if (pm.occlusion && pm.zstats.p) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(hipStreamSynchronize(e->up_stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        unsigned long long h[2] = {0, 0};
        HIP_TRY(hipMemcpy(h, pm.zstats.p, sizeof(h), hipMemcpyDeviceToHost));
        pm.occl_stats.hidden = (long long)h[0];
        pm.occl_stats.pixels_removed = (long long)h[1];
    }
    *out = pm.occl_stats;
    return ROFT_OK;
}

// Silhouettes gated against the depth of the pose's own frame.  Everything the hot path touches is allocated here.
int roft_default_pose_mask_gate(roft_pose_mask_gate* g)
{
    if (!g) return fail(ROFT_ERR_INVALID, "null argument");
    g->front_tolerance = 0.02f;
    g->behind_tolerance = 0.0f;
    return ROFT_OK;
}

int roft_engine_enable_pose_mask_depth_gate(roft_engine* e, const roft_pose_mask_gate* g)
{
    if (!e) return fail(ROFT_ERR_INVALID, "null engine");
    roft_pose_mask_gate prm;
    if (g) prm = *g; else (void)roft_default_pose_mask_gate(&prm);
    if (!pose_mask_gate_valid(prm.front_tolerance, prm.behind_tolerance))
        return fail(ROFT_ERR_INVALID, "pose mask depth gate: front_tolerance must be finite and > 0, behind_tolerance finite (<= 0: that test is off)");
    if (e->frame_counter > 0 || e->submitted) return fail(ROFT_ERR_STATE, "roft_engine_enable_pose_mask_depth_gate must precede the first frame");
    EnginePoseMasks& pm = e->pose_masks;
    if (!pm.enabled) return fail(ROFT_ERR_STATE, "pose mask depth gate: roft_engine_enable_pose_masks comes first");
    if (e->cfg.cam.width / 32 > kSilhouetteWindowWords / 3) return fail(ROFT_ERR_INVALID, "pose mask depth gate: an image row is wider than a third of the kernel's bit window");
    HIP_TRY(hipSetDevice(e->cfg.device));
    if (!pm.zpairs.p) {
        HIP_TRY(pm.zpairs.ensure((size_t)2 * kMaxBatch * e->cfg.max_objects));
        HIP_TRY(hipMemset(pm.zpairs.p, 0, sizeof(SilhouettePair) * pm.zpairs.n));
    }
    HIP_TRY(pm.gstats.ensure(3, true));
    pm.gate_prm = prm;
    pm.gate = true;
    return ROFT_OK;
}

// (emptied and the pixel counts are counted on the device: the call waits for the batches stepped so far)
int roft_engine_get_pose_mask_gate_stats(roft_engine* e, roft_engine_pose_mask_gate_stats* out)
{
    if (!e || !out) return fail(ROFT_ERR_INVALID, "null argument");
    EnginePoseMasks& pm = e->pose_masks;
    if (pm.gate && pm.gstats.p) {
        HIP_TRY(hipSetDevice(e->cfg.device));
        HIP_TRY(hipStreamSynchronize(e->up_stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        unsigned long long h[3] = {0, 0, 0};
        HIP_TRY(hipMemcpy(h, pm.gstats.p, sizeof(h), hipMemcpyDeviceToHost));
        pm.gate_stats.emptied = (long long)h[0];
        pm.gate_stats.pixels_front = (long long)h[1];
        pm.gate_stats.pixels_behind = (long long)h[2];
    }
    *out = pm.gate_stats;
    return ROFT_OK;
}

int roft_debug_pose_mask_kernel_ms(roft_engine* e, double* ms_out)
{
    if (!e || !ms_out) return fail(ROFT_ERR_INVALID, "null argument");
    const EnginePoseMasks& pm = e->pose_masks;
    if (!pm.enabled || pm.last_slot < 0) return fail(ROFT_ERR_STATE, "no silhouette launch so far");
    if (!pm.last_timed) return fail(ROFT_ERR_STATE, "the last silhouette launch ended with the preparation's event, which takes no time stamps (roft_engine_enable_timing times every launch)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipEventSynchronize(pm.ev_stop[pm.last_slot]));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, pm.ev_start[pm.last_slot], pm.ev_stop[pm.last_slot]));
    *ms_out = (double)ms;
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
    if (!e->depth.enabled && !e->rectify.enabled)
        return fail(ROFT_ERR_STATE, "the engine makes no depth: neither roft_engine_enable_raw_depth nor roft_engine_enable_rectification was called");
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

// ---- lens distortion (include/roft_engine.h section 3g) ---------------------------------------------------------------------------
int roft_engine_enable_rectification(roft_engine* e, const roft_lens* lens)
{
    if (!e || !lens) return fail(ROFT_ERR_INVALID, "null argument");
    if (e->frame_counter > 0 || e->submitted) return fail(ROFT_ERR_STATE, "roft_engine_enable_rectification must precede the first frame");
    if (int rc = rect_check_lens(*lens)) return rc;
    const roft_camera& cam = e->cfg.cam;
    if (lens->cam.width != cam.width || lens->cam.height != cam.height)
        return fail(ROFT_ERR_INVALID, "the lens' source camera must have the size of roft_config::cam (its intrinsics may differ)");
    if (int rc = rect_check_camera(cam, "target")) return rc;
    EngineRectify& r = e->rectify;
    rect_geometry(r.geom, *lens, cam);
    r.lens = *lens;
    r.enabled = true;
    return ROFT_OK;
}

int roft_engine_get_rectify_stats(roft_engine* e, roft_engine_rectify_stats* out)
{
    if (!e || !out) return fail(ROFT_ERR_INVALID, "null argument");
    *out = e->rectify.stats;
    return ROFT_OK;
}

int roft_debug_rectify_kernel_ms(roft_engine* e, double* ms_out)
{
    if (!e || !ms_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (!e->rectify.timed) return fail(ROFT_ERR_STATE, "the engine's last submit call made no rectified product");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipEventSynchronize(e->rectify.ev1));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, e->rectify.ev0, e->rectify.ev1));
    *ms_out = (double)ms;
    return ROFT_OK;
}
