// engine_internal.h -- what the translation units of the host side of libroft_hip.so share: device buffers, the arrays of an
// engine, the host-side mirrors of the reference's source / measurement state machines (Sched), the engine object itself and
// the few functions that cross a file boundary.  Not installed, not part of the ABI (that is include/roft_engine.h).
//
//   device_owned.h      fail / HIP_TRY / TRY, "is the device there", and the owners of device memory (DevBuf), pinned host memory (PinnedBuf)
//                       and events (Event): every allocation of the host side is a member of one of them (also flow_producer.hip, k_depth.hip)
//   engine.hip          error string, pinned host pool, defaults, stream sets, roft_engine_create / destroy, roft_object_add,
//                       roft_objects_restart
//   engine_submit.hip   roft_frames_submit: the frame programs (build_pose_program), HOST staging, the control blocks of a batch
//   batch_plan.h        SchedKnobs (the engine's switches, read at creation) and plan_batch: what a batch's launch graph will be, decided
//                       from counters before anything is enqueued (host-only C++, tested without a GPU)
//   engine_step.hip     roft_step / roft_sync: step_batch enqueues a BatchPlan on the engine's four streams; the timing marks
//   engine_results.hip  state, outputs, log, masks, timing and batch-trace readers
//   op_context.h        the ONE context of the operator-level entry points: it owns device memory, a stream and a mutex, never settings --
//                       the entry (lock, device, stream), the one-object arrays derived by value, typed scratch, the state's landing block
//   engine_ops.hip      the operator-level entry points on that context (roft_flow_measurement ... roft_outlier_test, roft_pose_errors,
//                       roft_pose_errors_vsd)
//   engine_quality.hip  track quality: roft_engine_enable_quality / _get_quality, the batch's quality launch; roft_track_quality (on op_context.h)
//   engine_hypotheses.hip  pose hypotheses: roft_pose_hypotheses_score (on op_context.h) and roft_engine_score_hypotheses, one launcher
//   engine_debug.hip    roft_debug_* (diagnostics and experiments)
//   scene.hip           the scene renderer: roft_scene_renderer_*, roft_render_scene
//   mesh_class.h        a caller's mesh on the host: has_mesh, the array check, classification, the three upload layouts (host-only C++)
//   mesh_clusters.h     the walk-order triangles cut into clusters of 64 for the outlier test's contract render (host-only C++ + the cone test)
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "device_owned.h"
#include "roft_device.h"
#include "mesh_class.h"
#include "mesh_clusters.h"
#include "scene.h"
#include "batch_plan.h"
#include "pose_mask_gate.h"
#include "opticalflow.h"
#include "depth.h"
#include "rectify.h"
#include "quality.h"
#include "symmetry.h"
#include "vsd.h"
#include "hypotheses.h"

static_assert(roft::host::kPlanLanes == roft::kNumLin, "batch_plan.h plans for the engine's pose lanes");


namespace roft {
namespace host {

// The one refusal (ROFT_ERR_INVALID, before any device is looked for) of a caller's mesh at every site that draws one; `what` names it
// in the text ("mesh 3").  The site's policy: may the mesh be absent; tri_index_bits > 0: n_tris must stay below 2^bits.
inline int check_mesh(const roft_mesh& m, const std::string& what, bool may_be_absent, int tri_index_bits = 0)
{
    if (!has_mesh(m)) return may_be_absent ? ROFT_OK : fail(ROFT_ERR_INVALID, what + ": no vertices or no triangles");
    if (tri_index_bits > 0 && m.n_tris >= (1 << tri_index_bits))
        return fail(ROFT_ERR_INVALID, what + ": 2^" + std::to_string(tri_index_bits) + " triangles or more (a triangle's index is kept in that many bits)");
    const MeshFault f = check_mesh_arrays(m.verts, m.n_verts, m.tris, m.n_tris);
    if (f.kind == MeshFault::kNullArray) return fail(ROFT_ERR_INVALID, what + ": null vertex or triangle array");
    if (f.kind == MeshFault::kBadIndex)
        return fail(ROFT_ERR_INVALID, what + ": triangle " + std::to_string(f.triangle) + " refers to vertex " + std::to_string(f.vertex) + " of " +
                                          std::to_string(m.n_verts));
    return ROFT_OK;
}

// ... and the one resident copy.  "No mesh" until a mesh that has_mesh has gone up; the buffers grow on demand and are kept, so a
// context uploads one mesh after the other into the same DeviceMesh.
struct DeviceMesh {
    DevBuf<float> verts;
    DevBuf<int32_t> tris;
    DevBuf<uint8_t> flip;
    DevBuf<uint32_t> cl_headers, cl_words;   // the triangles as clusters (mesh_clusters.h): uploads that ask for them
    DevBuf<float> cl_slots, box_corners;
    int n_verts = 0, n_tris = 0, n_clusters = 0;
    bool closed = false;   // the current upload was of a closed mesh in a layout with flip bits: `flip` holds them

    // `m` (which has passed check_mesh) in `layout` (mesh_class.h), copied on stream s.  Returns only when the copies have read
    // their host arrays: the prepared triangle order and flip bits live in this call.  An absent mesh, or a failed upload, leaves
    // "no mesh"; an absent mesh makes no device call.  MeshLayout::kWalkClusters: the triangles go up as clusters as well.
    int upload(const roft_mesh& m, MeshLayout layout, hipStream_t s)
    {
        const bool clusters = layout == MeshLayout::kWalkClusters;
        n_verts = n_tris = n_clusters = 0;
        closed = false;
        if (!has_mesh(m)) return ROFT_OK;
        PreparedMesh pm;
        prepare_mesh(m.verts, m.n_verts, m.tris, m.n_tris, layout, pm);
        HIP_TRY(verts.ensure((size_t)3 * m.n_verts));
        HIP_TRY(tris.ensure((size_t)3 * m.n_tris));
        HIP_TRY(hipMemcpyAsync(verts.p, m.verts, sizeof(float) * 3 * m.n_verts, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(tris.p, pm.tris(m.tris), sizeof(int32_t) * 3 * m.n_tris, hipMemcpyHostToDevice, s));
        if (pm.closed) {
            HIP_TRY(flip.ensure((size_t)m.n_tris));
            HIP_TRY(hipMemcpyAsync(flip.p, pm.flip.data(), (size_t)m.n_tris, hipMemcpyHostToDevice, s));
        }
        MeshClusters mc;
        if (clusters) {
            build_clusters(m.verts, m.n_verts, pm.tris(m.tris), m.n_tris, pm.closed ? pm.flip.data() : nullptr,
                           pm.bucket.empty() ? nullptr : pm.bucket.data(), mc);
            HIP_TRY(cl_headers.ensure(mc.headers.size()));
            HIP_TRY(cl_slots.ensure(mc.slots.size()));
            HIP_TRY(cl_words.ensure(mc.words.size()));
            HIP_TRY(box_corners.ensure(24));
            HIP_TRY(hipMemcpyAsync(cl_headers.p, mc.headers.data(), sizeof(uint32_t) * mc.headers.size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(cl_slots.p, mc.slots.data(), sizeof(float) * mc.slots.size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(cl_words.p, mc.words.data(), sizeof(uint32_t) * mc.words.size(), hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(box_corners.p, &mc.box[0][0], sizeof(float) * 24, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        n_verts = m.n_verts;
        n_tris = m.n_tris;
        n_clusters = mc.n_clusters;
        closed = pm.closed;
        return ROFT_OK;
    }

    // what a kernel is given: null pointers without a mesh, and no flip bits unless THIS upload made them
    MeshView view() const
    {
        const bool has = has_mesh(*this);
        return MeshView{has ? verts.p : nullptr, has ? tris.p : nullptr, closed ? flip.p : nullptr, n_verts, n_tris};
    }
    void describe(ObjParams& p) const   // (the mesh fields of an object's parameter block)
    {
        const MeshView m = view();
        p.verts = m.verts; p.tris = m.tris; p.tri_flip = m.flip;
        p.n_verts = m.n_verts; p.n_tris = m.n_tris;
        const bool cl = has_mesh(*this) && n_clusters > 0;
        p.cl_headers = cl ? cl_headers.p : nullptr; p.cl_slots = cl ? cl_slots.p : nullptr; p.cl_words = cl ? cl_words.p : nullptr;
        p.box_corners = cl ? box_corners.p : nullptr; p.n_clusters = cl ? n_clusters : 0;
    }
};

inline size_t flow_bytes(const DevFlowFmt& f)
{
    return (size_t)f.cols * f.rows * 2 * (f.type == ROFT_FLOW_S16C2 ? sizeof(int16_t) : sizeof(float));
}

inline DevCamera make_cam(const roft_camera& c)
{
    DevCamera d;
    d.W = c.width;
    d.H = c.height;
    d.wpr = c.width / 32;
    d.divider = (c.width == 640) ? 2 : 4;  // ROFTFilter.cpp:191-193
    d.fx = c.fx; d.fy = c.fy; d.cx = c.cx; d.cy = c.cy;
    return d;
}

inline int check_geometry(int W, int H)
{
    if (W <= 0 || H <= 0 || (W % 32) != 0 || (((size_t)W * H) % 64) != 0)
        return fail(ROFT_ERR_INVALID, "image width must be a multiple of 32 and width*height a multiple of 64");
    if ((size_t)W * H >= (1u << 24))
        return fail(ROFT_ERR_INVALID, "width*height must be < 2^24 (float-accumulated sampling index, hpp:237)");
    // (No bound from the LDS: the mask frames work on windows of a band's rows, the flow measurement and the feature kernel read
    //  planes that do not fit the LDS -- beyond ~1.1 Mpixel -- from memory, the general mask path lists its groups in pieces.
    //  The reference scans any cv::Mat, ImageOpticalFlowMeasurement.hpp:231-256.)
    return ROFT_OK;
}

// Device arrays for n objects of one geometry
struct Arrays {
    EngineArrays a{};
    DevBuf<ObjParams> params;
    DevBuf<ObjState> state;
    DevBuf<FrameCtrl> ctrl;
    DevBuf<uint32_t> planes;
    DevBuf<int32_t> map;
    DevBuf<FlowRec> cand, recs;
    DevBuf<double> norms;
    DevBuf<int> npts;
    DevBuf<MaskRec> mrec;
    DevBuf<unsigned> mask_general;
    DevBuf<uint32_t> feat_pix;
    DevBuf<float> feat_depth;
    DevBuf<uint32_t> zbuf;
    DevBuf<uint32_t> zmerge;   // merge slabs of the outlier test (EngineArrays::zmerge)
    DevBuf<int> zcount;
    // (re)allocates the merge slabs for n objects and tiles of tpix pixels: enough for the automatic band count at any number of
    // objects up to n (objects * bands <= max(n, CUs / 2)); a caller who asks for more bands than that gets the row split
    int ensure_zmerge(int n, size_t tpix)
    {
        const size_t slabs = std::max<size_t>((size_t)n, std::min<size_t>((size_t)n * kMaxOutlierParts, (size_t)std::max(device_cu_count() / 2, 1)));
        const size_t need = (size_t)kNumLin * slabs * 2 * tpix;
        if (need > zmerge.n || !zmerge.p || tpix != a.zmerge_stride || slabs != a.zmerge_slabs) {
            HIP_TRY(zmerge.ensure(need));
            a.zmerge_stride = tpix;
            a.zmerge_slabs = slabs;
        }
        HIP_TRY(zcount.ensure((size_t)kNumLin * n * 2 * kMaxOutlierParts, true));
        a.zmerge = zmerge.p;
        a.zcount = zcount.p;
        return ROFT_OK;
    }
    DevBuf<roft_object_output> log;
    DevBuf<unsigned long long> skf_started, residency;

    int alloc(int n_obj, int T, const DevCamera& cam, const DevFlowFmt& ffmt, int radius)
    {
        a.n_obj = n_obj;
        a.T = 1;
        a.cam = cam;
        a.ffmt = ffmt;
        a.plane_words = (size_t)cam.wpr * cam.H;
        const size_t npix = (size_t)cam.W * cam.H;
        a.cand_cap = ((int)((npix + radius - 1) / std::max(radius, 1)) + 9) & ~1;   // even: rows of a.cand stay 8-byte aligned
        a.feat_cap = (int)(npix / 2 + 8);
        a.tile_w = cam.W / cam.divider;
        a.tile_h = cam.H / cam.divider;
        HIP_TRY(params.ensure(n_obj, true));
        HIP_TRY(state.ensure(n_obj, true));
        HIP_TRY(ctrl.ensure((size_t)n_obj * T, true));
        HIP_TRY(planes.ensure((size_t)n_obj * kPlaneSlotsTotal * 2 * a.plane_words, true));
        HIP_TRY(mrec.ensure((size_t)2 * n_obj * (kMaxBatch + 1), true));   // two tables (batch parity)
        HIP_TRY(mask_general.ensure(n_obj, true));
        HIP_TRY(map.ensure((size_t)n_obj * npix, true));
        HIP_TRY(cand.ensure((size_t)n_obj * T * a.cand_cap));
        HIP_TRY(recs.ensure((size_t)n_obj * T * a.cand_cap));
        HIP_TRY(npts.ensure((size_t)n_obj * T, true));
        HIP_TRY(norms.ensure((size_t)n_obj * 3 * a.cand_cap));
        HIP_TRY(feat_pix.ensure((size_t)n_obj * kFeatRing * a.feat_cap));
        HIP_TRY(feat_depth.ensure((size_t)n_obj * kFeatRing * a.feat_cap));
        HIP_TRY(zbuf.ensure((size_t)2 * a.tile_w * a.tile_h));   // operator level only (roft_depth_likelihood)
        if (int rc = ensure_zmerge(n_obj, (size_t)a.tile_w * a.tile_h)) return rc;
        a.params = params.p; a.state = state.p; a.ctrl = ctrl.p; a.planes = planes.p; a.map = map.p;
        a.cand = cand.p; a.recs = recs.p; a.norms = norms.p; a.npts = npts.p; a.mrec = mrec.p;
        a.mask_general = mask_general.p;
        a.mrec_carry = mrec.p; a.slot_new = kSlotNew; a.slot_prev0 = -1; a.feat_pix = feat_pix.p; a.feat_depth = feat_depth.p;
        a.zbuf = zbuf.p;
        a.out_log = nullptr;
        a.log_cap = 0;
        a.max_tris = 0;
        a.max_verts = 0;
        a.meshes_without_clusters = 0;
        a.ukf_chol_guard = 0.0;
        a.ukf_chol_guard_bil = 0.0;
        a.mask_wgs = 0;
        a.outlier_parts = 0;
        a.dev_error = nullptr;
        a.k1_span = nullptr;
        HIP_TRY(skf_started.ensure(1, true));
        HIP_TRY(residency.ensure(32, true));
        a.residency = residency.p;
        a.skf_started = nullptr;   // (the batched engine sets it; the operator level runs its kernels one after the other)
        a.handoff = 0;
        return ROFT_OK;
    }
};

// Device scratch of the pose-error metrics (roft_pose_errors / roft_engine_score_log): grows on demand, kept between calls.
struct PoseErrorScratch {
    DevBuf<double> pts, est, ref, cloud, partial, out, sym;
    Event ev0, ev1;   // around the kernels of the last call (roft_debug_pose_errors_kernel_ms)
    bool timed = false;
};
// ADD / ADD-S of n pose pairs on stream s (engine_ops.hip).  d_pts: P x 3 doubles on the device.  The estimates are est_host
// (n x 7 host doubles, uploaded) or, when that is null, est_dev (already on the device).  ref_host: n x 7 host doubles;
// out_host: n doubles.  Returns when the results are in out_host.
int pose_errors_run(PoseErrorScratch& sc, int kind, const double* d_pts, int P, const double* est_host, PoseView est_dev,
                    const double* ref_host, int n, double* out_host, hipStream_t s);
// MSSD / MSPD under a symmetry group (roft_pose_errors_sym / roft_engine_score_log_sym).  check_pose_errors_sym: the refusals the
// two share -- unknown kind, a bad group (cap ROFT_MAX_SCORE_SYMMETRIES), MSPD without a usable camera -- on the host, no device.
// pose_errors_sym_run: as pose_errors_run; sym_host: n_sym x 7 host doubles, cam: read for MSPD only.
int check_pose_errors_sym(int kind, const double* sym, int n_sym, const roft_camera* cam);
int pose_errors_sym_run(PoseErrorScratch& sc, int kind, const double* d_pts, int P, const double* est_host, PoseView est_dev,
                        const double* ref_host, int n, const double* sym_host, int n_sym, const roft_camera* cam, double* out_host,
                        hipStream_t s);

// Device scratch of the VSD score (roft_pose_errors_vsd): grows on demand, kept between calls.  depth: the images of one chunk of
// pairs, or the one image under every pair.
struct VsdScratch {
    DevBuf<double> est, ref, out;
    DevBuf<float> depth;
    DevBuf<int32_t> counts, rows;
};

inline void init_state(ObjState& st)
{
    std::memset(&st, 0, sizeof(st));
    for (PoseLane& pl : st.lane) { pl.pending_frame = -1; pl.outlier_selected = -1; }
    st.n_flow_points = -1;
}

inline void clear_ctrl(FrameCtrl& c)
{
    std::memset(&c, 0, sizeof(c));
    c.outlier_step = -1;
    c.feat_write = c.feat_read = -1;
}



struct FlowEntry {
    const void* ptr;
    int frame;   // frame index the flow was delivered with
    int owned;   // index into HostObject::owned when the engine holds its own copy, else -1
    // the depth of the object's frame before the one that delivered the flow (Sched::depth_prev when the flow was pushed; null: none):
    // what a silhouette whose chase starts at this flow is gated against (pose_mask_gate.h).  Cloned with the flow (OwnedFlow::depth)
    const float* depth_before;
};

// Schedule-driven mirrors of the reference's source / measurement-model state machines.  Trivially copyable: a submit
// call works on the live copy and restores the snapshot taken at its start if it fails, so a failed call consumes
// nothing.
struct Sched {
    // TWO frame counters ("Restarting object slots").  frame_idx is the ENGINE's number of the object's next frame: every
    // ring -- plane slots, twist slots and their tags, hist[].frame, log and quality rows -- is indexed by it, so that the object's
    // slots agree with what the kernels derive from roft_engine::frame_counter.  track_frames counts the frames since the object's
    // track started (roft_object_add, roft_objects_restart) and answers the first-frame questions.  They differ after a restart.
    int frame_idx = 0;
    int track_frames = 0;
    bool seg_available = false;        // ImageSegmentationOFAidedSource::segmentation_available_
    bool of_first_frame = true;        // ...::is_first_frame_
    bool flow_first_frame = true;      // ImageOpticalFlowMeasurement::is_first_frame_
    bool features_initialized = false; // ROFTFilter::outlier_rejection_features_initialized_
    int feat_slot = 0;                 // feature ring slot holding the buffered outlier-rejection features
    int feat_next = 0;                 // next ring slot to write
    int feat_use[kFeatRing];           // last batch that reads or writes each feature ring slot (-1: never used)
    int feat_batch[kFeatRing];         // batch that last wrote each feature set (-1: none)
    int n_hist = 0;
    FlowEntry hist[kMaxFlowHist];      // last valid flows, newest first
    int n_stamps = 0;
    double stamps[30];                 // stamped source: RGB stamps of the last 30 valid flows, oldest first
    int n_vel = 0;
    int vel_buf[kTwistRing];           // twist_hist slots (CartesianQuaternionMeasurement::buffer_velocities_), oldest first
    int last_meas_slot = 0;            // slot of measurement_.head<6>()
    int cur_slot = 0;                  // B_LIN0 / B_LIN1: slot holding p_corr_belief_ (the other one holds buffered_belief_)
    int own[kNumLin] = {0, 1};         // pose chain lane that walks each of the two slots (always different lanes)
    int last_touch[kNumLin] = {-1, -1};   // last batch whose pose chain reads or writes each slot
    int flows_since_mask = 0;          // upper bound of the flows buffered since the last delivered mask
    // ... and the number itself where every delivered mask had pixels (the host cannot see an empty one: flow_buffer_ of the OF-aided
    // source, this frame's flow counted in; 0 again behind a delivered mask): what names the gate frame (pose_mask_gate.h)
    int flows_buffered = 0;
    const float* depth_prev = nullptr;
    // camera images (roft_frames_submit_images): the pyramid slot of the image the frame before carried, in that frame's
    // generation (EngineFlow::pyr; -1: it carried none), and the flow the engine produced for the last frame (null: none)
    int pyr_prev = -1;
    const void* flow_made = nullptr;
    Sched() { for (int i = 0; i < kFeatRing; ++i) feat_use[i] = feat_batch[i] = -1; }
};

struct OwnedFlow {
    DevBuf<unsigned char> buf;
    DevBuf<float> depth;       // engines with the depth gate: the clone of FlowEntry::depth_before
    int last_ref_frame = -1;   // last frame whose control block references the copy
};

struct HostObject {
    Sched s;
    int stepped_slot = 0, stepped_lane = 0;   // slot holding p_corr_belief_ after the last stepped frame, and its lane
    const void* stepped_flow = nullptr;       // the flow produced for the last stepped frame (roft_engine_get_flow), or null
    const float* stepped_depth = nullptr;     // the depth of the last stepped frame (roft_engine_get_depth reads it on a raw-depth engine)
    std::vector<OwnedFlow> owned;   // engine copies of flows that outlived the zero-copy retention window
    DeviceMesh mesh;   // what ObjParams of the object names (absent: the object was described without one)
    // roft_object_set_symmetry: the device copy of the object's group (16 elements: allocated once, at the first group), which
    // ObjParams::sym names while n_sym > 1.  Goes with the mesh: a restart that replaces the mesh drops it.
    DevBuf<double> sym;
    int n_sym = 0;
    // masks from poses (roft_engine_enable_pose_masks): the object is enrolled; the pose of roft_object_desc::p_mean0 (x, q = w x y z),
    // which stands in for a first frame that brings none
    bool pose_masks = false;
    // ... and the scene it shares with others (roft_engine_enable_pose_mask_occlusion; -1: a scene of its own), and that scene's
    // z-buffer where it has at least two members (-1: none, the object is always drawn alone)
    int pose_scene = -1, pose_zscene = -1;
    double pose0[7] = {0, 0, 0, 1, 0, 0, 0};
    // roft_objects_restart: what roft_get_outputs showed for the track that ended, shown until the new track's first step
    roft_object_output last_out{};
    bool last_out_valid = false;
};

// Camera images on the engine (roft_engine_enable_flow): what a submit call enqueues on the upload stream, frame by frame, behind
// the copies of its HOST inputs.  Built by submit_frames on the host only (PendingBatch::flow_jobs); enqueued when the whole batch has
// been accepted, so a refused submit leaves the pyramids on the device as they were (the per-object side, Sched::pyr_prev, rolls back
// with Sched).
struct FlowImageJob { const void* dev; int type; };            // a distinct image of a frame; its index is its pyramid slot
struct FlowPairJob { int pyr0, pyr1; unsigned char* out; };    // slots in the generations of frame - 1 and frame; the product's place
struct FlowCloneJob { void* dst; const void* src; };           // a flow that outlived the retention window (OwnedFlow), copied behind the batch's production
struct FlowFrameJobs {
    std::vector<FlowImageJob> images;
    std::vector<FlowPairJob> pairs;
    std::vector<FlowCloneJob> clones;
};
struct EngineFlow {
    bool enabled = false;
    roft_of_params prm{};
    OfGeom geom{};
    // One pyramid per distinct image of a frame, kept until the next frame's pairs have used it: a ring of max_batch_frames + 1
    // generations indexed by frame, so that the pyramids of ALL frames of a batch are built in one go while the last one of the
    // batch before is still there (a later batch overwrites a generation behind its readers in stream order); a generation
    // grows to the largest number of distinct images a frame ever brought.
    std::vector<std::vector<DevBuf<float>>> pyr;
    DevBuf<float> coarse, field;        // workspace of ONE chunk of kOfChunk pairs, reused chunk after chunk in stream order
    // the forward-backward check (roft_engine_enable_flow_consistency): a chunk is then kOfCheckChunk pairs, whose backward problems
    // take the upper half of `coarse` and the level-0 fields of `back`
    bool check = false;
    roft_of_consistency tol{};
    DevBuf<float> back;                 // [kOfCheckChunk][H * W * 2]
    roft_engine_flow_stats stats{};
};

// Raw sensor depth on the engine (roft_engine_enable_raw_depth): inputs[].depth carries the sensor's 16-bit frame; the float depth
// the kernels read is made on the upload stream behind the copies, where a staged HOST depth of the frame would have been copied
// (stage_alloc in the frame's staging slot: it lives exactly as long as one).  Built by submit_frames on the host only
// (PendingBatch::depth_jobs) and enqueued when the whole batch has been accepted, like the flow production: a refused submit leaves
// the device untouched.
struct DepthJob { int t; const uint16_t* raw; float* out; };   // a distinct raw image of frame t of the batch and its product's place
struct EngineDepth {
    bool enabled = false;
    roft_depth_source src{};
    size_t raw_pixels = 0;            // readings per raw image (the depth source's size)
    DepthAlignGeom geom{};            // src.align != 0
    roft_engine_depth_stats stats{};
    Event ev0, ev1;   // around the depth kernels of the last submit (roft_debug_depth_kernel_ms)
    bool timed = false;
};

// Lens distortion on the engine (roft_engine_enable_rectification, include/roft_engine.h section 3g): every frame image the caller
// hands over is the sensor's distorted one; its rectified product is made on the upload stream behind the copies and in front of the
// depth and the flow production, where a staged HOST image of the frame would have been copied (stage_alloc: it lives exactly as
// long as one).  Planned by submit_frames on the host only (PendingBatch::rect_jobs) and enqueued when the whole batch has been
// accepted: a refused submit leaves the device untouched.
struct RectJob { int t; const void* src; int kind; void* out; };   // a distinct (image, kind) of frame t of the batch and its product's place
struct EngineRectify {
    bool enabled = false;
    roft_lens lens{};
    RectGeom geom{};
    roft_engine_rectify_stats stats{};
    Event ev0, ev1;   // around the rectification launches of the last submit (roft_debug_rectify_kernel_ms)
    bool timed = false;
};

// Masks from poses on the engine (roft_engine_enable_pose_masks): enrolled objects take the silhouette of a delivered pose as the
// frame's mask where no mask and no label image arrives.  One launch per delivering batch, part of its preparation (engine_step.hip).
// The launch's events live here, one pair per slot of the batch ring; where the plan ends the preparation with the launch's stop
// event (ev_prep of the batch slot, which takes no time stamps) the launch is not timed.
struct EnginePoseMasks {
    bool enabled = false;
    bool all = false;                    // n_ids == 0: every object the engine has at its first frame (and a mesh)
    roft_engine_pose_mask_stats stats{};
    Event ev_start[8], ev_stop[8];
    int last_slot = -1;                  // batch-ring slot of the last launch
    bool last_timed = false;             // ... and whether it ended with ev_stop of that slot
    // objects of one scene hide each other (roft_engine_enable_pose_mask_occlusion).  Allocated when the mode is enabled: z-buffers
    // [batch parity][kMaxBatch delivering frames][n_zscenes][H * W] (the parity of the ingest slots: the preparation of batch b + 1
    // may run next to the chains of batch b), the pair records [batch parity][kMaxBatch][max_objects], the two device counters
    bool occlusion = false;
    int n_zscenes = 0;                   // scenes with at least two members
    roft_engine_pose_mask_occlusion_stats occl_stats{};   // (resolved: counted by submit; the rest is read from zstats)
    DevBuf<unsigned long long> zbuf, zstats;
    DevBuf<SilhouettePair> zpairs;
    // silhouettes gated against the depth of the pose's own frame (roft_engine_enable_pose_mask_depth_gate).  Allocated when the mode
    // is enabled: the pair records (zpairs, shared with the occlusion mode: a pair is drawn alone or resolved) and three counters
    bool gate = false;
    roft_pose_mask_gate gate_prm{};
    roft_engine_pose_mask_gate_stats gate_stats{};   // (gated: counted by submit; the rest is read from gstats)
    DevBuf<unsigned long long> gstats;
};

// Track quality on the engine (roft_engine_enable_quality): one record per (frame, object) in a ring of the log's capacity, written by
// one launch per batch behind both pose lanes (engine_step.hip).  The launch's events live here, one pair per slot of the batch
// ring, created when quality is enabled (with timing: roft_debug_quality_kernel_ms reads the pair of the last launch).
struct EngineQuality {
    bool enabled = false;
    roft_quality_params prm{};
    DevBuf<QualityRaw> ring;             // [cap][objects]
    int cap = 0;
    Event ev_start[8], ev_done[8];   // per batch-ring slot: bound to the launch's dispatch; ev_done is what the host waits for
    int last_slot = -1;                  // batch-ring slot of the last launch
};

// Pose hypotheses (roft_pose_hypotheses_score, roft_engine_score_hypotheses): what a call owns on the device -- one chunk of poses, its
// records, the plane's bit count.  Grows to the largest chunk it has held (at most kHypothesesChunk poses), never shrinks.
struct HypothesesScratch {
    DevBuf<double> poses;          // [chunk][7]
    DevBuf<QualityRaw> records;    // [chunk]
    DevBuf<int> n_mask;            // one word
};

// Device copies of HOST inputs: a ring of `retain` frame slots, each a bump allocator over chunks of device memory that
// are allocated when a frame first needs them and kept (a slot grows to the largest frame it ever held: 64 objects with
// their own 640x480 depth + CV_32FC2 flow + mask streams need 239 MB per slot, a shared scene 7 MB + the masks); identical
// host pointers within a frame (a scene shared by several objects) share one upload.
struct StageFrame {
    std::vector<DevBuf<unsigned char>> chunks;
    size_t cur = 0, used = 0;   // bump pointer: chunk index, bytes used of it
    std::vector<std::pair<const void*, void*>> seen;
};
constexpr size_t kStageChunk = (size_t)32 << 20;

// Room behind the control blocks of a batch (staging block and device copy) for its label table: at most one set and one member
// per object and frame, the member array 16-byte aligned behind the sets.
inline size_t label_table_cap(size_t objs_x_frames) { return (sizeof(LabelSet) + sizeof(LabelMember)) * objs_x_frames + 16; }
inline size_t ctrl_block_count(size_t objs_x_frames) { return objs_x_frames + (label_table_cap(objs_x_frames) + sizeof(FrameCtrl) - 1) / sizeof(FrameCtrl); }


}  // namespace host
}  // namespace roft

using namespace roft;
using namespace roft::host;

// The HIP streams of the engines of this process.  The runtime maps streams onto a few hardware queues in the order in
// which they are created; streams created after others were destroyed can end up sharing queues, and the chains of such
// an engine then run one after the other (measured: the second engine of a process tracked at a third of the rate of
// the first).  So a set of streams is created once per device and priority mode, handed to one engine at a time and
// never destroyed.
struct StreamSet {
    hipStream_t mask = nullptr, vel = nullptr, pose[kNumLin] = {nullptr, nullptr}, up = nullptr;
    int device = 0;
    bool priorities = true;
    bool in_use = false;   // handed to an engine
    bool parked = false;   // its busy streams share a hardware queue: kept alive (it shifts the runtime's round robin), handed out only
                           // when the device's cap of sets is reached
    int conflicts = 0;     // pairs of busy streams on one hardware queue when the set was created (-1: not probed)
};

struct GatherItem { const void* src; void* dst; size_t bytes; };   // one small pinned HOST image -> its staging copy
constexpr int kGatherCap = 8192;                                    // items per batch (8 frames x 1024 objects)
constexpr size_t kGatherMaxBytes = (size_t)2 << 20;                 // larger images go through the copy engine

// The submitted, not yet stepped batch: everything a submit call leaves behind for roft_step, and what it collects on its way.
// reset() is the ONE place where a new submit call starts from nothing; the vectors keep their capacity (a frame's flow job lists
// are built anew, as they always were).
struct PendingBatch {
    SubmitFacts facts;                 // what plan_batch reads (batch_plan.h)
    unsigned feat_frames = 0;          // bit t: some object buffers outlier-rejection features in frame t of the batch
    unsigned new_mask_frames = 0;      // bit t: some object receives a mask in frame t of the batch, of either form (facts.plain_mask_frames: byte masks)
    // masks from a label image (roft_frames_submit_labels): the batch's objects grouped by (frame, device image); written behind the
    // control blocks of the staging block by the submit, copied to the device with them (label_table_bytes, a multiple of 16)
    std::vector<LabelSet> label_sets;  // (facts.label_sets counts them)
    std::vector<std::vector<LabelMember>> label_members;   // per set
    size_t label_table_bytes = 0;
    // masks from poses: bit t: some enrolled object's mask of frame t is the silhouette of its pose (facts.pose_masks counts the pairs)
    unsigned pose_mask_frames = 0;
    int gated_pairs = 0;               // ... and the pairs among them that are compared with a depth image (the depth gate)
    std::vector<FlowFrameJobs> flow_jobs;   // [T] camera images: what enqueue_flow_production enqueues, frame by frame
    std::vector<DepthJob> depth_jobs;       // raw depth: what enqueue_depth_production enqueues
    std::vector<RectJob> rect_jobs;         // lens distortion: what enqueue_rectification enqueues, in front of the two above
    // Small HOST images in PINNED memory (the per-object masks of a delivery: 64 buffers of 300 KB) are not copied one
    // hipMemcpyAsync each but fetched by ONE kernel over the bus (engine_submit.hip, gather_copy_kernel): what to fetch
    std::vector<GatherItem> gather;         // collected by stage_host, launched by flush_gather
    double submit_t0 = 0.0, submit_us = 0.0, wait_us = 0.0;   // host times of the submit call (roft_batch_trace); like `throttled`, written by every call
    bool throttled = false;   // MEASURED, diagnostics only (roft_batch_trace): the submit had to wait for the in-flight bound
    std::vector<int> lane_tests;            // [objects][kNumLin] outlier tests of the object on the lane so far in the batch (-1: no frame on it yet)
    void reset(int n_obj, int T)
    {
        facts = SubmitFacts{};
        facts.T = T;
        feat_frames = new_mask_frames = pose_mask_frames = 0;
        gated_pairs = 0;
        label_sets.clear();
        label_members.clear();
        label_table_bytes = 0;
        flow_jobs.assign((size_t)T, FlowFrameJobs{});
        depth_jobs.clear();
        rect_jobs.clear();
        gather.clear();
        lane_tests.assign((size_t)n_obj * kNumLin, -1);
    }
};

// "A refused submit consumes nothing": what roft_frames_submit_images puts back when it fails.  The schedule mirrors of every object
// and the counters of the producers (flow, depth, rectification); NOT roft_engine_stats::h2d_bytes / h2d_copies, which count what crossed the bus -- a refused
// call's copies did.  (What else a submit writes is either the PendingBatch, which the next call resets, or staging memory of the
// batch's own frames, which the next call recycles.)
struct SubmitSnapshot {
    std::vector<Sched> sched;
    roft_engine_flow_stats flow{};
    roft_engine_depth_stats depth{};
    roft_engine_rectify_stats rectify{};
};

// What one batch in flight owns: a slot of the batch ring.
struct BatchSlot {
    Event ev_up;                   // uploads of the batch on the device, and the flows the submit produced from camera images behind them
    Event ev_host;                 // ... the copies alone, where production follows them: what the HOST waits for (its buffers are its own again)
    Event ev_ctrl;                 // FrameCtrl blocks of the batch on the device (and the mask chain of the batch before)
    Event ev_mask;                 // mask chain kernel of the batch complete
    Event ev_part;                 // the masks of the batch's frames 0 .. T - 2 complete (what its flow measurements read)
    Event ev_prep;                 // control blocks + ingested masks of the batch on the device (prepared on the upload stream)
    Event ev_feat;                 // features of the batch complete (a feature kernel on the mask stream)
    Event ev_vel;                  // the batch's velocity chain complete (velocity filter AND the feature kernel behind it)
    Event ev_skf;                  // twists of the batch complete (the velocity filter alone: what a pose lane waits for)
    Event ev_done[kNumLin];   // pose chain of the batch complete (per lane)
    hipError_t create_events()   // (they order streams: none takes time stamps)
    {
        for (Event* ev : {&ev_up, &ev_host, &ev_ctrl, &ev_mask, &ev_part, &ev_prep, &ev_feat, &ev_vel, &ev_skf, &ev_done[0], &ev_done[1]})
            if (const hipError_t err = ev->create(hipEventDisableTiming)) return err;
        return hipSuccess;
    }
    DevBuf<FrameCtrl> dctrl;             // control blocks on the device
    PinnedBuf<FrameCtrl> stage;          // ... and their pinned staging block
    PinnedBuf<GatherItem> gather_tab;    // pinned table gather_copy_kernel reads (kGatherCap entries; allocated on first use)
    // written by step_batch for wait_batch: which of the events the batch signals
    bool done_used[kNumLin] = {false, false};   // the lane had work
    bool vel_used = false;               // the velocity chain ended with ev_vel
    bool feat_used = false;              // a feature kernel ran on the mask stream and ended with ev_feat
    bool quality_used = false;           // the batch launched the quality kernel: it ends with EngineQuality::ev_done of this slot
    int end_frame = 0;                   // frame counter behind the batch
};

struct roft_engine {
    roft_config cfg{};
    Arrays arr;
    // Three in-order chains per batch, one HIP stream each (ROFT_ONE_STREAM=1 puts them on one stream):
    hipStream_t stream = nullptr;       // mask chain: FrameCtrl upload, mask chain kernel, features
    hipStream_t vel_stream = nullptr;   // velocity chain: flow measurement, velocity filter
    hipStream_t pose_stream[kNumLin] = {nullptr, nullptr};  // pose chain, one stream per lane (BeliefSlot): UKF segments, outlier rejection
    hipStream_t up_stream = nullptr;    // uploads of HOST inputs and the copies of aged-out flows
    struct StreamSet* streams = nullptr;   // the pooled set the four above come from
    // Batches in flight.  The image chains of batch b+1 do not depend on the pose chain of batch b, so they run ahead
    // of it.  The lead is bounded on the host: the submit call of batch b returns only when batch b - lead has ended
    // (its pose chain, which implies its other chains).  Rings are sized for it:
    //   batch ring (device FrameCtrl blocks, staging, events) kBatchRing > lead;
    //   plane ring kPlaneSlots > lead * T + T + 1;  twist ring kTwistRing > lead * T + pose_frames_between + 2;
    //   feature ring kFeatRing >= T + 2 (re-use is ordered by feat_use);
    //   caller buffers / HOST staging: retain = hist_cap + lead * T + 2 frames.
    //   The depth gate of masks from poses reads FlowEntry::depth_before, ONE frame older than the oldest flow a frame may name
    //   (age hist_cap instead of hist_cap - 1; older entries are clones).  The margin covers it: a frame in flight is at most
    //   (lead - 1) * T behind the counter C of the submit that recycles slots, so the oldest image named is C - (lead - 1) * T -
    //   hist_cap, and the newest slot recycled is C - retain + T - 1 = C - hist_cap - (lead - 1) * T - 3.  retain stays as it is.
    static constexpr int kBatchRing = 8;
    int T_max = 1;        // cfg.max_batch_frames
    int lead = 6;         // batches
    int hist_cap = 6;     // flows kept per object
    int retain = ROFT_RETAIN_FRAMES;
    BatchSlot ring[kBatchRing];                        // batch b lives in ring[b % kBatchRing]
    BatchSlot& slot_of(int b) { return ring[b % kBatchRing]; }
    SchedKnobs knobs;                                  // the switches, read when the engine is created
    bool multi() const { return !knobs.one_stream; }
    // ROFT_HOST_PROF=1: host time of the sections of the submit call / roft_step, printed by roft_engine_destroy
    double hp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long hp_batches = 0;
    std::vector<std::unique_ptr<HostObject>> objs;
    SubmitSnapshot snapshot;               // taken when a submit call starts
    std::vector<ObjParams> h_params;
    std::vector<StageFrame> staging;       // [retain]
    PinnedBuf<ObjState> state_host;   // pinned landing block of roft_get_state (velocity belief + corrected pose belief)
    PinnedBuf<int> dev_error;         // pinned word a kernel raises when it gives up (EngineArrays::dev_error)
    bool submitted = false;
    PendingBatch pending;                  // the submitted (or being submitted), not yet stepped batch
    EngineFlow flow;                       // camera images -> flows (roft_engine_enable_flow)
    EngineDepth depth;                     // raw sensor depth -> float depth (roft_engine_enable_raw_depth); its products ride on SubmitFacts::produced_flows
    EngineRectify rectify;                 // distorted frames -> the pinhole camera (roft_engine_enable_rectification); rides on produced_flows like the depth products
    EngineQuality quality;                 // track quality (roft_engine_enable_quality)
    HypothesesScratch hypotheses;          // roft_engine_score_hypotheses: the call's own buffers
    EnginePoseMasks pose_masks;            // masks from poses (roft_engine_enable_pose_masks)
    int prev_T = 0;                 // frames of the batch stepped before
    int batch_counter = 0, frame_counter = 0;
    int completed_batches = 0, completed_frames = 0;
    roft_engine_stats stats{};
    roft_engine_restart_stats restart_stats{};   // roft_objects_restart
    bool device_pointers_checked = false;   // ROFT_MEM_DEVICE inputs are looked up once, on the first submit
    // A batch is "steady" when at least `lead` batches have been stepped since the engine was last idle (creation, roft_sync and
    // everything that calls it), a burst otherwise: plan_batch.
    int idle_mark = 0;        // batch_counter when the engine was last known idle
    bool alone_on_device = true;   // no other engine of this process holds a stream set on the device (asked by a plan that would release a lane early: a count, not a timing)
    bool wait_value_ok = true;     // hipDeviceAttributeCanUseStreamWaitValue
    // trace of the last kTraceRing batches (roft_engine_get_batch_trace)
    static constexpr int kTraceRing = 64;
    roft_batch_trace trace[kTraceRing] = {};
    unsigned long long skf_total = 0;      // velocity-filter workgroups launched so far (the value the lanes' gates wait for)
    // timing
    bool timing = false;
    int timing_level = 2;   // 1: only flow_measure_kernel (two events per batch), 2: every launch group
    std::vector<Event> tev;
    std::vector<std::string> tnames_s;
    std::vector<const char*> tnames;
    std::vector<float> tms;
    std::vector<int> tlaunches;
    std::vector<int> tmark;    // kernel id per event interval (-1 = chain start)
    std::vector<int> tstream;  // stream of each mark (0 mask chain, 1 / 3 pose lanes, 2 velocity chain, 4 upload / preparation)
    // the flow measurement's launches on the device's own clock (timing runs): per launch and workgroup the 100 MHz wall clock at
    // its start and end, kSpanLaunches launches between two roft_engine_get_timing() calls (later ones are not stamped)
    static constexpr int kSpanLaunches = 64;
    DevBuf<unsigned long long> k1_span;
    std::vector<int> span_wgs;   // workgroups of each stamped launch
    PoseErrorScratch score;      // roft_engine_score_log
};

namespace roft {
namespace host {

inline double host_now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#define HP_MARK(e, slot, t) do { if ((e)->knobs.host_prof) { const double _n = host_now_us(); (e)->hp_acc[slot] += _n - (t); (t) = _n; } } while (0)


}  // namespace host
}  // namespace roft

// ---- functions that cross a file boundary ---------------------------------------------------------------------------
// engine.hip
const std::string& last_error();   // the calling thread's error string
int check_dev_error(roft_engine* e);   // a kernel gave up (EngineArrays::dev_error): sticky
int wait_batch(roft_engine* e, int b, bool* waited = nullptr);   // blocks until batch b (and every earlier one) has ended on the GPU
bool alone_on_device(const StreamSet* mine);
__global__ void probe_blocker_kernel(long long ticks);
__global__ void probe_tiny_kernel(int* p);
__global__ void probe_sectors_kernel(const unsigned* buf, unsigned sector_mask, unsigned salt, unsigned* sink);
// engine_submit.hip
bool build_pose_program(const roft_config& cfg, Sched& o, const roft_frame_input& in, FrameCtrl& c);
// engine_step.hip
int step_batch(roft_engine* e);
// engine_quality.hip
unsigned quality_frames_of_batch(const roft_engine* e, int* n_out);   // four bits per frame of the submitted batch that gets a record
