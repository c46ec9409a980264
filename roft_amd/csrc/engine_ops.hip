// engine_ops.hip -- the operator-level entry points of include/roft_engine.h (section 1): each runs the engine's own kernels on the
// one-object context of op_context.h.  An entry point checks its arguments, enters the context once, derives its arrays by value and
// leaves nothing behind.
#include "op_context.h"

OpContext& roft::host::op_context()
{
    static OpContext c;
    return c;
}

namespace {

// ROFT_POSE_ERRORS_FMA=0: the nearest-neighbour search squares and adds in the oracle's operation order (9 fp64 operations per
// pair instead of 7); read once per process
bool pose_errors_fma()
{
    static const bool fma = [] { const char* v = getenv("ROFT_POSE_ERRORS_FMA"); return !(v && v[0] == '0'); }();
    return fma;
}

}  // namespace

int roft::host::pose_errors_run(PoseErrorScratch& sc, int kind, const double* d_pts, int P, const double* est_host, PoseView est_dev,
                                const double* ref_host, int n, double* out_host, hipStream_t s)
{
    const int P_pad = pose_error_padded_points(P), waves = pose_error_waves(P);
    // poses per launch: the estimated clouds of a launch fit 256 MiB of scratch, and the grid's y extent
    constexpr size_t kCloudBytes = (size_t)256 << 20;
    const int per_launch = kind == ROFT_POSE_ERROR_ADDS
                               ? (int)std::min<size_t>(32768, std::max<size_t>(1, kCloudBytes / ((size_t)P_pad * 3 * sizeof(double))))
                               : 32768;
    const int chunk = std::min(n, per_launch);
    if (est_host) {
        HIP_TRY(sc.est.ensure((size_t)7 * n));
        HIP_TRY(hipMemcpyAsync(sc.est.p, est_host, sizeof(double) * 7 * n, hipMemcpyHostToDevice, s));
        est_dev = PoseView{sc.est.p, 7, 0, 0};
    }
    HIP_TRY(sc.ref.ensure((size_t)7 * n));
    HIP_TRY(hipMemcpyAsync(sc.ref.p, ref_host, sizeof(double) * 7 * n, hipMemcpyHostToDevice, s));
    if (kind == ROFT_POSE_ERROR_ADDS) HIP_TRY(sc.cloud.ensure((size_t)chunk * P_pad * 3));
    HIP_TRY(sc.partial.ensure((size_t)chunk * waves));
    HIP_TRY(sc.out.ensure((size_t)n));
    if (!sc.ev0) { HIP_TRY(sc.ev0.create()); HIP_TRY(sc.ev1.create()); }
    const PoseView ref_dev{sc.ref.p, 7, 0, 0};
    HIP_TRY(hipEventRecord(sc.ev0, s));
    for (int f0 = 0; f0 < n; f0 += chunk)   // (in order on one stream: a launch re-uses the scratch of the one before)
        launch_pose_errors(kind, d_pts, P, est_dev, ref_dev, f0, std::min(chunk, n - f0), sc.cloud.p, sc.partial.p, sc.out.p,
                           pose_errors_fma(), s);
    HIP_TRY(hipEventRecord(sc.ev1, s));
    sc.timed = true;
    HIP_TRY(hipMemcpyAsync(out_host, sc.out.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    return ROFT_OK;
}

int roft::host::check_pose_errors_sym(int kind, const double* sym, int n_sym, const roft_camera* cam)
{
    if (kind != ROFT_POSE_ERROR_MSSD && kind != ROFT_POSE_ERROR_MSPD) return fail(ROFT_ERR_INVALID, "unknown symmetry-aware pose error kind");
    if (const char* why = roft::sym::check(sym, n_sym, ROFT_MAX_SCORE_SYMMETRIES)) return fail(ROFT_ERR_INVALID, why);
    if (kind == ROFT_POSE_ERROR_MSPD) {
        if (!cam) return fail(ROFT_ERR_INVALID, "MSPD needs a camera");
        if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || !std::isfinite(cam->cx) || !std::isfinite(cam->cy))
            return fail(ROFT_ERR_INVALID, "MSPD: the camera's intrinsics are not finite");
    }
    return ROFT_OK;
}

int roft::host::pose_errors_sym_run(PoseErrorScratch& sc, int kind, const double* d_pts, int P, const double* est_host, PoseView est_dev,
                                    const double* ref_host, int n, const double* sym_host, int n_sym, const roft_camera* cam,
                                    double* out_host, hipStream_t s)
{
    if (est_host) {
        HIP_TRY(sc.est.ensure((size_t)7 * n));
        HIP_TRY(hipMemcpyAsync(sc.est.p, est_host, sizeof(double) * 7 * n, hipMemcpyHostToDevice, s));
        est_dev = PoseView{sc.est.p, 7, 0, 0};
    }
    HIP_TRY(sc.ref.ensure((size_t)7 * n));
    HIP_TRY(hipMemcpyAsync(sc.ref.p, ref_host, sizeof(double) * 7 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(sc.sym.ensure((size_t)roft::sym::kElement * n_sym));
    HIP_TRY(hipMemcpyAsync(sc.sym.p, sym_host, sizeof(double) * roft::sym::kElement * n_sym, hipMemcpyHostToDevice, s));
    HIP_TRY(sc.out.ensure((size_t)n));
    if (!sc.ev0) { HIP_TRY(sc.ev0.create()); HIP_TRY(sc.ev1.create()); }
    const PoseView ref_dev{sc.ref.p, 7, 0, 0};
    const SymCamera dc = cam ? SymCamera{cam->fx, cam->fy, cam->cx, cam->cy} : SymCamera{0.0, 0.0, 0.0, 0.0};
    constexpr int kPerLaunch = 1 << 20;   // (one workgroup per pair: well inside the grid's x extent)
    HIP_TRY(hipEventRecord(sc.ev0, s));
    for (int f0 = 0; f0 < n; f0 += kPerLaunch)
        launch_pose_errors_sym(kind, d_pts, P, est_dev, ref_dev, f0, std::min(kPerLaunch, n - f0), sc.sym.p, n_sym, dc, sc.out.p, s);
    HIP_TRY(hipEventRecord(sc.ev1, s));
    sc.timed = true;
    HIP_TRY(hipMemcpyAsync(out_host, sc.out.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    return ROFT_OK;
}

namespace {

// The velocity filter's operators on plain arrays: x, P and the operator's diagonal go up as one block, `launch(c, in, out)` uploads
// what else it needs and launches, x, P and the status come back.
struct KfBlock { double x[6], P[36], diag[6]; int status; };

template <class Launch>
int op_kf(const double x[6], const double P[36], const double* diag, int n_diag, double x_out[6], double P_out[36], int* status_out, Launch&& launch)
{
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    KfBlock h{}, *in, *out;
    std::memcpy(h.x, x, sizeof(h.x));
    std::memcpy(h.P, P, sizeof(h.P));
    std::memcpy(h.diag, diag, sizeof(double) * n_diag);
    TRY(c.upload(0, &h, 1, &in));
    TRY(c.room(1, 1, &out));
    TRY(launch(c, in, out));
    HIP_TRY(hipMemcpyAsync(&h, out, sizeof(h), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));   // (also keeps what `launch` uploaded alive until it has been read)
    HIP_TRY(hipGetLastError());
    std::memcpy(x_out, h.x, sizeof(h.x));
    std::memcpy(P_out, h.P, sizeof(h.P));
    if (status_out) *status_out = h.status;
    return ROFT_OK;
}

}  // namespace

extern "C" {

int roft_flow_measurement(const roft_camera* cam, const uint8_t* prev_mask, const float* prev_depth,
                          const roft_flow* flow, double dt, float radius, double depth_max, int capacity,
                          int32_t* uv, double* y, double* H, int* n_out)
{
    if (!cam || !prev_mask || !prev_depth || !flow || !flow->data || !n_out) return fail(ROFT_ERR_INVALID, "null argument");
    const int r = (int)(size_t)radius;
    if (r <= 0) return fail(ROFT_ERR_INVALID, "radius must be >= 1");
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    EngineArrays a;
    TRY(c.one_object(*cam, flow, r, 0, &a));
    const size_t npix = (size_t)cam->width * cam->height;
    uint8_t* d_mask;
    float* d_depth;
    unsigned char* d_flow;
    TRY(c.upload(0, prev_mask, npix, &d_mask));
    TRY(c.upload(1, prev_depth, npix, &d_depth));
    TRY(c.upload(2, static_cast<const unsigned char*>(flow->data), flow_bytes(a.ffmt), &d_flow));
    FrameCtrl fc;
    clear_ctrl(fc);
    fc.dt = dt;
    fc.has_new_mask = 1;
    fc.new_mask = d_mask;
    fc.slot_prev = kSlotNew;  // the ingested planes are "the previous frame's mask"
    fc.slot_cur = 0;
    fc.depth_prev = d_depth;
    fc.flow[0] = d_flow;
    fc.vel_stage = 1;
    init_state(c.st);
    TRY(c.begin_object(a, nullptr, fc));
    launch_mask_ingest(a, 0, c.stream);
    launch_flow_measure(a, depth_max, r, c.stream);
    int n = 0;
    HIP_TRY(hipMemcpyAsync(&n, a.npts, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipGetLastError());
    *n_out = n;
    if (n > capacity) return fail(ROFT_ERR_CAPACITY, "more flow points than the caller's capacity");
    if (n > 0 && uv && y && H) {
        int32_t* d_uv;
        double *d_y, *d_H;
        TRY(c.room(3, (size_t)2 * n, &d_uv));
        TRY(c.room(4, (size_t)2 * n, &d_y));
        TRY(c.room(5, (size_t)12 * n, &d_H));
        launch_expand_yh(a.recs, a.npts, a.cam, dt, d_uv, d_y, d_H, n, c.stream);
        HIP_TRY(hipMemcpyAsync(uv, d_uv, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(y, d_y, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipMemcpyAsync(H, d_H, sizeof(double) * 12 * n, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    return ROFT_OK;
}

int roft_kf_predict(const double x[6], const double P[36], const double Qdiag[6], double x_out[6], double P_out[36])
{
    if (!x || !P || !Qdiag || !x_out || !P_out) return fail(ROFT_ERR_INVALID, "null argument");
    return op_kf(x, P, Qdiag, 6, x_out, P_out, nullptr, [&](OpContext& c, KfBlock* in, KfBlock* out) -> int {
        launch_kf_predict(in->x, in->P, in->diag, out->x, out->P, c.stream);
        return ROFT_OK;
    });
}

int roft_skf_correct(const double x_pred[6], const double P_pred[36], int N, const double* y, const double* H,
                     const double Rdiag[2], int reweight, double x_out[6], double P_out[36], int* status_out)
{
    if (!x_pred || !P_pred || !Rdiag || !x_out || !P_out || (N > 0 && (!y || !H))) return fail(ROFT_ERR_INVALID, "null argument");
    const size_t n = (size_t)std::max(N, 0);
    return op_kf(x_pred, P_pred, Rdiag, 2, x_out, P_out, status_out, [&](OpContext& c, KfBlock* in, KfBlock* out) -> int {
        double *d_y, *d_H, *d_norms;
        TRY(c.upload(2, y, 2 * n, &d_y));
        TRY(c.upload(3, H, 12 * n, &d_H));
        TRY(c.room(4, 3 * std::max<size_t>(n, 1), &d_norms));
        launch_skf_arrays(in->x, in->P, N, d_y, d_H, in->diag, reweight, d_norms, out->x, out->P, &out->status, c.stream);
        return ROFT_OK;
    });
}

int roft_skf_correct_points(const roft_camera* cam, double dt, const double x_pred[6], const double P_pred[36], int N,
                            const int32_t* uv, const float* z, const float* flow_xy, const double Rdiag[2], int reweight,
                            double x_out[6], double P_out[36], int* status_out)
{
    if (!cam || !x_pred || !P_pred || !Rdiag || !x_out || !P_out || (N > 0 && (!uv || !z || !flow_xy)))
        return fail(ROFT_ERR_INVALID, "null argument");
    std::vector<FlowRec> recs((size_t)std::max(N, 0));
    for (size_t i = 0; i < recs.size(); ++i) recs[i] = FlowRec{uv[2 * i], uv[2 * i + 1], z[i], flow_xy[2 * i], flow_xy[2 * i + 1]};
    return op_kf(x_pred, P_pred, Rdiag, 2, x_out, P_out, status_out, [&](OpContext& c, KfBlock* in, KfBlock* out) -> int {
        FlowRec* d_recs;
        double* d_norms;
        TRY(c.upload(2, recs.data(), recs.size(), &d_recs));
        TRY(c.room(4, 3 * std::max<size_t>(recs.size(), 1), &d_norms));
        launch_skf_records(in->x, in->P, N, d_recs, make_cam(*cam), dt, in->diag, reweight, d_norms, out->x, out->P, &out->status, c.stream);
        return ROFT_OK;
    });
}

int roft_mask_propagate(uint8_t* mask, int W, int H, const roft_flow* flows, int n_flows, int frames_between)
{
    if (!mask || (n_flows > 0 && !flows)) return fail(ROFT_ERR_INVALID, "null argument");
    int start = 0;
    if (frames_between > 0) start = std::max(0, n_flows - frames_between);
    const int used = n_flows - start;
    if (used > kMaxFlowHist) return fail(ROFT_ERR_INVALID, "more than ROFT_MAX_FLOW_CHASE flow frames per propagation are not supported");
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    const roft_camera cam{W, H, 1.0, 1.0, 0.0, 0.0};
    const roft_flow* f0 = used > 0 ? &flows[start] : nullptr;
    EngineArrays a;
    TRY(c.one_object(cam, f0, 35, 0, &a));
    const size_t npix = (size_t)W * H;
    const size_t fb = flow_bytes(a.ffmt);
    uint8_t *d_mask, *d_out;
    unsigned char* d_flows;
    TRY(c.upload(0, mask, npix, &d_mask));
    TRY(c.room(1, fb * std::max(used, 1), &d_flows));
    FrameCtrl fc;
    clear_ctrl(fc);
    for (int j = 0; j < used; ++j) {
        const roft_flow& f = flows[start + j];
        if (f.type != f0->type || f.cols != f0->cols || f.rows != f0->rows || !f.data)
            return fail(ROFT_ERR_INVALID, "all flow frames must share one format");
        HIP_TRY(hipMemcpyAsync(d_flows + fb * j, f.data, fb, hipMemcpyHostToDevice, c.stream));
        fc.flow[used - 1 - j] = d_flows + fb * j;  // [0] = newest
    }
    fc.has_new_mask = 1;
    fc.new_mask = d_mask;
    fc.force_mode = 3;
    fc.n_hist = used;
    fc.slot_prev = 1;
    fc.slot_cur = 0;
    fc.flow_valid = 0;
    // decide_mode() uses fbuf_n + flow_valid as the number of buffered flows: state carried in = `used` buffered flows
    MaskRec rec0[2];
    std::memset(rec0, 0, sizeof(rec0));
    rec0[0].fbuf_n = used;
    HIP_TRY(hipMemcpyAsync(a.mrec, rec0, sizeof(rec0), hipMemcpyHostToDevice, c.stream));
    a.mrec_carry = a.mrec;   // row 0: rec0[0]
    // the chain kernel ORs into a zeroed destination (inside the engine the frame before leaves it zeroed)
    HIP_TRY(hipMemsetAsync(a.planes + plane_offset(a, 0, 0, 0), 0, sizeof(uint32_t) * 2 * a.plane_words, c.stream));
    init_state(c.st);
    TRY(c.begin_object(a, nullptr, fc));
    launch_mask_reset(a, c.stream);
    launch_mask_ingest(a, 0, c.stream);
    launch_mask_chain(a, frames_between, 1, 1u, c.stream);
    TRY(c.room(2, npix, &d_out));
    launch_planes_to_mask(a.planes + plane_offset(a, 0, 0, 0), a.planes + plane_offset(a, 0, 0, 1), (int)npix, d_out, c.stream);
    HIP_TRY(hipMemcpyAsync(mask, d_out, npix, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    HIP_TRY(hipGetLastError());
    return ROFT_OK;
}

int roft_labels_to_masks(const void* labels, int label_type, int W, int H, const int* values, int n, uint8_t* masks_out, int* counts_out)
{
    if (!labels || !values || n <= 0) return fail(ROFT_ERR_INVALID, "null argument, or no value");
    if (label_type != ROFT_LABEL_U8 && label_type != ROFT_LABEL_U16) return fail(ROFT_ERR_INVALID, "label_type must be ROFT_LABEL_U8 or ROFT_LABEL_U16");
    for (int i = 0; i < n; ++i)
        if (values[i] <= 0 || values[i] > (label_type == ROFT_LABEL_U8 ? 255 : 65535))
            return fail(ROFT_ERR_INVALID, "label " + std::to_string(values[i]) + ": 0 is the background, and the value must fit the label type");
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    TRY(check_geometry(W, H));
    const size_t npix = (size_t)W * H, plane_words = npix / 32;
    // the engine's kernel on a compact layout: object i = value i, one ingest slot, one set
    unsigned char *d_img, *d_masks;
    LabelSet* d_set;
    LabelMember* d_members;
    uint32_t* d_planes;
    MaskRec* d_rec;
    TRY(c.upload(0, static_cast<const unsigned char*>(labels), npix * (label_type == ROFT_LABEL_U8 ? 1 : 2), &d_img));
    LabelSet set{};
    set.img = d_img; set.type = label_type; set.t = 0; set.first = 0; set.n = n;
    std::vector<LabelMember> members((size_t)n);
    for (int i = 0; i < n; ++i) members[i] = LabelMember{i, values[i]};
    std::vector<MaskRec> rec((size_t)2 * n);
    TRY(c.upload(1, &set, 1, &d_set));
    TRY(c.upload(2, members.data(), members.size(), &d_members));
    TRY(c.room(3, (size_t)n * 2 * plane_words, &d_planes));
    TRY(c.room(4, rec.size(), &d_rec));
    HIP_TRY(hipMemsetAsync(d_rec, 0, sizeof(MaskRec) * rec.size(), c.stream));
    LabelIngestArgs la;
    la.sets = d_set;
    la.members = d_members;
    la.planes = d_planes;
    la.plane_words = plane_words;
    la.obj_stride = 2 * plane_words;
    la.slot0 = 0;
    la.mrec = d_rec;
    la.n_obj = n;
    la.n_grp = (int)(npix / 64);
    launch_label_ingest(la, 1, c.stream);
    HIP_TRY(hipGetLastError());
    if (masks_out) {
        TRY(c.room(5, npix * (size_t)n, &d_masks));
        for (int i = 0; i < n; ++i)
            launch_planes_to_mask(d_planes + (size_t)i * 2 * plane_words, d_planes + (size_t)i * 2 * plane_words + plane_words, (int)npix,
                                  d_masks + npix * (size_t)i, c.stream);
        HIP_TRY(hipMemcpyAsync(masks_out, d_masks, npix * (size_t)n, hipMemcpyDeviceToHost, c.stream));
    }
    HIP_TRY(hipMemcpyAsync(rec.data(), d_rec, sizeof(MaskRec) * rec.size(), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));   // (set, members and rec live in this call)
    HIP_TRY(hipGetLastError());
    if (counts_out)
        for (int i = 0; i < n; ++i) counts_out[i] = rec[(size_t)n + i].new_count;   // (row t + 1 = 1)
    return ROFT_OK;
}

// Masks from poses, stand-alone: the engine's silhouette kernels on a compact layout -- n objects of ONE scene, one ingest slot each,
// one frame.  With one object there is nothing to resolve: the one-pass launch, as in an engine without the occlusion mode.
// gate: every pair is compared with `depth` (one image: every object's gate frame) -- the pair drawn alone for n == 1, the resolve
// followed by the gate for n > 1.
static int pose_silhouettes(const char* what, const roft_camera* cam, const roft_mesh* meshes, int n, const double* x, const double* q, int bands,
                            int vertex_cache, uint8_t* masks_out, int* counts_out, bool gated = false, const float* depth = nullptr,
                            const roft_pose_mask_gate* gate = nullptr, int* removed_out = nullptr)
{
    if (!cam || !meshes || !x || !q || (gated && (!depth || !gate))) return fail(ROFT_ERR_INVALID, "null argument");
    if (gated && !pose_mask_gate_valid(gate->front_tolerance, gate->behind_tolerance))
        return fail(ROFT_ERR_INVALID, std::string(what) + ": front_tolerance must be finite and > 0, behind_tolerance finite (<= 0: that test is off)");
    if (n < 1 || n > ROFT_SCENE_MAX_INSTANCES) return fail(ROFT_ERR_INVALID, std::string(what) + ": n must be 1 .. ROFT_SCENE_MAX_INSTANCES");
    if (bands < 0) return fail(ROFT_ERR_INVALID, "bands must be >= 0 (0: the library's choice)");
    if (vertex_cache != 0 && vertex_cache != 1) return fail(ROFT_ERR_INVALID, "vertex_cache must be 0 or 1");
    for (int k = 0; k < n; ++k) TRY(check_mesh(meshes[k], n > 1 ? "mesh " + std::to_string(k) : "mesh", true));
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    TRY(check_geometry(cam->width, cam->height));
    const DevCamera dc = make_cam(*cam);
    const size_t npix = (size_t)cam->width * cam->height, plane_words = (size_t)dc.wpr * dc.H;
    if (c.meshes.size() < (size_t)n) c.meshes.resize((size_t)n);
    float* d_depth = nullptr;
    FrameCtrl* d_ctrl;
    ObjParams* d_prm;
    uint32_t* d_planes;
    MaskRec* d_rec;
    if (gated) TRY(c.upload(0, depth, npix, &d_depth));
    std::vector<ObjParams> prm((size_t)n);
    std::vector<FrameCtrl> fc((size_t)n);
    std::vector<MaskRec> rec((size_t)2 * n);
    std::memset(prm.data(), 0, sizeof(ObjParams) * prm.size());
    int max_verts = 0;
    for (int k = 0; k < n; ++k) {
        TRY(c.meshes[k].upload(meshes[k], MeshLayout::kWalkOrder, c.stream));
        c.meshes[k].describe(prm[k]);
        max_verts = std::max(max_verts, c.meshes[k].n_verts);
        clear_ctrl(fc[k]);
        fc[k].has_new_mask = 1;
        fc[k].label_type = kMaskFromPose;
        fc[k].label = n > 1 ? 1 : 0;   // (z-buffer 0 of the frame)
        fc[k].gate_depth = d_depth;
        for (int i = 0; i < 3; ++i) fc[k].pose_x[i] = x[3 * k + i];
        for (int i = 0; i < 4; ++i) fc[k].pose_q[i] = q[4 * k + i];
    }
    TRY(c.upload(1, fc.data(), fc.size(), &d_ctrl));
    TRY(c.upload(2, prm.data(), prm.size(), &d_prm));
    TRY(c.room(3, (size_t)n * 2 * plane_words, &d_planes));
    TRY(c.room(4, rec.size(), &d_rec));
    HIP_TRY(hipMemsetAsync(d_planes, 0xA5, sizeof(uint32_t) * (size_t)n * 2 * plane_words, c.stream));   // (stale words, as an engine's ingest slot holds)
    HIP_TRY(hipMemsetAsync(d_rec, 0, sizeof(MaskRec) * rec.size(), c.stream));
    SilhouetteArgs sa{};
    sa.ctrl = d_ctrl;
    sa.params = d_prm;
    sa.planes = d_planes;
    sa.plane_words = plane_words;
    sa.obj_stride = 2 * plane_words;
    sa.slot0 = 0;
    sa.mrec = d_rec;
    sa.n_obj = n;
    sa.W = dc.W; sa.H = dc.H; sa.wpr = dc.wpr;
    sa.fx = (float)dc.fx; sa.fy = (float)dc.fy; sa.cx = (float)dc.cx; sa.cy = (float)dc.cy;   // (divider 1: the camera as it is)
    sa.frames_packed = 0u;
    unsigned long long* d_zstats = nullptr;
    int* d_removed = nullptr;
    if (n > 1 || gated) {
        TRY(c.room(5, (size_t)n, &sa.zpairs));
        TRY(c.room(6, 2 + 3, &d_zstats));   // (the occlusion counters, then the gate's)
        HIP_TRY(hipMemsetAsync(sa.zpairs, 0, sizeof(SilhouettePair) * n, c.stream));
        HIP_TRY(hipMemsetAsync(d_zstats, 0, sizeof(unsigned long long) * 5, c.stream));
    }
    if (n > 1) {
        TRY(c.room(7, npix, &sa.zbuf));
        sa.n_zscenes = 1;
        sa.zstats = d_zstats;
    }
    if (gated) {
        TRY(c.room(8, (size_t)2 * n, &d_removed));
        HIP_TRY(hipMemsetAsync(d_removed, 0, sizeof(int) * 2 * n, c.stream));   // (an object without a mesh is drawn, and removes nothing)
        sa.gate = 1;
        sa.gate_tf = gate->front_tolerance;
        sa.gate_tb = gate->behind_tolerance;
        sa.gstats = d_zstats + 2;
        sa.gremoved = d_removed;
    }
    if (!launch_pose_silhouette(sa, 1, max_verts, bands, vertex_cache, c.stream))
        return fail(ROFT_ERR_INVALID, "pose silhouette: an image row is wider than the kernel's bit window");
    HIP_TRY(hipGetLastError());
    if (masks_out) {
        uint8_t* d_mask;
        TRY(c.room(9, npix * n, &d_mask));
        for (int k = 0; k < n; ++k) {
            const uint32_t* nz = d_planes + (size_t)k * 2 * plane_words;
            launch_planes_to_mask(nz, nz + plane_words, (int)npix, d_mask + (size_t)k * npix, c.stream);
        }
        HIP_TRY(hipMemcpyAsync(masks_out, d_mask, npix * n, hipMemcpyDeviceToHost, c.stream));
    }
    HIP_TRY(hipMemcpyAsync(rec.data(), d_rec, sizeof(MaskRec) * rec.size(), hipMemcpyDeviceToHost, c.stream));
    if (gated && removed_out) HIP_TRY(hipMemcpyAsync(removed_out, d_removed, sizeof(int) * 2 * n, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));   // (fc, prm and rec live in this call)
    HIP_TRY(hipGetLastError());
    if (counts_out)
        for (int k = 0; k < n; ++k) counts_out[k] = rec[(size_t)n + k].new_count;   // (row t + 1 = 1)
    return ROFT_OK;
}

int roft_pose_silhouette(const roft_camera* cam, const roft_mesh* mesh, const double x[3], const double q[4], int bands, int vertex_cache,
                         uint8_t* mask_out, int* count_out)
{
    return pose_silhouettes("roft_pose_silhouette", cam, mesh, 1, x, q, bands, vertex_cache, mask_out, count_out);
}

int roft_pose_silhouettes_occluded(const roft_camera* cam, const roft_mesh* meshes, int n, const double* x, const double* q, int bands,
                                   int vertex_cache, uint8_t* masks_out, int* counts_out)
{
    return pose_silhouettes("roft_pose_silhouettes_occluded", cam, meshes, n, x, q, bands, vertex_cache, masks_out, counts_out);
}

int roft_pose_silhouettes_gated(const roft_camera* cam, const roft_mesh* meshes, int n, const double* x, const double* q, const float* depth,
                                const roft_pose_mask_gate* g, int bands, int vertex_cache, uint8_t* masks_out, int* counts_out, int* removed_out)
{
    return pose_silhouettes("roft_pose_silhouettes_gated", cam, meshes, n, x, q, bands, vertex_cache, masks_out, counts_out, true, depth, g, removed_out);
}

int roft_pose_process_noise(const double psd[3], const double sig_w[3], double T, double Q[81])
{
    if (!psd || !sig_w || !Q) return fail(ROFT_ERR_INVALID, "null argument");
    // parameter packing only (CartesianQuaternionModel.cpp:127-141); the filter kernels build Q(T) themselves
    std::memset(Q, 0, sizeof(double) * 81);
    for (int i = 0; i < 3; ++i) {
        Q[i * 9 + i] = psd[i] * T;
        Q[(3 + i) * 9 + (3 + i)] = sig_w[i];
        Q[(6 + i) * 9 + (6 + i)] = psd[i] * (std::pow(T, 3.0) / 3.0);
        Q[i * 9 + (6 + i)] = psd[i] * (std::pow(T, 2.0) / 2.0);
        Q[(6 + i) * 9 + i] = psd[i] * (std::pow(T, 2.0) / 2.0);
    }
    return ROFT_OK;
}

static int op_ukf(const double mean[13], const double P[144], const double* Q81, double T, int type, const double* meas,
                  const double* Rdiag, const roft_ut_params* ut, double mean_out[13], double P_out[144], int* status)
{
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    EngineArrays a;
    TRY(c.one_object(&a));
    ObjState& st = c.st;
    init_state(st);
    std::memcpy(st.belief[B_CORR].mean, mean, sizeof(double) * 13);
    std::memcpy(st.belief[B_CORR].cov, P, sizeof(double) * 144);
    ObjParams prm;
    std::memset(&prm, 0, sizeof(prm));
    FrameCtrl fc;
    clear_ctrl(fc);
    fc.dt = T;
    fc.n_steps = 1;
    StepDesc& sd = fc.steps[0];
    sd.op = 1;
    sd.src = B_CORR;
    if (Q81) {
        double* d_q;
        TRY(c.upload(0, Q81, 81, &d_q));
        prm.q_override = d_q;
        sd.do_predict = 1;
        sd.n_corr = 0;
        sd.dst[0] = B_SPARE;
    } else {
        sd.do_predict = 0;
        sd.n_corr = 1;
        sd.type[0] = type;
        sd.dst[0] = B_SPARE;
        sd.twist_slot = 0;
        int k = 0;
        const bool has_vel = (type == ROFT_MEAS_VELOCITY || type == ROFT_MEAS_POSE_VELOCITY);
        const bool has_pose = (type == ROFT_MEAS_POSE || type == ROFT_MEAS_POSE_VELOCITY);
        if (has_vel) {
            for (int i = 0; i < 6; ++i) st.twist_hist[0][i] = meas[i];
            for (int i = 0; i < 3; ++i) prm.R_v[i] = Rdiag[k++];
            for (int i = 0; i < 3; ++i) prm.R_w[i] = Rdiag[k++];
        }
        if (has_pose) {
            const double* pm = meas + (has_vel ? 6 : 0);
            for (int i = 0; i < 3; ++i) fc.pose_x[i] = pm[i];
            for (int i = 0; i < 4; ++i) fc.pose_q[i] = pm[3 + i];
            for (int i = 0; i < 3; ++i) prm.R_x[i] = Rdiag[k++];
            for (int i = 0; i < 3; ++i) prm.R_q[i] = Rdiag[k++];
        }
    }
    TRY(c.begin_object(a, &prm, fc));
    launch_ukf_chain(a, *ut, true, 0, c.stream);
    TRY(c.read_state(a));
    std::memcpy(mean_out, st.belief[B_SPARE].mean, sizeof(double) * 13);
    std::memcpy(P_out, st.belief[B_SPARE].cov, sizeof(double) * 144);
    if (status) *status = st.lane[0].ukf_status & 0xF;
    return ROFT_OK;
}

int roft_ukf_predict(const double mean[13], const double P[144], const double Q[81], double T, const roft_ut_params* ut,
                     double mean_out[13], double P_out[144])
{
    if (!mean || !P || !Q || !ut || !mean_out || !P_out) return fail(ROFT_ERR_INVALID, "null argument");
    return op_ukf(mean, P, Q, T, 0, nullptr, nullptr, ut, mean_out, P_out, nullptr);
}

int roft_ukf_correct(const double mean[13], const double P[144], int type, const double* meas, const double* Rdiag,
                     const roft_ut_params* ut, double mean_out[13], double P_out[144], int* status_out)
{
    if (!mean || !P || !ut || !mean_out || !P_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (type != ROFT_MEAS_NONE && (!meas || !Rdiag)) return fail(ROFT_ERR_INVALID, "null measurement");
    if (type < ROFT_MEAS_NONE || type > ROFT_MEAS_POSE_VELOCITY) return fail(ROFT_ERR_INVALID, "bad measurement type");
    return op_ukf(mean, P, nullptr, 0.0, type, meas, Rdiag, ut, mean_out, P_out, status_out);
}

// The engine's outlier test on the one object: features of (depth, mask) buffered by features_kernel, both
// alternatives rendered and scored by outlier_fused_kernel, the decision taken by the pose chain segment that follows -- the
// three launches roft_step enqueues at a pose arrival.  depth / mask may be null (render only: no samples).
static int op_outlier(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                      const double* x2 /*2x3*/, const double* q2 /*2x4*/, const OutlierLaunchOpts& o_in, double L_out[2],
                      long samples_out[2], int* selected_out, float* tiles_out)
{
    TRY(check_mesh(*mesh, "mesh", false));
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    EngineArrays a;
    TRY(c.one_object(*cam, nullptr, 35, divider, &a));
    const size_t npix = (size_t)cam->width * cam->height, tpix = (size_t)a.tile_w * a.tile_h;
    // (GL render mode: the caller's triangles as they are, every one drawn -- roft_object_add does the same)
    TRY(c.mesh.upload(*mesh, o_in.render_mode == ROFT_RENDER_CONTRACT ? MeshLayout::kWalkClusters : MeshLayout::kAsItIs, c.stream));
    ObjParams prm;
    std::memset(&prm, 0, sizeof(prm));
    c.mesh.describe(prm);
    a.max_verts = mesh->n_verts;
    a.max_tris = mesh->n_tris;
    a.meshes_without_clusters = (prm.n_tris > 0 && prm.n_clusters <= 0) ? 1 : 0;
    FrameCtrl fc;
    clear_ctrl(fc);
    fc.n_steps = 1;        // (walked already: the segment below only decides)
    fc.outlier_step = 0;
    fc.cur_slot = B_LIN0;
    fc.lane = 0;
    fc.feat_read = 0;
    if (depth && mask) {
        uint8_t* d_mask;
        float* d_depth;
        TRY(c.upload(0, mask, npix, &d_mask));
        TRY(c.upload(1, depth, npix, &d_depth));
        fc.has_new_mask = 1;
        fc.new_mask = d_mask;
        fc.slot_cur = kSlotNew;
        fc.depth_cur = d_depth;
        fc.feat_write = 0;
    }
    ObjState& st = c.st;
    init_state(st);
    st.lane[0].pending_frame = 0;
    st.lane[0].pc_frame = 0;
    st.lane[0].pc_step = 1;
    for (int k = 0; k < 2; ++k) {
        PoseBelief& b = st.belief[b_alt(0, k)];
        for (int i = 0; i < 3; ++i) b.mean[6 + i] = x2[3 * k + i];
        for (int i = 0; i < 4; ++i) b.mean[9 + i] = q2[4 * k + i];
    }
    TRY(c.begin_object(a, &prm, fc));
    OutlierLaunchOpts o = o_in;
    if (tiles_out) {
        TRY(c.room(2, 2 * tpix, &o.tile_dump));
        HIP_TRY(hipMemsetAsync(o.tile_dump, 0, sizeof(float) * 2 * tpix, c.stream));
    }
    if (depth && mask) {
        launch_mask_ingest(a, 0, c.stream);
        launch_features(a, c.stream);
    }
    TRY(launch_outlier(a, 0, c.stream, nullptr, &o));
    roft_ut_params ut{1.0, 2.0, 0.0};
    launch_ukf_chain(a, ut, false, 0, c.stream);   // decision (ROFTFilter.cpp:581-583) as the engine's next segment takes it
    if (tiles_out) HIP_TRY(hipMemcpyAsync(tiles_out, o.tile_dump, sizeof(float) * 2 * tpix, hipMemcpyDeviceToHost, c.stream));
    TRY(c.read_state(a));
    for (int k = 0; k < 2; ++k) {
        if (L_out) L_out[k] = st.lane[0].outlier_L[k];
        if (samples_out) samples_out[k] = (long)st.lane[0].outlier_cnt[k];
    }
    if (selected_out) *selected_out = st.lane[0].outlier_selected;
    return ROFT_OK;
}

int roft_mesh_classify(const roft_mesh* mesh, uint8_t* flip_out, int* closed_out)
{
    if (!mesh || !mesh->verts || !mesh->tris || !has_mesh(*mesh) || !closed_out) return fail(ROFT_ERR_INVALID, "bad argument");
    std::vector<uint8_t> flip;
    *closed_out = classify_mesh(mesh->verts, mesh->n_verts, mesh->tris, mesh->n_tris, flip) ? 1 : 0;
    if (flip_out) std::memcpy(flip_out, flip.data(), (size_t)mesh->n_tris);
    return ROFT_OK;
}

int roft_render_depth(const roft_mesh* mesh, const double x[3], const double q[4], const roft_camera* cam, int divider,
                      float* tile)
{
    return roft_render_depth_mode(mesh, x, q, cam, divider, ROFT_RENDER_CONTRACT, tile);
}

int roft_render_depth_mode(const roft_mesh* mesh, const double x[3], const double q[4], const roft_camera* cam, int divider, int mode,
                           float* tile)
{
    if (!mesh || !x || !q || !cam || !tile || divider <= 0) return fail(ROFT_ERR_INVALID, "bad argument");
    if (mode != ROFT_RENDER_CONTRACT && mode != ROFT_RENDER_GL) return fail(ROFT_ERR_INVALID, "bad render mode");
    const size_t tpix = (size_t)(cam->width / divider) * (cam->height / divider);
    std::vector<float> tiles(2 * tpix);
    const double x2[6] = {x[0], x[1], x[2], x[0], x[1], x[2]};
    const double q2[8] = {q[0], q[1], q[2], q[3], q[0], q[1], q[2], q[3]};
    OutlierLaunchOpts o;
    o.render_mode = mode;
    if (int rc = op_outlier(cam, divider, nullptr, nullptr, mesh, x2, q2, o, nullptr, nullptr, nullptr, tiles.data())) return rc;
    std::memcpy(tile, tiles.data(), sizeof(float) * tpix);
    return ROFT_OK;
}

int roft_outlier_test(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                      const double x[6], const double q[8], int bands, int vertex_cache, int window_pixels, double L_out[2],
                      long samples_out[2], int* selected_out, float* tiles_out)
{
    return roft_outlier_test_split(cam, divider, depth, mask, mesh, x, q, bands, vertex_cache, window_pixels, -1, L_out, samples_out, selected_out, tiles_out);
}

int roft_outlier_test_split(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                            const double x[6], const double q[8], int bands, int vertex_cache, int window_pixels, int split, double L_out[2],
                            long samples_out[2], int* selected_out, float* tiles_out)
{
    return roft_outlier_test_mode(cam, divider, depth, mask, mesh, x, q, bands, vertex_cache, window_pixels, split, ROFT_RENDER_CONTRACT,
                                  L_out, samples_out, selected_out, tiles_out);
}

int roft_outlier_test_mode(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                           const double x[6], const double q[8], int bands, int vertex_cache, int window_pixels, int split, int mode,
                           double L_out[2], long samples_out[2], int* selected_out, float* tiles_out)
{
    if (!cam || !depth || !mask || !mesh || !x || !q || divider <= 0 || bands < 0 || bands > kMaxOutlierParts || window_pixels < 0)
        return fail(ROFT_ERR_INVALID, "bad argument");
    if (mode != ROFT_RENDER_CONTRACT && mode != ROFT_RENDER_GL) return fail(ROFT_ERR_INVALID, "bad render mode");
    OutlierLaunchOpts o;
    o.parts = bands;
    o.no_vertex_cache = vertex_cache ? 0 : 1;
    o.window_pixels = window_pixels;
    o.split = split < 0 ? -1 : (split ? 1 : 0);   // (this call only: nothing process-wide changes)
    o.render_mode = mode;
    return op_outlier(cam, divider, depth, mask, mesh, x, q, o, L_out, samples_out, selected_out, tiles_out);
}

int roft_depth_likelihood(const roft_camera* cam, const float* depth, const uint8_t* mask, const float* tile, int divider,
                          double* L_out, long* samples_out)
{
    if (!cam || !depth || !mask || !tile || !L_out || divider <= 0) return fail(ROFT_ERR_INVALID, "bad argument");
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    EngineArrays a;
    TRY(c.one_object(*cam, nullptr, 35, divider, &a));
    const size_t npix = (size_t)cam->width * cam->height, tpix = (size_t)a.tile_w * a.tile_h;
    uint8_t* d_mask;
    float* d_depth;
    TRY(c.upload(0, mask, npix, &d_mask));
    TRY(c.upload(1, depth, npix, &d_depth));
    // tile -> z-buffer bit pattern (0 = background -> +inf), used for both alternatives
    std::vector<uint32_t> zb(tpix * 2);
    for (size_t i = 0; i < tpix; ++i) {
        uint32_t bits;
        std::memcpy(&bits, &tile[i], 4);
        if (tile[i] == 0.0f) bits = 0x7F800000u;
        zb[i] = bits;
        zb[tpix + i] = bits;
    }
    HIP_TRY(hipMemcpyAsync(a.zbuf, zb.data(), zb.size() * 4, hipMemcpyHostToDevice, c.stream));
    FrameCtrl fc;
    clear_ctrl(fc);
    fc.has_new_mask = 1;
    fc.new_mask = d_mask;
    fc.slot_cur = kSlotNew;
    fc.depth_cur = d_depth;
    fc.feat_write = 0;
    fc.feat_read = 0;
    fc.outlier_step = 0;
    init_state(c.st);
    c.st.lane[0].pending_frame = 0;   // the test of frame 0 is pending
    TRY(c.begin_object(a, nullptr, fc));
    launch_mask_ingest(a, 0, c.stream);
    launch_features(a, c.stream);
    launch_outlier_only(a, c.stream);   // likelihood only (the z-buffers are already filled)
    TRY(c.read_state(a));
    *L_out = c.st.lane[0].outlier_L[0];
    if (samples_out) *samples_out = (long)c.st.lane[0].outlier_cnt[0];
    return ROFT_OK;
}

int roft_pose_errors(int kind, const double* points, int n_points, const double* est, const double* ref, int n_poses, double* out)
{
    if (kind != ROFT_POSE_ERROR_ADD && kind != ROFT_POSE_ERROR_ADDS) return fail(ROFT_ERR_INVALID, "unknown pose error kind");
    if (!points || !est || !ref || !out) return fail(ROFT_ERR_INVALID, "null argument");
    if (n_points <= 0 || n_poses < 0) return fail(ROFT_ERR_INVALID, "n_points must be > 0 and n_poses >= 0");
    if (n_poses == 0) return ROFT_OK;
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    PoseErrorScratch& sc = c.pose_errors;
    HIP_TRY(sc.pts.ensure((size_t)3 * n_points));
    HIP_TRY(hipMemcpyAsync(sc.pts.p, points, sizeof(double) * 3 * n_points, hipMemcpyHostToDevice, c.stream));
    return pose_errors_run(sc, kind, sc.pts.p, n_points, est, PoseView{}, ref, n_poses, out, c.stream);
}

int roft_pose_errors_sym(int kind, const double* points, int n_points, const double* est, const double* ref, int n_poses, const double* sym,
                         int n_sym, const roft_camera* cam, double* out)
{
    if (!points || !est || !ref || !out || !sym) return fail(ROFT_ERR_INVALID, "null argument");
    if (n_points <= 0 || n_poses < 0) return fail(ROFT_ERR_INVALID, "n_points must be > 0 and n_poses >= 0");
    TRY(check_pose_errors_sym(kind, sym, n_sym, cam));
    if (n_poses == 0) return ROFT_OK;
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    PoseErrorScratch& sc = c.pose_errors;
    HIP_TRY(sc.pts.ensure((size_t)3 * n_points));
    HIP_TRY(hipMemcpyAsync(sc.pts.p, points, sizeof(double) * 3 * n_points, hipMemcpyHostToDevice, c.stream));
    return pose_errors_sym_run(sc, kind, sc.pts.p, n_points, est, PoseView{}, ref, n_poses, sym, n_sym, cam, out, c.stream);
}

int roft_default_vsd_params(roft_vsd_params* p)
{
    if (!p) return fail(ROFT_ERR_INVALID, "null argument");
    std::memset(p, 0, sizeof(*p));
    p->delta = 0.015f;
    p->n_taus = 10;
    for (int k = 1; k <= 10; ++k) p->taus[k - 1] = (double)k / 20.0;   // (the double nearest to k * 0.05: one rounding)
    p->diameter = 0.0;
    p->window_pixels = 0;
    return ROFT_OK;
}

// VSD (section 3i).  The mesh goes up once, the poses once; the depth images go up in chunks of at most kVsdChunk pairs, so that
// the resident depth stays modest whatever n_poses is -- or once, when one image lies under every pair.  Every chunk's workgroups add
// to their pairs' integer rows; one finish launch divides.
int roft_pose_errors_vsd(const roft_camera* cam, const roft_mesh* mesh, const double* est, const double* ref, int n_poses, const float* depth,
                         int n_depth, const roft_vsd_params* p, double* errors_out, int32_t* counts_out)
{
    if (!cam || !mesh || !est || !ref || !depth || !p || !errors_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (n_poses < 0) return fail(ROFT_ERR_INVALID, "n_poses must be >= 0");
    if (n_poses > 0 && n_depth != 1 && n_depth != n_poses) return fail(ROFT_ERR_INVALID, "n_depth must be n_poses or 1");
    if (p->n_taus < 1 || p->n_taus > ROFT_VSD_MAX_TAUS) return fail(ROFT_ERR_INVALID, "n_taus must be 1 .. ROFT_VSD_MAX_TAUS");
    for (int k = 0; k < p->n_taus; ++k)
        if (!(std::isfinite(p->taus[k]) && p->taus[k] > 0.0)) return fail(ROFT_ERR_INVALID, "tau " + std::to_string(k) + " must be finite and > 0");
    if (!(std::isfinite(p->delta) && p->delta >= 0.0f)) return fail(ROFT_ERR_INVALID, "delta must be finite and >= 0");
    if (!(std::isfinite(p->diameter) && p->diameter >= 0.0)) return fail(ROFT_ERR_INVALID, "diameter must be finite and >= 0 (0: not normalised)");
    if (p->window_pixels < 0) return fail(ROFT_ERR_INVALID, "window_pixels must be >= 0 (0: the library's choice)");
    TRY(check_mesh(*mesh, "mesh", false));
    if (cam->width < 1 || cam->height < 1) return fail(ROFT_ERR_INVALID, "width and height must be >= 1");
    if ((long long)cam->width * cam->height >= (1ll << 24)) return fail(ROFT_ERR_INVALID, "width * height must be < 2^24");
    VsdArgs a;
    std::memset(&a, 0, sizeof(a));
    const RasterShape sh = vsd_shape(mesh->n_verts, cam->width, p->window_pixels);
    if (!sh.ok) return fail(ROFT_ERR_INVALID, "VSD: an image row is wider than the kernel's two depth windows");
    a.vcache_cap = sh.vcache_cap; a.win_alloc = sh.win_alloc; a.win_cap = sh.win_cap;
    if (n_poses == 0) return ROFT_OK;
    OpContext& c = op_context();
    std::unique_lock<std::mutex> lk;
    TRY(c.enter(lk));
    VsdScratch& sc = c.vsd;
    hipStream_t s = c.stream;
    TRY(c.mesh.upload(*mesh, MeshLayout::kWalkOrder, s));
    const size_t n = (size_t)n_poses, npix = (size_t)cam->width * cam->height;
    const int T = p->n_taus;
    const bool shared = n_depth == 1;
    constexpr int kVsdChunk = 64, kVsdSharedChunk = 32768;   // pairs per launch: with their own images / under one image
    const int chunk = std::min(n_poses, shared ? kVsdSharedChunk : kVsdChunk);
    HIP_TRY(sc.est.ensure(7 * n));
    HIP_TRY(sc.ref.ensure(7 * n));
    HIP_TRY(sc.depth.ensure(npix * (shared ? 1 : (size_t)chunk)));
    HIP_TRY(sc.counts.ensure(n * kVsdCounts));
    HIP_TRY(sc.out.ensure(n * T));
    HIP_TRY(sc.rows.ensure(n * (4 + T)));
    HIP_TRY(hipMemcpyAsync(sc.est.p, est, sizeof(double) * 7 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sc.ref.p, ref, sizeof(double) * 7 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(sc.counts.p, 0, sizeof(int32_t) * n * kVsdCounts, s));
    if (shared) HIP_TRY(hipMemcpyAsync(sc.depth.p, depth, sizeof(float) * npix, hipMemcpyHostToDevice, s));
    a.mesh = c.mesh.view();
    a.depth = sc.depth.p;
    a.depth_stride = shared ? 0 : npix;
    a.W = cam->width; a.H = cam->height;
    a.fx = (float)cam->fx; a.fy = (float)cam->fy; a.cx = (float)cam->cx; a.cy = (float)cam->cy;   // (divider 1: the camera as it is)
    a.dfx = cam->fx; a.dfy = cam->fy; a.dcx = cam->cx; a.dcy = cam->cy;
    a.delta = p->delta;
    a.n_taus = T;
    for (int k = 0; k < T; ++k) a.taus[k] = p->taus[k];
    a.diameter = p->diameter;
    for (int f0 = 0; f0 < n_poses; f0 += chunk) {   // (in order on one stream: a chunk re-uses the depth buffer of the one before)
        const int m = std::min(chunk, n_poses - f0);
        if (!shared) HIP_TRY(hipMemcpyAsync(sc.depth.p, depth + npix * (size_t)f0, sizeof(float) * npix * m, hipMemcpyHostToDevice, s));
        a.est = sc.est.p + (size_t)7 * f0;
        a.ref = sc.ref.p + (size_t)7 * f0;
        a.counts = sc.counts.p + (size_t)kVsdCounts * f0;
        // workgroups per pair: enough of them to fill the chip when the launch is small
        a.parts = (int)std::max<size_t>(1, std::min<size_t>(32, (size_t)2 * device_cu_count() / (size_t)m));
        launch_vsd(a, m, sh.lds, s);
        HIP_TRY(hipGetLastError());
    }
    launch_vsd_finish(sc.counts.p, n_poses, T, sc.out.p, sc.rows.p, s);
    HIP_TRY(hipMemcpyAsync(errors_out, sc.out.p, sizeof(double) * n * T, hipMemcpyDeviceToHost, s));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, sc.rows.p, sizeof(int32_t) * n * (4 + T), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    return ROFT_OK;
}

// host arithmetic alone (symmetry.h): no device is looked for
int roft_pose_nearest_equivalent(const double* sym, int n_sym, const double qh[4], const double x[3], const double q[4], double x_out[3],
                                 double q_out[4], int* index_out)
{
    if (!qh || !x || !q || !x_out || !q_out) return fail(ROFT_ERR_INVALID, "null argument");
    if (const char* why = roft::sym::check(sym, n_sym, ROFT_MAX_SYMMETRIES)) return fail(ROFT_ERR_INVALID, why);
    const int g = roft::sym::select(sym, n_sym, qh, q);
    if (g == 0) {   // the measurement as it was given, bit for bit
        std::memmove(x_out, x, sizeof(double) * 3);
        std::memmove(q_out, q, sizeof(double) * 4);
    } else {
        double xq[7];
        roft::sym::apply(qh, x, q, sym + roft::sym::kElement * g, xq);
        std::memcpy(x_out, xq, sizeof(double) * 3);
        std::memcpy(q_out, xq + 3, sizeof(double) * 4);
    }
    if (index_out) *index_out = g;
    return ROFT_OK;
}

int roft_debug_pose_errors_kernel_ms(double* ms_out)
{
    if (!ms_out) return fail(ROFT_ERR_INVALID, "null argument");
    OpContext& c = op_context();
    std::lock_guard<std::mutex> lk(c.mu);
    PoseErrorScratch& sc = c.pose_errors;
    if (!sc.timed) return fail(ROFT_ERR_STATE, "no roft_pose_errors call to report");
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, sc.ev0, sc.ev1));
    *ms_out = ms;
    return ROFT_OK;
}

}  // extern "C"
