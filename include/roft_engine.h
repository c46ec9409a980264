/*
 * roft_engine.h -- C ABI of the MI355X-native ROFT filtering engine (libroft_hip.so).
 *
 * This is the drop-in boundary for the per-frame filtering hot path of hsp-iit/roft
 * (`src/roft-lib`).  Plain C types only: pointers, sizes, POD structs.  Every entry point returns
 * an int status (ROFT_OK == 0, negative = error; nothing throws across the ABI) and
 * roft_last_error_string() describes the last failure of the calling thread.
 * Citations are relative to the reference checkout (hsp-iit/roft v1.2.1).
 *
 * Two levels:
 *  (1) operator-level entry points -- one per reference operator, host buffers in / host buffers
 *      out, used by the C++ facade classes in include/ROFT/ and by the parity tests:
 *        roft_flow_measurement   <- ImageOpticalFlowMeasurement<T>::freeze
 *                                   include/ROFT/ImageOpticalFlowMeasurement.hpp:231-283
 *        roft_kf_predict         <- bfl::KFPrediction over SpatialVelocityModel
 *                                   src/roft-lib/src/SpatialVelocityModel.cpp:15-27
 *        roft_skf_correct        <- SKFCorrection::correctStep  src/roft-lib/src/SKFCorrection.cpp:37-153
 *        roft_mask_propagate     <- ImageSegmentationOFAidedSource<T>::map + cv::remap
 *                                   include/ROFT/ImageSegmentationOFAidedSource.hpp:215,225,234-281
 *        roft_ukf_predict        <- bfl::UKFPrediction over CartesianQuaternionModel::motion
 *                                   src/roft-lib/src/CartesianQuaternionModel.cpp:86-141
 *        roft_ukf_correct        <- ROFT::UKFCorrection::correctStep over CartesianQuaternionMeasurement
 *                                   src/roft-lib/src/UKFCorrection.cpp:54-133,
 *                                   src/roft-lib/src/CartesianQuaternionMeasurement.cpp:357-487
 *        roft_render_depth       <- SICAD::superimpose(poses, ..., depth)  src/roft-lib/src/SICAD.cpp:924-1066
 *        roft_depth_likelihood   <- ROFTFilter::pick_best_alternative inner loop
 *                                   src/roft-lib/src/ROFTFilter.cpp:553-577
 *        roft_outlier_test       <- ROFTFilter::pick_best_alternative  src/roft-lib/src/ROFTFilter.cpp:467-621
 *        roft_pose_errors        <- add / adi of tools/third_party/bop_pose_error.py:73-108 (the evaluation's ADD / ADD-S)
 *        roft_render_scene       <- the evaluation's video / thumbnail renders: evaluation/results_renderer.py:591-778 over
 *                                   tools/object_renderer/src/renderer.cpp (section 3b)
 *  (2) the batched engine -- ROFTFilter::filtering_step (src/roft-lib/src/ROFTFilter.cpp:255-452)
 *      for many objects at once with all filter state resident in HBM:
 *        roft_engine_create / roft_object_add / roft_frame_submit | roft_frames_submit / roft_step / roft_get_state.
 *      roft_frames_submit hands over a BATCH of consecutive frames (a recorded sequence, or a live source read a few
 *      frames at a time): the engine then runs each of its three per-object chains (masks, velocity, pose) over the
 *      whole batch in one persistent kernel instead of a handful of launches per frame.
 */
#ifndef ROFT_ENGINE_H
#define ROFT_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the ABI's structs and entry points; roft_abi_version() returns the value the library was built with.  A binding
 * that mirrors the structs (roft_amd/_lib.py) refuses a library of another version.  2: roft_config::render_mode. */
#define ROFT_ABI_VERSION 2

#define ROFT_OK 0
#define ROFT_ERR_INVALID (-1)  /* bad argument */
#define ROFT_ERR_DEVICE (-2)   /* HIP runtime error / no device */
#define ROFT_ERR_CAPACITY (-3) /* caller buffer too small */
#define ROFT_ERR_STATE (-4)    /* call order violated */

/* OpenCV matrix type codes of the reference's .float flow files
 * (src/roft-lib/src/OpticalFlowUtilities.cpp:38-62) */
#define ROFT_FLOW_S16C2 11 /* CV_16SC2: S10.5 fixed point, scale 32, grid 4 (NVOF 1.0) */
#define ROFT_FLOW_F32C2 13 /* CV_32FC2: float pixels, grid 1 (NVOF 2.0) */

/* measurement types of CartesianQuaternionMeasurement (CartesianQuaternionMeasurement.h:54) */
#define ROFT_MEAS_NONE 0
#define ROFT_MEAS_VELOCITY 1
#define ROFT_MEAS_POSE 2
#define ROFT_MEAS_POSE_VELOCITY 3

/* memory kind of image pointers handed to the engine.  ROFT_MEM_DEVICE: memory the GPU can address as it is -- device or
 * managed memory, or pinned host memory that is mapped into the device's address space at the same address (hipHostMalloc,
 * hipHostRegister: zero-copy reads over the bus).  The pointers are looked up (hipPointerGetAttributes) on the first submit of
 * an engine: unregistered, pageable host memory declared as device memory is refused with ROFT_ERR_INVALID instead of
 * faulting on the GPU; later submits trust the caller (the look-up costs microseconds per pointer). */
#define ROFT_MEM_HOST 0
#define ROFT_MEM_DEVICE 1

/* How the outlier test renders the object (roft_config::render_mode, roft_render_depth_mode, roft_outlier_test_mode).  Both modes draw
 * the nearest surface's eye-space depth at the pixel centres; they differ in which triangles they draw and in the arithmetic.
 *  ROFT_RENDER_CONTRACT (default): the render contract of oracle/ro_render.c -- float arithmetic with one reciprocal per vertex and one
 *    quotient per pixel, inclusive edges, and a mesh that roft_mesh_classify calls closed drawn without the triangles that face away
 *    (while every vertex is in front of the near plane).  Limit: a closed mesh that intersects itself (a pocket pushed through another
 *    face) can lose pixels the reference draws, because a triangle that faces away can then be the nearest surface.
 *  ROFT_RENDER_GL: the numerics of the reference's OpenGL pipeline (SICAD.cpp:271-272, 1634-1637, shader_model.frag:33-51; oracle mode
 *    RO_RENDER_GL): every triangle drawn, u = (fx X) / Z + cx, window z interpolated linearly in screen space (double plane equation),
 *    24-bit depth buffer with GL_LESS (the first triangle in the caller's order wins a tie), the shader's float linearisation with
 *    near 0.001 / far 1000, the top-left rule.  Not modelled (implementation-defined in GL): sub-pixel vertex snapping and near-plane
 *    clipping (a triangle with a vertex at Z <= 0.001 is dropped).  Costs more: twice the triangles of a closed mesh, double-precision
 *    work per covered pixel, an 8-byte LDS window per pixel. */
#define ROFT_RENDER_CONTRACT 0
#define ROFT_RENDER_GL 1

/* frames per roft_frames_submit call (roft_config::max_batch_frames) */
#define ROFT_MAX_BATCH_FRAMES 8
/* optical-flow frames one mask can be chased through: the 30-entry queue of the time-stamped source
 * (OpticalFlowQueueHandler.cpp:18-26, at most 29 follow the matching entry) and the bound on "all buffered flows" of
 * ImageSegmentationOFAidedSource with an unknown number of frames between masks (hpp:186-198, 239-245) */
#define ROFT_MAX_FLOW_CHASE 30

typedef struct {
    int width, height;
    double fx, fy, cx, cy;
} roft_camera;

typedef struct {
    const void* data; /* rows*cols interleaved (dx,dy), row-major */
    int type;         /* ROFT_FLOW_* */
    int cols, rows;
    int grid;    /* image width / cols (DatasetImageOpticalFlow.cpp:46) */
    float scale; /* 32 for S16C2 else 1 (DatasetImageOpticalFlow.cpp:48-50) */
    int valid;
} roft_flow;

typedef struct {
    double alpha, beta, kappa;
} roft_ut_params;

typedef struct {
    const float* verts; /* n_verts x 3 (object frame, metres) */
    int n_verts;
    const int32_t* tris; /* n_tris x 3 */
    int n_tris;
} roft_mesh;

const char* roft_last_error_string(void);
/* number of visible HIP devices (0 when there is none); never fails */
int roft_device_count(void);
/* ROFT_ABI_VERSION of the library; never fails */
int roft_abi_version(void);

/* ---- (1) operator level: host buffers, device 0 ----------------------------------------- */

/* uv: 2 ints per kept point (u, v); y: 2N; H: 2N x 6 row-major; *n_out = N.
 * ROFT_ERR_CAPACITY if more than `capacity` points are kept. */
int roft_flow_measurement(const roft_camera* cam, const uint8_t* prev_mask, const float* prev_depth,
                          const roft_flow* flow, double dt, float radius, double depth_max,
                          int capacity, int32_t* uv, double* y, double* H, int* n_out);

int roft_kf_predict(const double x[6], const double P[36], const double Qdiag[6], double x_out[6],
                    double P_out[36]);

/* *status_out: 0 corrected, 1 measurement empty (corr = pred, SKFCorrection.cpp:61-69), 3 P_pred or the information matrix
 * P_pred^-1 + sum l H' R^-1 H is not positive definite (a pivot <= 0 or NaN): x_out / P_out are x_pred / P_pred bit for bit.
 * The call itself returns ROFT_OK in all three cases. */
int roft_skf_correct(const double x_pred[6], const double P_pred[36], int N, const double* y,
                     const double* H, const double Rdiag[2], int reweight, double x_out[6],
                     double P_out[36], int* status_out);

/* The same correction fed with the kept flow points themselves -- the form the engine's velocity filter consumes (H rows
 * rebuilt on the device from pixel, depth and camera): uv 2N ints (u, v), z N floats, flow_xy 2N floats (pixels, i.e.
 * already divided by the flow scale).  *status_out as for roft_skf_correct: 0, 1 or 3. */
int roft_skf_correct_points(const roft_camera* cam, double dt, const double x_pred[6], const double P_pred[36], int N,
                            const int32_t* uv, const float* z, const float* flow_xy, const double Rdiag[2],
                            int reweight, double x_out[6], double P_out[36], int* status_out);

/* mask (W*H u8) is propagated in place through flows[0..n_flows) (chronological); only the last
 * `frames_between` flows are used when frames_between > 0. */
int roft_mask_propagate(uint8_t* mask, int W, int H, const roft_flow* flows, int n_flows,
                        int frames_between);

int roft_pose_process_noise(const double psd_lin_acc[3], const double sigma_ang_vel[3], double T,
                            double Q[81]);
int roft_ukf_predict(const double mean[13], const double P[144], const double Q[81], double T,
                     const roft_ut_params* ut, double mean_out[13], double P_out[144]);
/* meas: [v w] | [x q] | [v w x q] with q = (w,x,y,z); Rdiag in the same order.
 * *status_out: 0 corrected, 1 no measurement, 2 singular innovation covariance (corr = pred) */
int roft_ukf_correct(const double mean[13], const double P[144], int type, const double* meas,
                     const double* Rdiag, const roft_ut_params* ut, double mean_out[13],
                     double P_out[144], int* status_out);

/* Is the mesh a closed orientable surface (host code, no device needed)?  *closed_out = 1 and flip_out[n_tris] (optional) = 1 for
 * every triangle wound clockwise seen from outside, else 0 and flip_out zeroed.  The reference draws every triangle (depth test
 * LESS, no culling: src/roft-lib/src/SICAD.cpp:271-272) and reads the NEAREST surface back; seen from outside, the nearest
 * surface of a closed mesh faces the camera, so the renders below leave the triangles of a closed mesh that face away out (while
 * every vertex is in front of the near plane) -- half the scan conversion.  Open, non-manifold or non-orientable meshes are drawn
 * whole.  Rules: oracle/ro_meshclass.c. */
int roft_mesh_classify(const roft_mesh* mesh, uint8_t* flip_out, int* closed_out);
/* tile: (H/divider) x (W/divider) float, 0 = background.  Drawn by the rasteriser of the engine's own outlier test
 * (outlier_fused_kernel: projected vertices and the depth window in LDS). */
int roft_render_depth(const roft_mesh* mesh, const double x[3], const double q[4],
                      const roft_camera* cam, int divider, float* tile);
/* *L_out = mean |depth - render| over every second mask pixel, DBL_MAX if no sample -- for a tile rendered elsewhere
 * (e.g. by the reference's SICAD); the engine itself never materialises a tile, see roft_outlier_test. */
int roft_depth_likelihood(const roft_camera* cam, const float* depth, const uint8_t* mask,
                          const float* tile, int divider, double* L_out, long* samples_out);
/* ROFTFilter::pick_best_alternative (src/roft-lib/src/ROFTFilter.cpp:467-621) for one object, on exactly the three launches
 * the engine enqueues at a pose arrival: the outlier-rejection features of (depth, mask) are buffered (:624-646), the two
 * alternatives x[0..2] q[0..3] (pose + velocity correction) and x[3..5] q[4..7] (velocity only) are rendered at
 * (W/divider) x (H/divider) and scored against every second mask pixel with 0 < depth < 2 (:553-577), and the decision
 * L_0 > 2 L_1 -> 1 (:581-583) is taken.  bands: workgroups one alternative is split over, 1..8 (0: by the CUs to spare, as
 * the engine does); vertex_cache 0: project the vertices per triangle instead of once into LDS (the GL render mode only:
 * the contract render walks the mesh in clusters of 64 triangles and keeps no projected vertices); window_pixels > 0 caps
 * the LDS depth window (a larger window is rendered in strips).  None of the three changes a bit of the depths.
 * tiles_out (optional): 2 x (H/divider) x (W/divider) floats, the renders as the kernel drew them, 0 = background.
 * L_out: DBL_MAX when an alternative has no sample. */
int roft_outlier_test(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                      const double x[6], const double q[8], int bands, int vertex_cache, int window_pixels, double L_out[2],
                      long samples_out[2], int* selected_out, float* tiles_out);
/* The same with the way the workgroups of an alternative share its work chosen FOR THIS CALL: split 1 = its triangles (windows
 * merged through memory), 0 = only the rows of its window, -1 = the library's choice.  No result depends on it. */
int roft_outlier_test_split(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                            const double x[6], const double q[8], int bands, int vertex_cache, int window_pixels, int split,
                            double L_out[2], long samples_out[2], int* selected_out, float* tiles_out);
/* roft_render_depth / roft_outlier_test_split in render mode `mode` (ROFT_RENDER_*).  ROFT_RENDER_CONTRACT returns exactly what those
 * two return.  ROFT_RENDER_GL renders with the reference's GL numerics (bit for bit RO_RENDER_GL of oracle/ro_render.c) on the same
 * kernel: bands, vertex_cache, window_pixels and split change no bit there either (its workgroups always split the rows of the window
 * only, so split is accepted and has no effect). */
int roft_render_depth_mode(const roft_mesh* mesh, const double x[3], const double q[4], const roft_camera* cam, int divider, int mode,
                           float* tile);
int roft_outlier_test_mode(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                           const double x[6], const double q[8], int bands, int vertex_cache, int window_pixels, int split, int mode,
                           double L_out[2], long samples_out[2], int* selected_out, float* tiles_out);

/* Pose errors of the evaluation (tools/third_party/bop_pose_error.py:73-108, evaluation/metrics.py:303-344) for n_poses pose pairs over
 * one point set, in double precision, by brute force on the device:
 *   ROFT_POSE_ERROR_ADD   mean_i |(R_e p_i + t_e) - (R_r p_i + t_r)|
 *   ROFT_POSE_ERROR_ADDS  mean_i min_j |(R_r p_i + t_r) - (R_e p_j + t_e)|   (BOP "adi": nearest neighbour from the ground-truth
 *                         cloud into the estimated cloud)
 * points: n_points x 3 doubles (object frame, metres); est / ref: n_poses x 7 doubles (x y z, q = w x y z); out: n_poses doubles
 * (metres).  The quaternion is used as it is given, not normalised.
 * Determinism contract: out[f] is a function of kind, the points and the pose pair f alone -- not of n_poses, of the position of
 * the pair in the call, of the other pairs or of the run (fixed summation order, no atomics): equal inputs give equal bits.
 * (ROFT_POSE_ERRORS_FMA=0 in the environment, read once per process, makes the ADD-S search square and add in the oracle's operation
 * order, 9 instead of 7 operations per pair: an A/B switch of tools/bench_pose_errors.py.  Both orders are inside the 1e-12 m the tests
 * ask for; their last bits differ, so the contract holds within a process.)
 * A pose pair with a non-finite component gives a non-finite out[f] (+inf, or NaN) and changes no other entry.
 * ROFT_ERR_INVALID: unknown kind, NULL pointer, n_points <= 0, n_poses < 0 -- checked before the device is looked for;
 * n_poses == 0 is ROFT_OK and touches nothing. */
#define ROFT_POSE_ERROR_ADD  0
#define ROFT_POSE_ERROR_ADDS 1   /* BOP "adi" */
int roft_pose_errors(int kind, const double* points, int n_points, const double* est, const double* ref, int n_poses,
                     double* out);

/* ---- (2) batched engine --------------------------------------------------------------------- */

typedef struct roft_engine roft_engine;

/* Mirrors the keys of config/config_fast_ycb.cfg consumed by ROFTFilter's constructor
 * (src/roft-lib/src/ROFTFilter.cpp:32-201, wiring src/roft/src/main.cpp:286-325). */
typedef struct {
    roft_camera cam;
    int flow_type;  /* ROFT_FLOW_* of every flow frame of this engine */
    int flow_grid;
    float flow_scale;
    double sample_time;
    roft_ut_params ut;
    double depth_maximum;       /* measurement_model.velocity.depth_maximum */
    double subsampling_radius;  /* measurement_model.velocity.subsampling_radius */
    int flow_weighting;         /* measurement_model.velocity.weight_flow */
    int use_pose, use_pose_resync, use_velocity; /* measurement_model.use_* */
    int outlier_rejection;                       /* outlier_rejection.enable */
    int flow_aided_segmentation;                 /* segmentation_dataset.flow_aided */
    /* original_fps / desired_fps of the mask source = segm_frames_between_iterations_: a new mask is chased through the
     * last mask_frames_between buffered flows; <= 0 = unknown: through ALL flows buffered since the last mask
     * (ImageSegmentationOFAidedSource.hpp:186-198, 239-245; at most ROFT_MAX_FLOW_CHASE, else roft_frames_submit fails
     * with ROFT_ERR_CAPACITY).  Values above ROFT_MAX_FLOW_CHASE are refused. */
    int mask_frames_between;
    int pose_frames_between;                     /* original_fps / desired_fps of the pose source */
    /* 1: masks come from a live source and carry the time stamp of the image they were computed on; a new mask is
     * propagated through the flows stored after the flow with that stamp (time-stamp keyed queue of the last 30 flows,
     * i.e. up to 29 flows; only the last mask_frames_between of them when that is > 0),
     * ImageSegmentationOFAidedSourceStamped.hpp:153-268 + OpticalFlowQueueHandler.cpp.  Needs
     * roft_frame_input::stamp / mask_stamp.  0: the frame-counting ImageSegmentationOFAidedSource. */
    int stamped_masks;
    int max_objects;
    /* Square root the sigma points are drawn from.  The reference (bfl) uses U sqrt(S) of the eigen-decomposition
     * of the covariance.  Any square root reproduces the first two moments; the choice only shows in fourth-order
     * terms: of the quaternion kinematics, ~ (var(theta) + T^2 var(omega))^2, in the prediction, and of the
     * quaternion measurement and the bilinear term w x r of the velocity measurement, ~ var(omega) var(x), in the
     * correction.  While these are small the engine draws the sigma points from the (much cheaper) Cholesky factor
     * and falls back to the eigen-decomposition otherwise:
     *   prediction:  max var(theta) + T^2 max var(omega) <= ukf_cholesky_guard
     *   correction:  max var(theta) <= ukf_cholesky_guard  and  max var(omega) max var(x) <= ukf_cholesky_guard_bilinear
     * Measured effect on the trajectories at the defaults (4e-4, 8e-3): <= 1e-10 (m, m/s, rad/s), DESIGN.md.
     * ukf_cholesky_guard = 0: always the eigen-decomposition; ukf_cholesky_guard_bilinear = 0: always for the
     * correction. */
    double ukf_cholesky_guard;
    double ukf_cholesky_guard_bilinear;
    int device;                                  /* HIP device ordinal */
    /* largest number of frames one roft_frames_submit may carry (1 .. ROFT_MAX_BATCH_FRAMES; 0 means 1).  Sizes the
     * engine's rings and, for zero-copy DEVICE inputs, the retention window (roft_engine_retain_frames). */
    int max_batch_frames;
    /* Bands (workgroups) the mask bit plane of an object is split over in the kernel that propagates the masks of one frame
     * (1..8; 0 = chosen by the engine: bands of ~20 image rows, a third of that on frames that deliver a mask).  A band is a
     * small workgroup -- four waves, a few KB of LDS -- that lives for one frame: nothing is persistent and no workgroup ever
     * waits for another one, so any number of engines and processes may share a device.  The propagation is an order-free OR:
     * the number of bands changes no bit of the masks (tests/test_batch_gpu.py).  (Rounds 2 - 3 walked a batch in one
     * persistent kernel whose workgroups met at a barrier in device memory and had to be resident together; the value then
     * had to be 1 for engines sharing a device.) */
    int mask_workgroups_per_object;
    /* Workgroups one alternative of an outlier test is rendered by: horizontal bands of the object's window, 1 .. 8; 0 = chosen
     * by the engine: from the device (CUs / (2 x max_objects), 2 for 64 objects on 256 CUs), and half of that while the host runs
     * ahead of the device by the whole in-flight bound, i.e. in the steady state of a long sequence (fewer bands occupy fewer CUs
     * for longer: with 64 objects one band tracks 5 % more object-frames/s in long runs and 2.5 % fewer in a 20-frame burst,
     * DESIGN.md section 4).  The likelihood's sums are exact (integer), so the band count changes no result. */
    int outlier_bands_per_alternative;
    /* How the outlier test renders (ROFT_RENDER_*; 0, the default, is the render contract): a semantics switch -- ROFT_RENDER_GL
     * scores the alternatives on the reference's GL numerics, slower.  Other values are refused by roft_engine_create. */
    int render_mode;
} roft_config;

typedef struct {
    double p_mean0[13];     /* v w x q(wxyz): initial_condition.pose */
    double p_cov0_diag[12];
    double v_mean0[6];      /* initial_condition.velocity */
    double v_cov0_diag[6];
    double p_sigma_ang_vel[3]; /* kinematic_model.pose.sigma_angular */
    double p_psd_lin_acc[3];   /* kinematic_model.pose.sigma_linear  */
    double v_q_diag[6];        /* kinematic_model.velocity.{sigma_linear, sigma_angular} */
    double p_meas_cov_v[3], p_meas_cov_w[3], p_meas_cov_x[3], p_meas_cov_q[3];
    double v_meas_cov_flow[2];
    roft_mesh mesh;            /* host pointers; copied */
} roft_object_desc;

/* One object's inputs for one frame.  Image pointers are HOST or DEVICE memory according to
 * mem_kind.  DEVICE buffers are used in place (zero copy): previous depth, the buffered flows a new mask is
 * chased through and the outlier-rejection features of ROFTFilter.cpp:624-646 are references into them, and
 * the engine keeps several frames in flight.  A DEVICE buffer handed over for frame k must therefore stay
 * valid and unmodified until the submit call that carries frame k + roft_engine_retain_frames() has returned (that
 * call blocks until every frame that can still read it has finished on the GPU).  ROFT_RETAIN_FRAMES is that number
 * for the default configuration (max_batch_frames 1, mask_frames_between 6).  A flow that outlives the window
 * because later flows were dropped (the reference clones every buffered flow) is copied into engine memory before
 * the window closes.  HOST buffers are copied into the engine's own ring before the submit call returns (the call
 * waits for the copies: the caller may re-use a HOST buffer as soon as it has returned); identical HOST pointers
 * within one frame -- a scene shared by several objects -- are uploaded once.  The ring holds
 * roft_engine_retain_frames() frames and grows, in 32 MiB pieces of device memory, to the bytes the largest frame
 * staged so far needed: retain x (depth + flow + mask) x objects when every object has images of its own (64 objects at
 * 640x480 CV_32FC2, batches of 8: 48 x 239 MB = 11.5 GB), retain x (one depth + flow + the masks) for a shared scene. */
#define ROFT_RETAIN_FRAMES 16
typedef struct {
    double dt;            /* RGB stamp delta; <= 0 means cfg.sample_time */
    const float* depth;   /* H x W metres, 0 = invalid; required.  On an engine with roft_engine_enable_raw_depth (section 3c): a
                             const uint16_t* image of the depth source's size instead, HOST or DEVICE like the others */
    const void* flow;     /* flow frame or NULL when absent (first frame) */
    const uint8_t* mask;  /* newly delivered mask or NULL */
    int pose_valid;       /* newly delivered pose measurement? */
    double pose_x[3];
    double pose_q[4];     /* (w,x,y,z) */
    int mem_kind;
    double stamp;         /* stamped_masks: RGB time stamp of this frame (s) */
    double mask_stamp;    /* stamped_masks: time stamp of the image `mask` was computed on */
} roft_frame_input;

typedef struct {
    double pose[13];   /* v w x q */
    double twist[6];   /* v_O, w */
    int n_flow_points; /* N of the velocity stage, -1 if it did not run */
    int outlier_selected; /* -1 no test this frame, 0 pose+velocity kept, 1 velocity-only chosen */
    double outlier_L[2];
} roft_object_output;

int roft_default_config(roft_config* cfg, int width, int height, int flow_type);
int roft_default_object(roft_object_desc* obj);

int roft_engine_create(const roft_config* cfg, roft_engine** out);
int roft_engine_destroy(roft_engine* e);
int roft_object_add(roft_engine* e, const roft_object_desc* desc, int* obj_id);

/* ---- restart object slots on a running engine: a new track in the same slot ------------------------------------------------------ *
 * The objects of an engine are fixed before its first frame; roft_objects_restart gives n of them (obj_ids[i], each named once) a new
 * description descs[i] -- initial pose and covariances, noise parameters, mesh -- while every other object keeps its state: a lost
 * track is re-initialised (section 3d tells the caller when), or a slot whose sequence has ended takes the next one.
 *
 * The contract.  Let the engine have stepped F frames when the call returns ROFT_OK.
 *  - A NAMED slot: everything the engine returns for it on engine frame F + k -- log row, roft_get_outputs, roft_get_state,
 *    roft_get_mask, roft_engine_get_flow, roft_engine_get_depth, quality records apart from their `frame` field -- is bit for bit
 *    what a NEW engine returns on its frame k: an engine with the same roft_config and the same enable calls, whose objects were
 *    added with the descriptions the slots have now, fed the inputs of frames F, F + 1, ...  Frame F is the slot's first frame in every
 *    sense the reference gives that word: a flow handed with it is not used, there is no previous depth, the first-mask rule applies
 *    (frame F must deliver a mask, or the object be enrolled for pose masks), outlier-rejection features are not initialised, the
 *    velocity buffer and the flow history are empty, the eigen-decomposition starts cold, on an engine with camera images the flow
 *    starts over, and an enrolled pose-mask object without pose_valid draws the silhouette of the new p_mean0.
 *  - A slot NOT named: bit for bit what the same engine returns without the call.
 *  - What persists: the slot id, pose-mask enrolment and scene membership, the quality, log, raw-depth and flow enables.  Log rows and
 *    quality records of earlier frames stay readable, and records keep the ENGINE's frame numbering (frame % every included): the
 *    engine's frame count never restarts.  Until the slot's next step roft_get_outputs shows the old track's last row and
 *    roft_get_mask is ROFT_ERR_STATE, as on a new engine; roft_get_state already returns the new initial belief.  roft_engine_score_log with points == NULL uses the slot's current mesh.
 *  - THE CALL WAITS for every stepped batch, exactly as roft_sync does, and the engine counts as idle afterwards (the next batches
 *    are a burst again): restart the slots that are due in ONE call.  Restarts are served on an idle engine by plain copies; the
 *    launch graph of a batch does not know about them.
 *  - ROFT_RESTART_KEEP_MESH: descs[i].mesh is not looked at; the slot keeps its resident mesh (no upload, no classification).
 *    A symmetry group (section 3h) goes with the mesh: the slot keeps it under KEEP_MESH and loses it when the mesh is replaced.
 *  - Refusals, all on the host before anything changes and before any wait, with the reason in roft_last_error_string.
 *    ROFT_ERR_INVALID, checked before a device is looked for: a NULL engine; n < 0, or n > 0 with a NULL array; an id outside the
 *    engine's objects; an id named twice; unknown flag bits; every check roft_object_add makes on a description; a description
 *    without a mesh (without KEEP_MESH) for an object that needs one -- outlier rejection with use_pose, or enrolled for pose masks.
 *    ROFT_ERR_STATE: a submitted batch that has not been stepped.  n == 0 is ROFT_OK and does not wait.
 *  - Before the first frame the call is equivalent to having added the object with that description.
 * Not offered: new slots after the first frame, ended or parked slots, a restart that does not wait. */
#define ROFT_RESTART_KEEP_MESH 1
int roft_objects_restart(roft_engine* e, const int* obj_ids, const roft_object_desc* descs, int n, int flags);
typedef struct { long long calls, objects, meshes_replaced; } roft_engine_restart_stats;   /* successful calls with n > 0, slots restarted, meshes uploaded by them; since roft_engine_create */
int roft_engine_get_restart_stats(roft_engine* e, roft_engine_restart_stats* out);

/* inputs: one entry per object, in obj_id order.  Enqueues uploads and builds the frame program.  On an error
 * nothing of the frame has been consumed: the call can be repeated with corrected inputs. */
int roft_frame_submit(roft_engine* e, const roft_frame_input* inputs, int n_inputs);
/* A batch of n_frames consecutive frames (1 .. roft_config::max_batch_frames): inputs[t * n_objects + obj]. */
int roft_frames_submit(roft_engine* e, const roft_frame_input* inputs, int n_objects, int n_frames);

/* Label-image masks: ONE segmentation image per camera frame (a network's output, YCB-Video's -label.png) instead of one H x W
 * byte mask per object.  An object whose entry names a label image behaves, bit for bit, as if it had been handed the mask
 * M(p) = (L(p) == label) ? 255 : 0 through roft_frame_input::mask: schedule, first-mask rule, the "new but empty mask is
 * ignored" rule (ImageSegmentationOFAidedSource.hpp:186-198) when the value does not occur in the image, mask_stamp,
 * propagation, features and the outlier test.
 *  - Membership is EQUALITY with `label`, not a threshold: value 3 selects the pixels that are 3, not those >= 3.
 *  - A label image gives every pixel to at most one value, so it cannot express OVERLAPPING instance masks (nor the
 *    three-valued {0, 1, 255} masks): the per-object form, roft_frame_input::mask, remains for those.
 * Two objects may name the same value, the objects of one frame may name different images, and objects with and without labels
 * may be mixed within a frame.  HOST images are uploaded once per distinct host pointer and frame however many objects name them
 * (roft_engine_stats counts them once); DEVICE images are read in place under the retention contract of roft_frame_input and
 * must be 16-byte aligned.  The engine makes one pass over each distinct image of a delivering frame for all objects that name it.
 * ROFT_ERR_INVALID, with nothing of the batch consumed: labels != NULL together with inputs[].mask != NULL; label 0 (background
 * by convention); a label outside the type's range; an unknown label_type; a misaligned DEVICE image. */
#define ROFT_LABEL_U8  1
#define ROFT_LABEL_U16 2
typedef struct {
    const void* labels;  /* H x W label image (HOST or DEVICE like the frame's other images: inputs[].mem_kind),
                            NULL: this object takes inputs[].mask as before */
    int label_type;      /* ROFT_LABEL_* */
    int label;           /* the object's pixels are those EQUAL to this value; 1 .. 255 / 65535 */
} roft_label_mask;
/* roft_frames_submit with masks taken from label images: labels[t * n_objects + obj], or labels == NULL (then exactly
 * roft_frames_submit) */
int roft_frames_submit_labels(roft_engine* e, const roft_frame_input* inputs, const roft_label_mask* labels, int n_objects, int n_frames);
/* Stand-alone operator (tests, tools): the n masks {0, 255} (masks_out: n x H x W bytes, optional) and their pixel counts
 * (counts_out: n ints, optional) of the values[0..n) in one HOST label image, by the engine's own ingest kernel.  Values may
 * repeat and may be absent from the image (count 0, all-zero mask); 0 and values outside the type's range are refused. */
int roft_labels_to_masks(const void* labels, int label_type, int W, int H, const int* values, int n, uint8_t* masks_out, int* counts_out);

/* Enqueues every kernel of ROFTFilter::filtering_step for all objects and all submitted frames; returns without
 * waiting. */
int roft_step(roft_engine* e);
/* retention window of zero-copy DEVICE inputs in frames (see roft_frame_input) */
int roft_engine_retain_frames(const roft_engine* e);
int roft_sync(roft_engine* e);
/* Blocks until the last step has finished.  Any of the output pointers may be NULL. */
int roft_get_state(roft_engine* e, int obj_id, double pose13[13], double P12[144], double twist6[6],
                   double Pv[36]);
/* outputs of the last finished step for all objects (n_objects entries) */
int roft_get_outputs(roft_engine* e, roft_object_output* outs, int n_outs);
/* current propagated, binarised mask (H*W u8, {0,255}) of one object -> host buffer */
int roft_get_mask(roft_engine* e, int obj_id, uint8_t* mask_out);

/* Device-side log of the per-frame outputs (what ROFTFilter logs per frame, ROFTFilter.cpp:386-394):
 * a ring of n_frames x n_objects records written by the step itself, read back in one copy. */
int roft_engine_enable_log(roft_engine* e, int n_frames);
int roft_engine_get_log(roft_engine* e, int first_frame, int n_frames, roft_object_output* outs);
/* the same log as the reference writes it: rows[(f * n_objects + obj) * 19 ..] = pose(13: v w x q) | twist(6)
 * (`pose_estimate` + `velocity_estimate`, ROFTFilter.cpp:386-394) -- the per-object records a multi-GPU job gathers */
int roft_engine_get_log_rows(roft_engine* e, int first_frame, int n_frames, double* rows);
/* roft_pose_errors for the poses of one object in the log: the estimates are read in place (pose[6..12] of the records, ring
 * wrap-around included) and never leave the device; the same device code, so the result equals roft_pose_errors on the rows
 * roft_engine_get_log_rows returns bit for bit.  ref: n_frames x 7 host doubles for frames first_frame .. first_frame + n_frames - 1;
 * points NULL (n_points ignored): every vertex of the mesh the object was added with (float -> double is exact).  Syncs the engine.
 * ROFT_ERR_INVALID: log off, bad obj_id, unknown kind, and a frame range that is not wholly inside what the ring still holds --
 * valid is first_frame >= 0, n_frames <= the log's capacity, first_frame + n_frames <= frames stepped and
 * first_frame >= frames stepped - capacity.  n_frames == 0 is ROFT_OK. */
int roft_engine_score_log(roft_engine* e, int kind, int obj_id, int first_frame, int n_frames, const double* points,
                          int n_points, const double* ref, double* out);

/* work enqueued since roft_engine_create */
typedef struct {
    long long frames;          /* frames stepped */
    long long batches;         /* roft_step calls */
    long long launches;        /* kernel launches + memsets + copies enqueued by roft_step */
    long long event_ops;       /* cross-stream waits + explicit event records enqueued by roft_step */
    long long h2d_bytes;       /* bytes of HOST inputs uploaded by the submit calls */
    long long h2d_copies;      /* ... in this many copies (images of consecutive frames that are consecutive in host memory go in one) */
} roft_engine_stats;
int roft_engine_get_stats(roft_engine* e, roft_engine_stats* out);

/* What the engine decided for, and the host spent on, each of the last batches (a ring of 64): a slow run explains itself.
 * The scheduling mode of a batch is a function of the batch INDEX, the object count and the number of engines this process holds on
 * the device (lanes are released early only by the ONLY engine of the device: a count taken at the submit, never a timing): `steady` = at least <batches in flight> batches have
 * been stepped since the engine was last idle (creation / roft_sync / anything that reads results); bursts release the pose
 * lanes early (`handoff`, `early_lanes`) and spread an outlier test over all the CUs to spare, steady batches halve that
 * (`outlier_parts_halved`); `early_lanes` is a bit mask: 1 / 2 = pose lane 0 / 1 released behind the batch's control blocks (its
 * objects start with the first step of a re-sync replay, whose twist an earlier batch published), 4 = both lanes because the
 * device has CUs to spare.  `throttled` is the MEASURED counterpart (the submit call had to wait for the in-flight bound) and
 * steers nothing.  Times: host steady clock in microseconds; t_done_us is when the HOST observed the batch complete (inside a
 * later submit call or roft_sync, which waits for the batches one by one in order), 0 while it has not. */
typedef struct {
    int batch;                 /* index since roft_engine_create */
    int frames;
    int steady, throttled, handoff, early_lanes, outlier_parts_halved;
    int launches, event_ops;   /* enqueued by roft_step for this batch */
    double t_submit_us;        /* entry of roft_frames_submit */
    double submit_us;          /* inside roft_frames_submit (frame programs, uploads) ... */
    double wait_us;            /* ... of which blocked on the in-flight bound */
    double step_us;            /* inside roft_step (launches) */
    double t_done_us;
} roft_batch_trace;
/* the last min(capacity, 64, batches so far) batches, oldest first */
int roft_engine_get_batch_trace(roft_engine* e, roft_batch_trace* out, int capacity, int* n_out);

/* HIP stream the engine enqueues on (as void*), for timing with hipEvents */
void* roft_engine_stream(roft_engine* e);

/* Kernel timing with HIP events on the engine's streams, accumulated over the steps since the last
 * roft_engine_get_timing.  enable: 0 off, 1 only flow_measure_kernel (a start / stop event pair bound to its dispatch, what
 * bench.py keeps on inside its timed region), 2 every launch group (adds ~10 event records per batch).
 * With timing on, the flow measurement's launches (the first 64 between two roft_engine_get_timing calls) are also timed
 * on the device's own 100 MHz clock -- every workgroup leaves its start and end, the entry "flow_measure_span" is first
 * workgroup in -> last workgroup out, the duration a kernel trace reports.  roft_engine_enable_timing creates its events
 * and sends one event-paired dispatch down the velocity stream before it returns (call it outside a timed region).
 * names/ms arrays are owned by the engine. */
int roft_engine_enable_timing(roft_engine* e, int enable);
int roft_engine_get_timing(roft_engine* e, int* n_out, const char*** names_out, const float** ms_out,
                           const int** launches_out);

/* ---- (2b) pinned host memory for images that are read in place ---------------------------------------------------- *
 * Image buffers handed over as ROFT_MEM_HOST are copied to the device by the submit call: every byte of depth, flow and mask
 * crosses the bus although the kernels read a few hundred KB of a frame (the pixels of the object's mask).  Buffers that live in
 * pinned, device-mapped host memory can be handed over as ROFT_MEM_DEVICE instead -- under the retention contract of DEVICE
 * inputs (roft_frame_input) -- and are then read in place: only the sectors the kernels touch cross the bus and nothing is
 * staged.  roft_host_alloc returns such memory from a pool (blocks are recycled by size; the first allocation of a size pins
 * pages, ~0.1 ms per MB), NULL when there is no device or the allocation fails: use ordinary memory and ROFT_MEM_HOST then.
 * The class facade (include/ROFT/Compat.h) allocates its image-sized buffers this way and ROFT::ROFTFilter keeps the frames of
 * the retention window alive, so the reference's executable reads its images from disk straight into memory the GPU reads. */
void* roft_host_alloc(size_t bytes);
void roft_host_free(void* p);              /* p from roft_host_alloc; NULL is ignored */
int roft_host_is_pinned(const void* p);    /* 1 when p lies inside a live block of the pool */

/* ---- (3) optical-flow producer (replaces the reference's NVIDIA-hardware flow source) ---------------- *
 * ROFT consumes pre-computed flow frames produced by cv::cuda::NvidiaOpticalFlow_{1_0,2_0}
 * (src/roft-lib/src/ImageOpticalFlowNVOF.cpp:100-159, tools/nvof/dumper/src/main.cpp:40-146).  MI355X has no
 * fixed-function flow unit: this is a dense pyramidal Lucas-Kanade on the CUs producing the same two products,
 * CV_32FC2 at grid 1 (NVOF 2.0 shape) or CV_16SC2 S10.5 at grid 4 (NVOF 1.0 shape), forward flow of the PREVIOUS
 * frame's pixels. */
typedef struct {
    int levels;      /* pyramid levels (1..6); width and height must be multiples of 2^(levels-1) */
    int radius;      /* window half size: (2r+1)^2 taps */
    int iterations;  /* Gauss-Newton iterations per level */
    float det_min;   /* pixels whose structure tensor determinant is below this keep the coarser estimate */
} roft_of_params;

int roft_default_of_params(roft_of_params* p);

/* host buffers: prev/cur gray u8 (H x W).  out_type ROFT_FLOW_F32C2 -> float[H][W][2];
 * ROFT_FLOW_S16C2 -> int16[H/4][W/4][2]. */
int roft_optical_flow(const uint8_t* prev_gray, const uint8_t* cur_gray, int W, int H, const roft_of_params* p,
                      int out_type, void* flow_out);

/* batched, device-resident producer: n image pairs per call, asynchronous on its own stream */
typedef struct roft_flow_producer roft_flow_producer;
int roft_flow_producer_create(int W, int H, int max_pairs, const roft_of_params* p, int out_type, int device,
                              roft_flow_producer** out);
int roft_flow_producer_destroy(roft_flow_producer* fp);
/* prev/cur/out: host arrays of n DEVICE pointers (u8 images in, flow frames out) */
int roft_flow_producer_run(roft_flow_producer* fp, const uint8_t* const* prev, const uint8_t* const* cur,
                           void* const* out, int n_pairs);
int roft_flow_producer_sync(roft_flow_producer* fp);
void* roft_flow_producer_stream(roft_flow_producer* fp);

/* ---- (3a) camera images on the engine --------------------------------------------------------------------------- *
 * Camera images instead of flow frames: the engine computes the optical flow itself (the producer of section 3) and the flow
 * never leaves the device.  Let G_k be the gray image of an object's frame k: a GRAY8 image as it is, a colour image through
 * OpenCV's 8-bit COLOR_BGR2GRAY, (R 4899 + G 9617 + B 1868 + 8192) >> 14, computed on the device.  An object whose entries
 * carry images behaves, bit for bit, as if inputs[].flow of frame k had been a HOST buffer holding
 * roft_optical_flow(G_{k-1}, G_k, W, H, p, roft_config::flow_type) when frames k - 1 and k both carried an image, and NULL
 * otherwise.  So the object's first frame has no flow, a frame without an image has none, and the image after it STARTS OVER:
 * no flow ever spans more than one sample time (ImageOpticalFlowNVOF keeps its last frame across an invalid camera frame; this
 * does not).  An object may still hand a flow directly (image NULL) for any frame, and both forms mix within a frame.
 *  - Images are HOST or DEVICE like the frame's other images (inputs[].mem_kind).  HOST images are uploaded once per distinct
 *    pointer and frame, so the objects of a shared scene name one image; DEVICE images (4-byte aligned) are read in place,
 *    during the submit call's own enqueued work, under the retention contract of roft_frame_input.
 *  - One pyramid is built per distinct image and one flow per distinct (previous, current) pair of a frame, however many objects
 *    name them: roft_engine_flow_stats.
 *  - ROFT_ERR_INVALID, nothing consumed: an entry with image AND flow, an unknown image_type, a misaligned DEVICE image.
 *    ROFT_ERR_STATE: images on an engine without roft_engine_enable_flow. */
#define ROFT_IMAGE_GRAY8 1   /* H x W bytes */
#define ROFT_IMAGE_BGR8  2   /* H x W x 3, OpenCV order: what the reference's camera delivers */
#define ROFT_IMAGE_RGB8  3   /* H x W x 3, PNG order */
typedef struct {
    const void* image;   /* NULL: no camera image for this object and frame */
    int image_type;      /* ROFT_IMAGE_* */
} roft_frame_image;
/* Before the first frame (ROFT_ERR_STATE afterwards); p NULL: roft_default_of_params.  ROFT_ERR_INVALID, with the reason in
 * roft_last_error_string, for a configuration the producer cannot serve -- flow_type F32C2 needs flow_grid 1 and flow_scale 1,
 * S16C2 grid 4 and scale 32; the width a multiple of 4 * 2^(levels-1), the height of 2^(levels-1) and of 4 -- and for parameters
 * outside roft_flow_producer_create's ranges. */
int roft_engine_enable_flow(roft_engine* e, const roft_of_params* p);
/* images[t * n_objects + obj]; images NULL: exactly roft_frames_submit_labels; labels may be NULL */
int roft_frames_submit_images(roft_engine* e, const roft_frame_input* inputs, const roft_label_mask* labels,
                              const roft_frame_image* images, int n_objects, int n_frames);
/* the flow the engine produced for obj's last stepped frame, in the engine's flow type (H / grid x W / grid x 2) -> host buffer;
 * syncs; ROFT_ERR_STATE when that frame had none */
int roft_engine_get_flow(roft_engine* e, int obj_id, void* flow_out);
typedef struct {
    long long images;       /* distinct images taken in */
    long long image_bytes;  /* ... their bytes uploaded (a DEVICE image adds none) */
    long long pyramids;     /* pyramids built */
    long long pairs;        /* flows produced */
} roft_engine_flow_stats;   /* since roft_engine_create */
int roft_engine_get_flow_stats(roft_engine* e, roft_engine_flow_stats* out);
/* Stand-alone operator (tests, tools): the gray image (W x H bytes) of a HOST image, any W, H >= 1, by the device's conversion. */
int roft_image_to_gray(const void* image, int image_type, int W, int H, uint8_t* gray_out);

/* ---- (3f) forward-backward check: occluded pixels of a produced flow are marked invalid --------------------------------- *
 * Dense Lucas-Kanade returns a vector for every pixel, also where frame k covers or uncovers something and no correspondence
 * exists.  With the check on, the producer also computes the flow of the swapped pair and keeps a vector only where the two
 * agree.  An invalid vector is what the consumers already skip (OpticalFlowUtilities.h:19-22: NaN, or magnitude >= 1e9): the flow
 * measurement draws no sample from it and the mask chain drops a pixel whose chase meets it.  Opt-in: a producer or an engine
 * that does not enable the check produces what it did before, bit for bit.
 *
 * The check, operation by operation (float; every product and sum one rounded operation, no fused multiply-add):
 *   F = the level-0 field of (prev, cur), H x W x 2: roft_optical_flow's CV_32FC2 product;  B = that of (cur, prev), same parameters
 *   for pixel (x, y), (fx, fy) = F[y][x]:
 *     xf = (float)x + fx;  yf = (float)y + fy
 *     inside = xf >= 0 && xf <= (float)(W-1) && yf >= 0 && yf <= (float)(H-1)          (false for a flow that is not finite)
 *     x0 = floorf(xf), ax = xf - x0, x1 = min((int)x0 + 1, W-1);  y0, ay, y1 likewise
 *     per component c of B:  top = (1 - ax) * B[y0][x0] + ax * B[y0][x1]
 *                            bot = (1 - ax) * B[y1][x0] + ax * B[y1][x1]
 *                            b_c = (1 - ay) * top + ay * bot
 *     ex = fx + bx;  ey = fy + by;  e2 = ex*ex + ey*ey;  m2 = (fx*fx + fy*fy) + (bx*bx + by*by)
 *     valid = inside && e2 <= tolerance_rel * m2 + tolerance_abs                       (multiply, then add)
 *   A valid pixel keeps its two floats untouched; an invalid one gets the bit pattern 0x7FC00000 (a quiet NaN) in both.  A
 *   pixel whose target leaves the image cannot be checked and is invalid.
 * Defaults: tolerance_abs 0.5, tolerance_rel 0.01 -- the customary values of the large-displacement-flow literature (Sundaram,
 * Brox, Keutzer, ECCV 2010).  NOBODY HAS TUNED THEM FOR THIS TRACKER.
 * CV_32FC2 only: CV_16SC2 has no representation of "invalid", so every entry point below refuses an S16C2 product with
 * ROFT_ERR_INVALID.  Tolerances must be finite and >= 0 (ROFT_ERR_INVALID). */
typedef struct {
    float tolerance_abs, tolerance_rel;
} roft_of_consistency;
int roft_default_of_consistency(roft_of_consistency* c);
/* host buffers, like roft_optical_flow with out_type ROFT_FLOW_F32C2; c NULL: the defaults.  Bad arguments (a null pointer,
 * parameters outside roft_flow_producer_create's ranges, bad tolerances) are refused before a device is looked for. */
int roft_optical_flow_checked(const uint8_t* prev_gray, const uint8_t* cur_gray, int W, int H, const roft_of_params* p,
                              const roft_of_consistency* c, float* flow_out);
/* Every later roft_flow_producer_run checks its products; c NULL turns the check off again (today's product, bit for bit).
 * Allocates the backward workspace on first use.  max_pairs keeps its meaning: pairs per call, not Lucas-Kanade problems.
 * ROFT_ERR_INVALID on an S16C2 producer or for bad tolerances; the producer is then as before the call. */
int roft_flow_producer_set_consistency(roft_flow_producer* fp, const roft_of_consistency* c);
/* The engine's own flows (section 3a) are checked: an object whose entries carry images behaves, bit for bit, as if inputs[].flow
 * of frame k had been a HOST buffer holding roft_optical_flow_checked(G_{k-1}, G_k, W, H, p, c).  roft_engine_get_flow returns
 * the checked field; roft_engine_flow_stats::pairs still counts flows produced, not Lucas-Kanade problems; a flow an object
 * hands in directly is never checked.  After roft_engine_enable_flow and before the first frame (ROFT_ERR_STATE otherwise);
 * c NULL: the defaults.  ROFT_ERR_INVALID when roft_config::flow_type is S16C2 or the tolerances are bad.  A refused call
 * leaves the engine as if it had not been made.  (roft_engine_enable_flow called again starts from "off".) */
int roft_engine_enable_flow_consistency(roft_engine* e, const roft_of_consistency* c);

/* ---- (3c) raw sensor depth on the engine -------------------------------------------------------------------------- *
 * No sensor delivers H x W floats in metres registered to the colour camera.  The reference's capture tool reads Z16 frames,
 * registers them to the colour stream with rs2::align and calls convertTo(CV_32FC1, 0.001) on every frame, on the host
 * (tools/rs-capture/src/main.cpp:23-67); YCB-Video and HO-3D store depth as 16-bit images too
 * (tools/dataset/conversion/ho3d_utils.py:35-46, 82-83).  On an engine with roft_engine_enable_raw_depth the caller hands over the
 * sensor's 16-bit frame: inputs[].depth then carries a `const uint16_t*` image of the depth source's size -- for every object and
 * every submit call (roft_frames_submit, _labels, _images), HOST or DEVICE memory as mem_kind says -- and the float depth the
 * kernels read is made on the device and never exists on the host.
 *
 * Equivalence that defines the feature: the engine behaves, bit for bit, as if inputs[].depth had been a HOST float image --
 * roft_depth_convert(raw) with align == 0, roft_depth_align(raw) otherwise.  HOST images are uploaded once per distinct pointer and
 * frame (two bytes per reading), DEVICE images (4-byte aligned) are read in place under the retention contract of roft_frame_input;
 * one product is made per distinct raw image and frame however many objects name it, and it lives exactly as long as a staged HOST
 * depth of that frame would (the next frame's flow measurement reads it as the previous depth).
 *
 * CONVERT: out = (float)d * scale, one float multiply; 0 stays 0, the engine's "invalid".
 *
 * ALIGN: float arithmetic in exactly this operation order, without contraction; the cameras' doubles are converted to float once.
 * For every depth pixel (x, y) with d != 0:  z = (float)d * scale;  for the two corners s in {-0.5f, +0.5f}:
 *     px = (float)x + s,  py = (float)y + s
 *     X = ((px - cx_d) / fx_d) * z,  Y = ((py - cy_d) / fy_d) * z
 *     P_i = ((R[i][0] * X + R[i][1] * Y) + R[i][2] * z) + t[i]        the pixel is skipped unless P_2 > 0
 *     u = (P_0 / P_2) * fx_c + cx_c,  v = (P_1 / P_2) * fy_c + cy_c
 * The pixel is skipped unless u0, v0, u1, v1 are all finite.  Its targets are the colour pixels whose CENTRES lie in the half-open
 * footprint, computed in float: x0 = max(ceilf(u0), 0), x1 = min(ceilf(u1) - 1, W_c - 1), rows likewise; empty when x1 < x0 or
 * y1 < y0; the pixel is skipped when x1 - x0 >= ROFT_DEPTH_ALIGN_MAX_SPAN or y1 - y0 >= ROFT_DEPTH_ALIGN_MAX_SPAN after clipping.
 * Every target keeps the MINIMUM RAW VALUE d of all source pixels that cover it; the output is (float)d_min * scale, and 0 where
 * nobody covers.  The value written is the sensor's reading, not P_2 (the two cameras of such a sensor are coplanar to a fraction of
 * a millimetre).  The minimum is over integers: the result depends neither on the execution order nor on the run.  Two consequences:
 * identity extrinsics with equal cameras give roft_depth_convert bit for bit, and an exact x2 camera replicates every reading into a
 * 2 x 2 block without holes or overlaps.
 * Deviation from librealsense, on purpose: rs2::align rounds both corners to nearest and fills inclusively, which takes a 2 x 2
 * minimum even under identity and drops footprints that are partly outside the image; this contract uses centres in a half-open
 * footprint and clips.  (librealsense was not at hand when this was written: that description of it is RECALLED, not read.)
 * Not modelled: a distorted depth camera of its own (section 3g rectifies what is in the colour camera), colour aligned to depth,
 * per-object depth formats.
 *
 * Refusals, all on the host before anything is enqueued, nothing consumed.  ROFT_ERR_STATE: enabling after the first frame.
 * ROFT_ERR_INVALID: a NULL argument; an unknown type; a scale that is not finite or not > 0; align == 0 with a size other than
 * roft_config::cam; a non-finite R or t; a focal length <= 0 or not finite; width * height >= 2^24; a DEVICE raw image that is
 * not 4-byte aligned. */
#define ROFT_DEPTH_Z16 1            /* H x W uint16, 0 = no reading */
#define ROFT_DEPTH_ALIGN_MAX_SPAN 16
typedef struct {
    int   type;        /* ROFT_DEPTH_* */
    float scale;       /* metres per unit (RealSense: 0.001f); finite, > 0 */
    int   align;       /* 0: the frame is already in the engine's camera (size must equal roft_config::cam; cam/R/t ignored) */
    roft_camera cam;   /* align != 0: the DEPTH camera, any width, height >= 1, pinhole (its own lens distortion is not modelled) */
    float R[9];        /* row-major; P_colour = R * P_depth + t */
    float t[3];        /* metres */
} roft_depth_source;
/* before the first frame */
int roft_engine_enable_raw_depth(roft_engine* e, const roft_depth_source* src);
/* the float depth (roft_config::cam: H x W) the engine made for obj's last stepped frame -> host buffer; syncs; ROFT_ERR_STATE on an
 * engine that makes no depth (neither raw depth nor the rectification of section 3g) or before the first step */
int roft_engine_get_depth(roft_engine* e, int obj_id, float* depth_out);
typedef struct {
    long long images;       /* distinct raw images taken in */
    long long image_bytes;  /* ... their bytes uploaded (a DEVICE image adds none) */
    long long products;     /* float depth images made */
} roft_engine_depth_stats;  /* since roft_engine_create */
int roft_engine_get_depth_stats(roft_engine* e, roft_engine_depth_stats* out);
/* stand-alone operators (tests, tools): HOST buffers, device 0.  raw: H x W; out: H x W floats (roft_depth_align: the colour
 * camera's size; src->align is not looked at, src->cam / R / t always are).  Any W, H >= 1. */
int roft_depth_convert(const uint16_t* raw, int W, int H, float scale, float* out);
int roft_depth_align(const uint16_t* raw, const roft_depth_source* src, const roft_camera* colour, float* out);

/* ---- (3g) lens distortion: frames rectified into the pinhole camera on the device ------------------------------------- *
 * A real colour camera has Brown-Conrady coefficients; ignored, pixels near the border move by whole pixels, which biases the
 * flow-to-twist Jacobian ((u - cx) / fx), the depth back-projection and every render-against-depth comparison.  On an engine with
 * roft_engine_enable_rectification the caller hands over the DISTORTED frames as the sensor delivers them and the engine resamples
 * them into its pinhole camera roft_config::cam on the device, once per distinct image, before anything else reads them.
 *
 * MODEL.  OpenCV's Brown-Conrady model with identity rectification rotation (the float counterpart of initUndistortRectifyMap).
 * A roft_lens holds the SOURCE (sensor) camera and k1, k2, p1, p2, k3; the target is a pinhole roft_camera.  All doubles are
 * converted to float once; everything below is float, one rounded operation per written operation, nothing contracted.
 *
 * MAP.  For target pixel (u, v), with (fx, fy, cx, cy) the target's and (fx_s, fy_s, cx_s, cy_s) the source's intrinsics:
 *     x = ((float)u - cx) / fx;  y = ((float)v - cy) / fy
 *     xx = x*x;  yy = y*y;  xy = x*y;  r2 = xx + yy
 *     rad = 1 + r2*(k1 + r2*(k2 + r2*k3))                     the innermost product first
 *     tx  = (2*p1)*xy + p2*(r2 + 2*xx)
 *     ty  = p1*(r2 + 2*yy) + (2*p2)*xy
 *     xd  = x*rad + tx;  yd = y*rad + ty
 *     sx  = xd*fx_s + cx_s;  sy = yd*fy_s + cy_s
 * roft_rectify_map writes (sx, sy).  The float map's distance from the same formula evaluated in double, with the lens of the
 * engine test (k1 -0.05, k2 0.01, p1 0.001, p2 0.0005, k3 0; source focal lengths x 1.02 / x 0.99, principal point moved by
 * (0.7, -0.4)) and a target focal length of 0.95 x the width: at most 5.6e-6 px at 64 x 48, 9.7e-5 px at 640 x 480, 1.9e-4 px at
 * 1280 x 720 and 2.5e-4 px at 1920 x 1080 -- the rounding of coordinates of that magnitude (recorded, not asserted).
 *
 * NEAREST (depth as Z16 or float, masks, label images; W_s x H_s the source size):
 *     jx = floorf(sx + 0.5f);  jy = floorf(sy + 0.5f)
 *     inside = jx >= 0 && jx <= (float)(W_s-1) && jy >= 0 && jy <= (float)(H_s-1)      in float, before any conversion to an
 *                                                                                      integer: false for anything not finite
 *     out = inside ? src[jy][jx] : 0                          zero is already "no reading" and "background"
 *
 * BILINEAR (8-bit images):
 *     sx or sy not finite: out = 0.  Otherwise x0 = floorf(sx), ax = sx - x0, and the taps are the columns
 *     clamp(x0, 0, W_s-1) and clamp(x0 + 1, 0, W_s-1), clamped in float and then converted; rows likewise (edge-extended, like the
 *     flow producer's images);  top = (1-ax)*p00 + ax*p01,  bot = (1-ax)*p10 + ax*p11,  val = (1-ay)*top + ay*bot,
 *     out = (uint8)fminf(rintf(val), 255).  A colour image rectifies its three channels independently.
 *
 * THE ENGINE.  roft_engine_enable_rectification(e, lens): before the first frame (ROFT_ERR_STATE afterwards), in any order with
 * the other roft_engine_enable_* calls.  The source size must equal roft_config::cam's (ROFT_ERR_INVALID otherwise); the
 * intrinsics may differ.  Equivalence that defines the feature: the engine behaves, bit for bit, as if every frame image it is
 * handed had been replaced by a HOST image holding the operator's product --
 *   - inputs[].depth, float: roft_rectify(ROFT_RECTIFY_F32);
 *   - inputs[].depth on a raw-depth engine with align == 0: the Z16 frame rectified (ROFT_RECTIFY_U16), then converted.  With
 *     align != 0 the depth is NOT touched: the alignment already lands in the pinhole colour camera.  A distorted depth camera of
 *     its own stays unmodelled;
 *   - inputs[].mask: ROFT_RECTIFY_U8; label images: ROFT_RECTIFY_U8 / ROFT_RECTIFY_U16;
 *   - camera images: G_k = roft_rectify(ROFT_RECTIFY_GRAY8) of the gray image of section 3a (the colour conversion is integer
 *     arithmetic, fused into the taps); the flow producer sees a GRAY8 image;
 *   - silhouettes of pose masks are drawn in the pinhole camera and are unaffected; their depth gate, track quality and the outlier
 *     test read the rectified products because they read the frame's depth.  roft_engine_get_depth returns the frame's depth as the
 *     kernels read it on a rectifying engine too.
 * One product is made per distinct pointer, kind and frame however many objects name it, and it lives where, and as long as, a
 * staged HOST image of that frame would (as the raw-depth product does).  HOST images are uploaded once as before, DEVICE images
 * are read in place during the submit call's own enqueued work.  Production goes on the upload stream in front of the depth and the
 * flow production: ONE launch per chunk of ROFT_RECTIFY_CHUNK jobs, every thread evaluating the map once for its four pixels and
 * serving its jobs of the chunk from it (all of them at large images; at small ones the grid deals the jobs out in slices).  An entry that carries inputs[].flow on such an engine is refused with ROFT_ERR_INVALID,
 * nothing consumed: a flow computed between distorted images cannot be rectified, the caller hands the image instead.
 * An engine that does not enable the feature enqueues exactly what it did before.
 *
 * Not modelled: a distorted depth camera of its own (align != 0), the inverse Brown-Conrady form (coefficients that map distorted
 * to ideal points), fisheye and rational models, a source of another size than roft_config::cam on the engine (the stand-alone
 * operators take any), the C++ facade.
 *
 * Refusals of the stand-alone operators, all before a device is looked for (ROFT_ERR_INVALID): a NULL pointer, an unknown kind, a
 * coefficient or intrinsic that is not finite, a focal length <= 0, width or height < 1, width * height >= 2^24 on either side. */
#define ROFT_RECTIFY_GRAY8 1   /* H x W bytes, bilinear */
#define ROFT_RECTIFY_RGB8  2   /* H x W x 3 bytes (any channel order), bilinear per channel */
#define ROFT_RECTIFY_U8    3   /* H x W bytes, nearest: masks, 8-bit label images */
#define ROFT_RECTIFY_U16   4   /* H x W uint16, nearest: Z16 depth, 16-bit label images */
#define ROFT_RECTIFY_F32   5   /* H x W floats, nearest: depth in metres */
#define ROFT_RECTIFY_CHUNK 32  /* jobs one launch of the engine serves */
typedef struct {
    roft_camera cam;           /* the SOURCE (sensor) camera: the size of the distorted frames and their intrinsics */
    double k1, k2, p1, p2, k3; /* OpenCV's order of distCoeffs */
} roft_lens;
/* the source camera = `target`, all coefficients 0: rectifies every image onto itself */
int roft_default_lens(roft_lens* lens, const roft_camera* target);
/* map_out: target H x W x 2 floats (sx, sy).  HOST buffer, device 0. */
int roft_rectify_map(const roft_lens* lens, const roft_camera* target, float* map_out);
/* src: one image of the lens' source size in the layout of `kind` (ROFT_RECTIFY_*); out: the same layout at the target's size.
 * HOST buffers, device 0. */
int roft_rectify(const void* src, int kind, const roft_lens* lens, const roft_camera* target, void* out);
int roft_engine_enable_rectification(roft_engine* e, const roft_lens* lens);
typedef struct {
    long long sources;    /* distinct images taken in (per frame) */
    long long products;   /* rectified images made: one per distinct (image, kind) of a frame */
    long long bytes;      /* source bytes + product bytes of those products */
} roft_engine_rectify_stats;   /* since roft_engine_create */
int roft_engine_get_rectify_stats(roft_engine* e, roft_engine_rectify_stats* out);

/* ---- (3d) track quality: silhouette overlap and depth residual of every estimate --------------------------------------- *
 * The outlier test scores two alternatives, on frames where a delayed pose arrives, against features buffered earlier.  Track
 * quality scores the estimate the engine RETURNS, on every frame (or every `every`-th), against that frame's own mask and depth,
 * on the device: one record per (frame, object).  It is opt-in, reads engine state, writes only its records and changes no result.
 * What a caller does with the numbers (thresholds, "lost", "occluded") is the caller's.
 *
 * Symbols.  (x, q): the frame's final estimate, pose[6..12] of its log row (roft_engine_get_log).  M: the frame's propagated,
 * binarised mask -- what roft_get_mask returns after the frame.  D: the frame's float depth as the engine used it (with raw depth
 * enabled: the converted / aligned product, roft_engine_get_depth).  d: the engine's render divider (2 when the image is 640 wide,
 * else 4; roft_track_quality: the argument).  w = W / d, h = H / d (integer division).  R: the h x w depth tile of the mesh at
 * (x, q) under ROFT_RENDER_CONTRACT -- bit for bit roft_render_depth(mesh, x, q, cam, d): the back-face rule for closed meshes,
 * 0 = background.  An object added without a mesh has R = 0 everywhere.
 * Every sum runs over the image pixels (u, v), 0 <= u < W, 0 <= v < H, with u / d < w and v / d < h; the render value of a pixel is
 * r = R[v / d][u / d] (the mapping of the outlier test's likelihood); pixels with u / d >= w or v / d >= h (H or W not a multiple
 * of d) have no render value: they count for n_mask only.
 *
 * Operation by operation:
 *   n_mask    pixels of the WHOLE image with M != 0
 *   n_render  pixels with r != 0
 *   n_both    pixels with M != 0 and r != 0
 *   n_depth   pixels of n_both whose D is valid: D > 0 and (double)D < depth_maximum; a NaN fails both comparisons
 *   for those: e = D - r, ONE float subtraction;  n_front counts e < -depth_tolerance, n_behind counts e > +depth_tolerance
 *              (float comparisons; e == -+depth_tolerance exactly is neither)
 *   S         the sum of |e| over n_depth, exact: each term t = min((double)|e|, 256.0) is split into two integers
 *                 hi = floor(t * 2^32),   lo = (integer part of) (t * 2^32 - hi) * 2^32
 *             -- units of 2^-32 m and 2^-64 m; for every float t >= 2^-41 both products are exact and hi 2^-32 + lo 2^-64 == t;
 *             a smaller t loses what lies below 2^-64 --, and HI = sum of hi, LO = sum of lo are 64-bit integer sums: they depend
 *             neither on the order of the terms nor on how the device spreads them over threads
 *   depth_err value(HI, LO) / (double)n_depth with
 *                 value(HI, LO) = (double)HI * 2^-32 + (double)LO * 2^-64
 *             in double arithmetic exactly as written: two conversions (round to nearest even), two multiplications by powers of
 *             two (exact), one addition, one division.  DBL_MAX when n_depth == 0.
 * So a record is a function of (x, q), M, D, the mesh, the camera, d, depth_tolerance and depth_maximum alone: equal inputs give
 * equal bits, whatever the batch shape, the stream layout or the launch shape.
 *
 * Engine.  roft_engine_enable_quality: before the first frame (else ROFT_ERR_STATE); the output log must be enabled first
 * (ROFT_ERR_STATE) -- the kernel reads the estimates where the step wrote them --, with a capacity of at least the frames that can
 * be in flight, (batches in flight) x max_batch_frames = 6 for one-frame engines and 5 x max_batch_frames otherwise: a smaller log
 * is refused with ROFT_ERR_INVALID and the error string names the least capacity.  The quality ring has the log's capacity; while
 * quality is on, roft_engine_enable_log with another capacity is ROFT_ERR_STATE.  every >= 1, depth_tolerance finite and >= 0, else
 * ROFT_ERR_INVALID.  An engine with render_mode == ROFT_RENDER_GL is refused with ROFT_ERR_INVALID: it keeps its meshes unsorted
 * and without the flip bits of the back-face rule, so the contract's render does not exist there.  depth_maximum is
 * roft_config::depth_maximum.  A frame gets records when frame % every == 0 (frame: the engine's frame counter, from 0); the rows
 * of other frames carry frame = -1 and zeros.
 * roft_engine_get_quality: syncs; out[n_frames][n_objects]; it accepts exactly the frame ranges roft_engine_score_log accepts --
 * first_frame >= 0, n_frames >= 0, the range stepped and still in the ring -- else ROFT_ERR_INVALID.
 * roft_track_quality: the engine's kernel on HOST buffers for one object (device 0): depth, mask H x W; M is the object plane the
 * engine's ingest makes of the byte mask, the pixels of value > 1 (a delivered mask's 0 and 1 are not the object); mesh may have 0
 * triangles;
 * window_pixels > 0 caps the kernel's LDS depth window (a larger window is drawn in strips: no bit changes), 0: the engine's shape.
 * out->frame is 0.  ROFT_ERR_INVALID before any device is looked for: a NULL pointer, divider <= 0, a negative or NaN
 * depth_tolerance, window_pixels < 0. */
typedef struct {
    int32_t frame;     /* engine frame counter of the record; -1: no record for this (frame, object) */
    int32_t n_mask;    /* pixels with M != 0 (over the WHOLE image, also outside the render's window) */
    int32_t n_render;  /* pixels with r != 0 */
    int32_t n_both;    /* both: overlap = n_both / (n_mask + n_render - n_both) is the caller's to form */
    int32_t n_depth;   /* pixels of n_both with D > 0 and (double)D < depth_maximum (NaN fails both) */
    int32_t n_front;   /* of those, e = D - r (float) < -depth_tolerance: something stands in front of the object */
    int32_t n_behind;  /* of those, e > +depth_tolerance: the surface is not where the estimate puts it */
    int32_t reserved;  /* 0 */
    double  depth_err; /* (sum of |e| over n_depth) / n_depth, DBL_MAX when n_depth == 0 */
} roft_quality_record;  /* 40 bytes */
typedef struct {
    int   every;            /* records on frames with frame % every == 0; default 1 */
    float depth_tolerance;  /* metres; default 0.01f */
} roft_quality_params;
int roft_default_quality_params(roft_quality_params* p);
int roft_engine_enable_quality(roft_engine* e, const roft_quality_params* p);   /* NULL = defaults */
int roft_engine_get_quality(roft_engine* e, int first_frame, int n_frames, roft_quality_record* out);
int roft_track_quality(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask, const roft_mesh* mesh,
                       const double x[3], const double q[4], float depth_tolerance, double depth_maximum, int window_pixels,
                       roft_quality_record* out);

/* ---- (3e) masks from poses: the silhouette of a delivered pose as the frame's mask ---------------------------------------- *
 * A caller with a pose estimator and a mesh but no segmentation network (DOPE, the reference's own pose source, delivers no masks)
 * enrols its objects, and the engine draws the mask itself, on the device, from what the submit call was handed: the object's mesh
 * is resident, the pose travels with the frame.  The equivalence below DEFINES the feature.
 *
 * roft_engine_enable_pose_masks(e, obj_ids, n_ids): after the objects it names were added, before the first frame.  n_ids == 0
 * (obj_ids may be NULL) enrols every object the engine has at its first frame.  It may be called more than once; the sets add up.
 *
 * For an enrolled object and a frame whose entry has mask == NULL and names no label image:
 *  - if inputs[].pose_valid, the engine behaves BIT FOR BIT as if inputs[].mask had been a HOST buffer holding
 *        M(p) = roft_render_depth(mesh, pose_x, pose_q, cam, 1)(p) > 0 ? 255 : 0
 *    -- the render contract at FULL resolution (divider 1), pose_q exactly as submitted (not normalised), the back-face rule for
 *    closed meshes (a closed mesh is drawn whole as soon as one vertex is not in front of the near plane), and a pixel counts only
 *    if its computed z > 0.  Whether roft_config::use_pose lets the filter use the pose does not matter;
 *  - on the object's FIRST frame without pose_valid the pose is roft_object_desc::p_mean0[6..12] (the reference initialises from
 *    the first detection);
 *  - otherwise no mask is delivered on that frame.
 * Everything downstream is what it is for a delivered mask: the first-mask rule; the "new but empty mask is ignored" rule
 * (ImageSegmentationOFAidedSource.hpp:186-198) for a pose off-screen or behind the camera; the chase through the last
 * mask_frames_between buffered flows -- a pose computed on an older image is chased like a delayed network mask, so a delayed pose
 * source wants mask_frames_between == pose_frames_between --; features, outlier test, quality records, roft_get_mask.
 * A delivered mask or label image takes precedence on any frame, so network masks and silhouettes may alternate for one object;
 * enrolled objects, plain-mask objects and label-image objects mix within one frame.  An object added without a mesh has an empty
 * silhouette; with n_ids == 0 such objects are not enrolled.
 *
 * LIMIT.  The silhouette is drawn from the pose MEASUREMENT, before any filtering: an outlier pose (the reference's data has them,
 * 30 degrees off) yields a wrong mask until the next pose arrives.  The UKF's outlier rejection protects the estimate, not the mask.
 * Nothing is dilated.  Objects hide each other's silhouettes only where the caller says they share a scene (below).
 *
 * Refused on the host, with nothing consumed and the reason in roft_last_error_string: ROFT_ERR_STATE after the first frame;
 * ROFT_ERR_INVALID for an id that is not an object of the engine, for an object added without a mesh, for an engine with
 * stamped_masks (a pose carries no stamp), and for an engine with render_mode == ROFT_RENDER_GL (its meshes are uploaded without
 * the flip bits of the back-face rule: the defining render does not exist there).
 *
 * roft_pose_silhouette: the same kernel on HOST buffers, device 0: mask_out H x W bytes {0, 255} (optional), count_out the number
 * of set pixels (optional).  bands: workgroups (bands of image rows) the image is split into, 0 = the library's choice;
 * vertex_cache: 1 = the projected vertices are kept in LDS where the mesh fits, 0 = projected per triangle.  Neither changes a
 * bit (the result is an order-free OR).  ROFT_ERR_INVALID before any device is looked for: a NULL camera, mesh, x or q, bands < 0,
 * a vertex_cache that is neither 0 nor 1, a triangle that names a vertex outside the vertex array. */
typedef struct {
    long long silhouettes;   /* (frame, object) pairs whose mask the engine drew */
    long long frames;        /* frames in which it drew at least one */
} roft_engine_pose_mask_stats;
int roft_engine_enable_pose_masks(roft_engine* e, const int* obj_ids, int n_ids);
int roft_engine_get_pose_mask_stats(roft_engine* e, roft_engine_pose_mask_stats* out);
int roft_pose_silhouette(const roft_camera* cam, const roft_mesh* mesh, const double x[3], const double q[4], int bands, int vertex_cache,
                         uint8_t* mask_out, int* count_out);

/* ---- (3e, continued) enrolled objects of one scene hide each other ----------------------------------------------------------- *
 * Two objects that overlap in the image both own the overlap as plain silhouettes: the rear object's flow samples, features,
 * outlier likelihood and quality records are then taken on the front object.  Opt-in: objects the caller declares to share a scene
 * are drawn against a common z-buffer, and each keeps only the pixels where it is the nearest surface.  Off, the engine enqueues
 * exactly what it does without this call.
 *
 * roft_engine_enable_pose_mask_occlusion(e, obj_ids, scene_ids, n_ids): after roft_engine_enable_pose_masks, before the first frame.
 * scene_ids[i] >= 0 names the scene of obj_ids[i]; n_ids == 0 (NULL arrays allowed) puts every object enrolled at the time of the
 * call into scene 0 (the shared-scene deployment).  A later call replaces an object's scene.  An enrolled object that is never named
 * is a scene of its own and is drawn exactly as without the mode.
 *
 * THE RESOLVED MASK.  For a frame t and a scene s let D be the objects of s whose mask on frame t is a silhouette (the pairs the
 * rules above give a silhouette, a first frame drawn from p_mean0 included).  For i in D let
 *        R_i = roft_render_depth(mesh_i, pose_x_i, pose_q_i, cam, 1)
 * (the float image, the pose exactly as above).  The engine behaves BIT FOR BIT as if object i had been handed the HOST mask
 *        M_i(p) = 255  when R_i(p) > 0 and for every other j in D:  R_j(p) == 0,  or R_i(p) < R_j(p),  or R_i(p) == R_j(p) and i < j
 *        M_i(p) = 0    otherwise
 * -- float comparisons on the rendered values; on an exact tie the lower object id keeps the pixel.  The masks of D are disjoint
 * and their union is the union of the plain silhouettes.
 *  - An object whose mask arrives another way on that frame (a delivered mask, a label image, no pose delivered) is not in D: it
 *    neither hides nor is hidden.
 *  - Objects of other scenes do not interact.
 *  - A silhouette that loses every pixel is a "new but empty mask" and is ignored by the existing rule: the object keeps
 *    propagating its last mask.
 *  - Downstream, everything is what it is for a delivered mask.
 *  - roft_engine_pose_mask_stats keeps its meaning: silhouettes are counted whether hidden or not.
 * LIMITS.  Only enrolled objects with silhouettes on the same frame hide each other: hands, clutter and plain-mask objects do not.
 * Those are what the depth gate below removes (roft_engine_enable_pose_mask_depth_gate: the silhouettes compared with the depth of
 * the image the pose was computed on -- a delayed pose belongs to an older image than the frame that carries it).
 * Memory: one z-buffer of width x height x 8 bytes per scene with at least two members, times 2 x ROFT_MAX_BATCH_FRAMES, allocated
 * by this call; nothing grows on the hot path.
 *
 * Refused on the host, with nothing consumed and the reason in roft_last_error_string: ROFT_ERR_STATE after the first frame or
 * when pose masks are not enabled; ROFT_ERR_INVALID for an id that is not an object of the engine, an id that is not enrolled
 * (explicitly or through enrol-all), a negative scene id, n_ids < 0, n_ids > 0 with a NULL array.
 *
 * roft_engine_get_pose_mask_occlusion_stats: waits for the batches stepped so far (hidden and pixels_removed are counted on the device).
 *
 * roft_pose_silhouettes_occluded: the same kernels on HOST buffers, device 0, ONE scene of n meshes (object id = index): masks_out
 * n x H x W bytes {0, 255} (optional), counts_out n pixel counts (optional).  bands and vertex_cache as for roft_pose_silhouette;
 * they change no bit (a per-pixel minimum and an equality test are order-free).  With n == 1 it is roft_pose_silhouette.
 * ROFT_ERR_INVALID before any device is looked for: a NULL cam, meshes, x or q, n < 1 or n > ROFT_SCENE_MAX_INSTANCES (256),
 * bands < 0, a vertex_cache that is neither 0 nor 1, a triangle that names a vertex outside its mesh. */
typedef struct {
    long long resolved;        /* (frame, object) silhouettes drawn against at least one other object of their scene */
    long long hidden;          /* of those, silhouettes that had pixels and lost every one */
    long long pixels_removed;  /* pixels the plain silhouettes had and the resolved ones have not */
} roft_engine_pose_mask_occlusion_stats;
int roft_engine_enable_pose_mask_occlusion(roft_engine* e, const int* obj_ids, const int* scene_ids, int n_ids);
int roft_engine_get_pose_mask_occlusion_stats(roft_engine* e, roft_engine_pose_mask_occlusion_stats* out);
int roft_pose_silhouettes_occluded(const roft_camera* cam, const roft_mesh* meshes, int n, const double* x /* [n][3] */,
                                   const double* q /* [n][4] */, int bands, int vertex_cache,
                                   uint8_t* masks_out /* [n][H][W], optional */, int* counts_out /* [n], optional */);

/* ---- (3e, continued) silhouettes gated against the depth of the pose's own frame ------------------------------------------------ *
 * A network mask leaves out the hand that holds the object; a drawn silhouette paints it in, and the engine then samples the hand's
 * flow and takes features and quality records on it.  Opt-in: every silhouette the engine draws is compared, pixel by pixel, with a
 * depth image the engine already holds, and loses the pixels where the sensor saw something clearly nearer (or, optionally, clearly
 * farther) than the rendered surface.  Off, the engine enqueues exactly what it does without this call; on, it adds no launch.
 *
 * THE KEEP PREDICATE.  With tf = front_tolerance, tb = behind_tolerance, R a rendered depth and D a sensor depth, all floats,
 *        keep(R, D) = !(D > 0.0f && D < R - tf) && !(tb > 0.0f && D > R + tb)
 * -- R - tf and R + tb each rounded once to float, nothing contracted.  A NaN depth keeps the pixel; so does a depth of 0 (the
 * sensor's "no reading").  No pixel fails both tests; pixels_front counts the first, pixels_behind the second.
 *
 * A PAIR DRAWN ALONE.  For an enrolled object and a frame on which its mask is a silhouette (the rules above: a delivered pose, or
 * p_mean0 on the first frame of a track) the engine behaves BIT FOR BIT as if the object had been handed the HOST mask
 *        M'(p) = (R(p) > 0 && keep(R(p), D_g(p))) ? 255 : 0,      R = roft_render_depth(mesh, pose_x, pose_q, cam, 1).
 * A PAIR OF A SCENE (roft_engine_enable_pose_mask_occlusion):
 *        M'_i(p) = (M_i(p) == 255 && keep(R_i(p), D_g,i(p))) ? 255 : 0
 * with M_i the resolved mask above.  The resolve is decided by the renders alone: a pixel the gate removes still hides the objects
 * behind it.  Each object uses the depth of its own gate frame.
 *
 * THE GATE FRAME g.  A pose that arrives on frame k was computed on an older image.  Let n be the number of buffered flows the chase
 * of this new mask uses (the last mask_frames_between of the flows buffered since the mask before, all of them when that number is
 * not given; 0 under the first-mask rule).  n == 0: g is frame k itself.  Otherwise g is the object's frame just before the frame
 * that delivered the oldest of those n flows -- frame k - n with a complete flow stream, the image a delayed pose source grabbed;
 * with dropped flow frames, the frame the chase itself starts from.  D_g is the float image the engine holds for that frame: with
 * roft_engine_enable_raw_depth the converted or aligned one (roft_depth_convert / roft_depth_align give the same bytes).  The engine
 * keeps that image as long as the flow (a clone where the flow is cloned); roft_engine_retain_frames() does not change -- the image
 * is one frame older than its flow, and the window's margin of two frames covers it.
 * The host counts the buffered flows as if every delivered mask had pixels (it cannot see an empty one): after a silhouette that was
 * empty, or emptied, on an engine with mask_frames_between > 0 the next chase may use more flows than the gate frame assumes.
 *
 * Downstream, everything is what it is for a delivered mask.  A silhouette the gate empties is a "new but empty mask", ignored by the
 * existing rule: the object goes on with its propagated mask.  roft_engine_pose_mask_stats keeps its meaning.  The gate applies to
 * every enrolled object of the engine; a delivered mask or label image is never gated.  roft_objects_restart starts a new history: the
 * first silhouette of the new track is gated against its own frame.
 *
 * OUT OF SCOPE.  No verdict and no loss policy: the counts are the caller's to judge.  Delivered masks are not gated.  One pair of
 * tolerances per engine.  stamped_masks and ROFT_RENDER_GL engines are refused for pose masks already.  The C++ facade has no switch.
 *
 * roft_engine_enable_pose_mask_depth_gate(e, g): after roft_engine_enable_pose_masks, before the first frame; g == NULL: the defaults
 * (0.02, 0).  Refused on the host, with nothing consumed and the reason in roft_last_error_string: ROFT_ERR_STATE after the first frame
 * or when pose masks are not enabled; ROFT_ERR_INVALID for a front_tolerance that is not finite or not > 0, a behind_tolerance that
 * is NaN or infinite.
 * roft_engine_get_pose_mask_gate_stats: waits for the batches stepped so far (all but `gated` are counted on the device).
 *
 * roft_pose_silhouettes_gated: the same kernels on HOST buffers, device 0, ONE scene of n meshes and ONE depth image: with n == 1 the
 * pair drawn alone, with n > 1 the resolve followed by the gate.  removed_out[i] = {front, behind} of object i.  bands and
 * vertex_cache change no bit.  ROFT_ERR_INVALID before any device is looked for: a NULL cam, meshes, x, q, depth or g, n < 1 or
 * n > ROFT_SCENE_MAX_INSTANCES, bands < 0, a vertex_cache that is neither 0 nor 1, a triangle that names a vertex outside its mesh,
 * tolerances as above. */
typedef struct {
    float front_tolerance;    /* metres, finite, > 0: a valid depth more than this in FRONT of the rendered surface is an occluder */
    float behind_tolerance;   /* metres; > 0: a depth more than this BEHIND the rendered surface means the object is not there; <= 0: test off */
} roft_pose_mask_gate;
int roft_default_pose_mask_gate(roft_pose_mask_gate* g);                 /* 0.02f, 0.0f */
int roft_engine_enable_pose_mask_depth_gate(roft_engine* e, const roft_pose_mask_gate* g);
typedef struct {
    long long gated;           /* (frame, object) silhouettes compared with a depth image */
    long long emptied;         /* of those, silhouettes that had pixels and lost every one to the gate */
    long long pixels_front;    /* pixels removed as occluded */
    long long pixels_behind;   /* pixels removed by the behind test (and not by the front test) */
} roft_engine_pose_mask_gate_stats;
int roft_engine_get_pose_mask_gate_stats(roft_engine* e, roft_engine_pose_mask_gate_stats* out);
int roft_pose_silhouettes_gated(const roft_camera* cam, const roft_mesh* meshes, int n, const double* x /* [n][3] */,
                                const double* q /* [n][4] */, const float* depth /* H x W, HOST */, const roft_pose_mask_gate* g,
                                int bands, int vertex_cache, uint8_t* masks_out /* [n][H][W], optional */,
                                int* counts_out /* [n], optional */, int* removed_out /* [n][2]: front, behind; optional */);

/* ---- (3b) scene renderer: tracked poses drawn over the camera frames ----------------------------------------------
 * The reference's evaluation draws the mesh at every estimated pose over the grayed camera frame (evaluation/results_renderer.py:
 * 591-778 through tools/object_renderer/src/renderer.cpp).  This is that stage for many frames and several objects per frame:
 * n_instances meshes per frame, each at its own pose, hiding each other; per pixel the nearest surface's eye-space depth, the
 * instance and the triangle (in the caller's triangle order) it belongs to, and a flat-shaded overlay on the camera image.
 *
 * Geometry is the render contract (ROFT_RENDER_CONTRACT above, oracle/ro_render.c) at full resolution, operation for operation:
 * the depth map of a scene is the per-pixel minimum of what roft_render_depth(mesh, x, q, cam, 1, ...) draws for its instances.
 * Among equal depths the lower instance wins, then the lower triangle index.  The quaternion is used as given (not normalised),
 * as in roft_pose_errors.  A pose with a non-finite component, or valid[...] == 0, draws nothing for that instance.
 *
 * Colour (float arithmetic, this operation order, no contraction): P_k = the triangle's corners in the camera frame as the contract
 * computes them, n = (P1 - P0) x (P2 - P0), s = |n_z| / sqrt((n_x^2 + n_y^2) + n_z^2) (0 when the length is 0 or not finite: a head
 * light, two-sided), level = ambient + (1 - ambient) s, per channel c = opacity (tint_c level) + (1 - opacity) background_c,
 * out = (uint8) min(max(floorf(c + 0.5f), 0), 255).  The background is the camera image, RGB; with gray_background each pixel
 * becomes (R 4899 + G 9617 + B 1868 + 8192) >> 14 in all three channels (the reference applies COLOR_RGB2GRAY to a BGR image,
 * which swaps the weights of R and B; these are the weights of the channels as named).  No background: zeros.
 *
 * Determinism contract: the outputs of frame f are a function of that frame's poses, validity flags and background, of the meshes,
 * the styles and the camera.  They do not depend on n_frames, on the frame's position in the call, on other frames, on
 * window_pixels or on the run: every pixel is the minimum of a fixed set of 64-bit keys, whatever order they are produced in.
 *
 * Every buffer is host memory.  Without a HIP device: ROFT_ERR_INVALID for a bad argument, ROFT_ERR_DEVICE otherwise. */
typedef struct {
    float tint[3];  /* colour of the lit surface, 0..255 per channel (R, G, B) */
    float opacity;  /* 0..1: weight of the surface over the background */
    float ambient;  /* 0..1: level of a surface seen edge-on */
} roft_scene_style;

#define ROFT_SCENE_MAX_INSTANCES 256

typedef struct {
    int n_frames;            /* 0: nothing is done, ROFT_OK */
    int n_instances;         /* 0 .. ROFT_SCENE_MAX_INSTANCES objects per frame (0: the background alone) */
    const int* mesh_index;   /* [n_instances] index into the renderer's meshes */
    const double* poses;     /* [n_frames][n_instances][7]: x y z, q = w x y z */
    const uint8_t* valid;    /* [n_frames][n_instances], 0 = not drawn; NULL: all drawn */
    const uint8_t* background; /* [background_frames][H][W][3] RGB, or NULL */
    int background_frames;   /* n_frames, or 1: the same image under every frame */
    int gray_background;     /* != 0: the background is converted to gray first */
    const roft_scene_style* styles; /* [n_instances], or NULL: ambient 0.35, opacity 0.75, tint from a palette of eight by instance % 8 */
    int window_pixels;       /* 0: the library's choice; > 0: at most this many pixels per on-chip window (tests: forces strips).  Changes no bit. */
} roft_scene_desc;

typedef struct roft_scene_renderer roft_scene_renderer;
/* Uploads the meshes once, in the caller's order (each non-empty, fewer than 2^24 triangles).  Any width, height >= 1 with
 * width * height < 2^24.  max_frames_per_call 1 .. 65536 sizes the resident buffers. */
int roft_scene_renderer_create(const roft_camera* cam, const roft_mesh* meshes, int n_meshes, int max_frames_per_call, int device,
                               roft_scene_renderer** out);
int roft_scene_renderer_destroy(roft_scene_renderer* r);
/* Any output may be NULL.  rgb_out [n_frames][H][W][3] u8; depth_out [n_frames][H][W] float, 0 = background;
 * instance_out / triangle_out [n_frames][H][W] int32, -1 = background. */
int roft_scene_render(roft_scene_renderer* r, const roft_scene_desc* desc, uint8_t* rgb_out, float* depth_out, int32_t* instance_out,
                      int32_t* triangle_out);
/* create + render + destroy on device 0 */
int roft_render_scene(const roft_camera* cam, const roft_mesh* meshes, int n_meshes, const roft_scene_desc* desc, uint8_t* rgb_out,
                      float* depth_out, int32_t* instance_out, int32_t* triangle_out);

/* ---- (3h) symmetric objects: equivalent poses in the pose UKF, MSSD / MSPD scores ------------------------------------------------- *
 * A pose source returns, for a box or a can, any of the object's equivalent orientations, and which one changes from delivery to
 * delivery.  Taken as given, a delivery that is the same pose up to a half turn of the object enters the UKF as a half-turn
 * innovation, and the outlier test cannot reject it: the alternative renders the same depth.  An object may therefore be given its
 * discrete symmetry group; the filter then replaces a delivered pose by its equivalent nearest to the belief it corrects, and the
 * evaluation has BOP's MSSD and MSPD next to ADD / ADD-S.  Opt-in: an engine that never names a group enqueues and computes exactly
 * what it did before.
 *
 * THE GROUP.  n elements, each a rigid transform of the object frame as 7 doubles `x y z, w x y z` (the row layout of
 * roft_pose_errors).  If (x, q) is a pose of the object, so is (x + R(q) t_g, q (x) g).  Host checks, ROFT_ERR_INVALID with the reason
 * in roft_last_error_string, made before a device is looked for: 1 <= n <= ROFT_MAX_SYMMETRIES for the filter and the selection
 * operator, 1 <= n <= ROFT_MAX_SCORE_SYMMETRIES for scoring; element 0 exactly the identity 0 0 0 1 0 0 0; every component finite;
 * | |q_g|^2 - 1 | <= 1e-6 for every element.  Closure is not checked.
 *
 * THE SELECTION RULE (roft_amd/csrc/symmetry.h: the kernel and the operator compile the same text).  Double precision, every product
 * and every sum one rounded operation, no fused multiply-add.  For a belief quaternion qh, a measurement (x, m), quaternions w x y z:
 *   p_g = m (x) g, the Hamilton product, the four terms of a component summed left to right:
 *       p.w = m.w g.w - m.x g.x - m.y g.y - m.z g.z        p.x = m.w g.x + m.x g.w + m.y g.z - m.z g.y
 *       p.y = m.w g.y - m.x g.z + m.y g.w + m.z g.x        p.z = m.w g.z + m.x g.y - m.y g.x + m.z g.w
 *   c_g = | qh.w p.w + qh.x p.x + qh.y p.y + qh.z p.z |, summed left to right; a c_g that is NaN counts as -1.
 *   g* = the element with the largest c_g, the lowest index among equal ones: the identity wins a tie.
 *   g* = 0: the measurement is returned BIT FOR BIT AS GIVEN -- no product, no sign change (a measurement in the opposite hemisphere
 *       of qh stays there, as it does without a group).
 *   otherwise m' = p_g*, negated in all four components when qh . m' < 0 (the same four-term sum), and
 *       x' = x + R(m) t_g*:  x'_i = x_i + (R_i0 t_0 + R_i1 t_1 + R_i2 t_2), R(m) in the operation order of roft_pose_errors' matrices:
 *       R00 = 1 - 2 (yy + zz)  R01 = 2 (xy - wz)      R02 = 2 (xz + wy)
 *       R10 = 2 (xy + wz)      R11 = 1 - 2 (xx + zz)  R12 = 2 (yz - wx)
 *       R20 = 2 (xz - wy)      R21 = 2 (yz + wx)      R22 = 1 - 2 (xx + yy)        (m as given, not normalised)
 * roft_pose_nearest_equivalent is that rule as a stand-alone operator in HOST arithmetic: it needs no device and looks for none.
 * index_out (may be NULL) receives g*.  x_out / q_out may alias x / q.
 *
 * THE ENGINE.  roft_object_set_symmetry gives object obj_id the group sym[n_sym][7]; n_sym 0 or 1: none (sym may be NULL for 0).
 *  - Callable before the first frame and later.  On a running engine it WAITS for every stepped batch exactly as roft_sync does and
 *    is served by plain copies on the idle engine, as roft_objects_restart is; the launch graph of a batch does not know about it.
 *    It takes effect from the next submitted frame.  (A call that sets none on an object that has none returns at once.)
 *  - ROFT_ERR_INVALID, before a device is looked for: NULL engine, a bad group, n_sym < 0, an id outside the engine's objects.
 *    ROFT_ERR_STATE: a submitted batch that has not been stepped.  A refused call changes nothing.
 *  - roft_object_desc and ROFT_ABI_VERSION are unchanged: the group has an entry point, not a field.
 *  - roft_objects_restart DROPS a slot's group when it replaces the mesh (the group describes the mesh) and KEEPS it with
 *    ROFT_RESTART_KEEP_MESH.
 *  - In the step: when the object has a group of more than one element and one of a UKF step's corrections carries the pose
 *    (type & ROFT_MEAS_POSE), the rule runs once, after the step's prediction and before its corrections, with qh = the quaternion of
 *    the belief the correction is applied to -- the buffered belief in a re-synchronisation step, the prediction otherwise.  Both
 *    corrections of an outlier-rejection step see the same rewritten measurement.
 *  - What does not change: pose masks draw the silhouette of the pose AS DELIVERED (an equivalent pose has the same silhouette);
 *    quality records and the log's columns.  No counter is added: a pose step can be executed by more than one lane and lineage, so
 *    a per-object "remapped" count needs a design of its own.  The C++ class facade (include/ROFT) gets no switch for it.
 *
 * SCORES.  roft_pose_errors_sym: for n_poses pose pairs over one point set, on the device, in double precision,
 *   p' = R_g p_i + t_g,  a = R_r p' + t_r,  b = R_e p_i + t_e     each row R_i0 p_0 + R_i1 p_1 + R_i2 p_2 + t_i, left to right, the matrices
 *                                                                 as above, quaternions as given
 *   ROFT_POSE_ERROR_MSSD  sqrt( min_g max_i ( (b-a)_x^2 + (b-a)_y^2 + (b-a)_z^2 ) )                    metres
 *   ROFT_POSE_ERROR_MSPD  the same over u = fx X / Z + cx, v = fy Y / Z + cy of a and b ((du)^2 + (dv)^2)   pixels; needs cam
 * MSPD: a pose pair that puts any point at Z <= 0 on either side, under any element, gives +inf.  A non-finite pose gives a
 * non-finite result and changes no other entry.  Determinism: the contract of roft_pose_errors -- out[f] is a function of (kind,
 * points, group, camera, pose pair f) alone; max and min are exact, there are no atomics.
 * ROFT_ERR_INVALID before a device is looked for: unknown kind, NULL pointer, n_points <= 0, n_poses < 0, a bad group, MSPD without
 * a camera (or with non-finite intrinsics; width and height are not read).  n_poses == 0 is ROFT_OK and touches nothing.
 * roft_engine_score_log_sym: the same for the poses of one object in the log, read in place, with the contract, the frame-range rules
 * and the points == NULL case (the slot's current mesh) of roft_engine_score_log; MSPD projects with the engine's camera.  Equal, bit
 * for bit, to roft_pose_errors_sym on the rows roft_engine_get_log_rows returns. */
#define ROFT_MAX_SYMMETRIES 16
#define ROFT_MAX_SCORE_SYMMETRIES 256
#define ROFT_POSE_ERROR_MSSD 2   /* metres */
#define ROFT_POSE_ERROR_MSPD 3   /* pixels; needs cam */
int roft_pose_nearest_equivalent(const double* sym, int n_sym, const double qh[4], const double x[3], const double q[4], double x_out[3],
                                 double q_out[4], int* index_out);
int roft_object_set_symmetry(roft_engine* e, int obj_id, const double* sym, int n_sym);
int roft_pose_errors_sym(int kind, const double* points, int n_points, const double* est, const double* ref, int n_poses, const double* sym,
                         int n_sym, const roft_camera* cam, double* out);
int roft_engine_score_log_sym(roft_engine* e, int kind, int obj_id, int first_frame, int n_frames, const double* points, int n_points,
                              const double* ref, const double* sym, int n_sym, double* out);

/* ---- (3i) VSD scores: BOP's third pose error, against the sensor's depth image ------------------------------------------------------ *
 * BOP scores a 6D pose method by the mean of three recalls: MSSD and MSPD (section 3h) and VSD, the Visible Surface Discrepancy --
 * the only one that looks at the depth image: an estimate hidden behind a hand is not punished for what nobody could see, and
 * symmetric views need no symmetry group.  roft_pose_errors_vsd computes it for n_poses pose pairs of one mesh on the device: two
 * depth renders per pair, which never leave the chip, and one pass over the pair's depth image.
 *
 * Inputs.  est / ref: rows of 7 doubles x y z, w x y z; the quaternion is used as given.  depth: [n_depth][height][width] floats,
 * metres, HOST memory, 0 = no measurement; n_depth = n_poses (image f belongs to pair f) or 1 (one image under every pair).
 *
 * For pose pair f, with D_t its depth image:
 *  - Renders.  D_e and D_g are what roft_render_depth(mesh, x, q, cam, 1, ..) draws for the estimated and the reference pose: the
 *    render contract, back-face rule included, 0 = background (at ANY width >= 1, as the scene renderer draws; roft_render_depth
 *    itself wants a multiple of 32).  A pose with a non-finite component draws nothing, as in the scene renderer.
 *  - Distance images (BOP's depth_im_to_dist_im_fast), in double, every operation rounded once, no contraction: for pixel (i, j) --
 *    column i, row j -- and depth d (float, promoted)
 *        a = (i - cx) / fx,  b = (j - cy) / fy,  dist = sqrt(((a d)^2 + (b d)^2) + d^2)
 *    give T, G and E from D_t, D_g and D_e.
 *  - Visibility (BOP's mode `bop19`).  For a model image M in {G, E}: diff = (float)M - (float)T, in float;
 *        vis(M) = (T > 0 && M > 0 && diff <= delta) || (T == 0 && M > 0);    V_g = vis(G);    V_e = vis(E) || (V_g && E > 0).
 *    A NaN depth pixel is neither a measurement nor a hole: it fails every comparison, and hides nothing and shows nothing.  The
 *    distance of a NEGATIVE depth is that of its magnitude (the squares), so the formulas take such a pixel for a measurement, as BOP's
 *    code does; a caller who means "no measurement" writes 0.
 *  - Counts.  n_union = |V_g u V_e|, n_inter = |V_g n V_e|, n_gt = |V_g|, n_est = |V_e|, fail[k] = the pixels of V_g n V_e with
 *    c >= taus[k] in double, c = |G - E| / diameter when diameter > 0, else c = |G - E| undivided.
 *  - Errors (BOP's cost `step`).  errors_out[f][k] = (double)(fail[k] + n_union - n_inter) / (double)n_union; 1.0 for every k when
 *    n_union == 0.  counts_out (optional) row f: n_union, n_inter, n_gt, n_est, fail[0 .. n_taus).
 *
 * Determinism: the contract of roft_pose_errors.  Row f is a function of the camera, the mesh, the parameters, pose pair f and its
 * depth image alone -- not of n_poses, the pair's position in the call, n_depth, window_pixels, strips or the run: every figure is a
 * sum of integers.
 *
 * ROFT_ERR_INVALID, the reason in roft_last_error_string, before a device is looked for: a NULL pointer other than counts_out;
 * n_poses < 0; n_depth neither 1 nor n_poses when n_poses > 0; n_taus outside 1 .. ROFT_VSD_MAX_TAUS; a tau that is not finite or not
 * > 0; delta or diameter negative or not finite; window_pixels < 0; a mesh the other operators refuse (no vertices or triangles, a
 * NULL array, an index out of range); width * height outside what the scene renderer accepts (each >= 1, the product < 2^24); an
 * image row wider than the kernel's two on-chip depth windows (about 19 000 pixels).  n_poses == 0 is ROFT_OK and touches nothing.
 * Without a device a well-formed call returns ROFT_ERR_DEVICE: there is no CPU path.
 *
 * Not in scope: BOP's cost `tlinear` and its visibility mode `bop18`; a roft_engine_score_log form (the engine does not keep a
 * sequence's depth frames); several objects in one VSD render (the other objects of a scene enter through the depth image only); the
 * C++ class facade (include/ROFT). */
#define ROFT_VSD_MAX_TAUS 16
typedef struct {
    float  delta;          /* metres; tolerance of the visibility test (BOP19: 0.015) */
    int    n_taus;         /* 1 .. ROFT_VSD_MAX_TAUS */
    double taus[ROFT_VSD_MAX_TAUS];  /* misalignment tolerances; in units of `diameter` when it is > 0, else metres */
    double diameter;       /* metres; 0: distances are not normalised */
    int    window_pixels;  /* 0: the library's choice; > 0: at most this many pixels per on-chip window (tests: forces strips). Changes no bit. */
} roft_vsd_params;
/* 0.015f, the ten BOP19 taus 0.05 k (k = 1 .. 10, each the double nearest to k * 0.05), diameter 0, window_pixels 0 */
int roft_default_vsd_params(roft_vsd_params* p);
int roft_pose_errors_vsd(const roft_camera* cam, const roft_mesh* mesh, const double* est, const double* ref, int n_poses,
                         const float* depth, int n_depth /* n_poses, or 1: one image under every pair */,
                         const roft_vsd_params* p, double* errors_out /* [n_poses][n_taus] */,
                         int32_t* counts_out /* [n_poses][4 + n_taus], may be NULL */);

/* ---- (3j) pose hypotheses: many candidate poses of one object scored against one frame in one launch ---------------------------------- *
 * Track quality (section 3d) says that an estimate is bad; it does not say where the object is instead.  A caller with several
 * candidate poses for one object and one frame -- a detector's N-best list, the equivalent orientations a detector does not
 * disambiguate, a neighbourhood of a drifting estimate -- scores all of them here in one call: the mask, the depth and the mesh are
 * uploaded once (on an engine: not at all, they are resident), one launch draws and scores every pose, and one record of section 3d
 * comes back per pose.  What the caller does with the records -- pick one, search (roft_amd/relocalise.py is a host-side compass
 * search over this call; its step sizes are those of one CPU experiment and nobody has tuned them), restart the track with
 * roft_objects_restart -- is the caller's.
 *
 * roft_pose_hypotheses_score: HOST buffers, device 0.  poses: n rows of 7 doubles x y z, q = w x y z, the quaternion used as given.
 * Operation by operation, by reference to section 3d:
 *   out[i]    bit for bit what roft_track_quality(cam, divider, depth, mask, mesh, poses[i], poses[i] + 3, depth_tolerance,
 *             depth_maximum, window_pixels, ..) returns -- M, D, d, w, h, R, every count, S and depth_err as defined there --,
 *             frame = 0 included
 *   out[i]    is a function of pose i and the shared inputs alone: not of n, of the pose's position in the call, of the other poses,
 *             of window_pixels (which caps the LDS depth window as in 3d: strips, no bit changes), of how the launch maps poses to
 *             workgroups, or of the run -- every figure is a sum of integers
 *   non-finite  a pose with a NaN or infinite component draws nothing: n_mask as for every other pose, all other counts 0, depth_err
 *             DBL_MAX; it changes no other entry.  (Such a pose is not part of the equivalence with roft_track_quality.)
 *   n == 0    ROFT_OK, nothing is touched.  Any n up to 2^20 is accepted; a call is scored in chunks of 65 536 poses.
 * ROFT_ERR_INVALID, the reason in roft_last_error_string, before a device is looked for: a NULL pointer (with n > 0); n < 0 or
 * n > 2^20; divider <= 0; a negative or NaN depth_tolerance; window_pixels < 0; a mesh the other operators refuse (a NULL array, an
 * index out of range; a mesh of 0 triangles is accepted and draws nothing, as in 3d).  Without a device a well-formed call returns
 * ROFT_ERR_DEVICE: there is no CPU path.
 *
 * roft_engine_score_hypotheses: the same launch on what the engine holds of object obj_id's LAST STEPPED FRAME; syncs like
 * roft_get_mask.  M is what roft_get_mask returns; D is the float depth of that frame as the kernels read it (with raw depth or
 * rectification enabled: the product roft_engine_get_depth returns; else the caller's image -- with DEVICE inputs the caller's buffer
 * must still hold it, as the next frame's velocity stage requires anyway); the mesh is the slot's resident mesh, an object without one
 * has R = 0; d is the engine's render divider; depth_maximum is roft_config::depth_maximum.  out[i] equals
 * roft_pose_hypotheses_score on those images bit for bit, except `frame`, which is the engine frame counter of the scored frame.
 * With track quality enabled, the record of the frame's own estimate (pose[6..12] of its log row) is the engine's
 * roft_quality_record of that frame when depth_tolerance is the one quality was enabled with.
 * The call reads engine state and writes only its own buffers: every later output of the engine is what it would have been without
 * it.  It needs neither the log nor track quality enabled.
 * ROFT_ERR_STATE: no stepped frame for the slot -- also a restarted slot before its next step: exactly where roft_get_mask
 * refuses --, or a submitted batch that has not been stepped.  ROFT_ERR_INVALID: a bad obj_id; the argument checks above; an engine
 * with render_mode == ROFT_RENDER_GL (the reason of section 3d); a render target too wide for the kernel's depth window.
 *
 * Not in scope: a search loop on the device; hypotheses for several objects in one call; ROFT_RENDER_GL; the C++ class facade
 * (include/ROFT). */
int roft_pose_hypotheses_score(const roft_camera* cam, int divider, const float* depth, const uint8_t* mask,
                               const roft_mesh* mesh, const double* poses /* n x 7: x y z, q = w x y z */, int n,
                               float depth_tolerance, double depth_maximum, int window_pixels,
                               roft_quality_record* out /* n */);
int roft_engine_score_hypotheses(roft_engine* e, int obj_id, const double* poses, int n, float depth_tolerance,
                                 roft_quality_record* out /* n */);

/* ---- (4) diagnostics (tests and profiling tools; not needed by an integration) --------------------------------- */
/* The per-frame program builder without a device: the host-side mirror of CartesianQuaternionMeasurement::freeze's
 * Standard / PopBufferedMeasurement / RepeatOnlyVelocity state machine (cpp:92-348) and of the re-sync loop of
 * ROFTFilter::filtering_step (ROFTFilter.cpp:327-367) over n_frames pose-validity flags: per frame the number of UKF
 * steps, of corrections, the index of the step followed by the outlier test (-1 none) and the twist-ring slots replayed
 * (slots: n_frames x 10, -1 padded).  Any output may be NULL. */
int roft_debug_plan(const roft_config* cfg, const int* pose_valid, int n_frames, int* n_steps, int* n_corrections,
                    int* outlier, int* slots);
/* The refusals of roft_objects_restart without a device: the same host checks against a DESCRIBED engine -- n_objects objects,
 * has_mesh[i] / enrolled[i]: object i has a mesh now / was named to roft_engine_enable_pose_masks, enrol_all: that call named nobody
 * (then every object with a mesh is enrolled).  Returns what the call would return before it looks at the engine's state. */
int roft_debug_restart_check(const roft_config* cfg, int n_objects, const int* has_mesh, const int* enrolled, int enrol_all,
                             const int* obj_ids, const roft_object_desc* descs, int n, int flags);
/* Which of the engine's HIP streams delay each other at the dispatch level (streams that the runtime mapped onto one hardware
 * queue): out[a * 5 + b] = microseconds until a one-workgroup kernel on stream b completes while stream a is placing a grid
 * larger than the device; ~15 = independent, >= 80 = queued behind it.  Order: pose lane 0, pose lane 1, velocity chain, mask
 * chain, upload stream.  Takes ~20 ms; not for a hot loop. */
int roft_debug_probe_streams(roft_engine* e, double out[25]);
/* The rate (sectors per second) at which the device serves scattered 64-byte sectors: 16 M reads at random sector-aligned offsets
 * of a 2 GiB scratch buffer, best of four launches -- the roofline of a gather-bound kernel such as the flow measurement (its
 * depth and flow samples are one sector each).  Allocates and frees 2 GiB of device memory; ~30 ms. */
int roft_debug_sector_rate(int device, double* sectors_per_second);
/* (100 MHz ticks, workgroups) per kernel the workgroups spent resident on the device since the last call, read and cleared; order:
 * mask_frame, mask_ingest, mask_general, flow_measure, skf_chain, features, ukf_chain, outlier_fused.  Only filled by libraries
 * built with -DROFT_RESIDENCY (tools/residency_budget.py: the CU x us budget of the pipeline). */
int roft_debug_get_residency(roft_engine* e, unsigned long long out[32]);
/* (A/B experiments on a whole engine only -- process-wide, so not for a process whose threads run other engines; a single
 * operator-level test takes the choice as an argument: roft_outlier_test_split.)
 * How the workgroups of one alternative of an outlier test share its work, for every test launched by this process from now on:
 * 1 = they split its TRIANGLES (windows merged in memory, the last workgroup scores; rows as well when the window does not fit
 * the LDS in one piece), 0 = they split only the ROWS of its window, -1 = the library's choice (1).  The results do not depend
 * on it (tests/test_parity_gpu.py). */
int roft_debug_outlier_split(int mode);
/* device time in milliseconds (HIP events) of the kernels of the calling process's last roft_pose_errors call, without its copies */
int roft_debug_pose_errors_kernel_ms(double* ms_out);
/* device time in milliseconds (HIP events) of the renderer's last roft_scene_render call, without its copies: ms_out[0] the visibility
 * pass (with the clear of its key buffer), ms_out[1] the resolve pass */
int roft_debug_scene_kernel_ms(roft_scene_renderer* r, double ms_out[2]);
/* device time in milliseconds (HIP events) of the raw-depth kernels the engine's last submit call enqueued (section 3c), without its
 * copies; waits for them.  ROFT_ERR_STATE when that call made no depth product. */
int roft_debug_depth_kernel_ms(roft_engine* e, double* ms_out);
/* device time in milliseconds (HIP events) of the rectification launches the engine's last submit call enqueued (section 3g), without
 * its copies; waits for them.  ROFT_ERR_STATE when that call made no rectified product. */
int roft_debug_rectify_kernel_ms(roft_engine* e, double* ms_out);
/* device time in milliseconds (the HIP events bound to its dispatch) of the engine's last quality launch (section 3d); waits for it.
 * ROFT_ERR_STATE when there was none. */
int roft_debug_quality_kernel_ms(roft_engine* e, double* ms_out);
/* device time in milliseconds (the HIP events bound to its dispatches) of the engine's last silhouette stage (section 3e: the one-pass
 * launch, or draw to resolve where silhouettes were resolved); waits for it.
 * ROFT_ERR_STATE: no launch so far, or the last one ended with the preparation's own event (a steady batch of a full device outside
 * roft_engine_enable_timing), which takes no time stamps. */
int roft_debug_pose_mask_kernel_ms(roft_engine* e, double* ms_out);
/* phase counters of one object's last kernels (only filled by libraries built with a -DROFT_*_PROFILE switch) */
int roft_debug_get_dbg(roft_engine* e, int obj_id, long long out[32]);

#ifdef __cplusplus
}
#endif
#endif
