"""ctypes binding of libroft_hip.so (the C ABI declared in include/roft_engine.h).

There is no CPU path: if the library is missing it is built with hipcc, and if that fails -- or if
a compute entry point is called without a HIP device -- an exception is raised.

The header is mirrored in three kinds of data, each checked whole against it by tests/test_abi_cpu.py: the integer constants
(ROFT_<X> is <X> here), one Structure per struct typedef (`_c_name_` names the C type) and the table ABI, one row per function.
"""
import collections
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO = os.environ.get("ROFT_LIB_SO") or os.path.join(CSRC, "libroft_hip.so")   # (override: A/B runs of two builds)

OK = 0
ERR_INVALID, ERR_DEVICE, ERR_CAPACITY, ERR_STATE = -1, -2, -3, -4
FLOW_S16C2 = 11
FLOW_F32C2 = 13
MEAS_NONE, MEAS_VELOCITY, MEAS_POSE, MEAS_POSE_VELOCITY = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
RETAIN_FRAMES = 16        # default configuration (roft_engine_retain_frames otherwise)
MAX_BATCH_FRAMES = 8
MAX_FLOW_CHASE = 30
RENDER_CONTRACT, RENDER_GL = 0, 1   # roft_config::render_mode
ABI_VERSION = 2                     # ROFT_ABI_VERSION: the structs below mirror this version of the header
POSE_ERROR_ADD, POSE_ERROR_ADDS = 0, 1   # ROFT_POSE_ERROR_*
RESTART_KEEP_MESH = 1               # ROFT_RESTART_KEEP_MESH
LABEL_U8, LABEL_U16 = 1, 2          # ROFT_LABEL_*
IMAGE_GRAY8, IMAGE_BGR8, IMAGE_RGB8 = 1, 2, 3   # ROFT_IMAGE_*
DEPTH_Z16 = 1                       # ROFT_DEPTH_*
DEPTH_ALIGN_MAX_SPAN = 16           # ROFT_DEPTH_ALIGN_MAX_SPAN
RECTIFY_GRAY8, RECTIFY_RGB8, RECTIFY_U8, RECTIFY_U16, RECTIFY_F32 = 1, 2, 3, 4, 5   # ROFT_RECTIFY_*: bilinear, bilinear, nearest x 3
RECTIFY_CHUNK = 32                  # ROFT_RECTIFY_CHUNK
SCENE_MAX_INSTANCES = 256   # ROFT_SCENE_MAX_INSTANCES
MAX_SYMMETRIES, MAX_SCORE_SYMMETRIES = 16, 256   # ROFT_MAX_SYMMETRIES, ROFT_MAX_SCORE_SYMMETRIES
POSE_ERROR_MSSD, POSE_ERROR_MSPD = 2, 3          # ROFT_POSE_ERROR_* of roft_pose_errors_sym
VSD_MAX_TAUS = 16                                # ROFT_VSD_MAX_TAUS


class RoftError(RuntimeError):
    pass


class Camera(C.Structure):
    _c_name_ = "roft_camera"
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double)]


class Flow(C.Structure):
    _c_name_ = "roft_flow"
    _fields_ = [("data", C.c_void_p), ("type", C.c_int), ("cols", C.c_int), ("rows", C.c_int),
                ("grid", C.c_int), ("scale", C.c_float), ("valid", C.c_int)]


class UT(C.Structure):
    _c_name_ = "roft_ut_params"
    _fields_ = [("alpha", C.c_double), ("beta", C.c_double), ("kappa", C.c_double)]


class OFParams(C.Structure):
    _c_name_ = "roft_of_params"
    _fields_ = [("levels", C.c_int), ("radius", C.c_int), ("iterations", C.c_int), ("det_min", C.c_float)]


class OFConsistency(C.Structure):
    _c_name_ = "roft_of_consistency"
    _fields_ = [("tolerance_abs", C.c_float), ("tolerance_rel", C.c_float)]


class Mesh(C.Structure):
    _c_name_ = "roft_mesh"
    _fields_ = [("verts", C.c_void_p), ("n_verts", C.c_int), ("tris", C.c_void_p), ("n_tris", C.c_int)]


class Config(C.Structure):
    _c_name_ = "roft_config"
    _fields_ = [("cam", Camera), ("flow_type", C.c_int), ("flow_grid", C.c_int), ("flow_scale", C.c_float),
                ("sample_time", C.c_double), ("ut", UT), ("depth_maximum", C.c_double),
                ("subsampling_radius", C.c_double), ("flow_weighting", C.c_int), ("use_pose", C.c_int),
                ("use_pose_resync", C.c_int), ("use_velocity", C.c_int), ("outlier_rejection", C.c_int),
                ("flow_aided_segmentation", C.c_int), ("mask_frames_between", C.c_int),
                ("pose_frames_between", C.c_int), ("stamped_masks", C.c_int), ("max_objects", C.c_int), ("ukf_cholesky_guard", C.c_double),
                ("ukf_cholesky_guard_bilinear", C.c_double),
                ("device", C.c_int), ("max_batch_frames", C.c_int), ("mask_workgroups_per_object", C.c_int),
                ("outlier_bands_per_alternative", C.c_int), ("render_mode", C.c_int)]


class ObjectDesc(C.Structure):
    _c_name_ = "roft_object_desc"
    _fields_ = [("p_mean0", C.c_double * 13), ("p_cov0_diag", C.c_double * 12), ("v_mean0", C.c_double * 6),
                ("v_cov0_diag", C.c_double * 6), ("p_sigma_ang_vel", C.c_double * 3),
                ("p_psd_lin_acc", C.c_double * 3), ("v_q_diag", C.c_double * 6),
                ("p_meas_cov_v", C.c_double * 3), ("p_meas_cov_w", C.c_double * 3),
                ("p_meas_cov_x", C.c_double * 3), ("p_meas_cov_q", C.c_double * 3),
                ("v_meas_cov_flow", C.c_double * 2), ("mesh", Mesh)]


class FrameInput(C.Structure):
    _c_name_ = "roft_frame_input"
    _fields_ = [("dt", C.c_double), ("depth", C.c_void_p), ("flow", C.c_void_p), ("mask", C.c_void_p),
                ("pose_valid", C.c_int), ("pose_x", C.c_double * 3), ("pose_q", C.c_double * 4),
                ("mem_kind", C.c_int), ("stamp", C.c_double), ("mask_stamp", C.c_double)]


class LabelMask(C.Structure):
    _c_name_ = "roft_label_mask"
    _fields_ = [("labels", C.c_void_p), ("label_type", C.c_int), ("label", C.c_int)]


class FrameImage(C.Structure):
    _c_name_ = "roft_frame_image"
    _fields_ = [("image", C.c_void_p), ("image_type", C.c_int)]


class EngineFlowStats(C.Structure):
    _c_name_ = "roft_engine_flow_stats"
    _fields_ = [("images", C.c_longlong), ("image_bytes", C.c_longlong), ("pyramids", C.c_longlong), ("pairs", C.c_longlong)]


class DepthSource(C.Structure):
    _c_name_ = "roft_depth_source"
    _fields_ = [("type", C.c_int), ("scale", C.c_float), ("align", C.c_int), ("cam", Camera), ("R", C.c_float * 9), ("t", C.c_float * 3)]


class EngineDepthStats(C.Structure):
    _c_name_ = "roft_engine_depth_stats"
    _fields_ = [("images", C.c_longlong), ("image_bytes", C.c_longlong), ("products", C.c_longlong)]


class Lens(C.Structure):
    _c_name_ = "roft_lens"
    _fields_ = [("cam", Camera), ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("k3", C.c_double)]


class EngineRectifyStats(C.Structure):
    _c_name_ = "roft_engine_rectify_stats"
    _fields_ = [("sources", C.c_longlong), ("products", C.c_longlong), ("bytes", C.c_longlong)]


class QualityRecord(C.Structure):
    _c_name_ = "roft_quality_record"
    _fields_ = [("frame", C.c_int32), ("n_mask", C.c_int32), ("n_render", C.c_int32), ("n_both", C.c_int32), ("n_depth", C.c_int32),
                ("n_front", C.c_int32), ("n_behind", C.c_int32), ("reserved", C.c_int32), ("depth_err", C.c_double)]


class QualityParams(C.Structure):
    _c_name_ = "roft_quality_params"
    _fields_ = [("every", C.c_int), ("depth_tolerance", C.c_float)]


class EnginePoseMaskStats(C.Structure):
    _c_name_ = "roft_engine_pose_mask_stats"
    _fields_ = [("silhouettes", C.c_longlong), ("frames", C.c_longlong)]


class EnginePoseMaskOcclusionStats(C.Structure):
    _c_name_ = "roft_engine_pose_mask_occlusion_stats"
    _fields_ = [("resolved", C.c_longlong), ("hidden", C.c_longlong), ("pixels_removed", C.c_longlong)]


class PoseMaskGate(C.Structure):
    _c_name_ = "roft_pose_mask_gate"
    _fields_ = [("front_tolerance", C.c_float), ("behind_tolerance", C.c_float)]


class EnginePoseMaskGateStats(C.Structure):
    _c_name_ = "roft_engine_pose_mask_gate_stats"
    _fields_ = [("gated", C.c_longlong), ("emptied", C.c_longlong), ("pixels_front", C.c_longlong), ("pixels_behind", C.c_longlong)]


class EngineRestartStats(C.Structure):
    _c_name_ = "roft_engine_restart_stats"
    _fields_ = [("calls", C.c_longlong), ("objects", C.c_longlong), ("meshes_replaced", C.c_longlong)]


class EngineStats(C.Structure):
    _c_name_ = "roft_engine_stats"
    _fields_ = [("frames", C.c_longlong), ("batches", C.c_longlong), ("launches", C.c_longlong),
                ("event_ops", C.c_longlong), ("h2d_bytes", C.c_longlong), ("h2d_copies", C.c_longlong)]


class BatchTrace(C.Structure):
    _c_name_ = "roft_batch_trace"
    _fields_ = [("batch", C.c_int), ("frames", C.c_int), ("steady", C.c_int), ("throttled", C.c_int), ("handoff", C.c_int),
                ("early_lanes", C.c_int), ("outlier_parts_halved", C.c_int), ("launches", C.c_int), ("event_ops", C.c_int),
                ("t_submit_us", C.c_double), ("submit_us", C.c_double), ("wait_us", C.c_double), ("step_us", C.c_double),
                ("t_done_us", C.c_double)]


class ObjectOutput(C.Structure):
    _c_name_ = "roft_object_output"
    _fields_ = [("pose", C.c_double * 13), ("twist", C.c_double * 6), ("n_flow_points", C.c_int),
                ("outlier_selected", C.c_int), ("outlier_L", C.c_double * 2)]


class SceneStyle(C.Structure):
    _c_name_ = "roft_scene_style"
    _fields_ = [("tint", C.c_float * 3), ("opacity", C.c_float), ("ambient", C.c_float)]


class SceneDesc(C.Structure):
    _c_name_ = "roft_scene_desc"
    _fields_ = [("n_frames", C.c_int), ("n_instances", C.c_int), ("mesh_index", C.c_void_p), ("poses", C.c_void_p),
                ("valid", C.c_void_p), ("background", C.c_void_p), ("background_frames", C.c_int), ("gray_background", C.c_int),
                ("styles", C.c_void_p), ("window_pixels", C.c_int)]


class VsdParams(C.Structure):
    _c_name_ = "roft_vsd_params"
    _fields_ = [("delta", C.c_float), ("n_taus", C.c_int), ("taus", C.c_double * VSD_MAX_TAUS), ("diameter", C.c_double),
                ("window_pixels", C.c_int)]


# ---- every function include/roft_engine.h declares, in the header's order: one row each --------------------------------------
# optional: a library loaded through ROFT_LIB_SO (an older build, for an A/B run) may lack the symbol -- the diagnostics and the
# entry points younger than ABI version 2 itself; tests/test_abi_cpu.py checks that the in-tree library has them all.
Fn = collections.namedtuple("Fn", "name restype argtypes optional")
_int, _vp, _ip, _dp = C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
_P = C.POINTER
_REQUIRED, _OPTIONAL = False, True
ABI = (
    Fn("roft_last_error_string", C.c_char_p, [], _REQUIRED),
    Fn("roft_device_count", _int, [], _REQUIRED),
    Fn("roft_abi_version", _int, [], _REQUIRED),
    # (1) operator level
    Fn("roft_flow_measurement", _int, [_P(Camera), _vp, _vp, _P(Flow), C.c_double, C.c_float, C.c_double, _int, _vp, _vp, _vp, _ip], _REQUIRED),
    Fn("roft_kf_predict", _int, [_vp] * 5, _REQUIRED),
    Fn("roft_skf_correct", _int, [_vp, _vp, _int, _vp, _vp, _vp, _int, _vp, _vp, _ip], _REQUIRED),
    Fn("roft_skf_correct_points", _int, [_P(Camera), C.c_double, _vp, _vp, _int, _vp, _vp, _vp, _vp, _int, _vp, _vp, _ip], _REQUIRED),
    Fn("roft_mask_propagate", _int, [_vp, _int, _int, _P(Flow), _int, _int], _REQUIRED),
    Fn("roft_pose_process_noise", _int, [_vp, _vp, C.c_double, _vp], _REQUIRED),
    Fn("roft_ukf_predict", _int, [_vp, _vp, _vp, C.c_double, _P(UT), _vp, _vp], _REQUIRED),
    Fn("roft_ukf_correct", _int, [_vp, _vp, _int, _vp, _vp, _P(UT), _vp, _vp, _ip], _REQUIRED),
    Fn("roft_mesh_classify", _int, [_P(Mesh), _vp, _ip], _REQUIRED),
    Fn("roft_render_depth", _int, [_P(Mesh), _vp, _vp, _P(Camera), _int, _vp], _REQUIRED),
    Fn("roft_depth_likelihood", _int, [_P(Camera), _vp, _vp, _vp, _int, _dp, _P(C.c_long)], _REQUIRED),
    Fn("roft_outlier_test", _int, [_P(Camera), _int, _vp, _vp, _P(Mesh), _vp, _vp, _int, _int, _int, _vp, _vp, _ip, _vp], _REQUIRED),
    Fn("roft_outlier_test_split", _int, [_P(Camera), _int, _vp, _vp, _P(Mesh), _vp, _vp, _int, _int, _int, _int, _vp, _vp, _ip, _vp], _REQUIRED),
    Fn("roft_render_depth_mode", _int, [_P(Mesh), _vp, _vp, _P(Camera), _int, _int, _vp], _REQUIRED),
    Fn("roft_outlier_test_mode", _int, [_P(Camera), _int, _vp, _vp, _P(Mesh), _vp, _vp, _int, _int, _int, _int, _int, _vp, _vp, _ip, _vp],
       _REQUIRED),
    Fn("roft_pose_errors", _int, [_int, _vp, _int, _vp, _vp, _int, _vp], _OPTIONAL),
    # (2) batched engine
    Fn("roft_default_config", _int, [_P(Config), _int, _int, _int], _REQUIRED),
    Fn("roft_default_object", _int, [_P(ObjectDesc)], _REQUIRED),
    Fn("roft_engine_create", _int, [_P(Config), _P(_vp)], _REQUIRED),
    Fn("roft_engine_destroy", _int, [_vp], _REQUIRED),
    Fn("roft_object_add", _int, [_vp, _P(ObjectDesc), _ip], _REQUIRED),
    Fn("roft_objects_restart", _int, [_vp, _ip, _P(ObjectDesc), _int, _int], _OPTIONAL),
    Fn("roft_engine_get_restart_stats", _int, [_vp, _P(EngineRestartStats)], _OPTIONAL),
    Fn("roft_frame_submit", _int, [_vp, _P(FrameInput), _int], _REQUIRED),
    Fn("roft_frames_submit", _int, [_vp, _P(FrameInput), _int, _int], _REQUIRED),
    Fn("roft_frames_submit_labels", _int, [_vp, _P(FrameInput), _P(LabelMask), _int, _int], _OPTIONAL),
    Fn("roft_labels_to_masks", _int, [_vp, _int, _int, _int, _ip, _int, _vp, _ip], _OPTIONAL),
    Fn("roft_step", _int, [_vp], _REQUIRED),
    Fn("roft_engine_retain_frames", _int, [_vp], _REQUIRED),
    Fn("roft_sync", _int, [_vp], _REQUIRED),
    Fn("roft_get_state", _int, [_vp, _int, _vp, _vp, _vp, _vp], _REQUIRED),
    Fn("roft_get_outputs", _int, [_vp, _P(ObjectOutput), _int], _REQUIRED),
    Fn("roft_get_mask", _int, [_vp, _int, _vp], _REQUIRED),
    Fn("roft_engine_enable_log", _int, [_vp, _int], _REQUIRED),
    Fn("roft_engine_get_log", _int, [_vp, _int, _int, _P(ObjectOutput)], _REQUIRED),
    Fn("roft_engine_get_log_rows", _int, [_vp, _int, _int, _vp], _REQUIRED),
    Fn("roft_engine_score_log", _int, [_vp, _int, _int, _int, _int, _vp, _int, _vp, _vp], _OPTIONAL),
    Fn("roft_engine_get_stats", _int, [_vp, _P(EngineStats)], _REQUIRED),
    Fn("roft_engine_get_batch_trace", _int, [_vp, _P(BatchTrace), _int, _ip], _REQUIRED),
    Fn("roft_engine_stream", _vp, [_vp], _REQUIRED),
    Fn("roft_engine_enable_timing", _int, [_vp, _int], _REQUIRED),
    Fn("roft_engine_get_timing", _int, [_vp, _ip, _P(_P(C.c_char_p)), _P(_P(C.c_float)), _P(_ip)], _REQUIRED),
    # (2b) pinned host memory
    Fn("roft_host_alloc", _vp, [C.c_size_t], _REQUIRED),
    Fn("roft_host_free", None, [_vp], _REQUIRED),
    Fn("roft_host_is_pinned", _int, [_vp], _REQUIRED),
    # (3) optical-flow producer
    Fn("roft_default_of_params", _int, [_P(OFParams)], _REQUIRED),
    Fn("roft_optical_flow", _int, [_vp, _vp, _int, _int, _P(OFParams), _int, _vp], _REQUIRED),
    Fn("roft_flow_producer_create", _int, [_int, _int, _int, _P(OFParams), _int, _int, _P(_vp)], _REQUIRED),
    Fn("roft_flow_producer_destroy", _int, [_vp], _REQUIRED),
    Fn("roft_flow_producer_run", _int, [_vp, _P(_vp), _P(_vp), _P(_vp), _int], _REQUIRED),
    Fn("roft_flow_producer_sync", _int, [_vp], _REQUIRED),
    Fn("roft_flow_producer_stream", _vp, [_vp], _REQUIRED),
    # (3a) camera images on the engine
    Fn("roft_engine_enable_flow", _int, [_vp, _P(OFParams)], _OPTIONAL),
    Fn("roft_frames_submit_images", _int, [_vp, _P(FrameInput), _P(LabelMask), _P(FrameImage), _int, _int], _OPTIONAL),
    Fn("roft_engine_get_flow", _int, [_vp, _int, _vp], _OPTIONAL),
    Fn("roft_engine_get_flow_stats", _int, [_vp, _P(EngineFlowStats)], _OPTIONAL),
    Fn("roft_image_to_gray", _int, [_vp, _int, _int, _int, _vp], _OPTIONAL),
    # (3f) forward-backward check
    Fn("roft_default_of_consistency", _int, [_P(OFConsistency)], _OPTIONAL),
    Fn("roft_optical_flow_checked", _int, [_vp, _vp, _int, _int, _P(OFParams), _P(OFConsistency), _vp], _OPTIONAL),
    Fn("roft_flow_producer_set_consistency", _int, [_vp, _P(OFConsistency)], _OPTIONAL),
    Fn("roft_engine_enable_flow_consistency", _int, [_vp, _P(OFConsistency)], _OPTIONAL),
    # (3c) raw sensor depth
    Fn("roft_engine_enable_raw_depth", _int, [_vp, _P(DepthSource)], _OPTIONAL),
    Fn("roft_engine_get_depth", _int, [_vp, _int, _vp], _OPTIONAL),
    Fn("roft_engine_get_depth_stats", _int, [_vp, _P(EngineDepthStats)], _OPTIONAL),
    Fn("roft_depth_convert", _int, [_vp, _int, _int, C.c_float, _vp], _OPTIONAL),
    Fn("roft_depth_align", _int, [_vp, _P(DepthSource), _P(Camera), _vp], _OPTIONAL),
    # (3g) lens distortion
    Fn("roft_default_lens", _int, [_P(Lens), _P(Camera)], _OPTIONAL),
    Fn("roft_rectify_map", _int, [_P(Lens), _P(Camera), _vp], _OPTIONAL),
    Fn("roft_rectify", _int, [_vp, _int, _P(Lens), _P(Camera), _vp], _OPTIONAL),
    Fn("roft_engine_enable_rectification", _int, [_vp, _P(Lens)], _OPTIONAL),
    Fn("roft_engine_get_rectify_stats", _int, [_vp, _P(EngineRectifyStats)], _OPTIONAL),
    # (3d) track quality
    Fn("roft_default_quality_params", _int, [_P(QualityParams)], _OPTIONAL),
    Fn("roft_engine_enable_quality", _int, [_vp, _P(QualityParams)], _OPTIONAL),
    Fn("roft_engine_get_quality", _int, [_vp, _int, _int, _vp], _OPTIONAL),
    Fn("roft_track_quality", _int, [_P(Camera), _int, _vp, _vp, _P(Mesh), _vp, _vp, C.c_float, C.c_double, _int, _P(QualityRecord)], _OPTIONAL),
    # (3e) masks from poses, occlusion, depth gate
    Fn("roft_engine_enable_pose_masks", _int, [_vp, _ip, _int], _OPTIONAL),
    Fn("roft_engine_get_pose_mask_stats", _int, [_vp, _P(EnginePoseMaskStats)], _OPTIONAL),
    Fn("roft_pose_silhouette", _int, [_P(Camera), _P(Mesh), _vp, _vp, _int, _int, _vp, _ip], _OPTIONAL),
    Fn("roft_engine_enable_pose_mask_occlusion", _int, [_vp, _ip, _ip, _int], _OPTIONAL),
    Fn("roft_engine_get_pose_mask_occlusion_stats", _int, [_vp, _P(EnginePoseMaskOcclusionStats)], _OPTIONAL),
    Fn("roft_pose_silhouettes_occluded", _int, [_P(Camera), _P(Mesh), _int, _vp, _vp, _int, _int, _vp, _ip], _OPTIONAL),
    Fn("roft_default_pose_mask_gate", _int, [_P(PoseMaskGate)], _OPTIONAL),
    Fn("roft_engine_enable_pose_mask_depth_gate", _int, [_vp, _P(PoseMaskGate)], _OPTIONAL),
    Fn("roft_engine_get_pose_mask_gate_stats", _int, [_vp, _P(EnginePoseMaskGateStats)], _OPTIONAL),
    Fn("roft_pose_silhouettes_gated", _int, [_P(Camera), _P(Mesh), _int, _vp, _vp, _vp, _P(PoseMaskGate), _int, _int, _vp, _ip, _ip], _OPTIONAL),
    # (3b) scene renderer
    Fn("roft_scene_renderer_create", _int, [_P(Camera), _P(Mesh), _int, _int, _int, _P(_vp)], _OPTIONAL),
    Fn("roft_scene_renderer_destroy", _int, [_vp], _OPTIONAL),
    Fn("roft_scene_render", _int, [_vp, _P(SceneDesc), _vp, _vp, _vp, _vp], _OPTIONAL),
    Fn("roft_render_scene", _int, [_P(Camera), _P(Mesh), _int, _P(SceneDesc), _vp, _vp, _vp, _vp], _OPTIONAL),
    # (3h) symmetric objects
    Fn("roft_pose_nearest_equivalent", _int, [_vp, _int, _vp, _vp, _vp, _vp, _vp, _ip], _OPTIONAL),
    Fn("roft_object_set_symmetry", _int, [_vp, _int, _vp, _int], _OPTIONAL),
    Fn("roft_pose_errors_sym", _int, [_int, _vp, _int, _vp, _vp, _int, _vp, _int, _P(Camera), _vp], _OPTIONAL),
    Fn("roft_engine_score_log_sym", _int, [_vp, _int, _int, _int, _int, _vp, _int, _vp, _vp, _int, _vp], _OPTIONAL),
    # (3i) VSD scores
    Fn("roft_default_vsd_params", _int, [_P(VsdParams)], _OPTIONAL),
    Fn("roft_pose_errors_vsd", _int, [_P(Camera), _P(Mesh), _vp, _vp, _int, _vp, _int, _P(VsdParams), _vp, _vp], _OPTIONAL),
    # (3j) pose hypotheses
    Fn("roft_pose_hypotheses_score", _int, [_P(Camera), _int, _vp, _vp, _P(Mesh), _vp, _int, C.c_float, C.c_double, _int, _P(QualityRecord)], _OPTIONAL),
    Fn("roft_engine_score_hypotheses", _int, [_vp, _int, _vp, _int, C.c_float, _P(QualityRecord)], _OPTIONAL),
    # (4) diagnostics
    Fn("roft_debug_plan", _int, [_P(Config), _vp, _int, _vp, _vp, _vp, _vp], _OPTIONAL),
    Fn("roft_debug_restart_check", _int, [_P(Config), _int, _ip, _ip, _int, _ip, _P(ObjectDesc), _int, _int], _OPTIONAL),
    Fn("roft_debug_probe_streams", _int, [_vp, _dp], _OPTIONAL),
    Fn("roft_debug_sector_rate", _int, [_int, _dp], _OPTIONAL),
    Fn("roft_debug_get_residency", _int, [_vp, _P(C.c_ulonglong)], _OPTIONAL),
    Fn("roft_debug_outlier_split", _int, [_int], _OPTIONAL),
    Fn("roft_debug_pose_errors_kernel_ms", _int, [_dp], _OPTIONAL),
    Fn("roft_debug_scene_kernel_ms", _int, [_vp, _dp], _OPTIONAL),
    Fn("roft_debug_depth_kernel_ms", _int, [_vp, _dp], _OPTIONAL),
    Fn("roft_debug_rectify_kernel_ms", _int, [_vp, _dp], _OPTIONAL),
    Fn("roft_debug_quality_kernel_ms", _int, [_vp, _dp], _OPTIONAL),
    Fn("roft_debug_pose_mask_kernel_ms", _int, [_vp, _dp], _OPTIONAL),
    Fn("roft_debug_get_dbg", _int, [_vp, _int, _P(C.c_longlong)], _OPTIONAL),
)
ABI_SYMBOLS = [f.name for f in ABI]
# entry points younger than ABI version 2 itself: a library built before them still loads through ROFT_LIB_SO
NEWER_SYMBOLS = tuple(f.name for f in ABI if f.optional and not f.name.startswith("roft_debug_"))


def build(force=False):
    """Compile libroft_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(_HERE, "..", "include", "roft_engine.h"))
    stale = (not os.path.exists(SO)) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs)
    if force or stale:
        jobs = str(min(8, os.cpu_count() or 1))
        r = subprocess.run(["make", "-C", CSRC, "-j", jobs, "libroft_hip.so"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RoftError("building libroft_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return SO


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO):
        build()
    L = C.CDLL(SO)
    # the structs above mirror one version of the header: a library of another version (or one from before the version was
    # exported) would read them with another layout
    version = L.roft_abi_version() if hasattr(L, "roft_abi_version") else None
    if version != ABI_VERSION:
        raise RoftError("%s has ABI version %s, this binding mirrors version %d: rebuild the library" % (SO, version, ABI_VERSION))
    for f in ABI:
        if f.optional and not hasattr(L, f.name):
            continue
        fn = getattr(L, f.name)
        fn.restype, fn.argtypes = f.restype, f.argtypes
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise RoftError("libroft_hip error %d: %s" % (rc, lib().roft_last_error_string().decode()))


def require_device():
    if lib().roft_device_count() <= 0:
        raise RoftError("no HIP device visible: roft_amd has no CPU fallback")
