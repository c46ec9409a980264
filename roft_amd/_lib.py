"""ctypes binding of libroft_hip.so (the C ABI declared in include/roft_engine.h).

There is no CPU path: if the library is missing it is built with hipcc, and if that fails -- or if
a compute entry point is called without a HIP device -- an exception is raised.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO = os.environ.get("ROFT_LIB_SO") or os.path.join(CSRC, "libroft_hip.so")   # (override: A/B runs of two builds)

OK = 0
FLOW_S16C2 = 11
FLOW_F32C2 = 13
MEAS_NONE, MEAS_VELOCITY, MEAS_POSE, MEAS_POSE_VELOCITY = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
RETAIN_FRAMES = 16        # default configuration (roft_engine_retain_frames otherwise)
MAX_BATCH_FRAMES = 8
MAX_FLOW_CHASE = 30
RENDER_CONTRACT, RENDER_GL = 0, 1   # roft_config::render_mode
ABI_VERSION = 2                     # ROFT_ABI_VERSION: the structs below mirror this version of the header


class RoftError(RuntimeError):
    pass


class Camera(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double)]


class Flow(C.Structure):
    _fields_ = [("data", C.c_void_p), ("type", C.c_int), ("cols", C.c_int), ("rows", C.c_int),
                ("grid", C.c_int), ("scale", C.c_float), ("valid", C.c_int)]


class UT(C.Structure):
    _fields_ = [("alpha", C.c_double), ("beta", C.c_double), ("kappa", C.c_double)]


class OFParams(C.Structure):
    _fields_ = [("levels", C.c_int), ("radius", C.c_int), ("iterations", C.c_int), ("det_min", C.c_float)]


class OFConsistency(C.Structure):
    _fields_ = [("tolerance_abs", C.c_float), ("tolerance_rel", C.c_float)]


class Mesh(C.Structure):
    _fields_ = [("verts", C.c_void_p), ("n_verts", C.c_int), ("tris", C.c_void_p), ("n_tris", C.c_int)]


class Config(C.Structure):
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
    _fields_ = [("p_mean0", C.c_double * 13), ("p_cov0_diag", C.c_double * 12), ("v_mean0", C.c_double * 6),
                ("v_cov0_diag", C.c_double * 6), ("p_sigma_ang_vel", C.c_double * 3),
                ("p_psd_lin_acc", C.c_double * 3), ("v_q_diag", C.c_double * 6),
                ("p_meas_cov_v", C.c_double * 3), ("p_meas_cov_w", C.c_double * 3),
                ("p_meas_cov_x", C.c_double * 3), ("p_meas_cov_q", C.c_double * 3),
                ("v_meas_cov_flow", C.c_double * 2), ("mesh", Mesh)]


class FrameInput(C.Structure):
    _fields_ = [("dt", C.c_double), ("depth", C.c_void_p), ("flow", C.c_void_p), ("mask", C.c_void_p),
                ("pose_valid", C.c_int), ("pose_x", C.c_double * 3), ("pose_q", C.c_double * 4),
                ("mem_kind", C.c_int), ("stamp", C.c_double), ("mask_stamp", C.c_double)]


LABEL_U8, LABEL_U16 = 1, 2          # ROFT_LABEL_*


class LabelMask(C.Structure):
    _fields_ = [("labels", C.c_void_p), ("label_type", C.c_int), ("label", C.c_int)]


IMAGE_GRAY8, IMAGE_BGR8, IMAGE_RGB8 = 1, 2, 3   # ROFT_IMAGE_*


class FrameImage(C.Structure):
    _fields_ = [("image", C.c_void_p), ("image_type", C.c_int)]


class EngineFlowStats(C.Structure):
    _fields_ = [("images", C.c_longlong), ("image_bytes", C.c_longlong), ("pyramids", C.c_longlong), ("pairs", C.c_longlong)]


DEPTH_Z16 = 1                       # ROFT_DEPTH_*
DEPTH_ALIGN_MAX_SPAN = 16           # ROFT_DEPTH_ALIGN_MAX_SPAN


class DepthSource(C.Structure):
    _fields_ = [("type", C.c_int), ("scale", C.c_float), ("align", C.c_int), ("cam", Camera), ("R", C.c_float * 9), ("t", C.c_float * 3)]


class EngineDepthStats(C.Structure):
    _fields_ = [("images", C.c_longlong), ("image_bytes", C.c_longlong), ("products", C.c_longlong)]


class QualityRecord(C.Structure):
    _fields_ = [("frame", C.c_int32), ("n_mask", C.c_int32), ("n_render", C.c_int32), ("n_both", C.c_int32), ("n_depth", C.c_int32),
                ("n_front", C.c_int32), ("n_behind", C.c_int32), ("reserved", C.c_int32), ("depth_err", C.c_double)]


class QualityParams(C.Structure):
    _fields_ = [("every", C.c_int), ("depth_tolerance", C.c_float)]


class EnginePoseMaskStats(C.Structure):
    _fields_ = [("silhouettes", C.c_longlong), ("frames", C.c_longlong)]


class EnginePoseMaskOcclusionStats(C.Structure):
    _fields_ = [("resolved", C.c_longlong), ("hidden", C.c_longlong), ("pixels_removed", C.c_longlong)]


class PoseMaskGate(C.Structure):
    _fields_ = [("front_tolerance", C.c_float), ("behind_tolerance", C.c_float)]


class EnginePoseMaskGateStats(C.Structure):
    _fields_ = [("gated", C.c_longlong), ("emptied", C.c_longlong), ("pixels_front", C.c_longlong), ("pixels_behind", C.c_longlong)]


RESTART_KEEP_MESH = 1               # ROFT_RESTART_KEEP_MESH


class EngineRestartStats(C.Structure):
    _fields_ = [("calls", C.c_longlong), ("objects", C.c_longlong), ("meshes_replaced", C.c_longlong)]


class EngineStats(C.Structure):
    _fields_ = [("frames", C.c_longlong), ("batches", C.c_longlong), ("launches", C.c_longlong),
                ("event_ops", C.c_longlong), ("h2d_bytes", C.c_longlong), ("h2d_copies", C.c_longlong)]


class BatchTrace(C.Structure):
    _fields_ = [("batch", C.c_int), ("frames", C.c_int), ("steady", C.c_int), ("throttled", C.c_int), ("handoff", C.c_int),
                ("early_lanes", C.c_int), ("outlier_parts_halved", C.c_int), ("launches", C.c_int), ("event_ops", C.c_int),
                ("t_submit_us", C.c_double), ("submit_us", C.c_double), ("wait_us", C.c_double), ("step_us", C.c_double),
                ("t_done_us", C.c_double)]


class ObjectOutput(C.Structure):
    _fields_ = [("pose", C.c_double * 13), ("twist", C.c_double * 6), ("n_flow_points", C.c_int),
                ("outlier_selected", C.c_int), ("outlier_L", C.c_double * 2)]


class SceneStyle(C.Structure):
    _fields_ = [("tint", C.c_float * 3), ("opacity", C.c_float), ("ambient", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int), ("n_instances", C.c_int), ("mesh_index", C.c_void_p), ("poses", C.c_void_p),
                ("valid", C.c_void_p), ("background", C.c_void_p), ("background_frames", C.c_int), ("gray_background", C.c_int),
                ("styles", C.c_void_p), ("window_pixels", C.c_int)]


SCENE_MAX_INSTANCES = 256   # ROFT_SCENE_MAX_INSTANCES

# every symbol include/roft_engine.h declares
ABI_SYMBOLS = [
    "roft_last_error_string", "roft_device_count", "roft_abi_version", "roft_flow_measurement", "roft_kf_predict",
    "roft_skf_correct", "roft_skf_correct_points", "roft_mask_propagate", "roft_pose_process_noise", "roft_ukf_predict",
    "roft_ukf_correct", "roft_mesh_classify", "roft_render_depth", "roft_render_depth_mode", "roft_depth_likelihood", "roft_outlier_test",
    "roft_outlier_test_split", "roft_outlier_test_mode", "roft_default_config",
    "roft_default_object", "roft_engine_create", "roft_engine_destroy", "roft_object_add",
    "roft_frame_submit", "roft_frames_submit", "roft_engine_retain_frames", "roft_engine_get_stats", "roft_step", "roft_sync", "roft_get_state", "roft_get_outputs", "roft_get_mask",
    "roft_engine_enable_log", "roft_engine_get_log", "roft_engine_get_log_rows", "roft_engine_stream", "roft_engine_enable_timing",
    "roft_engine_get_timing", "roft_engine_get_batch_trace", "roft_default_of_params", "roft_optical_flow", "roft_flow_producer_create",
    "roft_flow_producer_destroy", "roft_flow_producer_run", "roft_flow_producer_sync", "roft_flow_producer_stream",
    "roft_debug_plan", "roft_debug_get_dbg", "roft_debug_probe_streams", "roft_debug_sector_rate",
    "roft_host_alloc", "roft_host_free", "roft_host_is_pinned", "roft_debug_get_residency", "roft_debug_outlier_split",
    "roft_pose_errors", "roft_engine_score_log", "roft_debug_pose_errors_kernel_ms",
    "roft_scene_renderer_create", "roft_scene_renderer_destroy", "roft_scene_render", "roft_render_scene", "roft_debug_scene_kernel_ms",
    "roft_frames_submit_labels", "roft_labels_to_masks",
    "roft_engine_enable_flow", "roft_frames_submit_images", "roft_engine_get_flow", "roft_engine_get_flow_stats", "roft_image_to_gray",
    "roft_engine_enable_raw_depth", "roft_engine_get_depth", "roft_engine_get_depth_stats", "roft_depth_convert", "roft_depth_align",
    "roft_debug_depth_kernel_ms",
    "roft_default_quality_params", "roft_engine_enable_quality", "roft_engine_get_quality", "roft_track_quality", "roft_debug_quality_kernel_ms",
    "roft_engine_enable_pose_masks", "roft_engine_get_pose_mask_stats", "roft_pose_silhouette", "roft_debug_pose_mask_kernel_ms",
    "roft_engine_enable_pose_mask_occlusion", "roft_engine_get_pose_mask_occlusion_stats", "roft_pose_silhouettes_occluded",
    "roft_objects_restart", "roft_engine_get_restart_stats", "roft_debug_restart_check",
    "roft_default_pose_mask_gate", "roft_engine_enable_pose_mask_depth_gate", "roft_engine_get_pose_mask_gate_stats", "roft_pose_silhouettes_gated",
    "roft_default_of_consistency", "roft_optical_flow_checked", "roft_flow_producer_set_consistency", "roft_engine_enable_flow_consistency",
]
POSE_ERROR_ADD, POSE_ERROR_ADDS = 0, 1   # ROFT_POSE_ERROR_*
# entry points younger than ABI version 2 itself: a library built before them still loads through ROFT_LIB_SO
NEWER_SYMBOLS = ("roft_pose_errors", "roft_engine_score_log", "roft_scene_renderer_create", "roft_scene_renderer_destroy", "roft_scene_render",
                 "roft_render_scene", "roft_frames_submit_labels", "roft_labels_to_masks",
                 "roft_engine_enable_flow", "roft_frames_submit_images", "roft_engine_get_flow", "roft_engine_get_flow_stats", "roft_image_to_gray",
                 "roft_engine_enable_raw_depth", "roft_engine_get_depth", "roft_engine_get_depth_stats", "roft_depth_convert", "roft_depth_align",
                 "roft_default_quality_params", "roft_engine_enable_quality", "roft_engine_get_quality", "roft_track_quality",
                 "roft_engine_enable_pose_masks", "roft_engine_get_pose_mask_stats", "roft_pose_silhouette",
                 "roft_engine_enable_pose_mask_occlusion", "roft_engine_get_pose_mask_occlusion_stats", "roft_pose_silhouettes_occluded",
                 "roft_objects_restart", "roft_engine_get_restart_stats",
                 "roft_default_pose_mask_gate", "roft_engine_enable_pose_mask_depth_gate", "roft_engine_get_pose_mask_gate_stats",
                 "roft_pose_silhouettes_gated",
                 "roft_default_of_consistency", "roft_optical_flow_checked", "roft_flow_producer_set_consistency",
                 "roft_engine_enable_flow_consistency")


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
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.roft_last_error_string.restype = C.c_char_p
    L.roft_device_count.restype = C.c_int
    L.roft_flow_measurement.argtypes = [C.POINTER(Camera), vp, vp, C.POINTER(Flow), C.c_double, C.c_float,
                                        C.c_double, C.c_int, vp, vp, vp, ip]
    L.roft_kf_predict.argtypes = [vp] * 5
    L.roft_skf_correct.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, ip]
    L.roft_skf_correct_points.argtypes = [C.POINTER(Camera), C.c_double, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, ip]
    L.roft_mask_propagate.argtypes = [vp, C.c_int, C.c_int, C.POINTER(Flow), C.c_int, C.c_int]
    L.roft_pose_process_noise.argtypes = [vp, vp, C.c_double, vp]
    L.roft_ukf_predict.argtypes = [vp, vp, vp, C.c_double, C.POINTER(UT), vp, vp]
    L.roft_ukf_correct.argtypes = [vp, vp, C.c_int, vp, vp, C.POINTER(UT), vp, vp, ip]
    L.roft_render_depth.argtypes = [C.POINTER(Mesh), vp, vp, C.POINTER(Camera), C.c_int, vp]
    L.roft_depth_likelihood.argtypes = [C.POINTER(Camera), vp, vp, vp, C.c_int, dp, C.POINTER(C.c_long)]
    L.roft_outlier_test.argtypes = [C.POINTER(Camera), C.c_int, vp, vp, C.POINTER(Mesh), vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, ip, vp]
    L.roft_outlier_test_split.argtypes = [C.POINTER(Camera), C.c_int, vp, vp, C.POINTER(Mesh), vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, ip, vp]
    L.roft_render_depth_mode.argtypes = [C.POINTER(Mesh), vp, vp, C.POINTER(Camera), C.c_int, C.c_int, vp]
    L.roft_outlier_test_mode.argtypes = [C.POINTER(Camera), C.c_int, vp, vp, C.POINTER(Mesh), vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         vp, vp, ip, vp]
    L.roft_abi_version.argtypes = []
    L.roft_engine_get_batch_trace.argtypes = [vp, C.POINTER(BatchTrace), C.c_int, ip]
    L.roft_default_config.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int]
    L.roft_default_object.argtypes = [C.POINTER(ObjectDesc)]
    L.roft_engine_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.roft_engine_destroy.argtypes = [vp]
    L.roft_object_add.argtypes = [vp, C.POINTER(ObjectDesc), ip]
    L.roft_frame_submit.argtypes = [vp, C.POINTER(FrameInput), C.c_int]
    L.roft_frames_submit.argtypes = [vp, C.POINTER(FrameInput), C.c_int, C.c_int]
    L.roft_engine_retain_frames.argtypes = [vp]
    L.roft_engine_get_stats.argtypes = [vp, C.POINTER(EngineStats)]
    L.roft_step.argtypes = [vp]
    L.roft_sync.argtypes = [vp]
    L.roft_get_state.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.roft_get_outputs.argtypes = [vp, C.POINTER(ObjectOutput), C.c_int]
    L.roft_get_mask.argtypes = [vp, C.c_int, vp]
    L.roft_engine_enable_log.argtypes = [vp, C.c_int]
    L.roft_engine_get_log.argtypes = [vp, C.c_int, C.c_int, C.POINTER(ObjectOutput)]
    L.roft_engine_get_log_rows.argtypes = [vp, C.c_int, C.c_int, vp]
    L.roft_engine_stream.restype = vp
    L.roft_engine_stream.argtypes = [vp]
    L.roft_engine_enable_timing.argtypes = [vp, C.c_int]
    L.roft_engine_get_timing.argtypes = [vp, ip, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_float)),
                                         C.POINTER(ip)]
    L.roft_default_of_params.argtypes = [C.POINTER(OFParams)]
    L.roft_optical_flow.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(OFParams), C.c_int, vp]
    L.roft_flow_producer_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(OFParams), C.c_int, C.c_int, C.POINTER(vp)]
    L.roft_flow_producer_destroy.argtypes = [vp]
    L.roft_flow_producer_run.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_int]
    L.roft_flow_producer_sync.argtypes = [vp]
    L.roft_flow_producer_stream.restype = vp
    L.roft_flow_producer_stream.argtypes = [vp]
    L.roft_host_alloc.restype = vp
    L.roft_host_alloc.argtypes = [C.c_size_t]
    L.roft_host_free.restype = None
    L.roft_host_free.argtypes = [vp]
    L.roft_host_is_pinned.argtypes = [vp]
    if hasattr(L, "roft_pose_errors"):
        L.roft_pose_errors.argtypes = [C.c_int, vp, C.c_int, vp, vp, C.c_int, vp]
        L.roft_engine_score_log.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]
        L.roft_debug_pose_errors_kernel_ms.argtypes = [dp]
    if hasattr(L, "roft_render_scene"):
        L.roft_scene_renderer_create.argtypes = [C.POINTER(Camera), C.POINTER(Mesh), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.roft_scene_renderer_destroy.argtypes = [vp]
        L.roft_scene_render.argtypes = [vp, C.POINTER(SceneDesc), vp, vp, vp, vp]
        L.roft_render_scene.argtypes = [C.POINTER(Camera), C.POINTER(Mesh), C.c_int, C.POINTER(SceneDesc), vp, vp, vp, vp]
        L.roft_debug_scene_kernel_ms.argtypes = [vp, dp]
    if hasattr(L, "roft_frames_submit_labels"):
        L.roft_frames_submit_labels.argtypes = [vp, C.POINTER(FrameInput), C.POINTER(LabelMask), C.c_int, C.c_int]
        L.roft_labels_to_masks.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, vp, ip]
    if hasattr(L, "roft_frames_submit_images"):
        L.roft_engine_enable_flow.argtypes = [vp, C.POINTER(OFParams)]
        L.roft_frames_submit_images.argtypes = [vp, C.POINTER(FrameInput), C.POINTER(LabelMask), C.POINTER(FrameImage), C.c_int, C.c_int]
        L.roft_engine_get_flow.argtypes = [vp, C.c_int, vp]
        L.roft_engine_get_flow_stats.argtypes = [vp, C.POINTER(EngineFlowStats)]
        L.roft_image_to_gray.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    if hasattr(L, "roft_engine_enable_raw_depth"):
        L.roft_engine_enable_raw_depth.argtypes = [vp, C.POINTER(DepthSource)]
        L.roft_engine_get_depth.argtypes = [vp, C.c_int, vp]
        L.roft_engine_get_depth_stats.argtypes = [vp, C.POINTER(EngineDepthStats)]
        L.roft_depth_convert.argtypes = [vp, C.c_int, C.c_int, C.c_float, vp]
        L.roft_depth_align.argtypes = [vp, C.POINTER(DepthSource), C.POINTER(Camera), vp]
        L.roft_debug_depth_kernel_ms.argtypes = [vp, dp]
    if hasattr(L, "roft_track_quality"):
        L.roft_default_quality_params.argtypes = [C.POINTER(QualityParams)]
        L.roft_engine_enable_quality.argtypes = [vp, C.POINTER(QualityParams)]
        L.roft_engine_get_quality.argtypes = [vp, C.c_int, C.c_int, vp]
        L.roft_track_quality.argtypes = [C.POINTER(Camera), C.c_int, vp, vp, C.POINTER(Mesh), vp, vp, C.c_float, C.c_double, C.c_int,
                                         C.POINTER(QualityRecord)]
        L.roft_debug_quality_kernel_ms.argtypes = [vp, dp]
    if hasattr(L, "roft_pose_silhouette"):
        L.roft_engine_enable_pose_masks.argtypes = [vp, ip, C.c_int]
        L.roft_engine_get_pose_mask_stats.argtypes = [vp, C.POINTER(EnginePoseMaskStats)]
        L.roft_pose_silhouette.argtypes = [C.POINTER(Camera), C.POINTER(Mesh), vp, vp, C.c_int, C.c_int, vp, ip]
        L.roft_debug_pose_mask_kernel_ms.argtypes = [vp, dp]
    if hasattr(L, "roft_pose_silhouettes_gated"):
        L.roft_default_pose_mask_gate.argtypes = [C.POINTER(PoseMaskGate)]
        L.roft_engine_enable_pose_mask_depth_gate.argtypes = [vp, C.POINTER(PoseMaskGate)]
        L.roft_engine_get_pose_mask_gate_stats.argtypes = [vp, C.POINTER(EnginePoseMaskGateStats)]
        L.roft_pose_silhouettes_gated.argtypes = [C.POINTER(Camera), C.POINTER(Mesh), C.c_int, vp, vp, vp, C.POINTER(PoseMaskGate), C.c_int, C.c_int, vp, ip, ip]
    if hasattr(L, "roft_pose_silhouettes_occluded"):
        L.roft_engine_enable_pose_mask_occlusion.argtypes = [vp, ip, ip, C.c_int]
        L.roft_engine_get_pose_mask_occlusion_stats.argtypes = [vp, C.POINTER(EnginePoseMaskOcclusionStats)]
        L.roft_pose_silhouettes_occluded.argtypes = [C.POINTER(Camera), C.POINTER(Mesh), C.c_int, vp, vp, C.c_int, C.c_int, vp, ip]
    if hasattr(L, "roft_optical_flow_checked"):
        L.roft_default_of_consistency.argtypes = [C.POINTER(OFConsistency)]
        L.roft_optical_flow_checked.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(OFParams), C.POINTER(OFConsistency), vp]
        L.roft_flow_producer_set_consistency.argtypes = [vp, C.POINTER(OFConsistency)]
        L.roft_engine_enable_flow_consistency.argtypes = [vp, C.POINTER(OFConsistency)]
    if hasattr(L, "roft_objects_restart"):
        L.roft_objects_restart.argtypes = [vp, ip, C.POINTER(ObjectDesc), C.c_int, C.c_int]
        L.roft_engine_get_restart_stats.argtypes = [vp, C.POINTER(EngineRestartStats)]
        L.roft_debug_restart_check.argtypes = [C.POINTER(Config), C.c_int, ip, ip, C.c_int, ip, C.POINTER(ObjectDesc), C.c_int, C.c_int]
    for name in ABI_SYMBOLS:
        if (name.startswith("roft_debug_") or name in NEWER_SYMBOLS) and not hasattr(L, name):
            continue   # (an older build loaded through ROFT_LIB_SO for an A/B run: diagnostics and the pose errors only; tests/test_abi_cpu.py checks the in-tree library has them all)
        f = getattr(L, name)
        if name not in ("roft_last_error_string", "roft_engine_stream", "roft_flow_producer_stream", "roft_host_alloc", "roft_host_free"):
            f.restype = C.c_int
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise RoftError("libroft_hip error %d: %s" % (rc, lib().roft_last_error_string().decode()))


def require_device():
    if lib().roft_device_count() <= 0:
        raise RoftError("no HIP device visible: roft_amd has no CPU fallback")
