"""The refusals of the operator-level entry points (include/roft_engine.h, section 1, and the operators of 3d / 3e), one row per bad
call: each null argument and each range the code checks.  Return code and full error string were recorded from the library as it
was before the operators moved onto one context (tests/golden/make_operator_refusals.py -> tests/golden/operator_refusals.json), once
on a machine without a device and once on one with a device; this test asserts the same answers.  A refusal of an argument comes
before any device is looked for, so most rows read ROFT_ERR_INVALID in both records; the few checks that sit behind the device
(mixed flow formats) read ROFT_ERR_DEVICE without one.  One further row per entry point is a well-formed call: ROFT_ERR_DEVICE with
the one refusal text without a device, ROFT_OK with one."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import ops, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "operator_refusals.json")
NO_DEVICE_TEXT = "no HIP device (libroft_hip has no CPU path)"
W, H, DIV = 64, 32, 2
NPIX = W * H
_rng = np.random.default_rng(7)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


CAM = L.Camera(W, H, 60.0, 60.0, 32.0, 16.0)
MASK = ((_rng.random((H, W)) < 0.5) * 255).astype(np.uint8)
DEPTH = _rng.uniform(0.3, 0.6, (H, W)).astype(np.float32)
FLOW = _rng.standard_normal((H, W, 2)).astype(np.float32)
FLOW_S16 = np.zeros((H // 4, W // 4, 2), np.int16)
FL = ops.make_flow(FLOW, W)
FL_NO_DATA = L.Flow(None, L.FLOW_F32C2, W, H, 1, 1.0, 1)
FLOWS_31 = (L.Flow * 31)(*[FL] * 31)
FLOWS_MIXED = (L.Flow * 2)(FL, ops.make_flow(FLOW_S16, W))
FLOWS_LATER_NO_DATA = (L.Flow * 2)(FL, FL_NO_DATA)
TILE = np.full((H // DIV, W // DIV), 0.45, np.float32)
LABELS = _rng.integers(0, 4, (H, W)).astype(np.uint8)
VERTS, TRIS = (np.ascontiguousarray(a, d) for a, d in zip(synth.box_mesh((0.08, 0.10, 0.035), 2), (np.float32, np.int32)))
MESH = L.Mesh(VERTS.ctypes.data, len(VERTS), TRIS.ctypes.data, len(TRIS))
MESHES = (L.Mesh * 2)(MESH, MESH)
X, Q = np.array([0.0, 0.0, 0.45]), np.array([1.0, 0.0, 0.0, 0.0])
X2, Q2 = np.concatenate([X, X + 0.01]), np.concatenate([Q, Q])
UT = L.UT(1.0, 2.0, 0.0)
X6, P6, D6, R2 = np.zeros(6), np.eye(6) * 1e-3, np.full(6, 0.1), np.ones(2)
Y, HM = np.zeros(4), np.ones((4, 6))
UV, Z, FXY = np.array([[10, 10], [20, 12]], np.int32), np.array([0.4, 0.5], np.float32), np.ones((2, 2), np.float32)
M13, P12, Q9 = np.concatenate([np.zeros(6), X, Q]), np.eye(12) * 1e-3, np.eye(9) * 1e-4
MEAS6, R6 = np.zeros(6), np.full(6, 1e-2)
POINTS, POSES = np.ascontiguousarray(VERTS, np.float64), np.concatenate([X, Q])[None].copy()


def _values(*v):
    a = np.array(v, np.int32)
    _values.keep.append(a)
    return a.ctypes.data_as(C.POINTER(C.c_int))


_values.keep = []


def _gate(front, behind):
    g = L.PoseMaskGate(front, behind)
    _values.keep.append(g)
    return C.byref(g)


def _out(n, dtype=np.float64):
    """A fresh output buffer of n elements (kept alive by the table)."""
    a = np.zeros(max(n, 1), dtype)
    _values.keep.append(a)
    return _p(a)


def _ints(n):
    return C.cast(_out(n, np.int32), C.POINTER(C.c_int))


def _int_out():
    v = C.c_int(0)
    _values.keep.append(v)
    return C.byref(v)


_OUTLIER_HEAD = [("cam", C.byref(CAM)), ("divider", DIV), ("depth", _p(DEPTH)), ("mask", _p(MASK)), ("mesh", C.byref(MESH)), ("x", _p(X2)), ("q", _p(Q2)),
                 ("bands", 0), ("vertex_cache", 1), ("window_pixels", 0)]
_OUTLIER_TAIL = [("L_out", _out(2)), ("samples_out", _out(2, np.int64)), ("selected_out", _int_out()), ("tiles_out", None)]
_OUTLIER_NULLS = ["cam", "depth", "mask", "mesh", "x", "q"]
_OUTLIER_BAD = {"divider_zero": {"divider": 0}, "divider_negative": {"divider": -1}, "bands_negative": {"bands": -1}, "bands_nine": {"bands": 9},
                "window_pixels_negative": {"window_pixels": -1}}
_MODE_BAD = {"mode_two": {"mode": 2}, "mode_negative": {"mode": -1}}
_SIL_TAIL = [("bands", 0), ("vertex_cache", 1), ("masks_out", _out(2 * NPIX, np.uint8)), ("counts_out", _ints(2))]
_SIL_BAD = {"bands_negative": {"bands": -1}, "vertex_cache_two": {"vertex_cache": 2}, "vertex_cache_negative": {"vertex_cache": -1}}
_N_BAD = {"n_zero": {"n": 0}, "n_negative": {"n": -1}, "n_257": {"n": L.SCENE_MAX_INSTANCES + 1}}

# entry point -> (the arguments of a well-formed call, by name; the arguments whose null is refused; name -> the arguments a bad call replaces)
TABLE = {
    "roft_flow_measurement": (
        [("cam", C.byref(CAM)), ("prev_mask", _p(MASK)), ("prev_depth", _p(DEPTH)), ("flow", C.byref(FL)), ("dt", 1.0 / 30.0), ("radius", 3.0),
         ("depth_max", 2.0), ("capacity", NPIX), ("uv", _out(2 * NPIX, np.int32)), ("y", _out(2 * NPIX)), ("H", _out(12 * NPIX)), ("n_out", _int_out())],
        ["cam", "prev_mask", "prev_depth", "flow", "n_out"],
        {"flow_without_data": {"flow": C.byref(FL_NO_DATA)}, "radius_zero": {"radius": 0.0}, "radius_half": {"radius": 0.5}}),
    "roft_kf_predict": (
        [("x", _p(X6)), ("P", _p(P6)), ("Qdiag", _p(D6)), ("x_out", _out(6)), ("P_out", _out(36))],
        ["x", "P", "Qdiag", "x_out", "P_out"], {}),
    "roft_skf_correct": (
        [("x_pred", _p(X6)), ("P_pred", _p(P6)), ("N", 2), ("y", _p(Y)), ("H", _p(HM)), ("Rdiag", _p(R2)), ("reweight", 1), ("x_out", _out(6)),
         ("P_out", _out(36)), ("status_out", _int_out())],
        ["x_pred", "P_pred", "y", "H", "Rdiag", "x_out", "P_out"], {}),
    "roft_skf_correct_points": (
        [("cam", C.byref(CAM)), ("dt", 1.0 / 30.0), ("x_pred", _p(X6)), ("P_pred", _p(P6)), ("N", 2), ("uv", _p(UV)), ("z", _p(Z)), ("flow_xy", _p(FXY)),
         ("Rdiag", _p(R2)), ("reweight", 1), ("x_out", _out(6)), ("P_out", _out(36)), ("status_out", _int_out())],
        ["cam", "x_pred", "P_pred", "uv", "z", "flow_xy", "Rdiag", "x_out", "P_out"], {}),
    "roft_mask_propagate": (
        [("mask", _out(NPIX, np.uint8)), ("W", W), ("H", H), ("flows", C.cast(FLOWS_31, C.POINTER(L.Flow))), ("n_flows", 2), ("frames_between", 6)],
        ["mask", "flows"],
        {"31_flows_all_of_them": {"n_flows": 31, "frames_between": 0}, "31_flows_between_40": {"n_flows": 31, "frames_between": 40},
         "mixed_flow_formats": {"flows": C.cast(FLOWS_MIXED, C.POINTER(L.Flow))},
         "later_flow_without_data": {"flows": C.cast(FLOWS_LATER_NO_DATA, C.POINTER(L.Flow))}}),
    "roft_labels_to_masks": (
        [("labels", _p(LABELS)), ("label_type", L.LABEL_U8), ("W", W), ("H", H), ("values", _values(1, 3)), ("n", 2), ("masks_out", _out(2 * NPIX, np.uint8)),
         ("counts_out", _ints(2))],
        ["labels", "values"],
        {"n_zero": {"n": 0}, "n_negative": {"n": -1}, "label_type_zero": {"label_type": 0}, "label_type_three": {"label_type": 3},
         "label_zero": {"values": _values(1, 0)}, "label_negative": {"values": _values(-1, 1)}, "label_256_in_u8": {"values": _values(1, 256)},
         "label_65536_in_u16": {"label_type": L.LABEL_U16, "values": _values(65536, 1)}}),
    "roft_pose_silhouette": (
        [("cam", C.byref(CAM)), ("mesh", C.byref(MESH)), ("x", _p(X)), ("q", _p(Q))] + _SIL_TAIL,
        ["cam", "mesh", "x", "q"], _SIL_BAD),
    "roft_pose_silhouettes_occluded": (
        [("cam", C.byref(CAM)), ("meshes", C.cast(MESHES, C.POINTER(L.Mesh))), ("n", 2), ("x", _p(X2)), ("q", _p(Q2))] + _SIL_TAIL,
        ["cam", "meshes", "x", "q"], dict(_SIL_BAD, **_N_BAD)),
    "roft_pose_silhouettes_gated": (
        [("cam", C.byref(CAM)), ("meshes", C.cast(MESHES, C.POINTER(L.Mesh))), ("n", 2), ("x", _p(X2)), ("q", _p(Q2)), ("depth", _p(DEPTH)),
         ("gate", _gate(0.02, 0.0))] + _SIL_TAIL + [("removed_out", _ints(4))],
        ["cam", "meshes", "x", "q", "depth", "gate"],
        dict(_SIL_BAD, **_N_BAD, front_tolerance_zero={"gate": _gate(0.0, 0.0)}, front_tolerance_negative={"gate": _gate(-0.01, 0.0)},
             front_tolerance_nan={"gate": _gate(float("nan"), 0.0)}, front_tolerance_inf={"gate": _gate(float("inf"), 0.0)},
             behind_tolerance_nan={"gate": _gate(0.02, float("nan"))}, behind_tolerance_inf={"gate": _gate(0.02, float("inf"))})),
    "roft_ukf_predict": (
        [("mean", _p(M13)), ("P", _p(P12)), ("Q", _p(Q9)), ("T", 1.0 / 30.0), ("ut", C.byref(UT)), ("mean_out", _out(13)), ("P_out", _out(144))],
        ["mean", "P", "Q", "ut", "mean_out", "P_out"], {}),
    "roft_ukf_correct": (
        [("mean", _p(M13)), ("P", _p(P12)), ("type", L.MEAS_VELOCITY), ("meas", _p(MEAS6)), ("Rdiag", _p(R6)), ("ut", C.byref(UT)), ("mean_out", _out(13)),
         ("P_out", _out(144)), ("status_out", _int_out())],
        ["mean", "P", "meas", "Rdiag", "ut", "mean_out", "P_out"],
        {"type_negative": {"type": -1}, "type_four": {"type": 4}}),
    "roft_render_depth": (
        [("mesh", C.byref(MESH)), ("x", _p(X)), ("q", _p(Q)), ("cam", C.byref(CAM)), ("divider", DIV), ("tile", _out(NPIX, np.float32))],
        ["mesh", "x", "q", "cam", "tile"], {"divider_zero": {"divider": 0}, "divider_negative": {"divider": -1}}),
    "roft_render_depth_mode": (
        [("mesh", C.byref(MESH)), ("x", _p(X)), ("q", _p(Q)), ("cam", C.byref(CAM)), ("divider", DIV), ("mode", L.RENDER_GL), ("tile", _out(NPIX, np.float32))],
        ["mesh", "x", "q", "cam", "tile"], dict({"divider_zero": {"divider": 0}, "divider_negative": {"divider": -1}}, **_MODE_BAD)),
    "roft_outlier_test": (_OUTLIER_HEAD + _OUTLIER_TAIL, _OUTLIER_NULLS, _OUTLIER_BAD),
    "roft_outlier_test_split": (_OUTLIER_HEAD + [("split", 1)] + _OUTLIER_TAIL, _OUTLIER_NULLS, _OUTLIER_BAD),
    "roft_outlier_test_mode": (_OUTLIER_HEAD + [("split", -1), ("mode", L.RENDER_GL)] + _OUTLIER_TAIL, _OUTLIER_NULLS, dict(_OUTLIER_BAD, **_MODE_BAD)),
    "roft_depth_likelihood": (
        [("cam", C.byref(CAM)), ("depth", _p(DEPTH)), ("mask", _p(MASK)), ("tile", _p(TILE)), ("divider", DIV), ("L_out", C.cast(_out(1), C.POINTER(C.c_double))),
         ("samples_out", C.cast(_out(1, np.int64), C.POINTER(C.c_long)))],
        ["cam", "depth", "mask", "tile", "L_out"], {"divider_zero": {"divider": 0}, "divider_negative": {"divider": -1}}),
    "roft_track_quality": (
        [("cam", C.byref(CAM)), ("divider", DIV), ("depth", _p(DEPTH)), ("mask", _p(MASK)), ("mesh", C.byref(MESH)), ("x", _p(X)), ("q", _p(Q)),
         ("depth_tolerance", 0.01), ("depth_maximum", 2.0), ("window_pixels", 0), ("out", C.cast(_out(40, np.uint8), C.POINTER(L.QualityRecord)))],
        ["cam", "depth", "mask", "mesh", "x", "q", "out"],
        {"divider_zero": {"divider": 0}, "divider_negative": {"divider": -1}, "depth_tolerance_negative": {"depth_tolerance": -1.0},
         "depth_tolerance_nan": {"depth_tolerance": float("nan")}, "window_pixels_negative": {"window_pixels": -1}}),
    "roft_pose_errors": (
        [("kind", L.POSE_ERROR_ADD), ("points", _p(POINTS)), ("n_points", len(POINTS)), ("est", _p(POSES)), ("ref", _p(POSES)), ("n_poses", 1), ("out", _out(1))],
        ["points", "est", "ref", "out"],
        {"kind_two": {"kind": 2}, "kind_negative": {"kind": -1}, "n_points_zero": {"n_points": 0}, "n_points_negative": {"n_points": -3},
         "n_poses_negative": {"n_poses": -1}}),
}

WELL_FORMED = "well_formed"


def rows(entry):
    """[(row name, argument list)] of an entry point: the well-formed call, then one call per refusal."""
    good, nulls, bad = TABLE[entry]
    names = [n for n, _ in good]
    assert set(nulls) <= set(names) and all(set(r) <= set(names) for r in bad.values()), entry
    out = [(WELL_FORMED, [v for _, v in good])]
    out += [("null_" + a, [None if n == a else v for n, v in good]) for a in nulls]
    out += [(name, [repl.get(n, v) for n, v in good]) for name, repl in bad.items()]
    return out


def answer(lib, entry, args):
    """[return code, error string ("" behind ROFT_OK: the string is the last refusal's)] of one call."""
    rc = getattr(lib, entry)(*args)
    return [rc, lib.roft_last_error_string().decode() if rc != L.OK else ""]


def record(lib):
    return {entry: {name: answer(lib, entry, args) for name, args in rows(entry)} for entry in TABLE}


def test_the_table_names_every_operator_entry_point():
    section_1 = [f.name for f in L.ABI[3:L.ABI_SYMBOLS.index("roft_default_config")]]
    others = ["roft_labels_to_masks", "roft_track_quality", "roft_pose_silhouette", "roft_pose_silhouettes_occluded", "roft_pose_silhouettes_gated"]
    host_only = {"roft_pose_process_noise", "roft_mesh_classify"}   # (no device, no context)
    assert set(TABLE) == set(section_1 + others) - host_only


@pytest.mark.parametrize("entry", sorted(TABLE))
def test_refusals_are_what_they_were(entry):
    lib = L.lib()
    device = lib.roft_device_count() > 0
    with open(GOLDEN) as f:
        golden = json.load(f)["device" if device else "no_device"][entry]
    got = {name: answer(lib, entry, args) for name, args in rows(entry)}
    assert sorted(got) == sorted(golden)
    for name in got:
        assert got[name] == golden[name], (entry, name)
    # ... and the record itself says what the contract says: a well-formed call stops at the device or passes, an argument's refusal
    # does not depend on one
    assert got[WELL_FORMED] == ([L.OK, ""] if device else [L.ERR_DEVICE, NO_DEVICE_TEXT])
    with open(GOLDEN) as f:
        both = json.load(f)
    for name in got:
        if name != WELL_FORMED and both["no_device"][entry][name][0] == L.ERR_INVALID:
            assert both["device"][entry][name] == both["no_device"][entry][name], (entry, name)
