"""An operator's result does not depend on what the operator context did before.

Every operator-level entry point runs on one process-wide context (roft_amd/csrc/op_context.h).  The context owns device memory;
it holds no configuration, so a call must find nothing that an earlier call left.  For every operator `op`, and every operator `d`
as the disturber -- once at another geometry (B, other width AND height) and once at op's own (A, other inputs) --

    r0 = op(A);  d(.);  r1 = op(A)        r1 must equal r0 bit for bit

on the raw bytes of every returned array, count and status (NaN equals itself).  The geometries are the smallest the kernels take
(width % 32 == 0, width * height % 64 == 0).  So that the equality says something, r0 is checked to be non-trivial once per operator."""
import functools

import numpy as np
import pytest

import mesh_zoo
from oracle import binding as ob
from roft_amd import _lib as L
from roft_amd import ops

pytestmark = pytest.mark.gpu

A, B = (64, 32), (96, 64)
DT = 1.0 / 30.0


def _quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


@functools.lru_cache(maxsize=None)
def inputs(geometry, seed):
    """One fixed, seeded input set for all operators at a geometry: a box in front of the camera, the depth and the mask of its
    render (the oracle's, on the host), random flows and labels, random filter states.  Read-only."""
    W, H = geometry
    rng = np.random.default_rng(1000 * seed + W)
    s = {}
    fx = 0.78 * W
    s["cam"] = L.Camera(W, H, fx, fx, W / 2.0, H / 2.0)
    ocam = ob.camera(W, H, fx, fx, W / 2.0, H / 2.0)
    v, t = mesh_zoo.box(3)
    s["verts"], s["tris"], s["mesh"] = v, t, ops.make_mesh(v, t)
    x = np.array([0.01, -0.005, 0.45]) + 0.01 * rng.standard_normal(3)
    q = _quat(rng.standard_normal(3), 0.3 + rng.random())
    s["x"], s["q"] = x, q
    # n = 3 objects of one scene, side by side and one behind; two alternatives of the first
    s["xs"] = np.stack([x, x + [0.04, 0.0, 0.06], x + [-0.05, 0.01, -0.05]])
    s["qs"] = np.stack([q, _quat(rng.standard_normal(3), 1.0), _quat(rng.standard_normal(3), 2.0)])
    s["x2"] = np.stack([x, x + [0.004, -0.003, 0.006]])
    s["q2"] = np.stack([q, _quat(q[1:] + 0.05 * rng.standard_normal(3), 2 * np.arccos(q[0]) + 0.03)])
    omesh = ob.make_mesh(v, t)
    render = ob.render_depth(omesh, x, q, ocam, 1)
    s["mask"] = ((render > 0) * 255).astype(np.uint8)
    s["depth"] = (np.where(render > 0, render, 0.8) + 0.002 * rng.standard_normal((H, W))).astype(np.float32)
    gate_depth = s["depth"].copy()
    gate_depth[:, :3 * W // 8] = 0.2   # (something in front of the left of the scene: the gate removes pixels of the object there)
    s["gate_depth"] = gate_depth
    s["tile"] = ob.render_depth(omesh, s["x2"][1], s["q2"][1], ocam, 2)   # divider 2: not the default (4) of these widths
    s["flow"] = (1.5 * rng.standard_normal((H, W, 2))).astype(np.float32)
    s["flows"] = [(0.8 * rng.standard_normal((H, W, 2))).astype(np.float32) for _ in range(3)]
    s["labels"] = rng.integers(0, 4, (H, W)).astype(np.uint8)
    s["values"] = np.array([1, 3, 2], np.int32)
    n = 8 + W // 16   # (another number of measurements at the other geometry)
    A6 = rng.standard_normal((6, 6))
    s["x6"], s["P6"], s["q6"] = 0.1 * rng.standard_normal(6), A6 @ A6.T * 1e-3 + np.eye(6) * 1e-4, rng.random(6) * 0.1
    s["y"], s["Hm"] = rng.standard_normal(2 * n), rng.standard_normal((2 * n, 6))
    s["uv"] = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int32)
    s["z"], s["fxy"] = rng.uniform(0.3, 0.6, n).astype(np.float32), rng.standard_normal((n, 2)).astype(np.float32)
    s["mean"] = np.concatenate([0.05 * rng.standard_normal(6), x, q])
    s["P12"] = np.diag(rng.uniform(0.5, 1.5, 12)) * 1e-3
    s["Q9"] = ops.process_noise(np.full(3, 1.0), np.full(3, 0.1), DT)   # (host code: parameter packing)
    s["meas"] = np.concatenate([0.05 * rng.standard_normal(6), x + 0.002, q])
    s["R12"] = rng.uniform(0.5, 1.5, 12) * 1e-3
    s["points"] = np.ascontiguousarray(v, np.float64)
    s["est"] = np.concatenate([rng.standard_normal((n, 3)), rng.standard_normal((n, 4))], 1)
    s["ref"] = s["est"] + 0.01 * rng.standard_normal((n, 7))
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s


GL = L.RENDER_GL
# name -> (the call on an input set, "r0 is not trivial")
OPERATORS = {
    "flow_measurement": (lambda s: ops.flow_measurement(s["cam"], s["mask"], s["depth"], s["flow"], DT, radius=3.0), lambda r: r[0] > 0),
    "kf_predict": (lambda s: ops.kf_predict(s["x6"], s["P6"], s["q6"]), lambda r: np.all(np.isfinite(r[1])) and np.all(np.diag(r[1]) > 0)),
    "skf_correct": (lambda s: ops.skf_correct(s["x6"], s["P6"], s["y"], s["Hm"]), lambda r: r[0] == 0 and np.any(r[1] != 0)),
    "skf_correct_points": (lambda s: ops.skf_correct_points(s["cam"], DT, s["x6"], s["P6"], s["uv"], s["z"], s["fxy"]), lambda r: r[0] == 0 and np.any(r[1] != 0)),
    "mask_propagate": (lambda s: ops.mask_propagate(s["mask"], s["flows"], 6), lambda r: np.count_nonzero(r) > 0),
    "labels_to_masks": (lambda s: ops.labels_to_masks(s["labels"], s["values"]), lambda r: np.all(r[1] > 0) and np.count_nonzero(r[0]) > 0),
    "pose_silhouette": (lambda s: ops.pose_silhouette(s["cam"], (s["verts"], s["tris"]), s["x"], s["q"]), lambda r: r[1] > 0),
    "pose_silhouettes_occluded": (lambda s: ops.pose_silhouettes_occluded(s["cam"], [(s["verts"], s["tris"])] * 2, s["xs"][:2], s["qs"][:2]),
                                  lambda r: np.all(r[1] > 0)),
    "pose_silhouettes_gated": (lambda s: ops.pose_silhouettes_gated(s["cam"], [(s["verts"], s["tris"])] * 3, s["xs"], s["qs"], s["gate_depth"]),
                               lambda r: np.all(r[1] > 0) and np.sum(r[2]) > 0),
    "ukf_predict": (lambda s: ops.ukf_predict(s["mean"], s["P12"], s["Q9"], DT), lambda r: np.all(np.isfinite(r[1])) and np.all(np.diag(r[1]) > 0)),
    "ukf_correct": (lambda s: ops.ukf_correct(s["mean"], s["P12"], L.MEAS_POSE_VELOCITY, s["meas"], s["R12"]), lambda r: r[0] == 0 and np.all(np.isfinite(r[1]))),
    "render_depth": (lambda s: ops.render_depth(s["mesh"], s["x"], s["q"], s["cam"], 2), lambda r: np.count_nonzero(r) > 0),
    "render_depth_gl": (lambda s: ops.render_depth(s["mesh"], s["x"], s["q"], s["cam"], 1, mode=GL), lambda r: np.count_nonzero(r) > 0),
    "outlier_test": (lambda s: ops.outlier_test(s["cam"], 2, s["depth"], s["mask"], s["mesh"], s["x2"], s["q2"]), lambda r: np.all(r[1] > 0) and r[2] in (0, 1)),
    "outlier_test_gl": (lambda s: ops.outlier_test(s["cam"], 1, s["depth"], s["mask"], s["mesh"], s["x2"], s["q2"], bands=2, mode=GL),
                        lambda r: np.all(r[1] > 0) and r[2] in (0, 1)),
    "depth_likelihood": (lambda s: ops.depth_likelihood(s["cam"], s["depth"], s["mask"], s["tile"], 2), lambda r: r[1] > 0),
    "track_quality": (lambda s: ops.track_quality(s["cam"], 2, s["depth"], s["mask"], s["mesh"], s["x"], s["q"]),
                      lambda r: r["frame"] == 0 and r["n_render"] > 0 and r["n_both"] > 0 and r["n_depth"] > 0),
    "pose_errors": (lambda s: ops.pose_errors("adds", s["points"], s["est"], s["ref"]), lambda r: np.all(np.isfinite(r)) and np.all(r > 0)),
}


def raw(result):
    """The bytes of everything a call returned, item by item."""
    items = result if isinstance(result, tuple) else (result,)
    return [b"" if x is None else np.ascontiguousarray(x).tobytes() for x in items]


@pytest.mark.parametrize("name", sorted(OPERATORS))
def test_result_does_not_depend_on_the_call_before(oracle, name):
    op, not_trivial = OPERATORS[name]
    mine = inputs(A, 1)
    r0 = op(mine)
    assert not_trivial(r0), "the inputs give a trivial result: the comparison would say nothing"
    want = raw(r0)
    differing = []
    for other in sorted(OPERATORS):
        for geometry in (B, A):
            OPERATORS[other][0](inputs(geometry, 2))
            if raw(op(mine)) != want:
                differing.append((other, "%dx%d" % geometry))
    assert not differing, "%s gives other bits behind %s" % (name, differing)
