"""Shared cases of the scene renderer's tests: the mesh zoo with its classification, three poses per mesh, the two small cameras,
and references that are computed once per session and never modified."""
import functools

import numpy as np

import mesh_zoo
import scene_ref
from oracle import binding as ob

SIZES = ((160, 120), (93, 71))   # the small shape and an awkward one; fx = fy = 150


def cam(width, height):
    return scene_ref.Cam(width, height, 150.0, 150.0, width / 2.0, height / 2.0)


def oracle_cam(c):
    return ob.camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy)


def lib_cam(c):
    from roft_amd import _lib as L
    return L.Camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy)


def quat(axis, angle):
    axis = np.asarray(axis, float)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def pose(x, axis, angle):
    return np.concatenate([np.asarray(x, float), quat(axis, angle)])


# three poses per mesh: in front of the camera, tilted and off-centre, and the camera 2 cm from the object's centre (vertices
# behind the near plane: triangles are dropped and the back-face rule is off)
POSES = (pose([0.01, -0.02, 0.45], [1, 2, 3], 0.7), pose([-0.05, 0.03, 0.30], [3, -1, 2], 2.1), pose([0.005, 0.0, 0.02], [1, 1, 0], 0.4))


@functools.lru_cache(maxsize=None)
def zoo():
    """name -> (verts, tris, flip or None): the flip bits come from the oracle's classification."""
    out = {}
    for name, (v, t, _) in mesh_zoo.zoo(6).items():
        closed, flip = ob.mesh_classify(v, t)
        out[name] = (v, t, np.array(flip, np.uint8) if closed else None)
    return out


@functools.lru_cache(maxsize=None)
def oracle_depth(name, pose_id, size):
    v, t, _ = zoo()[name]
    p = POSES[pose_id]
    d = ob.render_depth(ob.make_mesh(v, t), p[:3], p[3:], oracle_cam(cam(*size)), 1)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, pose_id, size):
    """scene_ref's render of one zoo mesh alone (default style, no background)."""
    out = scene_ref.render(cam(*size), [zoo()[name]], [0], POSES[pose_id][None])
    for a in out.values():
        a.setflags(write=False)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
