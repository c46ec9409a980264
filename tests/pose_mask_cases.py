"""Shared cases of the pose-mask tests (include/roft_engine.h, section 3e): a table of (mesh, pose) operator cases at 160 x 120
-- five plane words per row, so the 64-pixel groups of the planes straddle rows --, each with the AIM it was chosen for stated as
a predicate on the oracle's mask, so that retuning a pose cannot silently drop a case; and the expected masks, which always come
from the oracle's ro_render_depth on the CPU (divider 1, > 0), computed once and never modified."""
import functools
import os
import tempfile

import numpy as np

import mesh_zoo
import util
from oracle import binding as ob
from roft_amd import io, synth

W, H = 160, 120
CAM = (W, H, 150.0, 150.0, W / 2.0, H / 2.0)    # width, height, fx, fy, cx, cy
CACHE_VERTS = 8192                              # kSilhouetteCacheVerts of roft_amd/csrc/roft_device.h
NEAR = 0.001                                    # the near plane of the render contract


def quat(axis, angle):
    axis = np.asarray(axis, float)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def pose(x, axis=(0, 0, 1), angle=0.0):
    return np.concatenate([np.asarray(x, float), quat(axis, angle)])


@functools.lru_cache(maxsize=None)
def meshes():
    """name -> (verts float32 [n, 3], tris int32 [m, 3])"""
    out = {"box12": synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, n=12)}
    for name, (v, t, _) in mesh_zoo.zoo(6).items():
        out["zoo_" + name] = (v, t)
    assert len(out) == 14, "the thirteen meshes of the zoo"
    out["cracker_box"] = io.load_obj(util.ref_cracker_box(os.path.join(tempfile.gettempdir(), "roft_ref_meshes_%d" % os.getuid())))
    assert out["cracker_box"][0].shape[0] == 7866 and out["cracker_box"][0].shape[0] <= CACHE_VERTS
    out["box_over_cache"] = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, n=37)
    assert out["box_over_cache"][0].shape[0] > CACHE_VERTS
    return {k: (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)) for k, (v, t) in out.items()}


def vertex_depths(mesh, p):
    v = meshes()[mesh][0].astype(np.float64)
    return v @ synth.quat_to_rot(p[3:])[2] + p[2]


def camera_inside_box12(p):
    local = synth.quat_to_rot(p[3:]).T @ (-p[:3])
    return bool((np.abs(local) < np.array(synth.CRACKER_BOX_HALF_EXTENTS)).all())


def _extent(m):
    vs, us = np.nonzero(m)
    return (int(vs.max() - vs.min() + 1), int(us.max() - us.min() + 1)) if len(vs) else (0, 0)


# name -> (mesh, pose, aim(mask bool [H, W], pose) -> bool)
AIMED = {
    "centred": ("box12", pose([0.0, 0.0, 0.45], [1, 2, 3], 0.7),
                lambda m, p: m.any() and not (m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any())),
    "touches_top": ("box12", pose([0.0, -0.15, 0.45], [1, 2, 3], 0.7), lambda m, p: m[0].any() and not m[-1].any()),
    "touches_bottom": ("box12", pose([0.0, 0.15, 0.45], [1, 2, 3], 0.7), lambda m, p: m[-1].any() and not m[0].any()),
    "touches_left": ("box12", pose([-0.2, 0.0, 0.45], [1, 2, 3], 0.7), lambda m, p: m[:, 0].any() and not m[:, -1].any()),
    "touches_right": ("box12", pose([0.2, 0.0, 0.45], [1, 2, 3], 0.7), lambda m, p: m[:, -1].any() and not m[:, 0].any()),
    "off_screen": ("box12", pose([1.0, 0.0, 0.45], [1, 2, 3], 0.7), lambda m, p: not m.any() and (vertex_depths("box12", p) > NEAR).all()),
    "behind_camera": ("box12", pose([0.0, 0.0, -0.5], [1, 2, 3], 0.7), lambda m, p: not m.any() and (vertex_depths("box12", p) < 0).all()),
    "straddles_near_plane": ("box12", pose([0.12, 0.0, 0.03], [1, 0, 0], np.pi / 2),
                             lambda m, p: m.any() and (vertex_depths("box12", p) <= NEAR).any() and (vertex_depths("box12", p) > NEAR).any()
                             and not camera_inside_box12(p)),
    "camera_inside": ("box12", pose([0.005, 0.0, 0.01], [1, 1, 0], 0.4), lambda m, p: m.any() and camera_inside_box12(p)),
    "under_two_pixels": ("box12", pose([0.3, -0.2, 22.0], [1, 2, 3], 0.7), lambda m, p: m.any() and max(_extent(m)) <= 2 and m.sum() <= 2),
    "covers_every_pixel": ("box12", pose([0.0, 0.0, 0.05]), lambda m, p: m.all()),
}

# every other mesh at two poses: in front of the camera, tilted; and the camera 2 cm from the object's centre
POSES = {"front": pose([0.01, -0.02, 0.45], [1, 2, 3], 0.7), "near": pose([0.005, 0.0, 0.02], [1, 1, 0], 0.4)}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (mesh name, pose [7])"""
    out = {name: (mesh, p) for name, (mesh, p, _) in AIMED.items()}
    for mesh in meshes():
        if mesh != "box12":
            for pname, p in POSES.items():
                out["%s_%s" % (mesh, pname)] = (mesh, p)
    return out


def oracle_camera(cam=CAM):
    return ob.camera(*cam)


@functools.lru_cache(maxsize=None)
def oracle_mesh(mesh):
    return ob.make_mesh(*meshes()[mesh])


def silhouette(mesh, p, cam=CAM):
    """The defining mask: ro_render_depth(mesh, x, q, cam, 1) > 0 ? 255 : 0, on the CPU."""
    d = ob.render_depth(oracle_mesh(mesh) if isinstance(mesh, str) else mesh, p[:3], p[3:], oracle_camera(cam), 1)
    return np.ascontiguousarray((d > 0).astype(np.uint8) * 255)


@functools.lru_cache(maxsize=None)
def expected(name):
    mesh, p = cases()[name]
    m = silhouette(mesh, p)
    m.setflags(write=False)
    return m
