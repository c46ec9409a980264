"""The four users of the mesh walk of roft_amd/csrc/raster.h (project_mesh, fetch_triangle, cull_table) held to ONE answer: the
outlier test's render (roft_render_depth), the scene renderer, masks from poses and track quality draw the same mesh at the same
pose on the same 160 x 120 target, and each is compared with the same oracle tile, ro_render_depth at divider 1 on the CPU,
computed once per case and never modified.  Depths bit for bit, the silhouette as (tile > 0) * 255, the counts as integers: no
tolerance anywhere.

Cases: the AIMED table of tests/pose_mask_cases.py (box12: the box's edges on every side of the target, off screen, behind the
camera, across the near plane, the camera inside, under two pixels, every pixel) with each case's aim predicate, and box_over_cache
at POSES["near"]: vertices behind the near plane on the per-triangle projection path of every user that has one at that size."""
import functools

import numpy as np
import pytest

import pose_mask_cases as pc
from oracle import binding as ob
from roft_amd import _lib as L
from roft_amd import ops

pytestmark = pytest.mark.gpu

CASES = dict({name: (mesh, p, aim) for name, (mesh, p, aim) in pc.AIMED.items()},
             box_over_cache_near=("box_over_cache", pc.POSES["near"],
                                  lambda m, p: m.any() and (pc.vertex_depths("box_over_cache", p) <= pc.NEAR).any()))


@functools.lru_cache(maxsize=None)
def oracle_tile(name):
    mesh, p, _ = CASES[name]
    tile = ob.render_depth(pc.oracle_mesh(mesh), p[:3], p[3:], pc.oracle_camera(), 1)
    tile.setflags(write=False)
    return tile


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_user_of_the_mesh_walk_draws_the_oracle_tile(name):
    mesh, p, aim = CASES[name]
    tile = oracle_tile(name)
    assert tile.shape == (pc.H, pc.W) and tile.dtype == np.float32
    covered = tile > 0
    assert aim(covered, p), "the case no longer shows what it was chosen for"
    n_covered = int(covered.sum())
    v, t = pc.meshes()[mesh]
    cam, x, q = L.Camera(*pc.CAM), p[:3], p[3:]

    assert same_bits(ops.render_depth(ops.make_mesh(v, t), x, q, cam, 1), tile), "roft_render_depth"

    scene = ops.render_scene(cam, [(v, t)], [0], p[None, None], outputs=("depth",))
    assert same_bits(scene["depth"][0], tile), "roft_render_scene"

    mask, count = ops.pose_silhouette(cam, (v, t), x, q)
    assert np.array_equal(mask, covered.astype(np.uint8) * 255), "roft_pose_silhouette"
    assert count == n_covered

    frame_mask = np.zeros((pc.H, pc.W), np.uint8)
    frame_mask[pc.H // 4: pc.H // 2, pc.W // 4: pc.W // 2] = 255
    rec = ops.track_quality(cam, 1, np.ones((pc.H, pc.W), np.float32), frame_mask, ops.make_mesh(v, t), x, q)
    assert int(rec["n_render"]) == n_covered, "roft_track_quality"


# ---- one resident mesh per context, reused call after call ---------------------------------------------------------------------------
# (mesh, pose, render mode) in the order of the calls: closed in walk order; the same mesh as it is (the flip bits of the call before
# must not be used); a larger mesh (the buffers grow); an open mesh (no flips behind a closed one); a smaller mesh in larger buffers
REUSE_STEPS = (("box12", "centred", L.RENDER_CONTRACT), ("box12", "centred", L.RENDER_GL), ("box_over_cache", "front", L.RENDER_CONTRACT),
               ("zoo_box_open", "front", L.RENDER_CONTRACT), ("box12", "centred", L.RENDER_CONTRACT))


@functools.lru_cache(maxsize=None)
def oracle_tile_of(mesh, pose_name, mode):
    p = pc.AIMED[pose_name][1] if pose_name in pc.AIMED else pc.POSES[pose_name]
    if mode == L.RENDER_GL:   # (as tests/test_render_gl_gpu.py obtains it)
        tile = ob.render_depth_mode(pc.oracle_mesh(mesh), p[:3], p[3:], pc.oracle_camera(), 1, ob.RENDER_GL)
    else:
        tile = ob.render_depth(pc.oracle_mesh(mesh), p[:3], p[3:], pc.oracle_camera(), 1)
    tile.setflags(write=False)
    return p, tile


def mesh_zoo_closed(mesh):
    return ob.mesh_classify(*pc.meshes()[mesh])[0]


def test_a_resident_mesh_reused_across_calls_shows_nothing_of_the_call_before():
    cam = L.Camera(*pc.CAM)
    sizes = [pc.meshes()[mesh][1].shape[0] for mesh, _, _ in REUSE_STEPS]
    assert sizes[2] > sizes[0] > 0 and sizes[4] < sizes[2], "the buffers grow, then hold a smaller mesh"
    assert mesh_zoo_closed("box12") and not mesh_zoo_closed("zoo_box_open")
    assert not same_bits(oracle_tile_of(*REUSE_STEPS[0])[1], oracle_tile_of(*REUSE_STEPS[1])[1]), "the two modes draw box12 differently"
    for step, (mesh, pose_name, mode) in enumerate(REUSE_STEPS):
        p, tile = oracle_tile_of(mesh, pose_name, mode)
        assert (tile > 0).sum() > 100, "the step draws something"
        got = ops.render_depth(ops.make_mesh(*pc.meshes()[mesh]), p[:3], p[3:], cam, 1, mode=mode)
        assert same_bits(got, tile), "step %d: %s, mode %d" % (step, mesh, mode)
    p, tile = oracle_tile_of("box12", "centred", L.RENDER_CONTRACT)
    n_covered = int((tile > 0).sum())
    frame_mask = np.zeros((pc.H, pc.W), np.uint8)
    frame_mask[pc.H // 4: pc.H // 2, pc.W // 4: pc.W // 2] = 255
    depth = np.ones((pc.H, pc.W), np.float32)
    absent = L.Mesh(None, 0, None, 0)
    for step, (mesh, want) in enumerate(((ops.make_mesh(*pc.meshes()["box12"]), n_covered), (absent, 0), (ops.make_mesh(*pc.meshes()["box12"]), n_covered))):
        rec = ops.track_quality(cam, 1, depth, frame_mask, mesh, p[:3], p[3:])
        assert int(rec["n_render"]) == want, "roft_track_quality, call %d" % step
        assert int(rec["n_mask"]) == int((frame_mask > 1).sum())
