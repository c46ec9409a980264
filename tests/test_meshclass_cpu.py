"""The closed-surface classification behind the render contract's back-face rule (round 6): the oracle's statement
(oracle/ro_meshclass.c) and the engine's own implementation (roft_amd/csrc/mesh_class.hip, roft_mesh_classify -- host code, what
roft_object_add applies) agree on closed, inside-out, inconsistently wound, open, non-manifold, degenerate, unwelded,
multi-component and non-orientable meshes; and the oracle's render of a closed mesh without the triangles that face away is the
render with them (the nearest surface of a closed mesh seen from outside faces the camera; reference: depth test LESS, no
culling, src/roft-lib/src/SICAD.cpp:271-272)."""

import os
import subprocess

import numpy as np
import pytest

import mesh_zoo
import util
from oracle import binding as ob
from roft_amd import io, ops, synth



def test_the_array_check_and_the_three_upload_layouts(tmp_path):
    """tests/cpp/mesh_check.cpp against mesh_class.hip ALONE, as plain C++ without a HIP include path: the array check reports null
    arrays and the triangle and vertex of a bad index; walk order is a permutation of the caller's triangles with the flips
    following it, the caller's order keeps the caller's pointer with classify_mesh's flips, "as it is" is never classified."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "roft_amd", "csrc")
    exe = str(tmp_path / "mesh_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", csrc, os.path.join(root, "tests", "cpp", "mesh_check.cpp"),
                           "-x", "c++", os.path.join(csrc, "mesh_class.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "mesh_check ok", r.stderr


@pytest.mark.parametrize("name", sorted(mesh_zoo.zoo()))
def test_oracle_and_engine_classify_alike(name):
    v, t, closed = mesh_zoo.zoo()[name]
    co, fo = ob.mesh_classify(v, t)
    ce, fe = ops.mesh_classify(v, t)
    assert co == ce == closed
    assert np.array_equal(fo, fe)
    if not closed:
        assert not fo.any()


def test_flip_marks_the_triangles_wound_clockwise_seen_from_outside():
    for name in ("box", "box_reversed", "box_random_windings"):
        v, t, _ = mesh_zoo.zoo()[name]
        _, flip = ob.mesh_classify(v, t)
        vd = v.astype(np.float64)
        n = np.cross(vd[t[:, 1]] - vd[t[:, 0]], vd[t[:, 2]] - vd[t[:, 0]])
        outward = (n * (vd[t].mean(1) - vd.mean(0))).sum(1) > 0     # (a box is star-shaped about its centroid)
        assert np.array_equal(flip.astype(bool), ~outward), name
    # the inside-out component of the two-component mesh gets the flips, the outward one of THIS generator gets its own
    v, t, _ = mesh_zoo.zoo()["two_components"]
    _, flip = ob.mesh_classify(v, t)
    _, f_box = ob.mesh_classify(*mesh_zoo.zoo()["box"][:2])
    assert np.array_equal(flip[:len(f_box)], f_box) and np.array_equal(flip[len(f_box):], 1 - f_box)


def test_the_bench_mesh_and_the_references_cracker_box_are_closed(tmp_path):
    v, t = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, 36)
    assert ob.mesh_classify(v, t)[0] and ops.mesh_classify(v, t)[0]
    v, t = io.load_obj(util.ref_cracker_box(tmp_path))   # (the reference's mesh, a fixture under tests/golden/ref_meshes)
    co, fo = ob.mesh_classify(v, t)
    ce, fe = ops.mesh_classify(v, t)
    assert co and ce and np.array_equal(fo, fe)


@pytest.mark.parametrize("name", ["box", "box_reversed", "box_random_windings", "box_unwelded", "two_components", "torus", "hollow_box"])
def test_leaving_out_the_triangles_that_face_away_does_not_change_the_render(name):
    """Oracle against oracle: the contract's render of a closed mesh (triangles facing away left out) against the same mesh drawn
    whole.  Equal in exact arithmetic; in float arithmetic a pixel centre within rounding of an edge may differ -- none does here
    (tools/render_gap.py counts them over the configs: RENDER_GL / RENDER_V1 draw both faces)."""
    v, t, _ = mesh_zoo.zoo(12)[name]
    cam = synth.Camera.shape_a()
    ocam = util.oracle_camera(ob, cam)
    culled = ob.make_mesh(v, t)
    whole = ob.make_mesh(v, t)
    assert culled.closed == 1
    whole.closed = 0
    rng = np.random.default_rng(11)
    for _ in range(6):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        x = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.45, 0.9)])
        a = ob.render_depth(culled, x, q, ocam, 2)
        b = ob.render_depth(whole, x, q, ocam, 2)
        assert (a > 0).sum() > 300
        assert np.array_equal(a, b)


def test_a_camera_inside_the_surface_sees_it_whole():
    """A vertex behind the near plane switches the back-face rule off for the render: from inside a closed mesh the nearest
    surface faces AWAY."""
    v, t, _ = mesh_zoo.zoo(12)["box"]
    cam = synth.Camera.shape_a()
    ocam = util.oracle_camera(ob, cam)
    big = (v * 20.0).astype(np.float32)      # a room of 3.2 x 4 x 1.4 m around the camera
    culled = ob.make_mesh(big, t)
    whole = ob.make_mesh(big, t)
    whole.closed = 0
    a = ob.render_depth(culled, [0.0, 0.0, 0.2], [1, 0, 0, 0], ocam, 2)
    b = ob.render_depth(whole, [0.0, 0.0, 0.2], [1, 0, 0, 0], ocam, 2)
    assert (a > 0).sum() > 10000 and np.array_equal(a, b)
