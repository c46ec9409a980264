"""The cluster builder of the outlier test (roft_amd/csrc/mesh_clusters.h: at most 64 triangles over at most 64 distinct vertices, one
wave's work) on the meshes of the classification tests and on the bench's box, through tests/cpp/cluster_check.cpp -- host C++, built
without HIP.  Every triangle is in exactly one cluster, no cluster crosses a direction bucket, the unpacked words give back the
corners, and by brute force over seeded poses (random, grazing, close to the surface) the cone test never rejects a cluster that holds a
triangle the render contract's own area test would draw."""

import os
import re
import subprocess

import numpy as np
import pytest

import mesh_zoo
from roft_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POSES = 320


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    csrc = os.path.join(ROOT, "roft_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("cluster_check") / "cluster_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", csrc,
                           os.path.join(ROOT, "tests", "cpp", "cluster_check.cpp"), "-x", "c++", os.path.join(csrc, "mesh_class.hip"), "-o", exe])
    return exe


def _meshes():
    out = {name: m for name, m in mesh_zoo.zoo().items() if name != "box_nan_vertex"}
    out["box_12"] = mesh_zoo.zoo(12)["box"]          # more than 64 triangles per bucket, vertex count no multiple of 64
    out["torus_12"] = mesh_zoo.zoo(12)["torus"]      # curved: cones with an opening angle
    v, t = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, 36)
    out["bench_box"] = (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32), True)
    return out


def _run(checker, tmp_path, v, t, poses, seed=7, extra=()):
    path = str(tmp_path / "mesh.bin")
    with open(path, "wb") as f:
        f.write(np.array([len(v), len(t)], np.int32).tobytes())
        f.write(np.ascontiguousarray(v, np.float32).tobytes())
        f.write(np.ascontiguousarray(t, np.int32).tobytes())
    r = subprocess.run([checker, path, str(poses), str(seed), *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("cluster_check ok"), r.stdout + r.stderr
    return {k: int(x) for k, x in re.findall(r"(\w+)=(\d+)", r.stdout)}


@pytest.mark.parametrize("name", sorted(_meshes()))
def test_clusters_cover_the_mesh_and_cones_are_sound(checker, tmp_path, name):
    v, t, closed = _meshes()[name]
    res = _run(checker, tmp_path, v, t, N_POSES if closed else 0)
    assert res["closed"] == int(closed)
    assert res["clusters"] >= (len(t) + 63) // 64
    if not closed:
        assert res["cones"] == 0 and res["rejected"] == 0
    else:
        assert res["not_rotations"] > 0     # (the poses of quaternions far off unit length were there, and were kept from the cones)
    print(name, res)


def test_the_cone_is_no_dead_letter_on_the_bench_box(checker, tmp_path):
    """Soundness alone is met by a test that never rejects.  On the bench's box, at the bench's distances (1.5 to 3 object sizes) and
    divider, the clusters are flat patches of a face and three faces are turned from the camera; the cone's margins cost a face that
    is within a few degrees of edge-on, which a random pose makes rare: four fifths of the clusters that face away must be rejected.
    And the patches reuse their vertices: a patch of 8 x 4 quads is 64 triangles over 45 vertices, 0.7 slots per triangle; the box's
    clusters must use fewer than 0.9 (a run of triangles along a row of quads uses one per triangle, separate triangles three)."""
    v, t = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, 36)
    res = _run(checker, tmp_path, v, t, 64, seed=3, extra=("near",))
    assert res["cones"] == res["clusters"]
    assert res["rejected"] >= 0.8 * res["facing_away"], res
    assert res["slots"] < 0.9 * len(t), res


def test_a_mesh_with_a_nan_vertex_gets_a_box_that_settles_nothing(checker, tmp_path):
    v, t, _ = mesh_zoo.zoo()["box_nan_vertex"]
    res = _run(checker, tmp_path, v, t, 0)
    assert res["closed"] == 0 and res["cones"] == 0
