"""The case plan_batch (roft_amd/csrc/batch_plan.h) has for masks from poses: one more launch of the preparation, behind the control
blocks and whatever ingest there is, decided from a count before anything is enqueued; a batch without silhouettes plans exactly
what it planned before.  tests/cpp/pose_mask_plan_check.cpp states the rules and sweeps them; it is built against the host-only
header alone and run here, without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roft_amd", "csrc")


def test_silhouette_launch_is_one_launch_and_changes_nothing_else(tmp_path):
    exe = str(tmp_path / "pose_mask_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "pose_mask_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) > 100000
