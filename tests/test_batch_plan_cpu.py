"""plan_batch (roft_amd/csrc/batch_plan.h): the launch graph of a batch is decided from counters before anything is enqueued, by a
host-only header that compiles without HIP.  tests/cpp/batch_plan_check.cpp holds the rules -- the progress conditions, the
description of roft_batch_trace, the switch paragraph of README.md -- and sweeps them; here it is built and run, and the traces
recorded under profiles/ are replayed through the plan."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roft_amd", "csrc")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_check")
    # batch_plan.h ALONE: no HIP include path, no include/ of the repository
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "batch_plan_check.cpp"), "-o", exe])
    return exe


def test_batch_plan_header_is_host_only():
    text = open(os.path.join(CSRC, "batch_plan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<c") for i in includes), includes   # C library headers only: no hip, no roft_engine*


def test_batch_plan_obeys_the_stated_rules(check_exe):
    r = subprocess.run([check_exe, "sweep"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) > 3000000


def _plan_trace(check_exe, n_obj, lead, frames):
    r = subprocess.run([check_exe, "trace", str(n_obj), "256", str(lead)] + [str(t) for t in frames], capture_output=True, text=True, check=True)
    return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]


@pytest.mark.parametrize("run", [1, 2, 3])
def test_recorded_driver_shaped_traces_follow_the_plan(check_exe, run):
    """64 objects, batches of 2, 6, 6, 6 frames after a sync: a burst -- `steady` 0, `handoff` 1, `outlier_parts_halved` 0."""
    d = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_driver_shaped_%d_detail.json" % run)))
    assert d["config"]["objects_per_gpu"] == 64
    for window in d["windows"]:
        rec = window["batches"]
        assert [b["frames"] for b in rec] == [2, 6, 6, 6]
        plan = _plan_trace(check_exe, 64, 5, [b["frames"] for b in rec])
        assert plan == [(0, 1, 0)] * 4
        assert [(b["steady"], b["handoff"], b["outlier_parts_halved"]) for b in rec] == plan


def test_recorded_steady_trace_follows_the_plan(check_exe):
    """240 steps of 64 objects: five burst batches after the sync (`lead` is 5 for batches of more than one frame), then `steady` 1
    and `outlier_parts_halved` 1 -- and no hand-over, the device being full."""
    d = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_steady_240_detail.json")))
    assert d["config"]["objects_per_gpu"] == 64
    for window in d["windows"]:
        rec = window["batches"]
        assert len(rec) > 5 and all(b["frames"] > 1 for b in rec)
        plan = _plan_trace(check_exe, 64, 5, [b["frames"] for b in rec])
        assert [s for s, _, _ in plan] == [0] * 5 + [1] * (len(rec) - 5)
        assert [(b["steady"], b["outlier_parts_halved"]) for b in rec] == [(s, h) for s, _, h in plan]
        assert [b["handoff"] for b in rec[5:]] == [h for _, h, _ in plan[5:]] == [0] * (len(rec) - 5)
