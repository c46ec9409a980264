"""tools/run_sequence.py --flow-on-engine: the camera frames of a sequence directory go to the engine, which computes the flow
itself -- the log files are those of --compute-flow (flow files written by the dumper, read back, handed over as flows), byte for
byte, and no flow directory appears."""
import importlib.util
import os
import shutil

import pytest

from roft_amd import io

import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_flow_on_engine_writes_the_logs_of_compute_flow(tmp_path, capsys):
    n = 20
    st = util.stream(702, n, 2, with_gray=True)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    mesh = io.write_sequence(a, st, "box")
    shutil.copytree(a, b)
    rs = load_tool("run_sequence")
    common = ["--object", "box", "--flow-set", "lk_2", "--mask-set", "gt"]
    assert rs.main(["--root", a, "--mesh", mesh, "--compute-flow", "nvof2", "--out", str(tmp_path / "a_")] + common) == 0
    assert rs.main(["--root", b, "--mesh", os.path.join(b, "model.obj"), "--flow-on-engine", "nvof2", "--out", str(tmp_path / "b_")] + common) == 0
    capsys.readouterr()
    assert not os.path.exists(os.path.join(b, "optical_flow")), "no flow directory is read or written"
    assert len(os.listdir(os.path.join(a, "optical_flow", "lk_2"))) == n - 1
    for name in ("pose_estimate", "velocity_estimate"):
        got, want = open(str(tmp_path / ("b_" + name)), "rb").read(), open(str(tmp_path / ("a_" + name)), "rb").read()
        assert len(want.splitlines()) == n and got == want, name
