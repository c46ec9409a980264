"""roft_objects_restart without a GPU: the header declares the entry points next to an unchanged ABI, every ROFT_ERR_INVALID
refusal comes before a device is looked for, the C++ facade's restart_objects compiles, and ROFT-tracker-batch explains --slots."""
import ctypes as C
import os
import subprocess

import numpy as np

import abi_header
from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roft_amd", "csrc")


def test_header_declares_the_calls_and_the_flag_next_to_abi_version_2():
    """(prototypes, struct, flag and argtypes: tests/test_abi_cpu.py checks them with every other name of the header)"""
    code = abi_header.code()
    assert L.ABI_VERSION == 2 and L.lib().roft_abi_version() == 2
    # the section follows roft_object_add, as the issue of this feature places it
    assert code.index("roft_object_add(") < code.index("roft_objects_restart(") < code.index("roft_frame_submit(")
    assert hasattr(E.ROFTFilterBatch, "restart_objects") and hasattr(E.ROFTFilterBatch, "restart_stats")


def test_every_invalid_refusal_comes_before_the_device():
    """A NULL engine through the entry point itself; the others through roft_debug_restart_check, which runs the entry point's own
    host checks against a DESCRIBED engine (objects, which of them have a mesh, which are enrolled for pose masks)."""
    lib = L.lib()
    st = L.EngineRestartStats()
    assert lib.roft_objects_restart(None, None, None, 0, 0) == -1 and b"null engine" in lib.roft_last_error_string()
    assert lib.roft_engine_get_restart_stats(None, C.byref(st)) == -1
    cfg = E.default_config(320, 240)
    verts, tris = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, 2)

    def desc(v=verts, t=tris, mesh=True):
        d = E.default_object()
        if mesh:
            d.mesh = L.Mesh(None if v is None else v.ctypes.data, verts.shape[0], None if t is None else t.ctypes.data, t.shape[0] if t is not None else 4)
        return d

    def check(ids, descs, n=None, flags=0, has_mesh=(1, 1, 1), enrolled=(0, 0, 0), enrol_all=0, config=cfg):
        n_obj = len(has_mesh)
        hm, en = (C.c_int * n_obj)(*has_mesh), (C.c_int * n_obj)(*enrolled)
        arr_i = (C.c_int * max(len(ids), 1))(*ids) if ids is not None else None
        arr_d = (L.ObjectDesc * max(len(descs), 1))(*descs) if descs is not None else None
        rc = lib.roft_debug_restart_check(C.byref(config), n_obj, hm, en, enrol_all, arr_i, arr_d, len(ids) if n is None else n, flags)
        return rc, lib.roft_last_error_string()

    good = desc()
    assert check([0, 2], [good, good])[0] == 0
    assert check([], [], n=0)[0] == 0 and check(None, None, n=0)[0] == 0
    assert check([0], [good], n=-1)[0] == -1
    assert check(None, [good], n=1)[0] == -1 and check([0], None, n=1)[0] == -1
    for bad_id in (-1, 3, 1 << 20):
        rc, msg = check([bad_id], [good])
        assert rc == -1 and b"not an object" in msg
    rc, msg = check([1, 2, 1], [good, good, good])
    assert rc == -1 and b"named twice" in msg
    for flags in (2, 4, 3, -1):
        rc, msg = check([0], [good], flags=flags)
        assert rc == -1 and b"flag" in msg
    # every check roft_object_add makes on a description
    assert check([0], [desc(v=None)])[0] == -1 and check([0], [desc(t=None)])[0] == -1
    for row, col, val in ((0, 0, -1), (5, 2, verts.shape[0]), (tris.shape[0] - 1, 1, 1 << 30)):
        bad = tris.copy()
        bad[row, col] = val
        rc, msg = check([1, 0], [good, desc(t=bad)])
        assert rc == -1 and b"refers to vertex" in msg
    # a description without a mesh for an object that needs one: outlier rejection with use_pose ...
    rc, msg = check([0], [desc(mesh=False)])
    assert rc == -1 and b"needs a mesh" in msg
    lenient = E.default_config(320, 240)
    lenient.outlier_rejection = 0
    assert check([0], [desc(mesh=False)], config=lenient)[0] == 0
    # ... or enrolled for pose masks, by id or because every object with a mesh is
    rc, msg = check([1], [desc(mesh=False)], enrolled=(0, 1, 0), config=lenient)
    assert rc == -1 and b"pose masks" in msg
    assert check([0], [desc(mesh=False)], enrolled=(0, 1, 0), config=lenient)[0] == 0
    assert check([1], [desc(mesh=False)], enrol_all=1, config=lenient)[0] == -1
    assert check([1], [desc(mesh=False)], has_mesh=(1, 0, 1), enrol_all=1, config=lenient)[0] == 0
    # with KEEP_MESH the description's mesh is not looked at
    assert check([0], [desc(mesh=False)], flags=L.RESTART_KEEP_MESH)[0] == 0
    assert check([0], [desc(v=None)], flags=L.RESTART_KEEP_MESH)[0] == 0
    assert check([3], [good], flags=L.RESTART_KEEP_MESH)[0] == -1


def test_cpp_facade_restart_objects_compiles(tmp_path):
    src = """
#include <ROFT/Filters.h>
int main(int argc, char**)
{
    if (argc > 100) {   // (never: the program is compiled and linked, not run against a device)
        roft_config cfg{};
        roft_default_config(&cfg, 320, 240, ROFT_FLOW_F32C2);
        ROFT::ROFTFilterBatch engine(cfg);
        roft_object_desc d{};
        roft_default_object(&d);
        engine.add_object(d);
        engine.restart_objects({0}, {d});
        engine.restart_objects(std::vector<int>{0}, std::vector<roft_object_desc>{d}, ROFT_RESTART_KEEP_MESH);
        roft_engine_restart_stats st{};
        return roft_engine_get_restart_stats(engine.engine(), &st) + (int)st.calls;
    }
    return 0;
}
"""
    (tmp_path / "r.cpp").write_text(src)
    L.build()
    exe = str(tmp_path / "r")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include", "compat"), "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "r.cpp"), "-o", exe, "-L", CSRC, "-lroft_hip", "-Wl,-rpath," + CSRC, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([exe]).returncode == 0


def test_tracker_usage_names_slots(tmp_path):
    L.build()
    exe = str(tmp_path / "ROFT-tracker-batch")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include", "compat"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "track_many.cpp"), "-o", exe, "-L", CSRC, "-lroft_hip", "-Wl,-rpath," + CSRC,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "usage: ROFT-tracker-batch --from config.cfg" in r.stderr and "[--slots N]" in r.stderr
    r = subprocess.run([exe, "--from", "x.cfg", "--log_root", str(tmp_path), "--slots", "0", "--object", str(tmp_path), "box"], capture_output=True, text=True)
    assert r.returncode == 1 and "--slots" in r.stderr
