"""The C-ABI shared library and its ctypes binding: every struct, function and integer constant include/roft_engine.h declares
(tests/abi_header.py reads them) has its mirror, its row and its name in roft_amd/_lib.py, and they agree; the library exports
every symbol and has no CPU fallback (compute entry points fail loudly without a HIP device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header
from roft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mirrors():
    """{C struct name: [its ctypes mirrors]}: every Structure of the binding, paired by the C type it names"""
    out = {}
    for cls in vars(L).values():
        if isinstance(cls, type) and issubclass(cls, C.Structure) and cls is not C.Structure:
            out.setdefault(getattr(cls, "_c_name_", "(no _c_name_: %s)" % cls.__name__), []).append(cls)
    return out


def test_every_struct_has_one_mirror_with_the_layout_gcc_gives_it(tmp_path):
    """Field names and order, every offset, every field's size and the struct's size, for every struct typedef of the header."""
    structs, layouts, mirrors = abi_header.structs(), abi_header.layouts(tmp_path), _mirrors()
    assert len(structs) >= 26
    assert sorted(mirrors) == sorted(s.name for s in structs), "a struct without a mirror, or a mirror of no struct"
    for s in structs:
        assert len(mirrors[s.name]) == 1, s.name
        mirror, (size, fields) = mirrors[s.name][0], layouts[s.name]
        assert [f for f, _ in mirror._fields_] == s.fields, s.name
        assert {f: (getattr(mirror, f).offset, getattr(mirror, f).size) for f in s.fields} == fields, s.name
        assert C.sizeof(mirror) == size, s.name


SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "long": C.c_long, "long long": C.c_longlong,
           "unsigned long long": C.c_ulonglong, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "char": C.c_char,
           "void": None}
# struct pointers the binding hands over as plain addresses (numpy buffers of records), as it always has
STRUCTS_AS_ADDRESSES = {("roft_engine_get_quality", "out")}


def _accepted(function, param, ctype, mirrors):
    """the ctypes a row may use for one C parameter (param None: the return value)"""
    base, depth = ctype
    if base in abi_header.opaque_handles():          # a handle is an address, an out-parameter for one a pointer to an address
        return {1: {C.c_void_p}, 2: {C.POINTER(C.c_void_p)}}[depth]
    if base in mirrors:                              # structs are passed by pointer only
        assert depth == 1, (function, param)
        return {C.c_void_p} if (function, param) in STRUCTS_AS_ADDRESSES else {C.POINTER(mirrors[base][0])}
    if depth == 0:
        return {SCALARS[base]}
    inner = _accepted(function, param, abi_header.CType(base, depth - 1), mirrors) - {None}
    return {C.c_void_p} | {C.POINTER(t) for t in inner} | ({C.c_char_p} if (base, depth) == ("char", 1) else set())


def test_library_builds_and_exports_every_declared_symbol():
    """... and every prototype has exactly one row of L.ABI, whose restype and argtypes agree with it, parameter by parameter."""
    L.build()
    lib = L.lib()
    protos, mirrors = abi_header.prototypes(), _mirrors()
    assert len(protos) >= 99
    # (the parser misses nothing that looks like a call of a roft_ name)
    assert sorted(p.name for p in protos) == sorted(set(re.findall(r"\b(roft_[a-z_0-9]+)\s*\(", abi_header.code())))
    assert sorted(L.ABI_SYMBOLS) == sorted(p.name for p in protos) and len(set(L.ABI_SYMBOLS)) == len(L.ABI)
    rows = {f.name: f for f in L.ABI}
    for p in protos:
        assert hasattr(lib, p.name), "libroft_hip.so does not export %s" % p.name
        row, fn = rows[p.name], getattr(lib, p.name)
        assert (fn.restype, list(fn.argtypes)) == (row.restype, list(row.argtypes)), p.name + ": lib() did not apply the row"
        assert row.restype in _accepted(p.name, None, p.ret, mirrors), p.name
        assert len(row.argtypes) == len(p.params), p.name
        for got, (param, ctype) in zip(row.argtypes, p.params):
            assert got in _accepted(p.name, param, ctype, mirrors), (p.name, param, got)
        assert row.optional == (p.name.startswith("roft_debug_") or p.name in L.NEWER_SYMBOLS), p.name
    assert not any(f.optional for f in L.ABI if f.name in ("roft_abi_version", "roft_last_error_string", "roft_device_count"))


def test_every_integer_define_has_its_constant():
    values, others = abi_header.defines()
    assert len(values) >= 30
    assert others == ["ROFT_ENGINE_H"], "the include guard is the only define without an integer value"
    for name, value in values.items():
        assert getattr(L, name[len("ROFT_"):], None) == value, name


def test_defaults_follow_the_reference_config():
    """config/config_fast_ycb.cfg + test/test.sh:70-71 defaults."""
    lib = L.lib()
    cfg = L.Config()
    assert lib.roft_default_config(C.byref(cfg), 1280, 720, L.FLOW_S16C2) == 0
    assert (cfg.flow_grid, cfg.flow_scale) == (4, 32.0)
    assert abs(cfg.cam.fx - 1229.4285612615463) < 1e-9 and cfg.cam.cx == 640.0 and cfg.cam.cy == 360.0
    assert abs(cfg.sample_time - 1 / 30) < 1e-12 and (cfg.ut.alpha, cfg.ut.beta, cfg.ut.kappa) == (1.0, 2.0, 0.0)
    assert cfg.depth_maximum == 2.0 and cfg.subsampling_radius == 35.0 and cfg.flow_weighting == 1
    assert (cfg.use_pose, cfg.use_pose_resync, cfg.use_velocity, cfg.outlier_rejection, cfg.flow_aided_segmentation) == (1,) * 5
    assert cfg.mask_frames_between == 6 and cfg.pose_frames_between == 6
    o = L.ObjectDesc()
    assert lib.roft_default_object(C.byref(o)) == 0
    assert list(o.p_cov0_diag) == [1e-3] * 12 and list(o.v_q_diag) == [0.1] * 6
    assert list(o.p_meas_cov_v) == [0.1] * 3 and list(o.p_meas_cov_w) == [1e-4] * 3
    assert list(o.p_meas_cov_x) == [1e-3] * 3 and list(o.p_meas_cov_q) == [1e-4] * 3
    assert list(o.v_meas_cov_flow) == [1.0, 1.0] and o.p_mean0[9] == 1.0


def test_no_cpu_fallback():
    lib = L.lib()
    if lib.roft_device_count() > 0:
        pytest.skip("a HIP device is present")
    from roft_amd import ops
    with pytest.raises(L.RoftError):
        ops.kf_predict(np.zeros(6), np.eye(6), np.ones(6))
    with pytest.raises(L.RoftError):
        ops.mask_propagate(np.zeros((64, 64), np.uint8), [])
    from roft_amd import engine as E
    with pytest.raises(L.RoftError):
        E.ROFTFilterBatch(E.default_config(640, 480))
    assert b"no HIP device" in lib.roft_last_error_string() or b"CPU" in lib.roft_last_error_string()


def test_argument_validation_without_device():
    lib = L.lib()
    assert lib.roft_default_config(None, 640, 480, L.FLOW_F32C2) == -1
    assert lib.roft_pose_process_noise(None, None, 0.1, None) == -1
    Q = np.zeros((9, 9))
    a = np.ones(3)
    assert lib.roft_pose_process_noise(a.ctypes.data, a.ctypes.data, 0.5, Q.ctypes.data) == 0
    assert Q[0, 0] == 0.5 and Q[3, 3] == 1.0 and Q[0, 6] == 0.125


def _plan(cfg, pose_valid):
    lib = L.lib()
    n = len(pose_valid)
    pv = (C.c_int * n)(*[int(v) for v in pose_valid])
    ns, nc, out = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    slots = (C.c_int * (n * 10))()
    assert lib.roft_debug_plan(C.byref(cfg), pv, n, ns, nc, out, slots) == 0
    return list(ns), list(nc), list(out), np.array(list(slots)).reshape(n, 10)


def test_frame_program_matches_the_oracle_state_machine(oracle):
    """Host logic, no GPU: the per-frame UKF program (re-sync replays, outlier step, velocity deque) built by
    the engine has exactly as many corrections per frame as the oracle's ROFTFilter restatement performs."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import util
    for seed, drop in ((71, 0.0), (72, 0.5)):
        st = util.stream(seed, 40, scale=8, pose_drop_prob=drop)
        for over in (dict(), dict(use_pose_resync=0), dict(outlier_rejection=0), dict(use_pose=0, use_pose_resync=0, outlier_rejection=0)):
            ref = util.run_oracle_tracker(oracle, st, **over)
            cfg = L.Config()
            L.lib().roft_default_config(C.byref(cfg), 640, 480, L.FLOW_F32C2)
            for k, v in over.items():
                setattr(cfg, k, v)
            ns, nc, out, slots = _plan(cfg, st.pose_valid)
            from oracle import binding as ob
            cfg_o = util.oracle_config(ob, st, **over)
            trk = ob.Tracker(cfg_o, *st.mesh)
            want = []
            for k in range(40):
                depth, flow, mask, pose = util.frame_inputs(st, k)
                want.append(trk.step(st.dt, depth, flow, mask, pose).n_ukf_corrections)
            trk.close()
            assert nc == want, (seed, over)
            tested = [k for k in range(40) if out[k] >= 0]
            assert tested == [k for k, r in enumerate(ref) if r["sel"] >= 0]
    # steady state with re-sync: a pose frame replays the D + 1 = 7 buffered twists, oldest first
    cfg = L.Config()
    L.lib().roft_default_config(C.byref(cfg), 640, 480, L.FLOW_F32C2)
    pv = [k % 6 == 0 for k in range(20)]
    ns, nc, out, slots = _plan(cfg, pv)
    assert ns[12] == 7 and nc[12] == 8 and out[12] == 0
    assert list(slots[12][:7]) == [6, 7, 8, 9, 10, 11, 12]
    assert ns[13] == 1 and nc[13] == 1 and out[13] == -1 and slots[13][0] == 13
