#!/usr/bin/env python3
"""Shader-cycle profile of the phases of one ukf_step launch.  Needs a library built with -DROFT_UKF_PROFILE:
  make -C roft_amd/csrc clean && make -C roft_amd/csrc CXXFLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DROFT_UKF_PROFILE"
Slots: 0 load, 1 process noise, 2 prediction square root, 3 fan-out + motion, 4 means, 5 covariance, 6 store,
7 correction square root, 8 fan-out + measurement, 9 means/deviations, 10 Py/Pxy, 11 Cholesky, 12 gain + update."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, util
from roft_amd import engine as E, synth, _lib as L
import test_engine_gpu as T
# --symmetry: the cost of the equivalent-pose selection (include/roft_engine.h section 3h), which is counted in slot 6.  Without
# re-synchronisation a pose frame is ONE step (prediction, selection, two corrections), so the frame's last step is the pose step:
# frames 6 and 12 are printed, first without a group, then with a box's four-element group, the pose of frame 12 delivered flipped
# by a half turn (the selection then rewrites the measurement).
SYM = "--symmetry" in sys.argv
if SYM:
    import symmetry_ref as S
    for group in (None, S.d2_group()):
        streams=[util.stream(100,14,scale=2,pose_drop_prob=0.0)]
        eng=T.make_engine(streams, use_pose_resync=0)
        if group is not None: eng.set_symmetry(0, group)
        for k in range(14):
            depth,flow,mask,pose=util.frame_inputs(streams[0],k)
            if k==12 and pose is not None: pose=S.flip_pose(pose[0],pose[1],S.d2_group()[1])
            eng.submit([dict(depth=depth,flow=flow,mask=mask,pose=pose,dt=streams[0].dt)]); eng.step(); eng.sync()
            buf=(C.c_longlong*32)()
            L.lib().roft_debug_get_dbg(eng._h,0,buf)
            if k in (6,12):
                print(json.dumps(dict(group=0 if group is None else len(group), frame=k, slot6_cycles=int(buf[6]), slots_0_12=[int(x) for x in buf][:13], step_cycles=int(sum(list(buf)[:13])))))
        eng.close()
    sys.exit(0)
streams=[util.stream(100,14,scale=2)]
eng=T.make_engine(streams)
for k in range(14):
    depth,flow,mask,pose=util.frame_inputs(streams[0],k)
    eng.submit([dict(depth=depth,flow=flow,mask=mask,pose=pose,dt=streams[0].dt)]); eng.step(); eng.sync()
    if k in (4,5,11,13):
        # read ObjState.dbg: find offset via struct size: use hipMemcpy through roft_get_state? not exposed -> use debug export
        buf=(C.c_longlong*32)()
        L.lib().roft_debug_get_dbg(eng._h,0,buf)
        print(k,[int(x) for x in buf][:13], 'sweeps n12/n4/n10:', [int(x) for x in buf][16:19], 'corr guard th/wv/xx (1e-9):', [int(x) for x in buf][20:23], 'sub 23..26 (means | sigma perturbation | K solve | KPy):', [int(x) for x in buf][23:27])
