#!/usr/bin/env python3
"""What a symmetry group costs the engine (include/roft_engine.h section 3h): the same device-resident streams tracked by an engine
whose objects all have a box's four-element group and by one without groups, in one process, alternated over --rounds rounds.

  bench_symmetry.py [--objects 64] [--frames 48] [--batch 8] [--scale 1] [--rounds 5] [--out FILE]

Every object is fed the same few streams (the engine does the same work per object whatever the content).  A round runs all frames
through a new engine of each kind and times submit + step + the final sync; the first --warmup frames are not timed.  Prints, and
writes to --out, the frames per second of every round and the medians."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from roft_amd import _lib as L  # noqa: E402
from roft_amd import engine as E  # noqa: E402
from roft_amd import synth  # noqa: E402

D2 = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0, 1]], float)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=64)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=4, help="distinct streams, dealt to the objects in turn")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    L.require_device()
    import util
    n = args.frames
    streams = [util.to_device(util.stream(9100 + i, n, scale=args.scale, device="cuda", pose_drop_prob=0.0)) for i in range(args.distinct)]
    per_object = [streams[o % args.distinct] for o in range(args.objects)]
    st0 = streams[0]

    def one_run(group):
        cfg = E.default_config(st0.camera.width, st0.camera.height, st0.flow_type, max_objects=args.objects, max_batch_frames=args.batch)
        c = st0.camera
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = c.fx, c.fy, c.cx, c.cy
        eng = E.ROFTFilterBatch(cfg)
        for o, st in enumerate(per_object):
            d = E.default_object()
            for i, v in enumerate(synth.initial_pose_from_stream(st)):
                d.p_mean0[i] = v
            eng.add_object(d, *st.mesh)
            if group is not None:
                eng.set_symmetry(o, group)
        batches = [eng.build_batch([[util.device_frame(st, k + j) for st in per_object] for j in range(min(args.batch, n - k))])
                   for k in range(0, n, args.batch)]
        t0, timed = None, 0
        done = 0
        for arr, keep, T in batches:
            if t0 is None and done >= args.warmup:
                eng.sync()
                t0 = time.perf_counter()
            eng.submit_batch_raw(arr, T)
            eng.step()
            done += T
            if t0 is not None:
                timed += T
        eng.sync()
        dt = time.perf_counter() - t0
        pose = np.array(eng.outputs()[0].pose)
        eng.close()
        return timed * args.objects / dt, pose

    rounds = []
    for r in range(args.rounds):
        fps_none, pose_none = one_run(None)
        fps_sym, pose_sym = one_run(D2)
        rounds.append(dict(round=r, object_frames_per_s_none=fps_none, object_frames_per_s_group=fps_sym,
                           same_final_pose=bool(np.abs(pose_none - pose_sym).max() < 1e-6)))
        print(json.dumps(rounds[-1]), flush=True)
    med = lambda k: float(np.median([x[k] for x in rounds]))   # noqa: E731
    record = dict(tool="tools/bench_symmetry.py", objects=args.objects, frames=n, warmup=args.warmup, batch=args.batch,
                  image=[st0.camera.width, st0.camera.height], group_elements=len(D2), rounds=rounds,
                  median_object_frames_per_s_none=med("object_frames_per_s_none"), median_object_frames_per_s_group=med("object_frames_per_s_group"))
    record["group_over_none"] = record["median_object_frames_per_s_group"] / record["median_object_frames_per_s_none"]
    print(json.dumps({k: v for k, v in record.items() if k != "rounds"}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
