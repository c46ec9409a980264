#!/usr/bin/env python3
"""Writes tests/golden/relocalise_traces.json: roft_amd/relocalise.compass_search over the exact CPU reference of a quality record
(tests/quality_ref.py on the oracle's render) for the two cases of tests/relocalise_cases.py -- per case the trace and the final
pose, its doubles as hex strings.  No GPU.  tests/test_pose_hypotheses_cpu.py reruns it; tests/test_pose_hypotheses_gpu.py
reproduces it on the device."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import mesh_zoo                      # noqa: E402
import relocalise_cases as rc        # noqa: E402
from oracle import binding as ob     # noqa: E402
from roft_amd import relocalise      # noqa: E402


def main():
    ob.build()
    out = {}
    mesh = mesh_zoo.box()
    for name in rc.CASES:
        mask, depth = rc.scene(ob, name)
        _, ocam = rc.cameras(ob)
        x0, q0 = rc.start_pose(name)
        x, q, trace = relocalise.compass_search(rc.cpu_scorer(ob, ocam, rc.D, depth, mask > 1, mesh), x0, q0)
        xt, qt = rc.CASES[name][:2]
        print(name, "%d rounds, mean vertex distance %.2f -> %.2f mm" % (len(trace), 1e3 * rc.mean_vertex_distance(mesh[0], x0, q0, xt, qt),
                                                                          1e3 * rc.mean_vertex_distance(mesh[0], x, q, xt, qt)))
        out[name] = dict(trace=[list(t) for t in trace], x=[float.hex(float(v)) for v in x], q=[float.hex(float(v)) for v in q])
    with open(rc.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
