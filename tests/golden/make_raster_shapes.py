#!/usr/bin/env python3
"""Writes tests/golden/raster_shapes.json: the LDS shapes the three rasteriser launchers derived BEFORE raster_shape.h existed, over a
grid of meshes, targets and window_pixels.  Run with a checkout of that commit and the libroft_hip.so built from it:

    python tests/golden/make_raster_shapes.py <parent checkout> <parent libroft_hip.so>

It restates nothing: quality_window_shape and vsd_shape are called in the parent's library, and the scene renderer's block -- which
was no function -- is compiled from the parent's own lines of scene.hip.  tests/cpp/raster_shape_check.cpp compares raster_shape.h
with the file.  Rows (all integers; an output a refused call left unset is 0):
    quality  n_verts, width, window_pixels -> ok, vcache_cap, win_cap, lds
    vsd      n_verts, width, window_pixels -> ok, vcache_cap, win_alloc, win_cap, lds
    scene    n_verts, target pixels, window_pixels -> vcache_cap, win_cap, lds        (targets: one row, and 4 : 3)"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
N_VERTS = [0, 8, 3000, 7600, 7700, 12900, 13100, 100000]
WIDTHS = [32, 320, 640, 4096, 20000, 39000, 40000]
WINDOW_PIXELS = [0, 1, 500, 10 ** 6]

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "raster.h"
namespace roft {
bool quality_window_shape(int max_verts, int tile_w, int window_pixels, int& vcache_cap, int& win_cap, size_t& lds);
bool vsd_shape(int n_verts, int width, int window_pixels, int& vcache_cap, int& win_alloc, int& win_cap, size_t& lds);
}
using namespace roft;
int main(int argc, char** argv)
{
    const int nv = atoi(argv[2]), wp = atoi(argv[4]);
    const size_t WH = (size_t)atoll(argv[3]);
    int vc = 0, wa = 0, wc = 0;
    size_t lds = 0;
    if (argv[1][0] == 'q') {
        const bool ok = quality_window_shape(nv, (int)WH, wp, vc, wc, lds);
        printf("%d %d %d %zu\n", ok ? 1 : 0, vc, wc, lds);
    } else if (argv[1][0] == 'v') {
        const bool ok = vsd_shape(nv, (int)WH, wp, vc, wa, wc, lds);
        printf("%d %d %d %d %zu\n", ok ? 1 : 0, vc, wa, wc, lds);
    } else {
        struct { int max_verts; } r_{nv}, *r = &r_;
        struct { int window_pixels; } d_{wp}, *d = &d_;
        struct { int vcache_cap, win_cap; } a;
#include "scene_block.inc"
        printf("%d %d %zu\n", a.vcache_cap, a.win_cap, lds);
    }
    return 0;
}
"""


def main():
    parent, so = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    csrc = os.path.join(parent, "roft_amd", "csrc")
    lines = open(os.path.join(csrc, "scene.hip")).read().split("\n")
    first = next(i for i, l in enumerate(lines) if "budget = kRasterLdsBudget" in l)
    last = next(i for i, l in enumerate(lines) if l.strip().startswith("const size_t lds ="))
    with tempfile.TemporaryDirectory() as tmp:
        open(os.path.join(tmp, "scene_block.inc"), "w").write("\n".join(lines[first:last + 1]) + "\n")
        open(os.path.join(tmp, "gen.hip"), "w").write(PROGRAM)
        exe = os.path.join(tmp, "gen")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", csrc, "-I", tmp, os.path.join(tmp, "gen.hip"),
                               "-Wl," + so, "-Wl,-rpath," + os.path.dirname(so), "-o", exe])

        def run(which, nv, width, wp):
            return [nv, width, wp] + [int(v) for v in subprocess.check_output([exe, which, str(nv), str(width), str(wp)]).split()]

        grid = [(nv, w, wp) for nv in N_VERTS for w in WIDTHS for wp in WINDOW_PIXELS]
        out = dict(quality=[run("q", *g) for g in grid], vsd=[run("v", *g) for g in grid],
                   scene=[run("s", nv, px, wp) for nv, w, wp in grid for px in (w, w * (3 * w // 4))])
    with open(os.path.join(HERE, "raster_shapes.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in v)) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main()
