#!/usr/bin/env python3
"""Compares two directories written by `bench.py --dump-outputs DIR` (old and new library on the same seeded inputs):
  python tools/compare_dumps.py DIR_A DIR_B [--atol 1e-9]
Flow point counts, outlier decisions and the mask arrays must be identical; the other arrays (poses, twists, covariances,
likelihoods) are reported with their largest absolute difference and must be identical or below --atol.
Exit status 0 when all of that holds, 1 otherwise."""
import argparse
import os
import sys

import numpy as np

EXACT = ("n_flow_points", "outlier_selected", "mask_pixels", "mask_sample")   # stored as floats, compared as what they count


def main():
    p = argparse.ArgumentParser()
    p.add_argument("a")
    p.add_argument("b")
    p.add_argument("--atol", type=float, default=1e-9, help="bar on max |a - b| of the floating-point arrays")
    args = p.parse_args()
    names = sorted(f for f in os.listdir(args.a) if f.endswith(".npy"))
    other = sorted(f for f in os.listdir(args.b) if f.endswith(".npy"))
    if names != other or not names:
        print("the directories hold different arrays: %s | %s" % (names, other))
        return 1
    bad = 0
    for f in names:
        x, y = np.load(os.path.join(args.a, f)), np.load(os.path.join(args.b, f))
        if x.shape != y.shape or x.dtype != y.dtype:
            print("%-24s shape / dtype differ: %s %s | %s %s" % (f, x.shape, x.dtype, y.shape, y.dtype))
            bad += 1
        elif np.array_equal(x, y, equal_nan=False):
            print("%-24s identical  %s %s" % (f, x.dtype, x.shape))
        elif np.issubdtype(x.dtype, np.floating) and f[:-4] not in EXACT:
            d = float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64))))
            ok = np.isfinite(x).all() and np.isfinite(y).all() and d < args.atol
            print("%-24s max |a - b| = %.3g  %s" % (f, d, "(below %g)" % args.atol if ok else "ABOVE THE BAR"))
            bad += 0 if ok else 1
        else:
            print("%-24s DIFFERS in %d of %d entries (must be identical)" % (f, int(np.sum(x != y)), x.size))
            bad += 1
    print("dumps agree" if not bad else "%d arrays disagree" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
