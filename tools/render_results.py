#!/usr/bin/env python3
"""Draws tracked poses over the camera frames of a sequence: the reference's `video` and `thumbnail` output heads
(evaluation/results_renderer.py:591-778 over tools/object_renderer/src/renderer.cpp), as frames, on the MI355X scene renderer
(roft_amd.ops.SceneRenderer).

  render_results.py --root SEQ --mesh model.obj --poses FILE [--mesh OBJ --poses FILE ...] --out DIR
                    [--frames i,j,k] [--crop x0 y0 x1 y1] [--thumbnail FILE] [--ids DIR] [--first-frame N]
                    [--frames-per-call 16] [--color] [--dry-run] [--lens k1,k2,p1,p2,k3 [--lens-camera fx,fy,cx,cy]]

SEQ holds rgb/<i>.png and cam_K.json.  Every --mesh / --poses pair is one pose source: FILE is a `pose_estimate` log of this
project or of the reference (13 columns, the pose in the last seven) or a `poses.txt` (7 columns), rows `x y z axis angle`.  Row k
of a source belongs to frame --first-frame + k.  All sources are drawn into ONE scene per frame over the grayed frame (--color:
over the frame as it is) and written to DIR/<i>.png.

  --frames     only these frame indices (default: every frame that every source has a row for)
  --crop       written images and thumbnails are cut to x0 <= x < x1, y0 <= y < y1
  --thumbnail  the contact sheet of results_renderer.py:748-776: the plain RGB frames in the first row, one row per pose source
               (that source alone) under it, 10-pixel white borders.  (The reference's sheet has one spare blank row at the bottom,
               `1 + len(paths)` rows with the RGB path already among the paths; this one has not.)
  --ids        instance maps as 8-bit PNGs DIR/<i>.png: the index of the pose source per pixel, 255 = background
  --lens       rgb/<i>.png are the sensor's DISTORTED frames with these Brown-Conrady coefficients (--lens-camera: the sensor's
               intrinsics where they differ from cam_K.json's): every background frame is rectified into the pinhole camera of
               cam_K.json with the 3-channel operator (roft_rectify; include/roft_engine.h section 3g), so the overlays line up
               (a list that starts with a minus sign is written --lens=-0.05,0.01,...)
  --dry-run    reads the poses, prints the plan as one JSON line and renders nothing (needs no GPU)

An invalid pose (x = y = z = 0: the reference's spelling of "no detection") repeats the last valid pose of its source, as
renderer.cpp:83-113 does; frames before the first valid pose show the background only.  (The reference drops those leading frames
and thereby shifts every later image by their number; here frame i is always image i.)

The sequence is processed in chunks of --frames-per-call frames, so memory does not grow with its length.  There is no ffmpeg on
the MI355X machines this was written for: the frames are not assembled into an mp4.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

BORDER = 10   # results_renderer.py:755


def load_pose_source(path):
    """(pose [F, 7] = x y z, q wxyz; valid [F]) of a pose_estimate log (>= 13 columns: velocities first) or a poses.txt."""
    from roft_amd import io
    with open(path) as f:
        first = f.readline().split()
    return io.read_poses(path, skip_cols=6 if len(first) >= 13 else 0)


def fill_poses(pose, valid):
    """Invalid rows repeat the last valid row; rows before the first valid one are not drawn.  Returns (pose [F, 7], drawn [F]):
    row k stays row k."""
    pose, valid = np.array(pose, float).reshape(-1, 7), np.asarray(valid, bool)
    out, drawn = pose.copy(), np.zeros(len(pose), bool)
    last = None
    for k in range(len(pose)):
        if valid[k]:
            last = pose[k]
        if last is not None:
            out[k], drawn[k] = last, True
    return out, drawn


def chunks(frames, size):
    frames = list(frames)
    return [frames[i:i + size] for i in range(0, len(frames), size)]


def crop_image(img, crop):
    if crop is None:
        return img
    x0, y0, x1, y1 = crop
    return img[y0:y1, x0:x1]


def thumbnail_sheet(rows, border=BORDER):
    """rows: one list of equally sized [h, w, 3] images per sheet row (the RGB frames first, then one row per source)."""
    n_rows, n_cols = len(rows), len(rows[0])
    h, w = rows[0][0].shape[:2]
    sheet = np.full(((n_rows - 1) * border + h * n_rows, (n_cols - 1) * border + w * n_cols, 3), 255, np.uint8)
    for i, row in enumerate(rows):
        for j, img in enumerate(row):
            sheet[(h + border) * i:(h + border) * i + h, (w + border) * j:(w + border) * j + w] = img
    return sheet


def plan(args):
    """What will be rendered: the filled poses of every source and the frame list."""
    if not args.mesh or not args.poses or len(args.mesh) != len(args.poses):
        raise SystemExit("every --mesh needs its --poses (and the other way round)")
    sources = []
    for path in args.poses:
        pose, valid = load_pose_source(path)
        sources.append(fill_poses(pose, valid))
    n_rows = min(len(p) for p, _ in sources)
    if args.frames:
        frames = [int(v) for v in args.frames.split(",") if v != ""]
    else:
        frames = list(range(args.first_frame, args.first_frame + n_rows))
    for i in frames:
        if not 0 <= i - args.first_frame < n_rows:
            raise SystemExit("frame %d has no pose row in every source (rows cover %d .. %d)" % (i, args.first_frame, args.first_frame + n_rows - 1))
    return sources, frames


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True)
    ap.add_argument("--mesh", action="append")
    ap.add_argument("--poses", action="append")
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", default=None)
    ap.add_argument("--crop", type=int, nargs=4, default=None, metavar=("X0", "Y0", "X1", "Y1"))
    ap.add_argument("--thumbnail", default=None)
    ap.add_argument("--ids", default=None)
    ap.add_argument("--first-frame", type=int, default=0)
    ap.add_argument("--frames-per-call", type=int, default=16)
    ap.add_argument("--color", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--lens", default=None, metavar="K1,K2,P1,P2,K3")
    ap.add_argument("--lens-camera", default=None, metavar="FX,FY,CX,CY")
    args = ap.parse_args(argv)
    dist = sensor = None
    if args.lens_camera is not None and args.lens is None:
        raise SystemExit("--lens-camera needs --lens")
    if args.lens is not None:
        try:
            dist = [float(v) for v in args.lens.split(",")]
            sensor = [float(v) for v in args.lens_camera.split(",")] if args.lens_camera else None
        except ValueError:
            dist = []
        if len(dist) != 5 or (sensor is not None and len(sensor) != 4):
            raise SystemExit("--lens takes k1,k2,p1,p2,k3 and --lens-camera fx,fy,cx,cy")
    sources, frames = plan(args)
    cam_k = json.load(open(os.path.join(args.root, "cam_K.json")))
    W, H = int(cam_k["width"]), int(cam_k["height"])
    if args.crop and not (0 <= args.crop[0] < args.crop[2] <= W and 0 <= args.crop[1] < args.crop[3] <= H):
        raise SystemExit("--crop must lie inside the %d x %d image" % (W, H))
    report = dict(frames=frames, sources=len(sources), chunks=len(chunks(frames, args.frames_per_call)), width=W, height=H,
                  background_only=[[i for i in frames if not drawn[i - args.first_frame]] for _, drawn in sources])
    if dist:
        report["lens"] = dist
    if args.dry_run:
        print(json.dumps(report))
        return 0
    if not (args.out or args.thumbnail or args.ids):
        raise SystemExit("nothing to write: give --out, --thumbnail or --ids")

    from roft_amd import _lib as L
    from roft_amd import io, ops
    L.require_device()
    cam = L.Camera(W, H, cam_k["fx"], cam_k["fy"], cam_k["cx"], cam_k["cy"])
    meshes = [io.load_obj(p) for p in args.mesh]
    for d in (args.out, args.ids):
        if d:
            os.makedirs(d, exist_ok=True)
    renderer = ops.SceneRenderer(cam, meshes, max_frames_per_call=args.frames_per_call)
    lens = ops.lens(L.Camera(W, H, *sensor) if sensor else cam, dist) if dist else None
    n_src = len(sources)
    sheet_rows = [[] for _ in range(1 + n_src)] if args.thumbnail else None
    for chunk in chunks(frames, args.frames_per_call):
        rows = [i - args.first_frame for i in chunk]
        bg = np.stack([io.read_png(os.path.join(args.root, "rgb", "%d.png" % i)) for i in chunk])
        if bg.ndim == 3:
            bg = np.repeat(bg[..., None], 3, axis=3)
        bg = np.ascontiguousarray(bg[..., :3])
        if lens is not None:
            bg = np.stack([ops.rectify(b, lens, cam, kind=L.RECTIFY_RGB8) for b in bg])
        poses = np.stack([p[rows] for p, _ in sources], 1)        # [chunk, source, 7]
        valid = np.stack([d[rows] for _, d in sources], 1)
        if args.out or args.ids:
            want = (("rgb",) if args.out else ()) + (("instance",) if args.ids else ())
            out = renderer.render(np.arange(n_src), poses, valid=valid, background=bg, gray_background=not args.color, outputs=want)
            for k, i in enumerate(chunk):
                if args.out:
                    io.write_png(os.path.join(args.out, "%d.png" % i), crop_image(out["rgb"][k], args.crop))
                if args.ids:
                    io.write_png(os.path.join(args.ids, "%d.png" % i), crop_image(np.where(out["instance"][k] < 0, 255, out["instance"][k]).astype(np.uint8), args.crop))
        if args.thumbnail:
            sheet_rows[0] += [crop_image(b, args.crop) for b in bg]
            for s in range(n_src):
                # (the source keeps its place among the instances, so it keeps its colour)
                only = np.zeros_like(valid)
                only[:, s] = valid[:, s]
                one = renderer.render(np.arange(n_src), poses, valid=only, background=bg, gray_background=not args.color, outputs=("rgb",))
                sheet_rows[1 + s] += [crop_image(img, args.crop) for img in one["rgb"]]
    renderer.close()
    if args.thumbnail:
        io.write_png(args.thumbnail, thumbnail_sheet(sheet_rows))
        report["thumbnail"] = args.thumbnail
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
