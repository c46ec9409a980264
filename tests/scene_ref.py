"""CPU statement of the scene renderer (include/roft_engine.h section 3b) in float32 numpy: the render contract's rasteriser
(oracle/ro_render.c, operation by operation) keeping per pixel the smallest key (depth bits << 32 | instance << 24 | triangle),
and the shading / blend formulas of the header.  tests/test_scene_cpu.py anchors its depth plane to the oracle bit for bit.

Every array that takes part in the arithmetic is float32 and every expression is written in the order of the C code, so numpy
rounds each operation exactly as the compiler (built with -ffp-contract=off) does."""
import numpy as np

F32 = np.float32
KEY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
PALETTE = np.array([[230, 60, 50], [50, 140, 230], [60, 190, 80], [240, 180, 40],
                    [170, 80, 200], [40, 200, 200], [240, 120, 170], [150, 150, 150]], F32)
DEFAULT_OPACITY, DEFAULT_AMBIENT = 0.75, 0.35


class Cam:
    def __init__(self, width, height, fx, fy, cx, cy):
        self.width, self.height, self.fx, self.fy, self.cx, self.cy = int(width), int(height), float(fx), float(fy), float(cx), float(cy)


def pose_f32(pose7):
    """make_pose: the rotation of the quaternion as given, in double, rounded to float."""
    x, y, z, w, qx, qy, qz = [np.float64(v) for v in pose7]
    with np.errstate(all="ignore"):
        R = np.array([1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - w * qz), 2.0 * (qx * qz + w * qy),
                      2.0 * (qx * qy + w * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - w * qx),
                      2.0 * (qx * qz - w * qy), 2.0 * (qy * qz + w * qx), 1.0 - 2.0 * (qx * qx + qy * qy)], np.float64).astype(F32)
        t = np.array([x, y, z], np.float64).astype(F32)
    return R, t


def eye_points(verts, R, t):
    v = np.ascontiguousarray(verts, F32)
    X = ((R[0] * v[:, 0] + R[1] * v[:, 1]) + R[2] * v[:, 2]) + t[0]
    Y = ((R[3] * v[:, 0] + R[4] * v[:, 1]) + R[5] * v[:, 2]) + t[1]
    Z = ((R[6] * v[:, 0] + R[7] * v[:, 1]) + R[8] * v[:, 2]) + t[2]
    return X, Y, Z


def draw_instance(keys, cam, verts, tris, flip, pose7, inst, max_pairs=1 << 21):
    """Merges the fragments of one mesh at one pose into keys [H * W] uint64.  flip: uint8 [n_tris] for a closed mesh, else None."""
    w, h = cam.width, cam.height
    if not np.all(np.isfinite(np.asarray(pose7, np.float64))):
        return
    tris = np.asarray(tris, np.int64)
    with np.errstate(all="ignore"):
        R, t = pose_f32(pose7)
        X, Y, Z = eye_points(verts, R, t)
        fx, fy, cx, cy = F32(cam.fx), F32(cam.fy), F32(cam.cx), F32(cam.cy)
        front = Z > F32(0.001)
        iz = F32(1.0) / Z
        sx = np.where(front, (fx * X) * iz + cx, F32(0.0)).astype(F32)
        sy = np.where(front, (fy * Y) * iz + cy, F32(0.0)).astype(F32)
        if not np.all(front):
            flip = None   # the back-face rule holds only while every vertex is in front of the near plane
        i0, i1, i2 = tris[:, 0], tris[:, 1], tris[:, 2]
        z0, z1, z2 = Z[i0], Z[i1], Z[i2]
        x0, y0, x1, y1, x2, y2 = sx[i0], sy[i0], sx[i1], sy[i1], sx[i2], sy[i2]
        ok = front[i0] & front[i1] & front[i2]
        area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        ok &= (area != 0) & (area == area)
        if flip is not None:
            ok &= ~((area < 0) == (np.asarray(flip) != 0))
        minx, maxx = np.fmin(x0, np.fmin(x1, x2)), np.fmax(x0, np.fmax(x1, x2))
        miny, maxy = np.fmin(y0, np.fmin(y1, y2)), np.fmax(y0, np.fmax(y1, y2))
        fi0, fi1 = np.ceil(minx - F32(0.5)), np.floor(maxx - F32(0.5))
        fj0, fj1 = np.ceil(miny - F32(0.5)), np.floor(maxy - F32(0.5))
        fi0 = np.where(fi0 < 0, F32(0), fi0)
        fj0 = np.where(fj0 < 0, F32(0), fj0)
        fi1 = np.where(fi1 > F32(w - 1), F32(w - 1), fi1)
        fj1 = np.where(fj1 > F32(h - 1), F32(h - 1), fj1)
        ok &= (fi0 <= fi1) & (fj0 <= fj1)
        sel = np.nonzero(ok)[0]
        if sel.size == 0:
            return
        ia, ib, ja, jb = fi0[sel].astype(np.int64), fi1[sel].astype(np.int64), fj0[sel].astype(np.int64), fj1[sel].astype(np.int64)
        bw = ib - ia + 1
        count = bw * (jb - ja + 1)
        # triangles in runs whose candidate pixels stay below max_pairs
        start = 0
        while start < sel.size:
            stop, pairs = start, 0
            while stop < sel.size and (stop == start or pairs + count[stop] <= max_pairs):
                pairs += count[stop]
                stop += 1
            s, n = sel[start:stop], count[start:stop]
            owner = np.repeat(np.arange(start, stop), n)             # index into sel
            local = np.arange(pairs) - np.repeat(np.cumsum(n) - n, n)
            pj = ja[owner] + local // bw[owner]
            pi = ia[owner] + local % bw[owner]
            tk = sel[owner]
            px, py = pi.astype(F32) + F32(0.5), pj.astype(F32) + F32(0.5)
            w0 = (x2 - x1)[tk] * (py - y1[tk]) - (y2 - y1)[tk] * (px - x1[tk])
            w1 = (x0 - x2)[tk] * (py - y2[tk]) - (y0 - y2)[tk] * (px - x2[tk])
            w2 = (x1 - x0)[tk] * (py - y0[tk]) - (y1 - y0)[tk] * (px - x0[tk])
            inside = np.where(area[tk] > 0, (w0 >= 0) & (w1 >= 0) & (w2 >= 0), (w0 <= 0) & (w1 <= 0) & (w2 <= 0))
            p12, p02, p01 = z1 * z2, z0 * z2, z0 * z1
            num = area * (z0 * p12)
            den = (w0 * p12[tk] + w1 * p02[tk]) + w2 * p01[tk]
            z = (num[tk] / den).astype(F32)
            keep = inside & (z > 0)
            zb = z[keep].view(np.uint32).astype(np.uint64)
            key = (zb << np.uint64(32)) | np.uint64(inst << 24) | tk[keep].astype(np.uint64)
            np.minimum.at(keys, pj[keep] * w + pi[keep], key)
            del s
            start = stop


def render_keys(cam, meshes, mesh_index, poses, valid=None):
    """meshes: [(verts, tris, flip or None)]; poses [I, 7]; one frame.  Returns keys [H * W] uint64."""
    keys = np.full(cam.width * cam.height, KEY_EMPTY, np.uint64)
    for inst, m in enumerate(mesh_index):
        if valid is not None and not valid[inst]:
            continue
        verts, tris, flip = meshes[m]
        draw_instance(keys, cam, verts, tris, flip, poses[inst], inst)
    return keys


def maps(keys, cam):
    """(depth f32 0 = background, instance i32 -1, triangle i32 -1) of a key plane."""
    zb = (keys >> np.uint64(32)).astype(np.uint32)
    covered = zb < np.uint32(0x7F800000)
    depth = np.where(covered, zb, np.uint32(0)).astype(np.uint32).view(F32)
    inst = np.where(covered, ((keys >> np.uint64(24)) & np.uint64(0xFF)).astype(np.int64), -1).astype(np.int32)
    tri = np.where(covered, (keys & np.uint64(0xFFFFFF)).astype(np.int64), -1).astype(np.int32)
    shape = (cam.height, cam.width)
    return depth.reshape(shape), inst.reshape(shape), tri.reshape(shape)


def gray(img):
    c = img[..., :3].astype(np.int64)
    y = ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)
    return np.repeat(y[..., None], 3, axis=-1)


def default_styles(n):
    return [(PALETTE[i % 8], DEFAULT_OPACITY, DEFAULT_AMBIENT) for i in range(n)]


def shade(keys, cam, meshes, mesh_index, poses, background=None, gray_background=False, styles=None):
    """rgb u8 [H, W, 3] of a key plane: the header's shading and blend, float32, operation by operation."""
    h, w = cam.height, cam.width
    if background is None:
        bg = np.zeros((h, w, 3), np.uint8)
    else:
        bg = gray(background) if gray_background else np.asarray(background, np.uint8)[..., :3]
    out = bg.reshape(-1, 3).copy()
    _, inst, tri = maps(keys, cam)
    inst, tri = inst.reshape(-1), tri.reshape(-1)
    styles = default_styles(len(mesh_index)) if styles is None else styles
    with np.errstate(all="ignore"):
        for i in np.unique(inst[inst >= 0]):
            verts, tris, _ = meshes[mesh_index[i]]
            tris = np.asarray(tris, np.int64)
            px = np.nonzero(inst == i)[0]
            R, t = pose_f32(poses[i])
            X, Y, Z = eye_points(verts, R, t)
            P = np.stack([X, Y, Z], 1)
            c = tris[tri[px]]
            a, b = P[c[:, 1]] - P[c[:, 0]], P[c[:, 2]] - P[c[:, 0]]
            nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
            ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
            nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
            length = np.sqrt((nx * nx + ny * ny) + nz * nz)
            good = (length > 0) & (length < np.inf)
            s = np.where(good, np.abs(nz) / np.where(good, length, F32(1)), F32(0)).astype(F32)
            tint, opacity, ambient = styles[i]
            tint, opacity, ambient = np.asarray(tint, F32), F32(opacity), F32(ambient)
            level = ambient + (F32(1) - ambient) * s
            for ch in range(3):
                col = opacity * (tint[ch] * level) + (F32(1) - opacity) * out[px, ch].astype(F32)
                assert col.dtype == F32
                out[px, ch] = np.clip(np.floor(col + F32(0.5)), 0, 255).astype(np.uint8)
    return out.reshape(h, w, 3)


def render(cam, meshes, mesh_index, poses, valid=None, background=None, gray_background=False, styles=None):
    """One frame: dict(rgb, depth, instance, triangle) as roft_scene_render returns them."""
    keys = render_keys(cam, meshes, mesh_index, poses, valid)
    depth, inst, tri = maps(keys, cam)
    return dict(rgb=shade(keys, cam, meshes, mesh_index, poses, background, gray_background, styles), depth=depth, instance=inst, triangle=tri)
