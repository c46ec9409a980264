"""Reference of the VSD score, written from the text of include/roft_engine.h (section 3i), not from the kernel and not from
roft_amd/metrics.py: the two renders come from the oracle's render_depth at divider 1 (pinned bit for bit against the HIP rasteriser
elsewhere), and every pixel that a render covers is scored on its own in Python floats -- IEEE doubles, one rounding per
operation -- and numpy float32 scalars where the header says float."""
import math

import numpy as np

F32 = np.float32


def render(ob, mesh, pose, cam):
    """D of one pose (x y z, w x y z): the oracle's render; a pose with a non-finite component draws nothing.
    mesh: (verts, tris); cam: an object with width, height, fx, fy, cx, cy."""
    pose = np.asarray(pose, np.float64)
    if not np.all(np.isfinite(pose)):
        return np.zeros((cam.height, cam.width), np.float32)
    d = ob.render_depth(ob.make_mesh(mesh[0], mesh[1]), pose[:3], pose[3:], ob.camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy), 1)
    return np.asarray(d, np.float32)


def dist(i, j, d, cam):
    """the distance image's value at column i, row j for the float depth d"""
    a = (float(i) - cam.cx) / cam.fx
    b = (float(j) - cam.cy) / cam.fy
    d = float(d)
    ad, bd = a * d, b * d
    s = (ad * ad + bd * bd) + d * d
    return math.sqrt(s) if s == s and s != math.inf else s   # (NaN and +inf pass through, as a hardware square root passes them)


def visible(M, T, delta, margins):
    """vis(M) of the header; margins receives |diff - delta| of every pixel with T > 0 and M > 0"""
    if T > 0 and M > 0:
        with np.errstate(all="ignore"):
            diff = F32(M) - F32(T)
        margins.append(abs(float(diff) - float(F32(delta))))
        if diff <= F32(delta):
            return True
    return T == 0 and M > 0


def vsd(depth_est, depth_gt, depth_test, cam, delta, taus, diameter, margins=None):
    """(errors float64 [n_taus], counts int32 [4 + n_taus]) of one pose pair.  margins: a dict that receives `delta`, the smallest
    |diff - delta| over the pixels with T > 0 and M > 0, and `tau`, the smallest |c - tau| (inf where there is no such pixel)."""
    De, Dg, Dt = (np.asarray(d, np.float32) for d in (depth_est, depth_gt, depth_test))
    taus = [float(t) for t in taus]
    n_union = n_inter = n_gt = n_est = 0
    fail = [0] * len(taus)
    m_delta, m_tau = [], []
    for j, i in zip(*np.nonzero((De > 0) | (Dg > 0))):   # elsewhere G = E = 0: in neither mask
        T, G, E = dist(i, j, Dt[j, i], cam), dist(i, j, Dg[j, i], cam), dist(i, j, De[j, i], cam)
        vg = visible(G, T, delta, m_delta)
        ve = visible(E, T, delta, m_delta) or (vg and E > 0)
        n_gt += vg
        n_est += ve
        n_union += vg or ve
        if vg and ve:
            n_inter += 1
            c = abs(G - E)
            if diameter > 0:
                c = c / float(diameter)
            for k, tau in enumerate(taus):
                m_tau.append(abs(c - tau))
                fail[k] += c >= tau
    if n_union > 0:
        errors = np.array([float(f + n_union - n_inter) / float(n_union) for f in fail])
    else:
        errors = np.ones(len(taus))
    if margins is not None:
        margins["delta"] = min(m_delta, default=math.inf)
        margins["tau"] = min(m_tau, default=math.inf)
    return errors, np.array([n_union, n_inter, n_gt, n_est] + fail, np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
