"""Relocalise a lost track: a compass search over pose hypotheses (include/roft_engine.h, section 3j).

Host only, numpy only: the device scores a round's candidates in one call (ops.pose_hypotheses_score,
ROFTFilterBatch.score_hypotheses), every decision is taken here on integers and one double, so a CPU reference that returns the same
records reproduces the search exactly -- trace and poses bit for bit.

The defaults of compass_search (8 mm, 4 degrees, 40 rounds, 4 halvings) are the values of one CPU experiment on a box mesh at
128 x 96 and 320 x 240.  Nobody has tuned them.
"""
import math

import numpy as np

N_CANDIDATES = 13


def disagreement(rec):
    """Pixels the pose explains wrongly: mask without surface, surface without mask, surface at the wrong depth --
    n_mask + n_render - 2 n_both + n_front + n_behind.  rec: one record or an array of them (ops.QUALITY_DTYPE, or a mapping with
    those keys).  An integer (int64 array for an array)."""
    def field(k):
        return np.asarray(rec[k]).astype(np.int64)
    d = field("n_mask") + field("n_render") - 2 * field("n_both") + field("n_front") + field("n_behind")
    return int(d) if d.ndim == 0 else d


def quat_mul(a, b):
    """a (x) b, quaternions as (w, x, y, z)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw])


def compass_candidates(x, q, t_step, r_step):
    """The 13 poses of one round, [13, 7] rows x y z, q = (w, x, y, z), in this order:
         0        the current pose (x, q)
         1 .. 6   x + t_step e_k, x - t_step e_k for the camera's axes k = x, y, z (+x, -x, +y, -y, +z, -z); q unchanged
         7 .. 12  dq (x) q with dq = (cos(r_step / 2), +sin(r_step / 2) e_k), then -sin, for k = x, y, z: a turn by +-r_step about the
                  camera-frame axis k through the object's origin; x unchanged.  The product is divided by its norm."""
    x = np.asarray(x, np.float64).reshape(3)
    q = np.asarray(q, np.float64).reshape(4)
    out = np.empty((N_CANDIDATES, 7))
    out[:, :3] = x
    out[:, 3:] = q
    c, s = math.cos(0.5 * r_step), math.sin(0.5 * r_step)
    for k in range(3):
        out[1 + 2 * k, k] = x[k] + t_step
        out[2 + 2 * k, k] = x[k] - t_step
        for j, sign in enumerate((1.0, -1.0)):
            dq = np.array([c, 0.0, 0.0, 0.0])
            dq[1 + k] = sign * s
            p = quat_mul(dq, q)
            out[7 + 2 * k + j, 3:] = p / math.sqrt(float(p @ p))
    return out


def compass_search(score, x, q, t_step=0.008, r_step=math.radians(4.0), rounds=40, max_halvings=4):
    """Minimise disagreement(score(pose)) from (x, q).  score: maps an [n, 7] array of poses to n records.  Each round scores
    compass_candidates(x, q, t_step, r_step) in ONE call and moves to the minimum of (disagreement, depth_err, index); when that is
    index 0 -- no neighbour is better -- both steps are halved.  It stops when the steps have been halved more than max_halvings
    times, or after `rounds` rounds.  Returns (x, q, trace); trace: one (winner index, its disagreement) per round.  The winner's
    disagreement never increases along the trace (candidate 0 is the last winner).
    The default steps, rounds and halvings are those of one CPU experiment; nobody has tuned them."""
    x = np.asarray(x, np.float64).reshape(3).copy()
    q = np.asarray(q, np.float64).reshape(4).copy()
    trace = []
    halvings = 0
    for _ in range(int(rounds)):
        cand = compass_candidates(x, q, t_step, r_step)
        rec = score(cand)
        dis = disagreement(rec)
        err = np.asarray(rec["depth_err"], np.float64)
        best = min(range(N_CANDIDATES), key=lambda i: (int(dis[i]), float(err[i]), i))
        trace.append((int(best), int(dis[best])))
        if best == 0:
            halvings += 1
            if halvings > max_halvings:
                break
            t_step *= 0.5
            r_step *= 0.5
        else:
            x, q = cand[best, :3].copy(), cand[best, 3:].copy()
    return x, q, trace
