"""A float64 numpy restatement of comet_pose_fuse (include/comet_hip.h, DESIGN.md "Pose fusion"):
the yardstick of tests/test_fuse_cpu.py and tests/test_fuse_gpu.py. Nothing here calls the library.

The accumulation and the translation arithmetic are written operation by operation as the kernel
writes them (IEEE double, no fused multiply-add on either side), the rotation is numpy.linalg.eigh
where the kernel runs a Jacobi iteration. Also here: the single-estimate chaining the streams use
without fusion (chain_reference), and the synthetic overlapping-window scenario of the drift test."""
import math

import numpy as np

ROW = 20
_TRI = [(i, j) for i in range(4) for j in range(i, 4)]  # ww wx wy wz xx xy xz yy yz zz


def qmul(a, b):
    """The raw quaternion product a (x) b, (w, x, y, z)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw], dtype=np.float64)


def unit_pos(q):
    """q / |q| with w >= 0 (the sign rule of qmul_std)."""
    q = np.asarray(q, dtype=np.float64)
    sg = (-1.0 if q[0] < 0.0 else 1.0) / math.sqrt(float(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
    return q * sg


def hypothesis(e, qr, xr, ratio):
    """One encoding row e [7] against the reference (qr [4], xr = (u, v, z)) -> (unit q, (u, v, z))."""
    e = [float(v) for v in e]
    q = unit_pos(qmul(e[3:7], qr))
    x = np.array([xr[0] + e[0] / ratio * 128.0, xr[1] + e[1] / ratio * 128.0, xr[2] * (e[2] / ratio + 1.0)])
    return q, x


def add_hypothesis(row, w, q, x):
    h = np.zeros(ROW)
    h[0] = w
    for k, (i, j) in enumerate(_TRI):
        h[1 + k] = w * (q[i] * q[j])
    for i in range(3):
        h[11 + i] = w * x[i]
        h[14 + i] = w * (x[i] * x[i])
    h[17] = 1.0
    row += h


def fused(row):
    """The fused pose of one accumulator row -> (unit q with w >= 0, (u, v, z), lambda_max, W)."""
    M = np.zeros((4, 4))
    for k, (i, j) in enumerate(_TRI):
        M[i, j] = M[j, i] = row[1 + k]
    lam, vec = np.linalg.eigh(M)  # ascending; the tests keep the largest eigenvalue simple
    W = row[0]
    return unit_pos(vec[:, 3]), row[11:14] / W, lam[3], W


def outputs(row, q, x, intr):
    """What the kernel writes for one (hop, position) from the updated row and its hypothesis."""
    fx, fy, cx, cy = intr
    fq, fu, lam, W = fused(row)
    var = row[14:17] / W - fu * fu
    return {"R": fq.astype(np.float32), "uvz": fu.copy(),
            "T": np.array([(fu[0] - cx) * fu[2] / fx, (fu[1] - cy) * fu[2] / fy, fu[2]]),
            "count": int(row[17]),
            "rot_spread": np.float32(2.0 * math.asin(math.sqrt(min(1.0, max(0.0, 1.0 - lam / W))))),
            "trans_spread": np.sqrt(np.maximum(0.0, var)).astype(np.float32),
            "hyp_R": q.astype(np.float32),
            "hyp_T": np.array([(x[0] - cx) * x[2] / fx, (x[1] - cy) * x[2] / fy, x[2]])}


class FuseRef:
    """The accumulator ring and one call per launch, as comet_pose_fuse."""

    def __init__(self, rows, ratio, intr):
        self.acc = np.zeros((rows, ROW))
        self.ratio, self.intr = float(ratio), tuple(float(v) for v in intr)

    def fuse(self, enc, slots, fresh, first, anchors, weights=None, want=True):
        """enc [n, T, 7] (read as f32), slots [n * T], fresh [n], first [n], anchors [n, 7],
        weights [n, T] (read as f32) or None -> {name: [n, T, ...]} (None when want is false: only
        the ring is updated)."""
        enc = np.asarray(enc, dtype=np.float32)
        n, T = enc.shape[:2]
        out = {}
        for h in range(n):
            s0 = slots[h * T]
            if first[h]:
                qr, xr = np.array(anchors[h][:4], dtype=np.float64), np.array(anchors[h][4:], dtype=np.float64)
            else:
                qr, xr, _, _ = fused(self.acc[s0])
            for i in range(T):
                row = self.acc[slots[h * T + i]]
                if i == 0:
                    q, x = unit_pos(qr), xr.copy()
                    if first[h]:
                        row[:] = 0.0
                        add_hypothesis(row, 1.0, q, x)
                else:
                    q, x = hypothesis(enc[h, i], qr, xr, self.ratio)
                    w = 1.0 if weights is None else float(np.float32(weights[h][i]))
                    if i >= fresh[h]:
                        row[:] = 0.0
                    add_hypothesis(row, w, q, x)
                if want:
                    for k, v in outputs(row, q, x, self.intr).items():
                        out.setdefault(k, []).append(v)
        if not want:
            return None
        return {k: np.array(v).reshape((n, T) + np.shape(v[0])) for k, v in out.items()}


def chain_reference(e, qr, xr, ratio):
    """Single-estimate chaining (comet_amd.stream._decode_chained without its f32 rounding): the
    next window's reference is this window's one hypothesis for the frame, row e of its encoding."""
    return hypothesis(e, qr, xr, ratio)


# ---- the synthetic scenario of the drift test ------------------------------------------------------
def axis_angle_quat(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[math.cos(0.5 * angle)], math.sin(0.5 * angle) * axis])


def rot_angle(a, b):
    """The angle of the rotation between unit quaternions a and b, radians."""
    return 2.0 * math.asin(min(1.0, 0.5 * min(np.linalg.norm(a - b), np.linalg.norm(a + b))))


def truth(rng, frames):
    """A smooth ground-truth trajectory: (q [frames, 4], uvz [frames, 3])."""
    q = [unit_pos(rng.normal(size=4))]
    x = [np.array([320.0, 240.0, 10.0]) + rng.normal(size=3) * np.array([20.0, 20.0, 0.5])]
    for _ in range(frames - 1):
        q.append(unit_pos(qmul(axis_angle_quat(rng.normal(size=3), rng.normal() * 0.05), q[-1])))
        x.append(x[-1] + rng.normal(size=3) * np.array([4.0, 4.0, 0.1]))
    return np.array(q), np.array(x)


def window_encoding(rng, q, x, first, T, ratio, sig_rot, sig_uv, sig_d):
    """The model's output for the window of frames first .. first + T - 1: the true encoding relative
    to its first frame plus iid noise on every row (a small random rotation, additive noise on the
    three translation entries). Row 0 is the identity, as the model forces it."""
    enc = np.zeros((T, 7), dtype=np.float32)
    enc[0, 3] = 1.0
    q0, x0 = q[first], x[first]
    inv = q0 * np.array([1.0, -1.0, -1.0, -1.0])
    for i in range(1, T):
        rel = qmul(q[first + i], inv)
        rel = unit_pos(qmul(axis_angle_quat(rng.normal(size=3), rng.normal() * sig_rot), rel))
        e = [(x[first + i][0] - x0[0]) * ratio / 128.0 + rng.normal() * sig_uv,
             (x[first + i][1] - x0[1]) * ratio / 128.0 + rng.normal() * sig_uv,
             (x[first + i][2] / x0[2] - 1.0) * ratio + rng.normal() * sig_d]
        enc[i] = np.concatenate([e, rel])
    return enc
