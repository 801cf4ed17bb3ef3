"""Restatement of comet_landmark_pnp (csrc/pnp.hip, contract in include/comet_hip.h) in float64 numpy:
the same IEEE operations in the same order as the kernel. The per-point arithmetic is written once and
evaluated elementwise over the slots (numpy neither reorders nor fuses elementwise float64 operations);
the sums follow the kernel's schedule: thread t adds its slots t, t + 256, ... in ascending order, and
the 256 partials are combined by p[t] += p[t + d] for d = 128 .. 1. The reference of
tests/test_pnp_cpu.py and tests/test_pnp_gpu.py."""
import numpy as np

from fuse_numpy import add_hypothesis
from landmark_numpy import rotation

THREADS = 256
SOLVED, FEW, DEGENERATE, NONFINITE = 1, 0, 2, -1
F = np.float64


def _tree(contrib, usable):
    """contrib [N, V] f64, usable [N] bool -> [V]: the kernel's strided per-thread sums and its tree. A
    slot that is not usable adds nothing (+0 to a sum that is never -0: the same bits)."""
    N, V = contrib.shape
    p = np.zeros((THREADS, V), np.float64)
    c = np.where(usable[:, None], contrib, 0.0)
    for base in range(0, N, THREADS):
        blk = c[base:base + THREADS]
        p[:blk.shape[0]] = p[:blk.shape[0]] + blk
    d = THREADS // 2
    while d >= 1:
        p[:d] = p[:d] + p[d:2 * d]
        d //= 2
    return p[0]


def _points(tracks, weights, X, state, m, t, intr):
    """One frame: tracks [N, 2] f32, weights [N] f32 or None, X [N, 3], state [N] at the pose (m, t) ->
    (usable [N], w, xc [3][N], r0, r1, rn)."""
    fx, fy, cx, cy = (F(v) for v in intr)
    px, py = tracks[:, 0], tracks[:, 1]
    w = weights.astype(np.float64) if weights is not None else np.ones(len(px), np.float64)
    usable = (state == 1) & np.isfinite(px) & np.isfinite(py) & np.isfinite(w) & (w > 0.0)
    x0, x1, x2 = X[:, 0], X[:, 1], X[:, 2]
    xc = [m[r][0] * x0 + m[r][1] * x1 + m[r][2] * x2 + t[r] for r in range(3)]
    usable = usable & (xc[2] > 0.0)
    r0 = fx * (xc[0] / xc[2]) + cx - px.astype(np.float64)
    r1 = fy * (xc[1] / xc[2]) + cy - py.astype(np.float64)
    rn = np.sqrt(r0 * r0 + r1 * r1)
    return usable, w, xc, r0, r1, rn


def normal_equations(tracks, weights, X, state, m, t, intr, huber_px):
    """-> v [28]: the upper triangle of H row by row (21), b (6), the usable count."""
    fx, fy = F(intr[0]), F(intr[1])
    usable, w, (x, y, z), r0, r1, rn = _points(tracks, weights, X, state, m, t, intr)
    wh = np.where(rn <= huber_px, 1.0, F(huber_px) / rn)
    ww = w * wh
    a0, a1 = fx / z, fy / z
    c0, c1 = a0 * (x / z), a1 * (y / z)
    zero = np.zeros_like(z)
    J0 = [-(c0 * y), a0 * z + c0 * x, -(a0 * y), a0, zero, -c0]
    J1 = [-(a1 * z) - c1 * y, c1 * x, a1 * x, zero, a1, -c1]
    cols = [ww * (J0[r] * J0[c] + J1[r] * J1[c]) for r in range(6) for c in range(r, 6)]
    cols += [ww * (J0[r] * r0 + J1[r] * r1) for r in range(6)]
    cols.append(np.ones_like(z))
    return _tree(np.stack(cols, -1), usable)


def solve(v, min_pivot):
    """The unpivoted LDL^T of H delta = -b -> (delta [6] or None when a pivot is at or below the bound,
    pivots [6], max(diag H))."""
    A = [[None] * 6 for _ in range(6)]
    k = 0
    for r in range(6):
        for c in range(r, 6):
            A[c][r] = F(v[k])
            k += 1
    top = A[0][0]
    for r in range(1, 6):
        top = np.fmax(top, A[r][r])
    thr = F(min_pivot) * top
    Lm = [[None] * 6 for _ in range(6)]
    U = [[None] * 6 for _ in range(6)]
    d = [None] * 6
    ill = False
    for j in range(6):
        for i in range(j, 6):
            c = A[i][j]
            for k in range(j):
                c = c - Lm[j][k] * U[i][k]
            if i == j:
                d[j] = c
            else:
                U[i][j] = c
                Lm[i][j] = c / d[j]
        ill = ill or bool(d[j] <= thr)
    if ill:
        return None, d, top
    y, x = [None] * 6, [None] * 6
    for i in range(6):
        c = -F(v[21 + i])
        for k in range(i):
            c = c - Lm[i][k] * y[k]
        y[i] = c
    for i in range(5, -1, -1):
        c = y[i] / d[i]
        for k in range(i + 1, 6):
            c = c - Lm[k][i] * x[k]
        x[i] = c
    return x, d, top


def _qmul(a, b):
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
            a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]


def retract(x, m, t, q, inverse):
    """delta = (omega, upsilon) applied to (m, t, q) -> (m, t, q)."""
    hx, hy, hz = F(0.5) * x[0], F(0.5) * x[1], F(0.5) * x[2]
    nrm = np.sqrt(F(1.0) + hx * hx + hy * hy + hz * hz)
    dq = [F(1.0) / nrm, hx / nrm, hy / nrm, hz / nrm]
    D = rotation(dq, 0)
    m2 = [[D[r][0] * m[0][c] + D[r][1] * m[1][c] + D[r][2] * m[2][c] for c in range(3)] for r in range(3)]
    t2 = [D[r][0] * t[0] + D[r][1] * t[1] + D[r][2] * t[2] + x[3 + r] for r in range(3)]
    q2 = _qmul(q, [dq[0], -dq[1], -dq[2], -dq[3]]) if inverse else _qmul(dq, q)
    qn = np.sqrt(q2[0] * q2[0] + q2[1] * q2[1] + q2[2] * q2[2] + q2[3] * q2[3])
    sg = (F(-1.0) if q2[0] < 0.0 else F(1.0)) / qn
    return m2, t2, [v * sg for v in q2]


def _finite(vals):
    return all(bool(np.isfinite(v)) for v in vals)


def solve_frame(tracks, weights, X, state, q0, t0, intr, huber_px, iters=4, min_pts=6, min_pivot=1e-8,
                inverse_rotation=0, trace=None):
    """One (hop, position): tracks [N, 2] f32, weights [N] f32 or None, X [N, 3] f64, state [N] int32, q0 [4]
    f32, t0 [3] f64 -> dict(q [4] f64, R [4] f32, t [3] f64, n_in, rms_px f32, state). trace: a list that
    takes, per iteration, dict(pivots, diag, count, q, t) (the pose after the step)."""
    q0 = np.asarray(q0, np.float32)
    t0 = np.asarray(t0, np.float64)
    fail = lambda st: dict(q=q0.astype(np.float64), R=q0.copy(), t=t0.copy(), n_in=0, rms_px=np.float32(np.inf), state=st)
    with np.errstate(all="ignore"):
        q = [F(v) for v in q0]
        m = rotation(q0, inverse_rotation)
        t = [F(v) for v in t0]
        if not _finite([v for row in m for v in row] + t):
            return fail(NONFINITE)
        for _ in range(iters):
            v = normal_equations(tracks, weights, X, state, m, t, intr, huber_px)
            if v[27] < min_pts:
                return fail(FEW)
            if not _finite(v[:27]):
                return fail(NONFINITE)
            x, piv, top = solve(v, min_pivot)
            if trace is not None:
                trace.append(dict(pivots=[float(p) for p in piv], diag=float(top), count=int(v[27])))
            if x is None:
                return fail(DEGENERATE)
            m2, t2, q2 = retract(x, m, t, q, inverse_rotation)
            if not _finite([v_ for row in m2 for v_ in row] + t2 + q2):
                return fail(NONFINITE)
            m, t, q = m2, t2, q2
            if trace is not None:
                trace[-1].update(q=np.array(q), t=np.array(t))
        usable, w, _, r0, r1, rn = _points(tracks, weights, X, state, m, t, intr)
        ones = np.ones_like(rn)
        f = _tree(np.stack([ones, np.where(rn <= huber_px, 1.0, 0.0), w * (r0 * r0 + r1 * r1), w], -1), usable)
        rms = np.sqrt(f[2] / f[3])
        if f[0] < min_pts:
            return fail(FEW)
        if not np.isfinite(rms):
            return fail(NONFINITE)
        qa = np.array(q, np.float64)
        return dict(q=qa, R=qa.astype(np.float32), t=np.array(t, np.float64), n_in=int(f[1]), rms_px=np.float32(rms),
                    state=SOLVED)


def pnp(tracks, X, state, R0, T0, intr, s, huber_px, weights=None, inverse_rotation=0, iters=4, min_pts=6,
        min_pivot=1e-8, fuse_acc=None, slots=None, inject_w=0.0, fuse_intr=None, trace=None):
    """tracks [n, T, N, 2] f32, X [n, N, 3] f64, state [n, N] int32, R0 [n, T, 4] f32, T0 [n, T, 3] f64,
    intr [n, 4] f64, weights [n, T, N] f32 or None -> dict(q [n, T, 4] f64, R [n, T, 4] f32, t [n, T, 3] f64,
    n_in [n, T] int32, rms_px [n, T] f32, state [n, T] int32). fuse_acc [rows, 20] f64 (updated in place),
    slots [n * T], inject_w, fuse_intr: the injection. trace: a dict that takes {(h, i): [per iteration]}."""
    n, Tw, N = tracks.shape[:3]
    out = dict(q=np.zeros((n, Tw, 4)), R=np.zeros((n, Tw, 4), np.float32), t=np.zeros((n, Tw, 3)),
               n_in=np.zeros((n, Tw), np.int32), rms_px=np.zeros((n, Tw), np.float32), state=np.zeros((n, Tw), np.int32))
    for h in range(n):
        for i in range(Tw):
            tr = [] if trace is not None else None
            r = solve_frame(tracks[h, i], None if weights is None else weights[h, i], X[h], state[h], R0[h, i], T0[h, i],
                            intr[h], huber_px, iters, min_pts, min_pivot, inverse_rotation, tr)
            if trace is not None:
                trace[(h, i)] = tr
            for k, v in r.items():
                out[k][h, i] = v
            if r["state"] == SOLVED and fuse_acc is not None and inject_w > 0.0 and i >= s:
                fx, fy, cx, cy = (F(v) for v in fuse_intr)
                tx, ty, tz = (F(v) for v in r["t"])
                with np.errstate(all="ignore"):
                    x = np.array([cx + fx * tx / tz, cy + fy * ty / tz, tz])
                if np.all(np.isfinite(x)):
                    add_hypothesis(fuse_acc[int(slots[h * Tw + i])], F(inject_w), r["q"], x)
    return out
