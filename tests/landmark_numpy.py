"""Loop restatement of comet_landmark_update (csrc/landmark.hip, contract in include/comet_hip.h) in
float64 numpy scalars: the same IEEE operations in the same order as the kernel, one (hop, slot) at a
time. The reference of tests/test_landmark_cpu.py and tests/test_landmark_gpu.py."""
import numpy as np

LM_ROW = 12
VALID, NONE, ILL, BEHIND, NONFINITE = 1, 0, 2, 3, -1
F = np.float64


def rotation(q, inverse):
    """Rows of the matrix of the quaternion q (w first; minipytorch3d.quaternion_to_matrix), transposed
    when `inverse`. q is widened to float64 first, as the kernel widens its f32 input."""
    r, i, j, k = (F(v) for v in q)
    two_s = F(2.0) / (r * r + i * i + j * j + k * k)
    m = [[F(1.0) - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r)],
         [two_s * (i * j + k * r), F(1.0) - two_s * (i * i + k * k), two_s * (j * k - i * r)],
         [two_s * (i * k - j * r), two_s * (j * k + i * r), F(1.0) - two_s * (i * i + j * j)]]
    if inverse:
        m = [[m[c][r_] for c in range(3)] for r_ in range(3)]
    return m


def _add_equation(r, w, a, c):
    r[0] += w * (a[0] * a[0])
    r[1] += w * (a[0] * a[1])
    r[2] += w * (a[0] * a[2])
    r[3] += w * (a[1] * a[1])
    r[4] += w * (a[1] * a[2])
    r[5] += w * (a[2] * a[2])
    r[6] += w * (a[0] * c)
    r[7] += w * (a[1] * c)
    r[8] += w * (a[2] * c)
    r[9] += w * (c * c)


def solve(r, min_pivot):
    """Unpivoted LDL^T of the row's M X = g -> (X or None when a pivot is at or below the bound, pivots)."""
    thr = F(min_pivot) * np.fmax(np.fmax(r[0], r[3]), r[5])
    d0 = r[0]
    l10, l20 = r[1] / d0, r[2] / d0
    d1 = r[3] - l10 * r[1]
    u12 = r[4] - l20 * r[1]
    l21 = u12 / d1
    d2 = r[5] - l20 * r[2] - l21 * u12
    if d0 <= thr or d1 <= thr or d2 <= thr:
        return None, (d0, d1, d2)
    y0 = r[6]
    y1 = r[7] - l10 * y0
    y2 = r[8] - l20 * y0 - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = y0 / d0 - l10 * x1 - l20 * x2
    return (x0, x1, x2), (d0, d1, d2)


def update(tracks, R, T, ids, src, stream_idx, intr, acc, acc_id, s, weights=None, inverse_rotation=0, min_obs=3,
           min_pivot=1e-8):
    """tracks [n, Tw, N, 2] f32, R [n, Tw, 4] f32, T [n, Tw, 3] f64, ids / src [n, N] int32, stream_idx [n],
    intr [n, 4] f64, weights [n, Tw, N] f32 or None. acc [rows, 12] f64 and acc_id [rows] int32 are updated
    in place -> dict(X [n, N, 3] f64, n_obs [n, N] int32, err_px [n, N] f32, state [n, N] int32, pivots
    [n, N, 3] f64 and diag [n, N] f64 = max(diag M), the scale of the pivot threshold, both NaN where nothing
    was solved)."""
    n, Tw, N = tracks.shape[:3]
    assert 1 <= s <= Tw - 1 and acc.shape[1] == LM_ROW and acc.dtype == np.float64
    X = np.zeros((n, N, 3), np.float64)
    n_obs = np.zeros((n, N), np.int32)
    err_px = np.full((n, N), np.inf, np.float32)
    state = np.zeros((n, N), np.int32)
    pivots = np.full((n, N, 3), np.nan)
    diag = np.full((n, N), np.nan)
    with np.errstate(all="ignore"):
        for h in range(n):
            fx, fy, cx, cy = (F(v) for v in intr[h])
            for j in range(N):
                row = int(stream_idx[h]) * N + j
                assert 0 <= row < acc.shape[0]
                ident = int(ids[h, j])
                if ident < 0:
                    acc[row] = 0.0
                    acc_id[row] = -1
                    continue
                fresh = int(src[h, j]) != j or int(acc_id[row]) != ident
                r = [F(0.0)] * LM_ROW if fresh else [F(v) for v in acc[row]]
                for i in range(s):
                    x, y = tracks[h, i, j]
                    w = F(weights[h, i, j]) if weights is not None else F(1.0)
                    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(w) and w > 0.0):
                        continue
                    m = rotation(R[h, i], inverse_rotation)
                    tx, ty, tz = (F(v) for v in T[h, i])
                    xn, yn = (F(x) - cx) / fx, (F(y) - cy) / fy
                    a1 = [m[0][k] - xn * m[2][k] for k in range(3)]
                    a2 = [m[1][k] - yn * m[2][k] for k in range(3)]
                    _add_equation(r, w, a1, xn * tz - tx)
                    _add_equation(r, w, a2, yn * tz - ty)
                    r[10] += F(1.0)
                r[11] = F(0.0)
                acc[row] = r
                acc_id[row] = ident
                n_obs[h, j] = int(r[10])
                if n_obs[h, j] < min_obs:
                    continue
                sol, piv = solve(r, min_pivot)
                pivots[h, j] = piv
                diag[h, j] = np.fmax(np.fmax(r[0], r[3]), r[5])
                if sol is None:
                    state[h, j] = ILL
                    continue
                x0, x1, x2 = sol
                m = rotation(R[h, s], inverse_rotation)
                t = [F(v) for v in T[h, s]]
                xc = m[0][0] * x0 + m[0][1] * x1 + m[0][2] * x2 + t[0]
                yc = m[1][0] * x0 + m[1][1] * x1 + m[1][2] * x2 + t[1]
                zc = m[2][0] * x0 + m[2][1] * x1 + m[2][2] * x2 + t[2]
                px, py = tracks[h, s, j]
                du, dv = fx * (xc / zc) + cx - F(px), fy * (yc / zc) + cy - F(py)
                e = np.sqrt(du * du + dv * dv)
                if not (np.isfinite(x0) and np.isfinite(x1) and np.isfinite(x2)):
                    state[h, j] = NONFINITE
                elif zc <= 0.0:
                    state[h, j] = BEHIND
                elif not np.isfinite(e):
                    state[h, j] = NONFINITE
                else:
                    state[h, j] = VALID
                    X[h, j] = (x0, x1, x2)
                    err_px[h, j] = np.float32(e)
    return dict(X=X, n_obs=n_obs, err_px=err_px, state=state, pivots=pivots, diag=diag)


def new_state(streams, N):
    return np.zeros((streams * N, LM_ROW), np.float64), np.full(streams * N, -1, np.int32)


# ---- geometry helpers of the tests ------------------------------------------------------------------
def quat_from_axis_angle(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def project(X, q, t, intr, inverse_rotation=0):
    """Body points X [P, 3] -> pixels [P, 2] f64 and depths [P] under the pose (q, t)."""
    m = np.array(rotation(q, inverse_rotation), np.float64)
    xc = X @ m.T + np.asarray(t, np.float64)
    fx, fy, cx, cy = intr
    return np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], -1), xc[:, 2]
