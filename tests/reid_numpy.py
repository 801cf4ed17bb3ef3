"""Loop restatement of comet_landmark_reid (csrc/reid.hip, contract in include/comet_hip.h) in float64 numpy
scalars: the same IEEE operations in the same order as the kernel, one hop at a time, with every read of the
state before any write (the restatement copies first). It reuses landmark_numpy's solve and rotation. The
reference of tests/test_reid_cpu.py, tests/test_reid_gpu.py and tests/test_reid_stream_gpu.py."""
import numpy as np

import landmark_numpy as lmn

ARCH_ROW = 20
NOT_BORN, MATCHED, NO_CANDIDATE, LOST = 0, 1, 2, 3
F = np.float64


def new_state(streams, N, C):
    """-> dict(arch [S C, 20] f64, arch_id [S C] int32, arch_cursor [S] int32, alias [S N] int32)."""
    return dict(arch=np.zeros((streams * C, ARCH_ROW), np.float64), arch_id=np.full(streams * C, -1, np.int32),
                arch_cursor=np.zeros(streams, np.int32), alias=np.full(streams * N, -1, np.int32))


def reset(state, acc_id, stream, N, C):
    """What LandmarkMap.reset(stream) does to the state."""
    acc_id[stream * N:(stream + 1) * N] = -1
    state["alias"][stream * N:(stream + 1) * N] = -1
    state["arch_id"][stream * C:(stream + 1) * C] = -1
    state["arch_cursor"][stream] = 0


def to_camera(m, t, X):
    return [m[k][0] * X[0] + m[k][1] * X[1] + m[k][2] * X[2] + t[k] for k in range(3)]


def view_dir(c, X):
    v = [c[k] - X[k] for k in range(3)]
    nv = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return [v[0] / nv, v[1] / nv, v[2] / nv]


def dist2(ex, ey, p):
    du, dv = ex - F(p[0]), ey - F(p[1])
    return du * du + dv * dv


def reid(tracks, R, T, ids, src, stream_idx, intr, acc, acc_id, state, C, reid_px, reid_min_cos=0.5, arch_min_obs=3,
         inverse_rotation=0, min_pivot=1e-8):
    """tracks [n, Tw, N, 2] f32, R [n, Tw, 4] f32, T [n, Tw, 3] f64, ids / src [n, N] int32, stream_idx [n],
    intr [n, 4] f64. acc [rows, 12] f64, acc_id [rows] int32 and the arrays of `state` (new_state) are updated in
    place -> dict(src_lm, lm_id, reid_state [n, N] int32, reid_dist [n, N] f32, stats [n, 4] int32) and, for the
    tests' margin checks: cand [n, C] bool, cos [n, C] (NaN for a free entry), best / second [n, N] f64 the
    least and the second least dist2 of a born slot over the candidates (inf where none), pivots [n, N, 3] and
    diag [n, N] of the dying rows with enough observations (NaN elsewhere)."""
    n, Tw, N = tracks.shape[:3]
    arch, arch_id, cursor_of, alias = state["arch"], state["arch_id"], state["arch_cursor"], state["alias"]
    assert arch.shape[1] == ARCH_ROW and Tw >= 2 and 1 <= C
    out = dict(src_lm=np.array(src, np.int32), lm_id=np.full((n, N), -1, np.int32),
               reid_state=np.zeros((n, N), np.int32), reid_dist=np.full((n, N), np.inf, np.float32),
               stats=np.zeros((n, 4), np.int32), cand=np.zeros((n, C), bool), cos=np.full((n, C), np.nan),
               best=np.full((n, N), np.inf), second=np.full((n, N), np.inf), pivots=np.full((n, N, 3), np.nan),
               diag=np.full((n, N), np.nan))
    gate2 = F(reid_px) * F(reid_px)
    with np.errstate(all="ignore"):
        for h in range(n):
            sidx = int(stream_idx[h])
            row0, ent0 = sidx * N, sidx * C
            assert sidx >= 0 and row0 + N <= acc.shape[0] and ent0 + C <= arch.shape[0]
            fx, fy, cx, cy = (F(v) for v in intr[h])
            m = lmn.rotation(R[h, 0], inverse_rotation)
            t = [F(v) for v in T[h, 0]]
            c = [F(0.0) - (m[0][k] * t[0] + m[1][k] * t[1] + m[2][k] * t[2]) for k in range(3)]
            # every read of the state comes first
            acc0, acc_id0, alias0 = acc[row0:row0 + N].copy(), acc_id[row0:row0 + N].copy(), alias[row0:row0 + N].copy()
            arch0, arch_id0 = arch[ent0:ent0 + C].copy(), arch_id[ent0:ent0 + C].copy()
            cursor = int(cursor_of[sidx]) % C

            # 1. the candidates and their projections
            ex, ey, cand, in_use = np.zeros(C), np.zeros(C), np.zeros(C, bool), arch_id0 >= 0
            for e in range(C):
                if not in_use[e]:
                    continue
                X = [F(v) for v in arch0[e, 12:15]]
                d = [F(v) for v in arch0[e, 15:18]]
                xc = to_camera(m, t, X)
                dn = view_dir(c, X)
                cosv = d[0] * dn[0] + d[1] * dn[1] + d[2] * dn[2]
                ex[e], ey[e] = fx * (xc[0] / xc[2]) + cx, fy * (xc[1] / xc[2]) + cy
                cand[e] = bool(xc[2] > 0.0 and cosv >= reid_min_cos and np.isfinite(ex[e]) and np.isfinite(ey[e]))
                out["cos"][h, e] = cosv
            out["cand"][h] = cand

            # 2. dying and retirable rows (in slot order: the rank), the picks of the born slots
            retire, pick = [], np.full(N, -1, np.int64)
            for j in range(N):
                ident, sr, aid = int(ids[h, j]), int(src[h, j]), int(acc_id0[j])
                if aid >= 0 and (ident != aid or sr != j):
                    r = [F(v) for v in acc0[j]]
                    sol, piv = lmn.solve(r, min_pivot)
                    if r[10] >= arch_min_obs:
                        out["pivots"][h, j], out["diag"][h, j] = piv, np.fmax(np.fmax(r[0], r[3]), r[5])
                    if sol is not None and all(np.isfinite(v) for v in sol) and r[10] >= arch_min_obs and \
                            to_camera(m, t, sol)[2] > 0.0:
                        retire.append((j, r, sol, int(alias0[j]) if alias0[j] >= 0 else aid))
                if ident >= 0 and sr < 0:
                    p = tracks[h, 0, j]
                    if np.isfinite(p[0]) and np.isfinite(p[1]):
                        best = F(np.inf)
                        for e in np.nonzero(cand)[0]:  # (ascending, as the kernel scans)
                            d2 = dist2(ex[e], ey[e], p)
                            if d2 < out["best"][h, j]:
                                out["second"][h, j], out["best"][h, j] = out["best"][h, j], d2
                            elif d2 < out["second"][h, j]:
                                out["second"][h, j] = d2
                            if d2 <= gate2 and d2 < best:
                                best, pick[j] = d2, e

            # 3. every entry accepts the nearest slot that picked it
            win = np.full(C, -1, np.int64)
            for e in range(C):
                best = F(np.inf)
                for j in np.nonzero(pick == e)[0]:
                    d2 = dist2(ex[e], ey[e], tracks[h, 0, j])
                    if d2 < best:
                        best, win[e] = d2, j

            # 4. matches and the outputs
            matched = 0
            for j in range(N):
                ident, sr, aid = int(ids[h, j]), int(src[h, j]), int(acc_id0[j])
                born = ident >= 0 and sr < 0
                lm = ident if ident >= 0 else -1
                if born and pick[j] >= 0 and win[pick[j]] == j:
                    e = int(pick[j])
                    acc[row0 + j] = arch0[e, :12]
                    acc_id[row0 + j] = ident
                    lm = int(arch_id0[e])
                    alias[row0 + j] = lm
                    arch_id[ent0 + e] = -1
                    in_use[e] = False
                    out["src_lm"][h, j] = j
                    out["reid_state"][h, j] = MATCHED
                    out["reid_dist"][h, j] = np.float32(np.sqrt(dist2(ex[e], ey[e], tracks[h, 0, j])))
                    matched += 1
                else:
                    if born:
                        out["reid_state"][h, j] = NO_CANDIDATE if pick[j] < 0 else LOST
                    if ident >= 0 and sr == j and aid == ident:
                        if alias0[j] >= 0:
                            lm = int(alias0[j])
                    else:
                        alias[row0 + j] = -1
                out["lm_id"][h, j] = lm

            # 5. retirements in rank order from the cursor
            over = 0
            for rank, (j, r, sol, sid) in enumerate(retire):
                e = (cursor + rank) % C
                over += bool(in_use[e])
                in_use[e] = True
                arch[ent0 + e, :12] = r
                arch[ent0 + e, 12:15] = sol
                arch[ent0 + e, 15:18] = view_dir(c, sol)
                arch[ent0 + e, 18:] = 0.0
                arch_id[ent0 + e] = sid
            cursor_of[sidx] = (cursor + len(retire)) % C
            out["stats"][h] = (len(retire), matched, int((arch_id[ent0:ent0 + C] >= 0).sum()), over)
    return out


def snapshot(state, stream, C, min_pivot=1e-8):
    """(ids, X [L, 3], n_obs) of the stream's entries in use, in entry order: LandmarkMap.archive_snapshot."""
    sl = slice(stream * C, (stream + 1) * C)
    on = state["arch_id"][sl] >= 0
    a = state["arch"][sl][on]
    return state["arch_id"][sl][on].copy(), a[:, 12:15].copy(), a[:, 10].astype(np.int32)


# ---- input builders of the tests (inputs only: nothing here has to match the kernel's rounding) ------------
INT_MIN = -2 ** 31


def rows_of(X, qs, ts, intr, inverse, n_frames=None):
    """Accumulator rows [P, 12] of the points X [P, 3] seen exactly in the frames (qs [F, 4], ts [F, 3])."""
    X = np.asarray(X, np.float64)
    rows = np.zeros((len(X), 12))
    fx, fy, cx, cy = intr
    for q, t in list(zip(qs, ts))[:n_frames]:
        m = np.array(lmn.rotation(np.float32(q), inverse), np.float64)
        px, _ = lmn.project(X, np.float32(q), t, intr, inverse)
        xn, yn = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
        for a, c in ((m[0] - xn[:, None] * m[2], xn * t[2] - t[0]), (m[1] - yn[:, None] * m[2], yn * t[2] - t[1])):
            rows[:, 0:3] += a[:, :1] * a
            rows[:, 3:5] += a[:, 1:2] * a[:, 1:]
            rows[:, 5] += a[:, 2] * a[:, 2]
            rows[:, 6:9] += a * c[:, None]
            rows[:, 9] += c * c
        rows[:, 10] += 1.0
    return rows


def entries_of(X, rows, c_ret):
    """Archive entries [P, 20] of the points X with the rows `rows`, retired with the camera centre at c_ret."""
    X = np.asarray(X, np.float64)
    d = np.asarray(c_ret, np.float64) - X
    return np.concatenate([rows, X, d / np.linalg.norm(d, axis=-1, keepdims=True), np.zeros((len(X), 2))], -1)


def camera_centre(q, t, inverse):
    m = np.array(lmn.rotation(np.float32(q), inverse), np.float64)
    return -(m.T @ np.asarray(t, np.float64))
