"""The constructed inputs of the comet_landmark_reid tests (tests/test_reid_cpu.py on the restatement alone,
tests/test_reid_gpu.py on the kernel): one launch in which every state, every reason a dying row is not
retirable, both tie rules, a pad, NaN / Inf pixels and a retirement on a just-consumed entry occur; the
restatement's answer to it; and the check that every comparison deciding an outcome sits at least 1e-6
(relative) from its threshold, but for the constructed exact ties."""
import numpy as np

import landmark_numpy as lmn
import reid_numpy as rn

INTR = (3000.0, 3100.0, 635.0, 600.0)  # the unit sphere at depth 6 is a disc of 500 px: entries lie ~100 px apart
REID_PX, MIN_COS, MIN_OBS, MIN_PIVOT = 2.0, 0.5, 3, 1e-8
SHAPES = [(1, 64, 32, 4), (3, 70, 300, 5), (1, 1, 1, 2), (2, 300, 257, 4), (1, 4096, 4096, 3)]
BORN = -5  # a src of a born slot


def _pose(f, seed):
    q = lmn.quat_from_axis_angle((0.3, 1.0, 0.2), 0.3 * seed + np.deg2rad(6.0) * f).astype(np.float32)
    return q, np.array([0.1, -0.05, 6.0]) + 0.01 * f * np.array([1.0, 0.5, 2.0])


def _sphere(P, seed):
    v = np.random.default_rng(seed).normal(size=(P, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _case(n, N, C, T, inverse, seed=0):
    """-> inputs (numpy) of one launch: S = n + 1 streams, hop h on stream n - h."""
    S = n + 1
    rng = np.random.default_rng(seed)
    acc, acc_id = lmn.new_state(S, N)
    st = rn.new_state(S, N, C)
    tracks = np.zeros((n, T, N, 2), np.float32)
    R, Tx = np.zeros((n, T, 4), np.float32), np.zeros((n, T, 3))
    ids, src = np.full((n, N), -1, np.int32), np.full((n, N), rn.INT_MIN, np.int32)
    sidx = np.arange(n, 0, -1, dtype=np.int32)
    marks = []
    for h in range(n):
        s = int(sidx[h])
        past = [_pose(f, h) for f in range(-4, 0)]  # the frames the rows were built from
        q0, t0 = _pose(0, h)
        for i in range(T):
            R[h, i], Tx[h, i] = _pose(i, h)
        c0 = rn.camera_centre(q0, t0, inverse)
        qs, ts = [p[0] for p in past], [p[1] for p in past]
        # body points on the unit sphere, those that face the camera at position 0 first
        pts = _sphere(6 * (N + 64) + 200, 10 * seed + h)
        facing = pts @ (c0 / np.linalg.norm(c0)) > 0.5
        front, back = pts[facing], pts[pts @ (c0 / np.linalg.norm(c0)) < -0.5]
        px_front = lmn.project(front, q0, t0, INTR, inverse)[0]
        rows_front = rn.rows_of(front, qs, ts, INTR, inverse)
        take = iter(range(len(front)))
        mark = dict(stream=s)

        def slot(j, ident, source, old=None, old_row=None, alias=-1, pixel=(-500.0, -500.0)):
            if j >= N:
                return False
            ids[h, j], src[h, j] = ident, source
            if old is not None:
                acc[s * N + j], acc_id[s * N + j], st["alias"][s * N + j] = old_row, old, alias
            tracks[h, :, j] = pixel
            return True

        def entry(e, k, ident, centre=c0):
            st["arch"][s * C + e] = rn.entries_of(front[k:k + 1], rows_front[k:k + 1], centre)[0]
            st["arch_id"][s * C + e] = ident

        nid = 1000 * (h + 1)  # fresh ids
        if N == 1:  # one slot, one entry: a born slot takes the entry its own old row then retires to
            k, k2 = next(take), next(take)
            entry(0, k, 77)
            slot(0, nid, BORN, old=5, old_row=rows_front[k2], pixel=px_front[k] + (0.3, -0.2))
            mark.update(matched_own_retires=0, consumed_entry=0)
        else:
            assert N >= 64 and C >= 32
            e8, e12, eta, etb, e16 = 3, 5, 7, 9, 11
            st["arch_cursor"][s] = e8  # the first retirement lands on the entry slot 8 consumes
            k = [next(take) for _ in range(16)]
            slot(0, -1, rn.INT_MIN)                                                   # a pad
            slot(1, 11, 1, old=11, old_row=rows_front[k[0]], alias=4)                 # carried, restored earlier
            slot(2, 12, 2, old=12, old_row=rows_front[k[1]])                          # carried
            slot(3, -1, rn.INT_MIN, old=13, old_row=rows_front[k[2]], alias=6)        # dies: retirable, under its alias
            still = rn.rows_of(front[k[3]:k[3] + 1], qs[:1] * 4, ts[:1] * 4, INTR, inverse)[0]
            slot(4, -1, rn.INT_MIN, old=14, old_row=still)                            # dies: ill-conditioned
            slot(5, -1, rn.INT_MIN, old=15, old_row=rn.rows_of(front[k[4]:k[4] + 1], qs, ts, INTR, inverse, 2)[0])  # too few
            behind = rn.rows_of(front[k[5]:k[5] + 1] * 0 + c0 * 1.5, qs, ts, INTR, inverse)[0]
            slot(6, -1, rn.INT_MIN, old=16, old_row=behind)                           # dies: behind the camera
            bad = rows_front[k[6]].copy()
            bad[7] = np.nan
            slot(7, -1, rn.INT_MIN, old=17, old_row=bad)                              # dies: X not finite
            entry(e8, k[7], 70)
            slot(8, nid, BORN, old=18, old_row=rows_front[k[8]], pixel=px_front[k[7]] + (0.3, -0.2))  # matched, own row retires
            slot(9, nid + 1, BORN)                                                    # born far from everything
            slot(10, nid + 2, BORN, pixel=(np.nan, 10.0))
            slot(11, nid + 3, BORN, pixel=(10.0, np.inf))
            entry(e12, k[9], 71)
            slot(12, nid + 4, BORN, pixel=px_front[k[9]] + (0.2, 0.1))                # the nearer of two: matched
            slot(13, nid + 5, BORN, pixel=px_front[k[9]] + (-0.6, 0.5))               # its pick took slot 12
            entry(eta, k[10], 72)
            entry(etb, k[10], 73)                                                     # a duplicate: the lower entry is picked
            slot(14, nid + 6, BORN, pixel=px_front[k[10]] + (0.4, 0.4))
            slot(15, nid + 7, BORN, pixel=px_front[k[10]] + (0.4, 0.4))               # the same pixel: the lower slot wins
            # archived while it faced the camera from the other side: in front, on the pixel, but turned away
            kb = 0
            st["arch"][s * C + e16] = rn.entries_of(back[kb:kb + 1], rn.rows_of(back[kb:kb + 1], qs, ts, INTR, inverse),
                                                    -c0)[0]
            st["arch_id"][s * C + e16] = 74
            slot(16, nid + 8, BORN, pixel=lmn.project(back[kb:kb + 1], q0, t0, INTR, inverse)[0][0])
            slot(17, nid + 9, BORN, pixel=px_front[k[11]] + (REID_PX * 1.2, 0.0))     # outside the gate
            entry(13, k[11], 75)
            if C > 32:
                entry(C - 1, next(take), 76)                                          # the last entry: a plain candidate
            for e in range(14, min(C, 14 + 24)):                                     # entries in use the ring runs over
                entry(e, next(take), 100 + e)
            for j in range(18, N):  # three of four die and are retirable
                kk = next(take)
                if j % 4 == 0:
                    slot(j, 20 + j, j, old=20 + j, old_row=rows_front[kk])
                elif j % 4 == 1:
                    slot(j, -1, rn.INT_MIN, old=20 + j, old_row=rows_front[kk])
                elif j % 4 == 2:
                    slot(j, nid + 20 + j, BORN, old=20 + j, old_row=rows_front[kk], pixel=rng.uniform(-900.0, -600.0, 2))
                else:
                    slot(j, nid + 20 + j, j, old=20 + j, old_row=rows_front[kk])      # carried by src, another id
            mark.update(matched_own_retires=8, consumed_entry=e8, e12=e12, eta=eta, etb=etb, e16=e16)
        marks.append(mark)
    intr = np.tile(np.array(INTR), (n, 1))
    return dict(tracks=tracks, R=R, T=Tx, ids=ids, src=src, sidx=sidx, intr=intr, acc=acc, acc_id=acc_id, state=st,
                marks=marks, S=S)


def _reference(c, C, inverse):
    acc, acc_id = c["acc"].copy(), c["acc_id"].copy()
    st = {k: v.copy() for k, v in c["state"].items()}
    out = rn.reid(c["tracks"], c["R"], c["T"], c["ids"], c["src"], c["sidx"], c["intr"], acc, acc_id, st, C, REID_PX,
                  MIN_COS, MIN_OBS, inverse, MIN_PIVOT)
    return out, acc, acc_id, st


def _check_margins(c, out, ties):
    """Every comparison that decides an outcome sits 1e-6 (relative) from its threshold; `ties`: the (hop,
    slot) pairs whose best and second-best distances are equal by construction."""
    gate2 = REID_PX * REID_PX
    best, second = out["best"], out["second"]
    fin = np.isfinite(best)
    assert (np.abs(best[fin] - gate2) >= 1e-6 * gate2).all(), "a distance at the gate"
    for h, j in zip(*np.nonzero(np.isfinite(second) & (best <= gate2))):  # (outside the gate nothing is picked)
        if (h, j) in ties:
            assert second[h, j] == best[h, j]
        else:
            assert second[h, j] - best[h, j] >= 1e-6 * second[h, j], (h, j, "best against second best")
    cos = out["cos"][np.isfinite(out["cos"])]
    assert (np.abs(cos - MIN_COS) >= 1e-6).all(), "a cosine at the bound"
    piv, thr = out["pivots"], MIN_PIVOT * out["diag"]
    on = np.isfinite(piv).all(-1) & np.isfinite(thr)
    assert (np.abs(piv[on] - thr[on][:, None]) >= 1e-6 * thr[on][:, None]).all(), "a pivot at its bound"
    # the slots that picked one entry: their distances differ, but for the constructed tie
    n, N = best.shape
    for h in range(n):
        picked = {}
        for j in np.nonzero(out["reid_state"][h] != rn.NOT_BORN)[0]:
            if np.isfinite(best[h, j]) and best[h, j] <= gate2:
                picked.setdefault(round(float(best[h, j]), 12), []).append(j)
        for d, js in picked.items():
            assert len(js) == 1 or all((h, j) in ties for j in js[1:]), (h, js)
