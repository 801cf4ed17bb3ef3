"""Float64 restatement of comet_motion_fit (include/comet_hip.h, csrc/motion.hip): the same operations
in the same order, the 64-lane shuffle tree included, with numpy's arctan2 / sin / cos where the kernel
calls the device library's. Every quantity of a hop is a 64-vector, one entry per lane."""
import numpy as np

LANES = 64
ROW = 8
COUNT_FOLD = 1 << 30


def qmul(a, b):
    """Hamilton product, w first; a, b [..., 4]."""
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw], -1)


def qconj(a):
    return np.stack([a[..., 0], -a[..., 1], -a[..., 2], -a[..., 3]], -1)


def qlog(d):
    """d [..., 4] -> (phi [..., 3], theta [...]); d negated where its w < 0."""
    d = np.where(d[..., :1] < 0.0, -d, d)
    x, y, z = d[..., 1], d[..., 2], d[..., 3]
    nv = np.sqrt(x * x + y * y + z * z)
    zero = nv == 0.0
    theta = 2.0 * np.arctan2(nv, d[..., 0])
    f = theta / np.where(zero, 1.0, nv)
    phi = np.stack([f * x, f * y, f * z], -1)
    return np.where(zero[..., None], 0.0, phi), np.where(zero, 0.0, theta)


def qexp(p):
    """p [..., 3] -> [..., 4]."""
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    theta = np.sqrt(px * px + py * py + pz * pz)
    zero = theta == 0.0
    half = 0.5 * theta
    f = np.sin(half) / np.where(zero, 1.0, theta)
    q = np.stack([np.cos(half), f * px, f * py, f * pz], -1)
    ident = np.zeros_like(q)
    ident[..., 0] = 1.0
    return np.where(zero[..., None], ident, q)


def wave_sum(p):
    """p[l] += p[l + d], d = 32 .. 1 -> lane 0's value."""
    p = np.array(p, dtype=np.float64)
    d = 32
    while d >= 1:
        p[:d] = p[:d] + p[d:2 * d]
        d >>= 1
    return p[0]


def _line(usable, wk, wt, x, Sw, St, D):
    Sp = wave_sum(np.where(usable, wk * x, 0.0))
    Stp = wave_sum(np.where(usable, wt * x, 0.0))
    slope = (Sw * Stp - St * Sp) / D
    return slope, (Sp - slope * St) / Sw


def _frame(R, T, weights, h, i, inverse):
    q = R[h, i].astype(np.float64)
    if inverse:
        q = qconj(q)
    t = T[h, i].astype(np.float64)
    w = 1.0 if weights is None else float(np.float64(weights[h, i]))
    ok = np.isfinite(q).all() and np.isfinite(t).all() and np.isfinite(w) and w > 0.0
    return np.concatenate([q, t, [w if ok else 0.0]])


def motion_fit(R, T, first, stream_idx, hist, hist_n, s, weights=None, fit_len=16, min_frames=3, iters=2, horizon=1,
               max_angle=2.0, inverse_rotation=0):
    """R [n, T, 4] f32, T [n, T, 3] f64, first [n], stream_idx [n]; hist [S, cap, 8] f64 and hist_n [S]
    int32 are updated in place -> dict of the kernel's outputs."""
    R, T = np.asarray(R, np.float32), np.asarray(T, np.float64)
    n, Tw = R.shape[:2]
    cap = hist.shape[1]
    P = Tw - s + horizon
    out = dict(omega=np.zeros((n, 3)), q0=np.zeros((n, 4)), vel=np.zeros((n, 3)), t0=np.zeros((n, 3)),
               rot_rms=np.zeros(n, np.float32), trans_rms=np.zeros((n, 3), np.float32), n_used=np.zeros(n, np.int32),
               state=np.zeros(n, np.int32), pred_q=np.zeros((n, P, 4)), pred_t=np.zeros((n, P, 3)),
               innov_rot=np.zeros((n, Tw - s), np.float32), innov_trans=np.zeros((n, Tw - s), np.float32))
    inf32 = np.float32(np.inf)
    with np.errstate(all="ignore"):
        for h in range(n):
            sidx = int(stream_idx[h])
            c = 0 if first[h] else max(int(hist_n[sidx]), 0)
            c1 = c + s
            old = hist[sidx].copy()  # (the kernel reads only rows that its append does not write)
            for i in range(s):
                if s - i <= cap:
                    hist[sidx, (c + i) % cap] = _frame(R, T, weights, h, i, inverse_rotation)
            hist_n[sidx] = c1 if c1 < COUNT_FOLD else cap + c1 % cap
            m = min(c1, fit_len)
            rows = np.zeros((LANES, ROW))
            rows[:, 0] = 1.0
            for k in range(m):
                rows[k] = _frame(R, T, weights, h, s - 1 - k, inverse_rotation) if k < s else old[(c1 - 1 - k) % cap]
            q, t, w = rows[:, :4], rows[:, 4:7], rows[:, 7]
            k = np.arange(LANES)
            usable = (k < m) & ~(w == 0.0)
            n_used = int(usable.sum())
            tau = -k.astype(np.float64)
            wk = np.where(usable, w, 0.0)
            wt = wk * tau
            qn, tn = q[0].copy(), t[0].copy()

            st = 1
            om, vel, t0, qr = np.zeros(3), np.zeros(3), tn.copy(), qn.copy()
            rot_rms, trans_rms = inf32, np.full(3, inf32)
            if n_used < min_frames:
                st = 0
            else:
                Sw = wave_sum(np.where(usable, wk, 0.0))
                St = wave_sum(np.where(usable, wt, 0.0))
                Stt = wave_sum(np.where(usable, wt * tau, 0.0))
                D = Sw * Stt - St * St
                if not (np.isfinite(Sw) and np.isfinite(St) and np.isfinite(Stt) and np.isfinite(D)):
                    st = -1
                elif D <= 0.0:
                    st = 2
            if st == 1:
                qr = q[int(np.argmax(usable))].copy()
                for _ in range(iters):
                    phi, theta = qlog(qmul(q, qconj(qr)[None]))
                    if (usable & (theta > max_angle)).any():
                        st = 3
                        break
                    off = np.zeros(3)
                    for j in range(3):
                        om[j], off[j] = _line(usable, wk, wt, phi[:, j], Sw, St, D)
                    if not (np.isfinite(om).all() and np.isfinite(off).all()):
                        st = -1
                        break
                    qq = qmul(qexp(off), qr)
                    nrm = np.sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3])
                    sg = (-1.0 if qq[0] < 0.0 else 1.0) / nrm
                    qr = qq * sg
                    if not np.isfinite(qr).all():
                        st = -1
                        break
                if st == 1:
                    phi, theta = qlog(qmul(q, qconj(qr)[None]))
                    if (usable & (theta > max_angle)).any():
                        st = 3
                    else:
                        r0, r1, r2 = phi[:, 0] - om[0] * tau, phi[:, 1] - om[1] * tau, phi[:, 2] - om[2] * tau
                        rms = np.sqrt(wave_sum(np.where(usable, wk * (r0 * r0 + r1 * r1 + r2 * r2), 0.0)) / Sw)
                        if not np.isfinite(rms):
                            st = -1
                        rot_rms = np.float32(rms)
                if st == 1:
                    for j in range(3):
                        vel[j], t0[j] = _line(usable, wk, wt, t[:, j], Sw, St, D)
                        r = (t[:, j] - t0[j]) - vel[j] * tau
                        rms = np.sqrt(wave_sum(np.where(usable, wk * (r * r), 0.0)) / Sw)
                        if not (np.isfinite(vel[j]) and np.isfinite(t0[j]) and np.isfinite(rms)):
                            st = -1
                        trans_rms[j] = np.float32(rms)
                if st != 1:
                    om, vel, t0, qr = np.zeros(3), np.zeros(3), tn.copy(), qn.copy()
                    rot_rms, trans_rms = inf32, np.full(3, inf32)

            out["omega"][h], out["q0"][h], out["vel"][h], out["t0"][h] = om, qr, vel, t0
            out["rot_rms"][h], out["trans_rms"][h], out["n_used"][h], out["state"][h] = rot_rms, trans_rms, n_used, st
            for j in range(P):
                tp = float(j + 1)
                pq = qmul(qexp(om * tp), qr) if st == 1 else qr.copy()
                if inverse_rotation:
                    pq = qconj(pq)
                pt = t0 + vel * tp if st == 1 else t0.copy()
                out["pred_q"][h, j], out["pred_t"][h, j] = pq, pt
                if j < Tw - s:
                    ir = it = inf32
                    if st == 1:
                        _, th = qlog(qmul(R[h, s + j].astype(np.float64), qconj(pq)))
                        d = T[h, s + j] - pt
                        ir, it = np.float32(th), np.float32(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
                    out["innov_rot"][h, j], out["innov_trans"][h, j] = ir, it
    return out
