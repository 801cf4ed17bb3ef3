"""comet_motion_fit on the GPU against its float64 restatement (tests/motion_numpy.py).

Integers and states must be equal, the history bit-identical (it is only copied), every floating output
within |a - b| <= 1e-10 max(1, |b|): the device's atan2 / sin / cos are not libm's, so bit identity is not
expected there. Every input set is checked on the CPU first to lie 100 x on its side of the two decisions a
rounding could flip: max_angle against the largest relative rotation, and D > 0."""
import itertools

import numpy as np
import pytest
import torch

import motion_numpy as mn

pytestmark = pytest.mark.gpu

TOL = 1e-10
WORST = {"err": 0.0}  # the measured maximum over the module, printed by the last kernel test
FLOATS = ("omega", "q0", "vel", "t0", "rot_rms", "trans_rms", "pred_q", "pred_t", "innov_rot", "innov_trans")


def _device_fit(R, Tx, first, stream_idx, hist, hist_n, s, weights=None, **kw):
    """ops.motion_fit on copies of the numpy arguments -> (outputs as numpy, hist, hist_n after the launch)."""
    import ctypes
    from comet_amd import ops
    dev = "cuda"
    h, hn = torch.tensor(hist, device=dev), torch.tensor(hist_n, device=dev)
    idx = [int(v) for v in stream_idx]
    out = ops.motion_fit(torch.tensor(R, dtype=torch.float32, device=dev), torch.tensor(Tx, dtype=torch.float64, device=dev),
                         torch.tensor(first, dtype=torch.int32, device=dev), torch.tensor(idx, dtype=torch.int32, device=dev),
                         (ctypes.c_int32 * len(idx))(*idx), h, hn, s,
                         None if weights is None else torch.tensor(weights, dtype=torch.float32, device=dev), **kw)
    torch.cuda.synchronize()
    names = ("omega", "q0", "vel", "t0", "rot_rms", "trans_rms", "n_used", "state", "pred_q", "pred_t", "innov_rot",
             "innov_trans")
    return {k: v.cpu().numpy() for k, v in zip(names, out)}, h.cpu().numpy(), hn.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _compare(got, ref, what):
    assert (got["n_used"] == ref["n_used"]).all() and (got["state"] == ref["state"]).all(), \
        (what, got["state"], ref["state"], got["n_used"], ref["n_used"])
    for k in FLOATS:
        a, b = got[k].astype(np.float64), ref[k].astype(np.float64)
        assert a.shape == b.shape, (what, k)
        fin = np.isfinite(b)
        assert (np.isfinite(a) == fin).all() and (a[~fin] == b[~fin])[~np.isnan(b[~fin])].all(), (what, k)
        assert (np.isnan(a) == np.isnan(b)).all(), (what, k)
        err = float((np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))).max()) if fin.any() else 0.0
        WORST["err"] = max(WORST["err"], err)
        assert err <= TOL, (what, k, err)


def _margins(hist, hist_n, R, Tx, first, stream_idx, s, weights, fit_len, max_angle, inverse):
    """The CPU check of an input set that is meant to be fitted: 100 x clear of max_angle and of D > 0."""
    for h, sid in enumerate(stream_idx):
        hs, hn = hist.copy(), hist_n.copy()
        mn.motion_fit(R[h:h + 1], Tx[h:h + 1], first[h:h + 1], [sid], hs, hn, s,
                      weights=None if weights is None else weights[h:h + 1], fit_len=fit_len, inverse_rotation=inverse)
        cap = hist.shape[1]
        c1 = int(hn[sid])
        m = min(c1, fit_len)
        rows = np.stack([hs[sid, (c1 - 1 - k) % cap] for k in range(m)])
        use = rows[:, 7] != 0
        if use.sum() < 2:
            continue
        q = rows[use, :4]
        ref = q[0]
        theta = max(float(mn.qlog(mn.qmul(qk, mn.qconj(ref)))[1]) for qk in q)
        assert theta * 100.0 <= max_angle, (h, theta)
        w, tau = rows[use, 7], -np.arange(m)[use].astype(np.float64)
        Sw, St, Stt = w.sum(), (w * tau).sum(), (w * tau * tau).sum()
        assert Sw * Stt - St * St >= 100.0 * 2.0 ** -52 * Sw * Stt, h


def _case(n, Tw, s, cap, fit_len, committed, weighted, inverse, seed):
    """n hops on n of n + 1 streams, each with `committed` frames behind it (planted in float64, as if a run
    had stored them), slowly spinning bodies with a little noise."""
    rng = np.random.default_rng(seed)
    S = n + 1
    stream_idx = list(rng.permutation(S)[:n])
    hist, hist_n = np.zeros((S, cap, 8)), np.zeros(S, np.int32)
    R, Tx = np.zeros((n, Tw, 4), np.float32), np.zeros((n, Tw, 3))
    for h, sid in enumerate(stream_idx):
        frames = committed + Tw
        omega = 4e-3 / fit_len * rng.normal(size=3)  # (the span of the fit stays 100 x inside max_angle = 2)
        base = mn.qexp(rng.normal(size=3))
        q = np.stack([mn.qmul(mn.qexp(omega * f + 1e-5 * rng.normal(size=3)), base) for f in range(frames)])
        q = np.where(q[:, :1] < 0, -q, q).astype(np.float32).astype(np.float64)
        t = rng.normal(size=3) + 0.01 * rng.normal(size=3) * np.arange(frames)[:, None] + 1e-4 * rng.normal(size=(frames, 3))
        for f in range(max(0, committed - cap), committed):
            hist[sid, f % cap] = np.concatenate([mn.qconj(q[f]) if inverse else q[f], t[f], [rng.uniform(0.5, 1.5)]])
        if committed >= 3:
            hist[sid, (committed - 2) % cap, 7] = 0.0  # one weightless row inside the span
        hist_n[sid] = committed
        R[h], Tx[h] = q[committed:], t[committed:]
    weights = None
    if weighted:
        weights = rng.uniform(0.5, 1.5, (n, Tw)).astype(np.float32)
        if s >= 2:
            weights[0, 0] = np.nan  # stored with w = 0
    first = [int(committed == 0)] * n
    return R, Tx, first, stream_idx, hist, hist_n, weights


SHAPES = [(1, 2, 1, 2, 2, 0), (1, 4, 1, 16, 16, 2), (3, 5, 3, 8, 5, 7), (2, 4, 2, 64, 64, 62), (1, 4, 1, 64, 63, 200)]


@pytest.mark.parametrize("n,Tw,s,cap,fit_len,committed", SHAPES)
@pytest.mark.parametrize("weighted,inverse", list(itertools.product([False, True], [0, 1])))
def test_kernel_equals_the_restatement(n, Tw, s, cap, fit_len, committed, weighted, inverse):
    R, Tx, first, idx, hist, hist_n, weights = _case(n, Tw, s, cap, fit_len, committed, weighted, inverse,
                                                      seed=100 * n + 10 * Tw + s + committed)
    min_frames = min(3, fit_len)
    _margins(hist, hist_n, R, Tx, first, idx, s, weights, fit_len, 2.0, inverse)
    fitted = 0
    for iters, horizon in itertools.product([1, 2], [0, 3]):
        kw = dict(weights=weights, fit_len=fit_len, min_frames=min_frames, iters=iters, horizon=horizon, max_angle=2.0,
                  inverse_rotation=inverse)
        got, h_dev, n_dev = _device_fit(R, Tx, first, idx, hist, hist_n, s, **kw)
        h_ref, n_ref = hist.copy(), hist_n.copy()
        ref = mn.motion_fit(R, Tx, first, idx, h_ref, n_ref, s, **kw)
        what = f"n={n} T={Tw} s={s} cap={cap} fit_len={fit_len} committed={committed} iters={iters} horizon={horizon}"
        assert (n_dev == n_ref).all() and (n_ref[idx] == committed + s).all(), what
        assert (_bits(h_dev) == _bits(h_ref)).all(), (what, "hist")
        assert got["pred_q"].shape == (n, Tw - s + horizon, 4) and got["innov_rot"].shape == (n, Tw - s), what
        _compare(got, ref, what)
        fitted += int((ref["state"] == 1).sum())
    if committed + s >= min_frames + 1:
        assert fitted == 4 * n, "a case meant to be fitted was not"
    print(f"max |kernel - restatement| / max(1, |restatement|) so far: {WORST['err']:.3e}")


@pytest.mark.parametrize("inverse", [0, 1])
def test_every_state_in_one_launch(inverse):
    """Five hops, one per state: 1 fitted, 0 a first hop, 2 weights whose products underflow, 3 a 1.5 rad
    jump against max_angle = 0.01, -1 a NaN weight in the caller's history."""
    rng = np.random.default_rng(5)
    cap, Tw, s, n = 8, 3, 1, 5
    hist, hist_n = np.zeros((n, cap, 8)), np.full(n, 6, np.int32)
    R, Tx = np.zeros((n, Tw, 4), np.float32), np.zeros((n, Tw, 3))
    for h in range(n):
        omega = 1e-5 * rng.normal(size=3)
        base = mn.qexp(rng.normal(size=3))
        q = np.stack([mn.qmul(mn.qexp(omega * f), base) for f in range(6 + Tw)])
        if h == 3:
            q[6:] = [mn.qmul(mn.qexp(np.array([0.0, 1.5, 0.0])), qq) for qq in q[6:]]
        q = np.where(q[:, :1] < 0, -q, q).astype(np.float32).astype(np.float64)
        t = rng.normal(size=3) + 0.01 * np.arange(6 + Tw)[:, None]
        for f in range(6):
            hist[h, f] = np.concatenate([mn.qconj(q[f]) if inverse else q[f], t[f], [1.0]])
        R[h], Tx[h] = q[6:], t[6:]
    hist[2, :, 7] = 1e-170
    R[2] = np.nan  # (its committed frame is stored weightless, so only the vanishing weights are summed)
    hist[4, 3, 7] = np.nan
    first = [0, 1, 0, 0, 0]
    kw = dict(fit_len=8, min_frames=3, iters=2, horizon=2, max_angle=0.01, inverse_rotation=inverse)
    keep = [0]
    _margins(hist, hist_n, R[keep], Tx[keep], [0], [0], s, None, 8, 0.01, inverse)
    got, h_dev, n_dev = _device_fit(R, Tx, first, list(range(n)), hist, hist_n, s, **kw)
    h_ref, n_ref = hist.copy(), hist_n.copy()
    ref = mn.motion_fit(R, Tx, first, list(range(n)), h_ref, n_ref, s, **kw)
    assert ref["state"].tolist() == [1, 0, 2, 3, -1], ref["state"]
    assert n_ref.tolist() == [7, 1, 7, 7, 7] and (n_dev == n_ref).all()
    assert (_bits(h_dev) == _bits(h_ref)).all()
    _compare(got, ref, "states")
    for h in (1, 2, 3, 4):  # the newest committed pose bit for bit, no rate, no residual
        assert (_bits(got["q0"][h]) == _bits(h_ref[h, (n_ref[h] - 1) % cap, :4])).all(), h
        assert (_bits(got["t0"][h]) == _bits(Tx[h, 0])).all() and (_bits(got["pred_t"][h]) == _bits(Tx[h, 0])).all(), h
        assert (got["omega"][h] == 0).all() and (got["vel"][h] == 0).all() and np.isposinf(got["rot_rms"][h]), h
        assert np.isposinf(got["innov_rot"][h]).all() and np.isposinf(got["innov_trans"][h]).all(), h
        assert (_bits(got["pred_q"][h]) == _bits(R[h, 0].astype(np.float64))).all(), h


def test_the_count_saturates_on_the_device_as_in_the_restatement():
    R, Tx, first, idx, hist, hist_n, _ = _case(1, 4, 2, 6, 6, 20, False, 0, seed=9)
    hist_n[idx[0]] = mn.COUNT_FOLD - 1
    got, h_dev, n_dev = _device_fit(R, Tx, first, idx, hist, hist_n, 2, fit_len=6)
    h_ref, n_ref = hist.copy(), hist_n.copy()
    ref = mn.motion_fit(R, Tx, first, idx, h_ref, n_ref, 2, fit_len=6)
    assert (n_dev == n_ref).all() and n_ref[idx[0]] == 6 + (mn.COUNT_FOLD + 1) % 6
    assert (_bits(h_dev) == _bits(h_ref)).all()
    assert (got["state"] == ref["state"]).all() and (got["n_used"] == ref["n_used"]).all()


def test_three_hops_in_one_launch_equal_three_single_hop_launches():
    R, Tx, first, idx, hist, hist_n, weights = _case(3, 5, 3, 8, 5, 7, True, 1, seed=77)
    kw = dict(fit_len=5, min_frames=3, iters=2, horizon=3, inverse_rotation=1)
    got, h_all, n_all = _device_fit(R, Tx, first, idx, hist, hist_n, 3, weights=weights, **kw)
    h_one, n_one = hist, hist_n
    for h in range(3):
        one, h_one, n_one = _device_fit(R[h:h + 1], Tx[h:h + 1], first[h:h + 1], idx[h:h + 1], h_one, n_one, 3,
                                        weights=weights[h:h + 1], **kw)
        for k in got:
            assert got[k][h].tobytes() == one[k][0].tobytes(), (h, k)
    assert (_bits(h_all) == _bits(h_one)).all() and (n_all == n_one).all()
    print(f"max |kernel - restatement| / max(1, |restatement|) over the module: {WORST['err']:.3e}")


def test_motion_fit_wrapper_rejects_bad_arguments():
    import ctypes
    from comet_amd import _lib, ops
    dev = "cuda"
    R, Tx = torch.zeros(1, 4, 4, device=dev), torch.zeros(1, 4, 3, dtype=torch.float64, device=dev)
    first, idx = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    host = (ctypes.c_int32 * 1)(0)
    hist, hist_n = torch.zeros(1, 16, 8, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.CometHipError, match="device tensors"):
        ops.motion_fit(R.cpu(), Tx, first, idx, host, hist, hist_n, 1)
    with pytest.raises(_lib.CometHipError, match=r"R must be a dense f32 \[n, T, 4\]"):
        ops.motion_fit(R.double(), Tx, first, idx, host, hist, hist_n, 1)
    with pytest.raises(_lib.CometHipError, match="T must be a dense"):
        ops.motion_fit(R, Tx.float(), first, idx, host, hist, hist_n, 1)
    with pytest.raises(_lib.CometHipError, match="hist must be a dense f64"):
        ops.motion_fit(R, Tx, first, idx, host, hist[:, :, :7].contiguous(), hist_n, 1)
    with pytest.raises(_lib.CometHipError, match="hist_n must be a dense int32"):
        ops.motion_fit(R, Tx, first, idx, host, hist, hist_n.long(), 1)
    with pytest.raises(_lib.CometHipError, match="weights must be a dense"):
        ops.motion_fit(R, Tx, first, idx, host, hist, hist_n, 1, weights=torch.ones(1, 3, device=dev))
    with pytest.raises(_lib.CometHipError, match=r"s outside \[1, T - 1\]"):
        ops.motion_fit(R, Tx, first, idx, host, hist, hist_n, 4)
    with pytest.raises(_lib.CometHipError, match="fit_len outside"):
        ops.motion_fit(R, Tx, first, idx, host, hist, hist_n, 1, fit_len=17)
    assert int(hist_n[0]) == 0, "a rejected call launches nothing"
