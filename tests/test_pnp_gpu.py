"""PnP refinement on the GPU (comet_landmark_pnp in csrc/pnp.hip, ops.landmark_pnp, LandmarkMap.pnp,
PoseStream / StreamPool pnp=True; DESIGN.md "PnP refinement").

Kernel: against the float64 restatement tests/pnp_numpy.py, which performs the same IEEE operations in the
same order, the strided per-thread sums and the reduction tree included. Bounds: q, t, rms_px and the
injected accumulator rows within 1e-10 relative, n_in and state equal; bit identity is expected and the
measured maxima are printed. Every input set is first checked on the CPU: the smallest pivot of a solved
step lies at least 100 x above min_pivot * max(diag H), that of a degenerate one at least 100 x below.
A hop of three positions holds three of the four states; the others hold all four.

End to end: the golden configuration of tests/test_landmark_gpu.py. Random weights give arbitrary
geometry, so only the mechanics are asserted there, never accuracy."""
import ctypes

import numpy as np
import pytest
import torch

import fuse_numpy as fn
import landmark_numpy as ln
import pnp_numpy as pn
from test_landmark_gpu import (HOPS, N, SEED_X, T, TRACK_INTR, _anchor, _frames, _kw, _np, _poses, _run, _stream,  # noqa: F401
                               mapped, model, plain)

pytestmark = pytest.mark.gpu

INTR = (300.0, 310.0, 63.5, 60.0)
FINTR = (268.4, 270.1, 320.0, 240.0)
HUBER, MIN_PIVOT, TOL, FAR = 3.0, 1e-8, 1e-10, 100.0
WORST = {"q": 0.0, "t": 0.0, "rms": 0.0, "row": 0.0}
LINE = 12  # points of every hop that lie on one line


def _case(n, Tw, N_, s, weighted, inverse, seed=0):
    """n hops of exact projections (f32) with a start pose 1 degree and 1 % off. Per hop: the first LINE
    points are collinear; some landmarks are not valid, one is NaN, one lies behind the camera, some pixels
    and weights are not usable. Special positions (from the last one down, while the window has room):
    only the collinear points usable (state 2), three points usable (state 0), a NaN start (state -1)."""
    rng = np.random.default_rng(seed + 1000 * N_)
    X = rng.uniform(-1.0, 1.0, (n, N_, 3))
    k = min(LINE, N_)
    X[:, :k] = np.linspace(-1.0, 1.0, k)[None, :, None] * np.array([0.6, -0.3, 0.2])
    state = np.ones((n, N_), np.int32)
    tracks = np.zeros((n, Tw, N_, 2), np.float32)
    R0 = np.zeros((n, Tw, 4), np.float32)
    T0 = np.zeros((n, Tw, 3))
    for h in range(n):
        q, t = _poses(seed + h, Tw)
        for i in range(Tw):
            tracks[h, i] = ln.project(X[h], q[i].astype(np.float64), t[i], INTR, inverse)[0].astype(np.float32)
            dq = ln.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(1.0))
            R0[h, i] = fn.unit_pos(fn.qmul(dq, q[i].astype(np.float64))).astype(np.float32)
            T0[h, i] = t[i] * (1.0 + 0.01 * rng.normal(size=3))
    w = rng.uniform(0.5, 1.5, (n, Tw, N_)).astype(np.float32) if weighted else None
    if N_ > 2 * LINE:
        free = np.arange(LINE, N_)
        for h in range(n):
            pick = rng.permutation(free)[:10]
            state[h, pick[0:4]] = (0, 2, 3, -1)
            X[h, pick[4]] = np.nan
            X[h, pick[5]] += np.array(ln.rotation(R0[h, 0], inverse)).T @ [0.0, 0.0, -30.0]
            tracks[h, :, pick[6], 0] = np.nan
            tracks[h, 0, pick[7], 1] = np.inf
            if weighted:
                w[h, :, pick[8]] = 0.0
                w[h, 0, pick[9]] = np.nan
                w[h, Tw - 1, pick[9]] = -1.0
    h = n - 1
    if Tw >= 3:
        tracks[h, Tw - 1, k:] = np.nan     # only the line: degenerate
        T0[h, Tw - 2, 1] = np.nan          # a start that is not finite
    if Tw >= 4:
        tracks[h, Tw - 3, 3:] = np.nan     # three points: too few
    return dict(tracks=tracks, X=X, state=state, R0=R0, T0=T0, intr=np.array([INTR] * n), weights=w)


def _device(c, s, iters, inverse, acc=None, slots=None, inject_w=0.0, rows=None):
    from comet_amd import ops
    d = {k: None if v is None else torch.as_tensor(v).cuda().contiguous() for k, v in c.items()}
    flat = [float(v) for v in c["intr"].ravel()]
    kw = {}
    if acc is not None:
        kw = dict(fuse_acc=acc, slots=torch.tensor(slots, dtype=torch.int32, device="cuda"),
                  slots_host=(ctypes.c_int32 * len(slots))(*slots), inject_w=inject_w, fuse_intr=FINTR)
    out = ops.landmark_pnp(d["tracks"], d["X"], d["state"], d["R0"], d["T0"], d["intr"], (ctypes.c_double * len(flat))(*flat),
                           s, HUBER, d["weights"], inverse, iters, 6, MIN_PIVOT, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out._asdict().items()}


def _reference(c, s, iters, inverse, acc=None, slots=None, inject_w=0.0):
    trace = {}
    ref = pn.pnp(c["tracks"], c["X"], c["state"], c["R0"], c["T0"], c["intr"], s, HUBER, c["weights"], inverse, iters, 6,
                 MIN_PIVOT, acc, slots, inject_w, FINTR, trace)
    for (h, i), its in trace.items():
        for k, it in enumerate(its):
            m = min(it["pivots"]) / (MIN_PIVOT * it["diag"])
            solved = "q" in it
            if solved:
                assert m >= FAR, f"hop {h} position {i} iteration {k}: a pivot at {m:.3e} of the bound"
            elif ref["state"][h, i] == pn.DEGENERATE:
                assert m <= 1.0 / FAR, f"hop {h} position {i} iteration {k}: a degenerate pivot at {m:.3e} of the bound"
    return ref


def _rel(a, b):
    return float((np.abs(a - b) / (1.0 + np.abs(b))).max()) if a.size else 0.0


def _compare(got, ref, c, what):
    assert got["state"].dtype == np.int32 and (got["state"] == ref["state"]).all(), (what, got["state"], ref["state"])
    assert (got["inliers"] == ref["n_in"]).all(), what
    on = ref["state"] == 1
    assert got["R"][~on].tobytes() == c["R0"][~on].tobytes() and got["T"][~on].tobytes() == c["T0"][~on].tobytes(), what
    assert got["q"][~on].tobytes() == c["R0"][~on].astype(np.float64).tobytes(), what
    assert np.isposinf(got["rms_px"][~on]).all() and (got["inliers"][~on] == 0).all(), what
    dq, dt = _rel(got["q"][on], ref["q"][on]), _rel(got["T"][on], ref["t"][on])
    dr = _rel(got["rms_px"][on].astype(np.float64), ref["rms_px"][on].astype(np.float64))
    WORST["q"], WORST["t"], WORST["rms"] = max(WORST["q"], dq), max(WORST["t"], dt), max(WORST["rms"], dr)
    assert dq <= TOL and dt <= TOL and dr <= TOL, (what, dq, dt, dr)
    assert got["R"][on].tobytes() == got["q"][on].astype(np.float32).tobytes(), (what, "R is q rounded")


SHAPES = [(1, 4, 64, 1), (3, 5, 70, 2), (1, 2, 1, 1), (2, 4, 257, 3), (1, 3, 4096, 1)]


@pytest.mark.parametrize("n,Tw,N_,s", SHAPES)
def test_kernel_equals_the_restatement(n, Tw, N_, s):
    seen = set()
    for weighted in (False, True):
        for inverse in (0, 1):
            c = _case(n, Tw, N_, s, weighted, inverse)
            for iters in (1, 4):
                rows = n * Tw + 3
                slots = [int(v) for v in np.random.default_rng(5).permutation(rows)[:n * Tw]]
                acc0 = np.random.default_rng(6).normal(size=(rows, fn.ROW))
                acc_ref = acc0.copy()
                ref = _reference(c, s, iters, inverse, acc_ref, slots, 0.75)
                acc = torch.as_tensor(acc0).cuda()
                got = _device(c, s, iters, inverse, acc, slots, 0.75)
                what = f"n={n} T={Tw} N={N_} s={s} weighted={weighted} inverse={inverse} K={iters}"
                _compare(got, ref, c, what)
                rows_got = acc.cpu().numpy()
                touched = [slots[h * Tw + i] for h in range(n) for i in range(s, Tw) if ref["state"][h, i] == 1]
                rest = [r for r in range(rows) if r not in touched]
                assert rows_got[rest].tobytes() == acc0[rest].tobytes(), (what, "untouched rows")
                dr = _rel(rows_got[touched], acc_ref[touched])
                WORST["row"] = max(WORST["row"], dr)
                assert dr <= TOL, (what, "injected rows", dr)
                assert (rows_got[touched][:, 17] == acc0[touched][:, 17] + 1).all()
                seen |= set(int(v) for v in ref["state"].ravel())
    if N_ == 1:
        assert seen == {0}
    elif Tw >= 4:
        assert seen == {1, 0, 2, -1}, seen
    else:
        assert seen == {1, 2, -1}, seen
    print(f"N={N_}: max relative difference so far: q {WORST['q']:.3e}, t {WORST['t']:.3e}, rms_px {WORST['rms']:.3e}, "
          f"injected rows {WORST['row']:.3e}")


def test_three_hops_in_one_launch_equal_three_single_hop_launches():
    c = _case(3, 5, 70, 2, True, 0)
    rows = 20
    slots = list(range(15))
    acc0 = np.random.default_rng(6).normal(size=(rows, fn.ROW))
    acc = torch.as_tensor(acc0).cuda()
    whole = _device(c, 2, 4, 0, acc, slots, 0.5)
    acc1 = torch.as_tensor(acc0).cuda()
    for h in range(3):
        one = {k: None if v is None else v[h:h + 1] for k, v in c.items()}
        part = _device(one, 2, 4, 0, acc1, slots[h * 5:(h + 1) * 5], 0.5)
        for k, v in part.items():
            assert v.tobytes() == whole[k][h:h + 1].tobytes(), (h, k)
    assert torch.equal(acc.view(torch.int64), acc1.view(torch.int64))


def test_no_accumulator_or_no_weight_writes_nothing():
    c = _case(1, 4, 64, 1, False, 0)
    acc0 = np.random.default_rng(6).normal(size=(6, fn.ROW))
    acc = torch.as_tensor(acc0).cuda()
    a = _device(c, 1, 4, 0, acc, [0, 1, 2, 3], 0.0)
    b = _device(c, 1, 4, 0)
    assert acc.cpu().numpy().tobytes() == acc0.tobytes()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["state"] == 1).any()


def test_landmark_pnp_wrapper_rejects_bad_arguments():
    from comet_amd import _lib, ops
    c = _case(1, 4, 64, 1, False, 0)
    d = {k: None if v is None else torch.as_tensor(v).cuda().contiguous() for k, v in c.items()}
    host = (ctypes.c_double * 4)(*INTR)
    args = lambda **kw: [kw.get(k, d[k]) for k in ("tracks", "X", "state", "R0", "T0", "intr")]  # noqa: E731
    with pytest.raises(_lib.CometHipError, match="X must be a dense"):
        ops.landmark_pnp(*args(X=d["X"].float()), host, 1, HUBER)
    with pytest.raises(_lib.CometHipError, match="intr_host needs 4 n"):
        ops.landmark_pnp(*args(), (ctypes.c_double * 3)(1.0, 1.0, 1.0), 1, HUBER)
    with pytest.raises(_lib.CometHipError, match="fuse_acc needs slots"):
        ops.landmark_pnp(*args(), host, 1, HUBER, fuse_acc=torch.zeros(4, 20, dtype=torch.float64, device="cuda"))
    with pytest.raises(_lib.CometHipError, match="huber_px must be finite and positive"):
        ops.landmark_pnp(*args(), host, 1, 0.0)


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
PNP = dict(landmarks=True, track_intr=TRACK_INTR, lm_min_obs=2, pnp=True, pnp_huber_px=HUBER)


@pytest.fixture(scope="module")
def posed(model):
    """The golden stream with landmarks and pnp=True, report only."""
    return _run(_stream(model, **PNP), _frames(SEED_X, T + HOPS))


def _pnp_fields(r):
    return dict(R=_np(r.pnp_R)[None], T=_np(r.pnp_T)[None], inliers=_np(r.pnp_inliers)[None], rms_px=_np(r.pnp_rms_px)[None],
                state=_np(r.pnp_state)[None])


def test_report_only_changes_nothing_and_equals_the_restatement(posed, mapped):
    base, _ = mapped
    assert len(posed) == len(base) == HOPS + 1
    for k, (r, b) in enumerate(zip(posed, base)):
        for name in ("pred_pose_enc", "pred_tracks", "pred_score", "fused_R", "fused_T", "fused_count", "track_ids",
                     "track_age", "track_src", "landmark_obs", "landmark_state"):
            assert torch.equal(getattr(r, name), getattr(b, name)), (k, name)
        assert torch.equal(r.landmarks.view(torch.int64), b.landmarks.view(torch.int64)), k
        assert torch.equal(r.landmark_err.view(torch.int32), b.landmark_err.view(torch.int32)), k
        assert len(r) == 12 and b.pnp_R is None
        ref = pn.pnp(_np(r.pred_tracks)[None], _np(r.landmarks)[None], _np(r.landmark_state)[None], _np(r.fused_R)[None],
                     _np(r.fused_T)[None], np.array([TRACK_INTR]), 1, HUBER)
        got = _pnp_fields(r)
        hist = {v: int((got["state"] == v).sum()) for v in (-1, 0, 1, 2)}
        print(f"hop {k}: pnp states {hist}, inliers {got['inliers'][0].tolist()}, rms_px {got['rms_px'][0].tolist()}")
        assert (got["state"] == ref["state"]).all() and (got["inliers"] == ref["n_in"]).all(), k
        on = ref["state"] == 1
        assert got["R"][~on].tobytes() == _np(r.fused_R)[None][~on].tobytes(), k
        assert got["T"][~on].tobytes() == _np(r.fused_T)[None][~on].tobytes(), k
        assert _rel(got["T"][on], ref["t"][on]) <= TOL and got["R"][on].tobytes() == ref["R"][on].tobytes(), k
        assert got["rms_px"][on].tobytes() == ref["rms_px"][on].tobytes(), k


def test_feedback_adds_one_hypothesis_per_solved_position(model, posed):
    """pnp_weight = 1: the first hop is the report-only run's; afterwards the fused count of a frame is the
    report-only run's plus the solved PnP poses injected on it by the earlier hops. With the golden
    configuration's random weights only position 0 of a hop is ever solved (measured: 0 hypotheses injected
    over 6 hops), so what this run shows is that the accounting holds and nothing else is written; the
    feedback on geometry, against the restatement chain, is tests/test_pnp_stream_gpu.py."""
    got = _run(_stream(model, **dict(PNP, pnp_weight=1.0)), _frames(SEED_X, T + HOPS))
    for name in ("pred_pose_enc", "fused_R", "fused_T", "fused_count", "pnp_R", "pnp_T", "pnp_state", "landmark_state"):
        assert torch.equal(getattr(got[0], name), getattr(posed[0], name)), name
    injected, total = {}, 0
    for k, (g, p) in enumerate(zip(got, posed)):
        want = [int(p.fused_count[i]) + injected.get(g.frame_index + i, 0) for i in range(T)]
        assert g.fused_count.tolist() == want, (k, g.fused_count.tolist(), want)
        for i in range(1, T):
            if int(g.pnp_state[i]) == 1:
                injected[g.frame_index + i] = injected.get(g.frame_index + i, 0) + 1
                total += 1
    print(f"feedback: {total} hypotheses injected over {len(got)} hops")


def test_pool_of_one_stream_equals_the_stream_bit_for_bit(model, posed):
    from comet_amd.stream import StreamPool
    kw = dict(PNP, track_intrs=[TRACK_INTR])
    del kw["track_intr"]
    pool = StreamPool(model, streams=1, anchors=[_anchor()], **_kw(**kw))
    frames = _frames(SEED_X, T + HOPS)
    got = [r for f in range(frames.shape[0]) for _, r in pool.push(frames[f][None])]
    assert len(got) == len(posed)
    for k, (g, b) in enumerate(zip(got, posed)):
        assert torch.equal(g.pnp_T.view(torch.int64), b.pnp_T.view(torch.int64)), k
        assert torch.equal(g.pnp_R.view(torch.int32), b.pnp_R.view(torch.int32)), k
        assert torch.equal(g.pnp_rms_px.view(torch.int32), b.pnp_rms_px.view(torch.int32)), k
        assert torch.equal(g.pnp_inliers, b.pnp_inliers) and torch.equal(g.pnp_state, b.pnp_state), k
