"""PnP refinement without a GPU (DESIGN.md "PnP refinement"): the float64 restatement tests/pnp_numpy.py of
comet_landmark_pnp on synthetic rigid-body scenes, its states, its pivots, the injection into the fusion
accumulator, the drift with and without the feedback on the restatement chain, and the host logic
(constructor checks, config plumbing, the CSV writer, the appended result fields).

HUBER = 3 px is the threshold of these tests (six times the 0.5 px noise they add), not a recommendation.
Measured figures: DESIGN.md "PnP refinement"."""
import math

import numpy as np
import pytest
import torch

import fuse_numpy as fn
import landmark_numpy as ln
import pnp_numpy as pn
from test_fuse_cpu import HOPS, RATIO, SIG_D, SIG_ROT, SIG_UV, STRIDE, T
from test_landmark_cpu import INTR, P, _scene

HUBER, MIN_PIVOT = 3.0, 1e-8
FRAME = 5  # the frame of the scene the single-frame tests pose (25 degrees from the identity)
FAR = 100.0  # a pivot that decides a state lies at least this factor from min_pivot * max(diag H)


def _angle(a, b):
    """The angle of the rotation between the unit quaternions a and b, radians (fuse_numpy.rot_angle is the
    angle between the quaternions themselves, half of this)."""
    return 2.0 * fn.rot_angle(a, b)


def _perturbed(q, t, deg, frac, seed=0):
    """The pose (q, t) turned by `deg` degrees about a random axis (on the left) and moved by frac |t|."""
    rng = np.random.default_rng(seed)
    dq = ln.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(deg))
    d = rng.normal(size=3)
    return fn.unit_pos(fn.qmul(dq, q)), t + frac * np.linalg.norm(t) * d / np.linalg.norm(d)


def _frame(inverse, frame=FRAME):
    X, q, t, px = _scene(inverse)
    return X, q[frame], t[frame], px[frame]


def _solve(px, X, q0, t0, inverse=0, state=None, weights=None, huber=HUBER, iters=4, min_pts=6, trace=None):
    state = np.ones(len(X), np.int32) if state is None else state
    return pn.solve_frame(px, weights, X, state, q0, t0, INTR, huber, iters, min_pts, MIN_PIVOT, inverse, trace)


def _margins(trace):
    """min over the iterations of min(pivot) / (min_pivot * max(diag H)): how far the smallest pivot of a
    solved step lies above the bound."""
    return min(min(it["pivots"]) / (MIN_PIVOT * it["diag"]) for it in trace)


@pytest.mark.parametrize("inverse", [0, 1])
def test_exact_projections_recover_the_pose(inverse):
    X, q, t, px = _frame(inverse)
    q0, t0 = _perturbed(q, t, 2.0, 0.02)
    assert _angle(q0, q) > 0.03 and np.linalg.norm(t0 - t) > 0.1
    trace = []
    out = _solve(px, X, q0, t0, inverse, iters=8, trace=trace)
    assert out["state"] == pn.SOLVED and out["n_in"] == P
    bound_t = 1e-9 * (1.0 + np.linalg.norm(t))
    rot, tr = _angle(out["q"], q), np.linalg.norm(out["t"] - t)
    met = [k + 1 for k, it in enumerate(trace) if _angle(it["q"], q) <= 1e-9 and np.linalg.norm(it["t"] - t) <= bound_t]
    print(f"inverse={inverse}: rotation error {rot:.3e} rad, |t - t_true| {tr:.3e}, rms {out['rms_px']:.3e} px, bound "
          f"first met after iteration {met[0] if met else None}, pivot margin {_margins(trace):.3e}")
    assert rot <= 1e-9 and tr <= bound_t
    assert out["rms_px"] <= 1e-6
    assert _margins(trace) >= FAR
    # the other convention on the same pixels is a different problem: it must not recover the pose
    other = _solve(px, X, q0, t0, 1 - inverse, iters=8)
    assert other["state"] != pn.SOLVED or _angle(other["q"], q) > 1e-3


def test_the_huber_weight_reduces_the_error_under_outliers():
    """20 % of the points moved by 50 px, sigma 0.5 px on the rest, seeds 0..49: the mean pose error with
    HUBER is below that with a threshold that never acts. Only the direction is asserted."""
    X, q, t, px = _frame(0)
    q0, t0 = _perturbed(q, t, 2.0, 0.02)
    err = {HUBER: [], 1e9: []}
    for seed in range(50):
        rng = np.random.default_rng(seed)
        noisy = px + rng.normal(0.0, 0.5, px.shape)
        bad = rng.permutation(P)[:P // 5]
        ang = rng.uniform(0.0, 2.0 * np.pi, len(bad))
        noisy[bad] = px[bad] + 50.0 * np.stack([np.cos(ang), np.sin(ang)], -1)
        for huber, sink in err.items():
            trace = []
            out = _solve(noisy, X, q0, t0, huber=huber, iters=8, trace=trace)
            assert out["state"] == pn.SOLVED and _margins(trace) >= FAR
            sink.append((_angle(out["q"], q), np.linalg.norm(out["t"] - t)))
    (hr, ht), (pr, pt) = np.mean(err[HUBER], 0), np.mean(err[1e9], 0)
    print(f"outliers: rotation huber {hr:.4e} rad plain {pr:.4e} rad ratio {hr / pr:.3f}; translation huber {ht:.4e} "
          f"plain {pt:.4e} ratio {ht / pt:.3f}")
    assert hr < pr and ht < pt


def _same_pose(out, q0, t0):
    return (out["R"].tobytes() == np.asarray(q0, np.float32).tobytes() and
            out["t"].tobytes() == np.asarray(t0, np.float64).tobytes() and out["n_in"] == 0 and np.isposinf(out["rms_px"]))


def test_states_and_skipped_points():
    X, q, t, px = _frame(0)
    q0, t0 = _perturbed(q, t, 2.0, 0.02)
    # fewer than min_pts valid landmarks
    state = np.zeros(P, np.int32)
    state[:5] = 1
    few = _solve(px, X, q0, t0, state=state)
    assert few["state"] == pn.FEW and _same_pose(few, q0, t0)
    state[5] = 1
    assert _solve(px, X, q0, t0, state=state)["state"] == pn.SOLVED
    # every landmark state but 1 is skipped
    for other in (0, 2, 3, -1):
        assert _solve(px, X, q0, t0, state=np.full(P, other, np.int32))["state"] == pn.FEW
    # collinear points: the rotation about their line is free
    line = np.outer(np.linspace(-1.0, 1.0, P), [0.6, -0.3, 0.2])
    lpx = ln.project(line, q, t, INTR)[0]
    trace = []
    col = _solve(lpx, line, q0, t0, trace=trace)
    assert col["state"] == pn.DEGENERATE and _same_pose(col, q0, t0)
    low = min(trace[-1]["pivots"]) / (MIN_PIVOT * trace[-1]["diag"])
    print(f"collinear: smallest pivot / bound {low:.3e}")
    assert low <= 1.0 / FAR
    # points behind the camera, pixels and weights that are not usable: skipped, the rest solves as if alone
    keep = np.arange(P) >= 10
    Xb, pxb, w = X.copy(), px.copy(), np.ones(P, np.float32)
    Xb[0:2] = X[0:2] + np.array(ln.rotation(q, 0)).T @ [0.0, 0.0, -20.0]  # 20 units back along the optical axis
    assert (ln.project(Xb[0:2], q0, t0, INTR)[1] < 0).all()
    pxb[2, 0], pxb[3, 1], pxb[4, 0] = np.nan, np.inf, -np.inf
    w[5], w[6], w[7], w[8], w[9] = 0.0, -1.0, np.nan, np.inf, -0.0
    a = _solve(pxb, Xb, q0, t0, weights=w)
    b = _solve(px[keep], X[keep], q0, t0, weights=np.ones(keep.sum(), np.float32))
    assert a["state"] == b["state"] == pn.SOLVED and a["n_in"] == b["n_in"] == P - 10
    assert a["q"].tobytes() == b["q"].tobytes() and a["t"].tobytes() == b["t"].tobytes() and a["rms_px"] == b["rms_px"]
    # a start pose that is not finite
    for bad_q, bad_t in ((np.array([np.nan, 0, 0, 0]), t0), (q0, np.array([0.0, np.inf, 6.0])), (np.zeros(4), t0)):
        out = _solve(px, X, bad_q, bad_t)
        assert out["state"] == pn.NONFINITE and out["n_in"] == 0 and np.isposinf(out["rms_px"])
        assert out["R"].tobytes() == bad_q.astype(np.float32).tobytes() and out["t"].tobytes() == bad_t.tobytes()
    # a landmark that is not finite poisons nothing: NaN is not in front of the camera, so it is skipped
    Xn = X.copy()
    Xn[0] = np.nan
    assert _solve(px, Xn, q0, t0)["n_in"] == P - 1
    # an infinite landmark in front of the camera gives sums that are not finite
    Xn[0] = (0.0, 0.0, np.inf)
    inf = _solve(px, Xn, q0, t0)
    assert inf["state"] == pn.NONFINITE and _same_pose(inf, q0, t0)


def _rows(rows):
    rng = np.random.default_rng(3)
    acc = np.zeros((rows, fn.ROW))
    for r in acc:
        fn.add_hypothesis(r, 1.0, fn.unit_pos(rng.normal(size=4)), rng.normal(size=3) + [60.0, 60.0, 6.0])
    return acc


@pytest.mark.parametrize("s", [1, 2])
def test_injection_adds_one_hypothesis_to_the_rows_that_stay(s):
    Tw = 4
    X, q, t, px = _scene(0)
    state = np.ones((1, P), np.int32)
    q0, t0 = zip(*[_perturbed(q[f], t[f], 1.0, 0.01, seed=f) for f in range(Tw)])
    q0, t0 = np.array(q0, np.float32)[None], np.array(t0)[None]
    tracks = px[:Tw][None].astype(np.float32)
    tracks[0, 3, 5:] = np.nan  # position 3 has too few points: state 0, nothing is added
    acc = _rows(9)
    before = acc.copy()
    slots = [7, 2, 5, 0]
    fintr = (268.4, 268.4, 320.0, 240.0)
    kw = dict(tracks=tracks, X=X[None], state=state, R0=q0, T0=t0, intr=np.array([INTR]), s=s, huber_px=HUBER)
    out = pn.pnp(fuse_acc=acc, slots=slots, inject_w=0.75, fuse_intr=fintr, **kw)
    assert list(out["state"][0]) == [1, 1, 1, 0]
    for i, slot in enumerate(slots):
        want = before[slot].copy()
        if i >= s and out["state"][0, i] == 1:
            tx, ty, tz = out["t"][0, i]
            fn.add_hypothesis(want, 0.75, out["q"][0, i], np.array([320.0 + 268.4 * tx / tz, 240.0 + 268.4 * ty / tz, tz]))
            assert want[17] == before[slot, 17] + 1 and want[0] == before[slot, 0] + 0.75
        assert acc[slot].tobytes() == want.tobytes(), (i, slot)
    rest = [r for r in range(9) if r not in slots]
    assert acc[rest].tobytes() == before[rest].tobytes()
    # no accumulator, or a weight of zero: nothing is written and the poses are the same
    for kw2 in (dict(), dict(fuse_acc=acc, slots=slots, inject_w=0.0, fuse_intr=fintr)):
        keep = acc.copy()
        again = pn.pnp(**kw, **kw2)
        assert acc.tobytes() == keep.tobytes() and again["q"].tobytes() == out["q"].tobytes()


# ---- drift with the feedback ---------------------------------------------------------------------
SEEDS = 50
FINTR = (268.44444444, 268.44444444, 320.0, 240.0)  # test_fuse_cpu's: the fuser's and the tracks' pixels


def _pose_T(x):
    return np.array([(x[0] - FINTR[2]) * x[2] / FINTR[0], (x[1] - FINTR[3]) * x[2] / FINTR[1], x[2]])


def _drift(seed, weight, margins=None):
    """The scenario of test_fuse_cpu._drift with a 40-point body seen at sigma 0.5 px: FuseRef, the
    landmark restatement and the PnP restatement chained per hop -> (RMS rotation error, RMS (u, v, z)
    error) of the final fused poses."""
    rng = np.random.default_rng(seed)
    frames = HOPS + T - 1
    q, x = fn.truth(rng, frames)
    anchor = np.concatenate([q[0], x[0]])
    ref = fn.FuseRef(T, RATIO, FINTR)
    encs = [fn.window_encoding(rng, q, x, k, T, RATIO, SIG_ROT, SIG_UV, SIG_D) for k in range(HOPS)]
    body = rng.uniform(-1.0, 1.0, (P, 3))
    px = np.stack([ln.project(body, q[f], _pose_T(x[f]), FINTR)[0] for f in range(frames)])
    px = (px + rng.normal(0.0, 0.5, px.shape)).astype(np.float32)
    acc, acc_id = ln.new_state(1, P)
    ids = np.arange(P, dtype=np.int32)[None]
    intr = np.array([FINTR])
    er, ex = [], []
    for k in range(HOPS):
        slots = [(k + i) % T for i in range(T)]
        out = ref.fuse(encs[k][None], slots, [1 if k == 0 else T - STRIDE], [int(k == 0)], [anchor])
        fq, fu, _, _ = fn.fused(ref.acc[slots[0]])  # position 0 is final (stride 1)
        er.append(fn.rot_angle(fq, q[k]))
        ex.append(np.linalg.norm(fu - x[k]))
        if k == HOPS - 1:
            for i in range(1, T):
                er.append(fn.rot_angle(out["R"][0, i].astype(np.float64), q[k + i]))
                ex.append(np.linalg.norm(out["uvz"][0, i] - x[k + i]))
        if weight > 0.0:
            tr = px[k:k + T][None]
            lo = ln.update(tr, out["R"], out["T"], ids, (-1 - ids) if k == 0 else ids, [0], intr, acc, acc_id, STRIDE)
            trace = {} if margins is not None else None
            po = pn.pnp(tr, lo["X"], lo["state"], out["R"], out["T"], intr, STRIDE, HUBER, fuse_acc=ref.acc, slots=slots,
                        inject_w=weight, fuse_intr=FINTR, trace=trace)
            if margins is not None:
                margins += [_margins(tr_) for (h, i), tr_ in trace.items() if po["state"][h, i] == 1]
    rms = lambda v: math.sqrt(float(np.mean(np.square(v))))  # noqa: E731
    return rms(er), rms(ex)


def test_drift_with_and_without_the_feedback():
    """pnp_weight = 1 against 0, seeds 0..49: the mean RMS rotation and (u, v, z) drift of the final fused
    poses. The (u, v, z) drift falls and its direction is asserted. The rotation drift does NOT fall in this
    scenario: a finding about the design, not a tolerance to loosen, so the rotation figures are printed,
    not asserted, and pnp_weight stays 0 by default. The measured figures are in DESIGN.md "PnP refinement"."""
    margins = []
    on = np.array([_drift(seed, 1.0, margins) for seed in range(SEEDS)])
    off = np.array([_drift(seed, 0.0) for seed in range(SEEDS)])
    (nr, nx), (fr, fx) = on.mean(0), off.mean(0)
    better = ((on[:, 0] < off[:, 0]).sum(), (on[:, 1] < off[:, 1]).sum())
    print(f"drift, T={T} stride={STRIDE} hops={HOPS} seeds={SEEDS}: rotation with feedback {nr:.4e} rad without {fr:.4e} "
          f"rad ratio {nr / fr:.3f} (better on {better[0]} seeds); (u, v, z) with {nx:.4e} without {fx:.4e} ratio "
          f"{nx / fx:.3f} (better on {better[1]} seeds); smallest pivot margin {min(margins):.3e} over {len(margins)} solves")
    assert min(margins) >= FAR
    assert np.isfinite(on).all() and np.isfinite(off).all()
    assert nx < fx, f"(u, v, z): with the feedback {nx:.4e} >= without {fx:.4e}"


# ---- host logic ------------------------------------------------------------------------------------
def test_pnp_needs_landmarks_and_a_huber_threshold():
    from comet_amd.stream import PoseStream, StreamPool
    intr = (100.0, 100.0, 64.0, 64.0)
    anchor = ([1.0, 0, 0, 0], [64.0, 64.0, 5.0], 1.0, 1.0, "YT")
    base = dict(window=4, stride=1, anchor=anchor, fuse=True, carry=True, carry_tracks=8, carry_min_score=0.5,
                candidate_fn=lambda frame: None)
    lm = dict(landmarks=True, track_intr=intr)
    with pytest.raises(ValueError, match="pnp=True needs landmarks=True"):
        PoseStream(None, pnp=True, pnp_huber_px=3.0, **base)
    with pytest.raises(ValueError, match="pnp=True needs pnp_huber_px"):
        PoseStream(None, pnp=True, **base, **lm)
    for bad in (dict(pnp_huber_px=0.0), dict(pnp_huber_px=float("inf")), dict(pnp_huber_px=float("nan")),
                dict(pnp_huber_px=3.0, pnp_iters=0), dict(pnp_huber_px=3.0, pnp_iters=17),
                dict(pnp_huber_px=3.0, pnp_min_pts=3), dict(pnp_huber_px=3.0, pnp_weight=-1.0),
                dict(pnp_huber_px=3.0, pnp_weight=float("nan"))):
        with pytest.raises(ValueError, match="pnp"):
            PoseStream(None, pnp=True, **bad, **base, **lm)
    ok = PoseStream(None, pnp=True, pnp_huber_px=3, **base, **lm)
    assert ok.pnp and ok._pnp == dict(iters=4, huber_px=3.0, min_pts=6, weight=0.0)
    off = PoseStream(None, pnp_huber_px=0.0, pnp_iters=99, **base, **lm)  # off: the other keywords are not looked at
    assert not off.pnp and off._pnp is None
    pool = dict(base, streams=2, anchors=[anchor, anchor])
    del pool["anchor"]
    with pytest.raises(ValueError, match="pnp=True needs landmarks=True"):
        StreamPool(None, pnp=True, pnp_huber_px=3.0, **pool)
    with pytest.raises(ValueError, match="pnp=True needs pnp_huber_px"):
        StreamPool(None, pnp=True, landmarks=True, track_intrs=[intr, intr], **pool)
    ok = StreamPool(None, pnp=True, pnp_huber_px=2.5, pnp_iters=2, pnp_min_pts=8, pnp_weight=0.5, landmarks=True,
                    track_intrs=[intr, intr], **pool)
    assert ok._pnp == dict(iters=2, huber_px=2.5, min_pts=8, weight=0.5)


def test_landmark_map_pnp_checks_its_hops_before_anything_is_launched():
    from comet_amd.ops import LandmarkOut
    from comet_amd.stream import LandmarkMap
    intr = (100.0, 100.0, 64.0, 64.0)
    lm = LandmarkMap(window=4, stride=1, streams=2, tracks=8, intrs=[intr, intr])
    lo = LandmarkOut(torch.zeros(2, 8, 3, dtype=torch.float64), torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 8),
                     torch.zeros(2, 8, dtype=torch.int32))
    tr, R, Tx = torch.zeros(2, 4, 8, 2), torch.zeros(2, 4, 4), torch.zeros(2, 4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="one hop per stream"):
        lm.pnp([0, 0], tr, R, Tx, lo, huber_px=3.0)
    with pytest.raises(ValueError, match="unknown stream"):
        lm.pnp([0, 2], tr, R, Tx, lo, huber_px=3.0)
    with pytest.raises(ValueError, match="huber_px"):
        lm.pnp([0, 1], tr, R, Tx, lo)
    with pytest.raises(ValueError, match="LandmarkOut of the same"):
        lm.pnp([0], tr[:1], R[:1], Tx[:1], lo, huber_px=3.0)


def test_result_keeps_its_twelve_positions_with_the_pnp_fields():
    from comet_amd.ops import PnpOut
    from comet_amd.stream import StreamResult
    r = StreamResult(0, torch.zeros(4, 7), None, None)
    assert len(r) == 12 and all(getattr(r, k) is None for k in ("pnp_R", "pnp_T", "pnp_inliers", "pnp_rms_px", "pnp_state"))
    po = PnpOut(torch.zeros(2, 4, 4, dtype=torch.float64), torch.ones(2, 4, 4), torch.zeros(2, 4, 3, dtype=torch.float64),
                torch.full((2, 4), 7, dtype=torch.int32), torch.zeros(2, 4), torch.ones(2, 4, dtype=torch.int32))
    r2 = r.with_tracks(torch.zeros(3), None, None).with_pnp(po, 1)._replace(final=1)
    assert len(r2) == 12 and r2.final == 1 and r2.track_ids is not None
    assert r2.pnp_R.shape == (4, 4) and r2.pnp_T.dtype == torch.float64 and r2.pnp_inliers.tolist() == [7] * 4
    assert r2.pnp_rms_px.shape == (4,) and r2.pnp_state.tolist() == [1] * 4
    assert r.pnp_R is None
    fields = list(StreamResult.__annotations__)
    assert fields[-5:] == ["pnp_R", "pnp_T", "pnp_inliers", "pnp_rms_px", "pnp_state"], "appended after the existing ones"


def test_config_plumbing_of_cfg_stream_pnp():
    from comet_amd import loop
    lm = dict(landmarks=True)
    assert loop._stream_pnp({}, lm) == {}
    assert loop._stream_pnp({"stream": {"pnp": False, "pnp_huber_px": 3}}, {}) == {}
    assert loop._stream_pnp({"stream": {"pnp": True, "pnp_huber_px": 3}}, lm) == dict(
        pnp=True, pnp_iters=4, pnp_huber_px=3.0, pnp_min_pts=6, pnp_weight=0.0)
    full = {"stream": {"pnp": True, "pnp_iters": 2, "pnp_huber_px": 2.5, "pnp_min_pts": 9, "pnp_weight": 1}}
    kw = loop._stream_pnp(full, lm)
    assert kw == dict(pnp=True, pnp_iters=2, pnp_huber_px=2.5, pnp_min_pts=9, pnp_weight=1.0)
    assert isinstance(kw["pnp_weight"], float) and isinstance(kw["pnp_huber_px"], float)
    with pytest.raises(ValueError, match="cfg.stream.pnp needs cfg.stream.landmarks"):
        loop._stream_pnp(full, {})
    with pytest.raises(ValueError, match="cfg.stream.pnp needs cfg.stream.pnp_huber_px"):
        loop._stream_pnp({"stream": {"pnp": True}}, lm)
    # the keywords are the constructor's own
    from comet_amd.stream import PoseStream
    anchor = ([1.0, 0, 0, 0], [64.0, 64.0, 5.0], 1.0, 1.0, "AMD")
    st = PoseStream(None, window=4, stride=1, anchor=anchor, fuse=True, carry=True, carry_tracks=8, carry_min_score=0.5,
                    candidate_fn=lambda f: None, landmarks=True, track_intr=(100.0, 100.0, 64.0, 64.0), **kw)
    assert st._pnp == dict(iters=2, huber_px=2.5, min_pts=9, weight=1.0)


def test_pnp_csv_holds_one_row_per_hop_for_position_stride(tmp_path):
    import csv
    from comet_amd import loop
    from comet_amd.ops import PnpOut
    from comet_amd.stream import StreamResult
    path = str(tmp_path / "seq.csv")
    assert loop.pnp_csv(path) == str(tmp_path / "seq_pnp.csv")
    logger = loop.CsvLogger(loop.pnp_csv(path), loop.PNP_FIELDS)
    Tw = 4
    po = PnpOut(torch.zeros(1, Tw, 4, dtype=torch.float64), torch.arange(Tw * 4, dtype=torch.float32).view(1, Tw, 4) / 3,
                torch.arange(Tw * 3, dtype=torch.float64).view(1, Tw, 3) / 7,
                torch.tensor([[5, 6, 7, 8]], dtype=torch.int32), torch.tensor([[0.5, 1.5, float("inf"), 3.5]]),
                torch.tensor([[1, 1, 0, 2]], dtype=torch.int32))
    r = StreamResult(10, torch.zeros(Tw, 7), None, None).with_pnp(po, 0)
    loop._log_pnp(logger, 0, r, 1)
    loop._log_pnp(logger, 1, r._replace(frame_index=11), 2)
    rows = list(csv.DictReader(open(loop.pnp_csv(path))))
    assert tuple(rows[0].keys()) == loop.PNP_FIELDS == ("hop", "frame", "state", "inliers", "rms_px", "qw", "qx", "qy",
                                                        "qz", "tx", "ty", "tz")
    assert [int(rows[0][k]) for k in ("hop", "frame", "state", "inliers")] == [0, 11, 1, 6]
    assert [int(rows[1][k]) for k in ("hop", "frame", "state", "inliers")] == [1, 13, 0, 7]
    assert float(rows[0]["rms_px"]) == 1.5 and math.isinf(float(rows[1]["rms_px"]))
    # (floats are written so that they read back exactly)
    assert [float(rows[0][k]) for k in ("qw", "qx", "qy", "qz")] == po.R[0, 1].double().tolist()
    assert [float(rows[1][k]) for k in ("tx", "ty", "tz")] == po.T[0, 2].tolist()
