"""The motion estimate on the CPU: the float64 restatement of comet_motion_fit (tests/motion_numpy.py)
against known motions, its states and its ring, and the host logic of comet_amd.stream / comet_amd.loop
(no GPU needed)."""
import math

import numpy as np
import pytest
import torch

import motion_numpy as mn

AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])  # a skew axis
RATE = 0.05  # rad / frame
OMEGA = RATE * AXIS
VEL = np.array([0.01, -0.02, 0.03])
Q_START = mn.qexp(np.array([0.4, 0.2, -0.3]))
T_START = np.array([0.5, -0.25, 6.0])


def spin(frames, omega=OMEGA, vel=VEL, inverse=0, noise=None):
    """The poses of frames 0 .. frames - 1 of a body with R(f) = Exp(omega f) R(0), t(f) = t(0) + vel f, as the
    fuser would hand them over: q [frames, 4] f64 (conjugated when inverse: the kernel conjugates on load) and
    t [frames, 3]. noise [frames, 3]: a rotation vector applied on the left of every frame."""
    q = np.stack([mn.qmul(mn.qexp(omega * f), Q_START) for f in range(frames)])
    if noise is not None:
        q = np.stack([mn.qmul(mn.qexp(noise[f]), q[f]) for f in range(frames)])
    q = np.where(q[:, :1] < 0, -q, q)
    t = T_START + vel * np.arange(frames)[:, None]
    return (mn.qconj(q) if inverse else q), t


def run(q, t, T, s, hops, cap=16, weights=None, **kw):
    """Push `hops` windows of T frames, stride s, through one stream -> (the outputs of every hop, hist, hist_n).
    Window h holds frames [h s, h s + T)."""
    hist, hist_n = np.zeros((1, cap, 8)), np.zeros(1, np.int32)
    outs = []
    for h in range(hops):
        sl = slice(h * s, h * s + T)
        outs.append(mn.motion_fit(q[None, sl].astype(np.float32), t[None, sl], [int(h == 0)], [0], hist, hist_n, s,
                                  weights=None if weights is None else weights[None, sl].astype(np.float32),
                                  fit_len=kw.pop("fit_len", cap), **kw))
    return outs, hist, hist_n


def angle(qa, qb):
    return float(mn.qlog(mn.qmul(qa, mn.qconj(qb)))[1])


# ---- exact motion ----------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [0, 1])
def test_a_constant_spin_through_f32_poses_is_recovered_to_their_rounding(inverse):
    """|omega| = 0.05 rad / frame about a skew axis, constant velocity, m = 16, through the interface as the
    stream uses it: R arrives as f32 quaternions. Rounding a unit quaternion to f32 moves each component by
    at most 2^-25, the rotation by at most e = 2 sqrt(3) 2^-25 = 1.1e-7 rad. A line through 16 such errors
    has a slope error of at most e sum |tau - mean| / sum (tau - mean)^2 = e 64 / 340 = 2e-8 and an offset
    error of at most e (1 + 7.5 * 64 / 340) = 2.5e-7; the bounds below are those, rounded up. The
    translations are float64 and exact to the 1e-10 of the sibling tests."""
    T, s, hops = 5, 1, 16
    q, t = spin(hops + T, inverse=inverse)
    outs, _, hist_n = run(q, t, T, s, hops, horizon=0, inverse_rotation=inverse)
    o = outs[-1]
    assert o["state"][0] == 1 and o["n_used"][0] == 16 and hist_n[0] == 16
    q_body, _ = spin(hops + T)
    err_w, err_q = np.abs(o["omega"][0] - OMEGA).max(), angle(o["q0"][0], q_body[15])
    err_v, err_t = np.abs(o["vel"][0] - VEL).max(), np.abs(o["t0"][0] - t[15]).max()
    print(f"spin through f32 (inverse={inverse}): omega {err_w:.2e} q0 {err_q:.2e} rad vel {err_v:.2e} t0 {err_t:.2e}")
    assert err_v <= 1e-10 and err_t <= 1e-10 and err_w <= 3e-8 and err_q <= 3e-7
    for tau in range(1, 5):  # the window positions 1 .. 4 are the frames 16 .. 19
        assert angle(o["pred_q"][0, tau - 1], q[15 + tau]) <= 3e-7 + tau * 3e-8
        assert np.abs(o["pred_t"][0, tau - 1] - t[15 + tau]).max() <= 1e-10
    assert (o["innov_rot"][0] <= 5e-7).all() and (o["innov_trans"][0] <= 1e-6).all()


@pytest.mark.parametrize("inverse", [0, 1])
def test_a_constant_spin_in_float64_is_recovered_to_rounding(inverse):
    """The same motion with every row float64 (the history planted, the committed frame's quaternion a
    power-of-two one so that f32 holds it): omega, vel, q0, t0 and the predictions at tau = 1 .. 4 against
    the truth at the 1e-10 bound of the sibling tests; the measured error is printed (about 1e-15)."""
    T, s = 2, 1
    # rotate the start so that the newest committed frame (number 15) is the identity: exact in f32
    q_body = np.stack([mn.qexp(OMEGA * (f - 15)) for f in range(20)])
    q_body = np.where(q_body[:, :1] < 0, -q_body, q_body)
    t = T_START + VEL * np.arange(20)[:, None]
    hist, hist_n = np.zeros((1, 16, 8)), np.zeros(1, np.int32)
    for f in range(15):
        hist[0, f] = np.concatenate([q_body[f], t[f], [1.0]])  # (stored after the conjugation on load)
    hist_n[0] = 15
    ident = np.array([1.0, 0, 0, 0])
    q_in = mn.qconj(ident) if inverse else ident
    R = np.tile(q_in.astype(np.float32), (1, T, 1))
    Tx = t[None, 15:15 + T]
    o = mn.motion_fit(R, Tx, [0], [0], hist, hist_n, s, fit_len=16, horizon=3, inverse_rotation=inverse)
    assert o["state"][0] == 1 and o["n_used"][0] == 16 and o["pred_q"].shape == (1, 4, 4)
    errs = dict(omega=np.abs(o["omega"][0] - OMEGA).max(), vel=np.abs(o["vel"][0] - VEL).max(),
                q0=np.abs(o["q0"][0] - ident).max(), t0=np.abs(o["t0"][0] - t[15]).max())
    for tau in range(1, 5):
        truth = mn.qexp(OMEGA * tau)
        truth = mn.qconj(truth) if inverse else truth
        errs[f"pred_q{tau}"] = np.abs(o["pred_q"][0, tau - 1] - truth).max()
        errs[f"pred_t{tau}"] = np.abs(o["pred_t"][0, tau - 1] - (t[15] + VEL * tau)).max()
    print(f"exact spin in float64 (inverse={inverse}): max error {max(errs.values()):.2e}", errs)
    for name, e in errs.items():
        assert e <= 1e-10, (name, e)
    assert o["rot_rms"][0] <= 1e-10 and (o["trans_rms"][0] <= 1e-10).all()
    # the innovation on window position 1: the fused pose there is the identity again, one frame of spin away
    assert abs(float(o["innov_rot"][0, 0]) - RATE) <= 1e-6
    assert float(o["innov_trans"][0, 0]) <= 1e-6


def test_noise_is_averaged_down_by_the_line_fit():
    """Rotation-vector noise of sigma 0.02 rad per frame, m = 16, seeds 0 .. 49: the rms error of omega over
    that of the two-frame difference of the newest two poses is 1 / sqrt(680) = 0.038 in theory (var =
    sigma^2 / sum (tau - mean tau)^2 with sum = 16 * 255 / 12 = 340, against 2 sigma^2 for the difference)."""
    sigma, T, s, hops = 0.02, 2, 1, 16
    e_fit, e_diff = [], []
    for seed in range(50):
        rng = np.random.default_rng(seed)
        noise = rng.normal(0.0, sigma, (hops + T, 3))
        q, t = spin(hops + T, noise=noise)
        outs, _, _ = run(q, t, T, s, hops)
        o = outs[-1]
        assert o["state"][0] == 1 and o["n_used"][0] == 16
        e_fit.append(o["omega"][0] - OMEGA)
        q32 = q.astype(np.float32).astype(np.float64)
        diff = mn.qlog(mn.qmul(q32[15], mn.qconj(q32[14])))[0]
        e_diff.append(diff - OMEGA)
    rms_fit = float(np.sqrt(np.mean(np.square(e_fit))))
    rms_diff = float(np.sqrt(np.mean(np.square(e_diff))))
    ratio = rms_fit / rms_diff
    print(f"noise: rms omega error {rms_fit:.3e} rad/frame (fit) against {rms_diff:.3e} (two-frame difference), "
          f"ratio {ratio:.4f}, theory {1 / math.sqrt(680):.4f}")
    assert ratio < 0.1


# ---- states ----------------------------------------------------------------------------------------
def test_too_few_frames_give_state_0_and_the_newest_pose():
    q, t = spin(8)
    outs, hist, hist_n = run(q, t, 3, 1, 3, min_frames=3, horizon=2)
    for h, o in enumerate(outs[:2]):  # m = 1, m = 2
        assert o["state"][0] == 0 and o["n_used"][0] == h + 1
        q32 = q[h].astype(np.float32).astype(np.float64)
        assert (o["q0"][0] == q32).all() and (o["t0"][0] == t[h]).all(), "the newest committed pose bit for bit"
        assert (o["omega"][0] == 0).all() and (o["vel"][0] == 0).all()
        assert np.isposinf(o["rot_rms"][0]) and np.isposinf(o["trans_rms"][0]).all()
        assert np.isposinf(o["innov_rot"][0]).all() and np.isposinf(o["innov_trans"][0]).all()
        assert (o["pred_q"][0] == q32).all() and (o["pred_t"][0] == t[h]).all() and o["pred_q"].shape == (1, 4, 4)
    assert outs[2]["state"][0] == 1 and outs[2]["n_used"][0] == 3 and hist_n[0] == 3


def test_a_weightless_row_in_the_middle_keeps_the_time_axis():
    """Frame 5 of 10 has weight 0: it is stored (its age still counts) and skipped; the fit is exact."""
    q, t = spin(12)
    w = np.ones(12)
    w[5] = 0.0
    t = t.copy()
    t[5] += 100.0  # (would wreck the fit if it were used)
    outs, hist, _ = run(q, t, 2, 1, 10, weights=w)
    o = outs[-1]
    assert o["state"][0] == 1 and o["n_used"][0] == 9 and hist[0, 5, 7] == 0.0 and hist[0, 4, 7] == 1.0
    assert np.abs(o["vel"][0] - VEL).max() <= 1e-10 and np.abs(o["omega"][0] - OMEGA).max() <= 1e-7


def test_a_jump_beyond_max_angle_gives_state_3():
    q, t = spin(10)
    q = q.copy()
    jump = mn.qexp(2.5 * AXIS)
    for f in range(6, 10):
        q[f] = mn.qmul(jump, q[f])
    q = np.where(q[:, :1] < 0, -q, q)
    outs, _, _ = run(q, t, 2, 1, 8, max_angle=2.0)
    assert [int(o["state"][0]) for o in outs[:6]] == [0, 0, 1, 1, 1, 1]
    assert int(outs[6]["state"][0]) == 3 and outs[6]["n_used"][0] == 7
    assert (outs[6]["omega"][0] == 0).all() and np.isposinf(outs[6]["rot_rms"][0])
    # a wider bound takes the same poses
    outs, _, _ = run(q, t, 2, 1, 8, max_angle=3.0)
    assert int(outs[6]["state"][0]) == 1


def test_a_pose_that_is_not_finite_is_stored_weightless():
    q, t = spin(8)
    t = t.copy()
    t[3, 1] = np.nan
    w = np.ones(8)
    w[4], w[5] = -1.0, np.inf
    outs, hist, hist_n = run(q, t, 2, 1, 7, weights=w)
    assert hist_n[0] == 7 and hist[0, :7, 7].tolist() == [1, 1, 1, 0, 0, 0, 1]
    assert np.isnan(hist[0, 3, 5]), "stored as it came"
    assert outs[-1]["state"][0] == 1 and outs[-1]["n_used"][0] == 4
    assert np.abs(outs[-1]["vel"][0] - VEL).max() <= 1e-10
    # the hop that commits the bad frame reports it bit for bit as the newest pose only when it has no fit
    assert outs[3]["state"][0] == 1 and outs[3]["n_used"][0] == 3


def test_a_weight_sum_that_is_not_finite_gives_state_minus_1_and_a_vanishing_one_state_2():
    """The kernel stores finite weights > 0 or 0 only; the history is the caller's, and what it holds is summed
    as it is. Six planted rows, then one hop that commits frame 6."""
    q, t = spin(8)
    Tx = t[None, 6:8]

    def planted(w, R):
        hist, hist_n = np.zeros((1, 16, 8)), np.array([6], np.int32)
        for f in range(6):
            hist[0, f] = np.concatenate([q[f], t[f], [w[f]]])
        return mn.motion_fit(R, Tx, [0], [0], hist, hist_n, 1)

    R = q[None, 6:8].astype(np.float32)
    nan_row = planted([1, 1, np.nan, 1, 1, 1], R)
    assert nan_row["state"][0] == -1 and nan_row["n_used"][0] == 7
    overflow = planted([1e308] * 6, R)  # Sw = inf
    assert overflow["state"][0] == -1
    # weights whose products underflow (the committed frame is not finite, so its weight is 0): D = 0 - 0
    vanishing = planted([1e-170] * 6, np.full((1, 2, 4), np.nan, np.float32))
    assert vanishing["state"][0] == 2 and vanishing["n_used"][0] == 6
    for o in (nan_row, overflow, vanishing):
        assert (o["omega"][0] == 0).all() and (o["vel"][0] == 0).all() and np.isposinf(o["trans_rms"][0]).all()
        assert np.isposinf(o["innov_rot"][0]).all() and (o["t0"][0] == t[6]).all()


def test_first_clears_the_history():
    q, t = spin(12)
    hist, hist_n = np.zeros((1, 16, 8)), np.zeros(1, np.int32)
    for h in range(5):
        mn.motion_fit(q[None, h:h + 2].astype(np.float32), t[None, h:h + 2], [int(h == 0)], [0], hist, hist_n, 1)
    assert hist_n[0] == 5
    o = mn.motion_fit(q[None, 9:11].astype(np.float32), t[None, 9:11], [1], [0], hist, hist_n, 1)
    assert hist_n[0] == 1 and o["state"][0] == 0 and o["n_used"][0] == 1
    assert (hist[0, 0, 4:7] == t[9]).all() and (hist[0, 1, 4:7] == t[1]).all(), "row 0 rewritten, the rest left"


def test_the_ring_wraps_around():
    """70 frames with cap 64: the fit spans the newest 64, in age order across the wrap."""
    q, t = spin(72, omega=0.01 * AXIS)
    outs, hist, hist_n = run(q, t, 2, 1, 70, cap=64, max_angle=2.0)
    o = outs[-1]
    assert hist_n[0] == 70 and o["state"][0] == 1 and o["n_used"][0] == 64
    assert (hist[0, 5, 4:7] == t[69]).all() and (hist[0, 6, 4:7] == t[6]).all()
    assert np.abs(o["vel"][0] - VEL).max() <= 1e-10 and np.abs(o["t0"][0] - t[69]).max() <= 1e-10
    assert np.abs(o["omega"][0] - 0.01 * AXIS).max() <= 1e-8
    # a stride that wraps inside one append, and more frames than the ring holds
    hist, hist_n = np.zeros((1, 4, 8)), np.array([3], np.int32)
    mn.motion_fit(q[None, :8].astype(np.float32), t[None, :8], [0], [0], hist, hist_n, 6, fit_len=4)
    assert hist_n[0] == 9 and [hist[0, r, 4:7].tolist() for r in range(4)] == [t[f].tolist() for f in (5, 2, 3, 4)]


def test_the_count_saturates_without_losing_the_row():
    q, t = spin(6)
    cap = 6
    c = mn.COUNT_FOLD - 1
    hist, hist_n = np.zeros((1, cap, 8)), np.array([c], np.int32)
    for f in range(cap):
        hist[0, f, 0], hist[0, f, 7] = 1.0, 1.0
    o = mn.motion_fit(q[None, :3].astype(np.float32), t[None, :3], [0], [0], hist, hist_n, 2, fit_len=cap)
    assert (hist[0, c % cap, 4:7] == t[0]).all() and (hist[0, (c + 1) % cap, 4:7] == t[1]).all()
    assert hist_n[0] == cap + (c + 2) % cap and hist_n[0] % cap == (c + 2) % cap and o["n_used"][0] == cap


def test_hops_grouped_into_one_call_equal_single_calls():
    q, t = spin(12)
    hist, hist_n = np.zeros((3, 8, 8)), np.zeros(3, np.int32)
    one, one_n = hist.copy(), hist_n.copy()
    R = np.stack([q[i:i + 4] for i in (0, 3, 5)]).astype(np.float32)
    Tx = np.stack([t[i:i + 4] for i in (0, 3, 5)])
    for rep in range(3):
        first = [int(rep == 0)] * 3
        o = mn.motion_fit(R, Tx, first, [2, 0, 1], hist, hist_n, 2, fit_len=8)
        for h, sid in enumerate([2, 0, 1]):
            o1 = mn.motion_fit(R[h:h + 1], Tx[h:h + 1], first[:1], [sid], one, one_n, 2, fit_len=8)
            for k in o:
                assert np.array_equal(o[k][h], o1[k][0], equal_nan=True), k
    assert np.array_equal(hist, one) and np.array_equal(hist_n, one_n)


# ---- host logic ------------------------------------------------------------------------------------
ANCHOR = ([1.0, 0, 0, 0], [64.0, 64.0, 5.0], 1.0, 1.0, "YT")


def test_motion_needs_fuse_and_sane_keywords():
    from comet_amd.stream import PoseStream, StreamPool
    with pytest.raises(ValueError, match="motion=True needs fuse=True"):
        PoseStream(None, window=4, stride=1, motion=True)
    with pytest.raises(ValueError, match="motion=True needs fuse=True"):
        PoseStream(None, window=4, stride=1, anchor=ANCHOR, motion=True)
    base = dict(window=4, stride=1, anchor=ANCHOR, fuse=True)
    for bad in (dict(motion_len=1), dict(motion_len=65), dict(motion_min_frames=1), dict(motion_min_frames=17),
                dict(motion_iters=0), dict(motion_iters=9), dict(motion_horizon=-1), dict(motion_horizon=65),
                dict(motion_max_angle=0.0), dict(motion_max_angle=math.pi), dict(motion_max_angle=float("nan")),
                dict(motion_inverse_rotation=2)):
        with pytest.raises(ValueError, match="motion_"):
            PoseStream(None, motion=True, **bad, **base)
    ok = PoseStream(None, motion=True, **base)
    assert ok.motion and ok.motion_tracker._kw == dict(fit_len=16, min_frames=3, iters=2, horizon=1, max_angle=2.0,
                                                       inverse_rotation=0)
    off = PoseStream(None, motion_len=999, **base)  # off: the other keywords are not looked at
    assert not off.motion and off.motion_tracker is None
    with pytest.raises(ValueError, match="motion=True needs fuse=True"):
        StreamPool(None, 2, 4, motion=True)
    pool = StreamPool(None, 2, 4, anchors=[ANCHOR, ANCHOR], fuse=True, motion=True, motion_len=8, motion_horizon=0)
    assert pool.motion_tracker.streams == 2 and pool.motion_tracker._kw["fit_len"] == 8


def test_motion_tracker_checks_its_hops_before_anything_is_launched():
    from comet_amd.ops import FuseOut
    from comet_amd.stream import Hop, MotionTracker
    with pytest.raises(ValueError, match="stride < window"):
        MotionTracker(window=4, stride=4)
    mt = MotionTracker(window=4, stride=2, streams=2)
    z = torch.zeros(2, 4)
    fo = FuseOut(torch.zeros(2, 4, 4), None, torch.zeros(2, 4, 3, dtype=torch.float64), z, z, z, z, z)
    with pytest.raises(ValueError, match="one hop per stream"):
        mt.update([(0, Hop(0, 0)), (0, Hop(2, 2))], fo)
    with pytest.raises(ValueError, match="unknown stream"):
        mt.update([(0, Hop(0, 0)), (2, Hop(0, 0))], fo)
    with pytest.raises(ValueError, match="need fused poses"):
        mt.update([(0, Hop(0, 0))], fo)
    # a stream's hops follow one another (the bookkeeping of a launch that went out, set by hand here)
    mt._first[1], mt._next[1] = False, 6
    with pytest.raises(ValueError, match="does not follow the last one"):
        mt.update([(0, Hop(0, 0)), (1, Hop(4, 0))], fo)
    mt.reset(1)
    assert mt._first == [True, True] and mt._next[1] is None


def test_result_keeps_its_twelve_positions_with_the_motion_fields():
    from comet_amd.ops import MotionOut
    from comet_amd.stream import StreamResult
    names = ("motion_omega", "motion_vel", "motion_q0", "motion_t0", "motion_rot_rms", "motion_trans_rms",
             "motion_frames", "motion_state", "motion_pred_R", "motion_pred_T", "motion_innov_rot", "motion_innov_trans")
    r = StreamResult(0, torch.zeros(4, 7), None, None)
    assert len(r) == 12 and all(getattr(r, k) is None for k in names)
    f64 = torch.float64
    mo = MotionOut(torch.ones(2, 3, dtype=f64), torch.zeros(2, 4, dtype=f64), torch.zeros(2, 3, dtype=f64),
                   torch.zeros(2, 3, dtype=f64), torch.zeros(2), torch.zeros(2, 3), torch.full((2,), 5, dtype=torch.int32),
                   torch.ones(2, dtype=torch.int32), torch.zeros(2, 4, 4, dtype=f64), torch.zeros(2, 4, 3, dtype=f64),
                   torch.zeros(2, 3), torch.zeros(2, 3))
    r2 = r.with_tracks(torch.zeros(3), None, None).with_motion(mo, 1)._replace(final=1)
    assert len(r2) == 12 and r2.final == 1 and r2.track_ids is not None
    assert all(getattr(r2, k) is not None for k in names) and r.motion_omega is None
    assert r2.motion_omega.tolist() == [1.0] * 3 and int(r2.motion_frames) == 5 and int(r2.motion_state) == 1
    assert r2.motion_pred_R.shape == (4, 4) and r2.motion_pred_T.shape == (4, 3) and r2.motion_innov_rot.shape == (3,)
    assert len(StreamResult._fields) == 12


def test_config_plumbing_and_the_motion_csv(tmp_path):
    import csv
    from comet_amd import loop
    from comet_amd.ops import MotionOut
    from comet_amd.stream import PoseStream, StreamResult
    assert loop._stream_motion({}, True) == {}
    assert loop._stream_motion({"stream": {"motion": False}}, False) == {}
    with pytest.raises(ValueError, match="cfg.stream.motion needs cfg.stream.fuse"):
        loop._stream_motion({"stream": {"motion": True}}, False)
    assert loop._stream_motion({"stream": {"motion": True}}, True) == dict(
        motion=True, motion_len=16, motion_min_frames=3, motion_iters=2, motion_horizon=1, motion_max_angle=2.0,
        motion_inverse_rotation=0)
    kw = loop._stream_motion({"stream": {"motion": True, "motion_len": 8, "motion_min_frames": 4, "motion_iters": 1,
                                         "motion_horizon": 0, "motion_max_angle": 1, "motion_inverse_rotation": 1}}, True)
    st = PoseStream(None, window=4, stride=1, anchor=ANCHOR, fuse=True, **kw)  # the keywords are the constructor's own
    assert st.motion_tracker._kw == dict(fit_len=8, min_frames=4, iters=1, horizon=0, max_angle=1.0, inverse_rotation=1)

    path = str(tmp_path / "seq.csv")
    assert loop.motion_csv(path) == str(tmp_path / "seq_motion.csv")
    logger = loop.CsvLogger(loop.motion_csv(path), loop.MOTION_FIELDS)
    f64 = torch.float64
    mo = MotionOut(torch.tensor([[0.1, 0.2, 0.3]], dtype=f64), torch.tensor([[1.0, 0, 0, 0]], dtype=f64),
                   torch.tensor([[1.0, 2, 3]], dtype=f64) / 7, torch.tensor([[4.0, 5, 6]], dtype=f64) / 3,
                   torch.tensor([0.5]), torch.tensor([[0.25, float("inf"), 1.0]]), torch.tensor([9], dtype=torch.int32),
                   torch.tensor([1], dtype=torch.int32), torch.zeros(1, 3, 4, dtype=f64), torch.zeros(1, 3, 3, dtype=f64),
                   torch.tensor([[0.125, 7.0]]), torch.tensor([[0.75, 8.0]]))
    r = StreamResult(10, torch.zeros(4, 7), None, None, final=2).with_motion(mo, 0)
    loop._log_motion(logger, 3, r)
    rows = list(csv.DictReader(open(loop.motion_csv(path))))
    assert tuple(rows[0].keys()) == loop.MOTION_FIELDS and len(rows) == 1
    assert [int(rows[0][k]) for k in ("hop", "frame", "state", "frames")] == [3, 11, 1, 9]
    assert [float(rows[0][k]) for k in ("wx", "wy", "wz")] == [0.1, 0.2, 0.3]
    assert [float(rows[0][k]) for k in ("vx", "vy", "vz")] == mo.vel[0].tolist()  # (floats read back exactly)
    assert [float(rows[0][k]) for k in ("tx", "ty", "tz")] == mo.t0[0].tolist()
    assert float(rows[0]["rot_rms"]) == 0.5 and math.isinf(float(rows[0]["trans_rms_y"]))
    assert float(rows[0]["innov_rot"]) == 0.125 and float(rows[0]["innov_trans"]) == 0.75
