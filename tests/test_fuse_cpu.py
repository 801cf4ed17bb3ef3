"""Pose fusion without a GPU (DESIGN.md "Pose fusion"): the host-only FuseSchedule, the sanity of the
numpy restatement tests/fuse_numpy.py, and the drift property the feature exists for, shown on the
restatement.

Drift property: T = 8, stride 1, 40 hops, a synthetic ground-truth trajectory of 3-D rotations and
(u, v, z), iid noise on every window's relative encodings (a random rotation of N(0, 0.02 rad) about
a random axis; N(0, 0.02) on the two pixel entries and N(0, 0.005) on the depth entry, ratio 0.5),
seeds 0 .. 199. Required: the mean over the seeds of the RMS error of the fused final poses is at
most 0.5 x that of single-estimate chaining, for the rotation angle and for (u, v, z) separately.
0.5 is a condition with margin, not a measurement: a 1-D additive model of the chaining gives 0.20
at this window and stride. The noise level was fixed after confirming that the restatement stays
within the bound; it enters both sides alike, so the ratio does not depend on it to first order.
Measured ratios: DESIGN.md "Pose fusion"."""
import math

import numpy as np
import pytest

import fuse_numpy as fn

INTR = (268.44444444, 268.44444444, 320.0, 240.0)


# ------------------------------------------------------------------------------------------------
# FuseSchedule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,stride,cap", [(4, 1, 4), (4, 3, 6), (5, 2, 7)])
def test_schedule_against_a_record_of_the_frames_seen(T, stride, cap):
    """Over 3 x capacity frames (a reset after 2 x capacity): a hop's first flag is set exactly for
    the first hop since the reset; positions >= fresh_from are exactly the frames no earlier hop of
    the run has seen; the first `final` positions are exactly the frames no later hop sees."""
    from comet_amd.stream import FuseSchedule, RingSchedule
    ring, sched = RingSchedule(T, stride, cap), FuseSchedule(T, stride)
    assert sched.final == stride
    runs, hops = [[]], 0
    for f in range(3 * cap):
        if f == 2 * cap:
            ring.reset()
            sched.reset()
            runs.append([])
        _, hop = ring.push()
        if hop is None:
            continue
        assert sched.is_first() == (not runs[-1])
        first, fresh = sched.hop()
        assert first == (not runs[-1]) and not sched.is_first()
        seen = {g for w in runs[-1] for g in w}
        window = list(range(hop.frame_index, hop.frame_index + T))
        assert fresh == (1 if first else T - stride)
        assert [i for i in range(1, T) if window[i] not in seen] == list(range(fresh, T))
        assert first or window[0] in seen
        runs[-1].append(window)
        hops += 1
    assert hops >= 3 and all(len(r) >= 1 for r in runs)
    for run in runs:
        for k, w in enumerate(run[:-1]):
            later = {g for v in run[k + 1:] for g in v}
            assert [i for i in range(T) if w[i] not in later] == list(range(sched.final))


def test_schedule_resets_one_stream_of_a_pool():
    from comet_amd.stream import FuseSchedule
    sched = FuseSchedule(4, 1, streams=3)
    assert [sched.hop(s) for s in range(3)] == [(True, 1)] * 3
    assert [sched.hop(s) for s in range(3)] == [(False, 3)] * 3
    sched.reset(1)
    assert [sched.is_first(s) for s in range(3)] == [False, True, False]
    assert [sched.hop(s) for s in (0, 1)] == [(False, 3), (True, 1)]
    assert sched.hop(1) == (False, 3) and sched.is_first(2) is False
    sched.reset()
    assert all(sched.is_first(s) for s in range(3))
    with pytest.raises(ValueError):
        sched.hop(3)


@pytest.mark.parametrize("window,stride", [(4, 4), (4, 5), (2, 2), (4, 0)])
def test_schedule_rejects_strides_outside_1_to_window(window, stride):
    from comet_amd.stream import FuseSchedule
    with pytest.raises(ValueError):
        FuseSchedule(window, stride)


def test_fuse_needs_an_anchor_and_an_overlap():
    from comet_amd.stream import PoseStream, StreamPool
    anchor = ([1.0, 0.0, 0.0, 0.0], [320.0, 240.0, 10.0], 268.4, 0.5, "AMD")
    with pytest.raises(ValueError, match="anchor"):
        PoseStream(None, window=4, stride=1, fuse=True, precision="f32")
    with pytest.raises(ValueError, match="anchor"):
        StreamPool(None, streams=2, window=4, stride=1, fuse=True, precision="f32")
    for stride in (4, 6):
        with pytest.raises(ValueError, match="stride"):
            PoseStream(None, window=4, stride=stride, anchor=anchor, fuse=True, precision="f32")
        with pytest.raises(ValueError, match="stride"):
            StreamPool(None, streams=2, window=4, stride=stride, anchors=[anchor, anchor], fuse=True, precision="f32")
    with pytest.raises(ValueError, match="fuse_weight"):
        PoseStream(None, window=4, anchor=anchor, fuse=True, fuse_weight="median", precision="f32")
    with pytest.raises(ValueError, match="one ratio"):
        StreamPool(None, streams=2, window=4, anchors=[anchor, anchor[:3] + (0.25, "AMD")], fuse=True, precision="f32")
    ok = PoseStream(None, window=4, stride=3, anchor=anchor, fuse=True, fuse_weight="score", precision="f32")
    assert ok.fuse and ok.fuse_weight == "score"
    assert PoseStream(None, window=4, precision="f32").fuse is False


def test_stream_result_keeps_its_positional_fields():
    from comet_amd.stream import StreamResult
    r = StreamResult(3, "enc", "tracks", "score", "R", "T")
    assert (r.frame_index, r.pred_pose_enc, r.pred_tracks, r.pred_score, r.R, r.T) == (3, "enc", "tracks", "score", "R", "T")
    assert r[6:] == (None,) * 6 and r._fields[6:] == ("fused_R", "fused_T", "fused_count", "rot_spread",
                                                       "trans_spread", "final")
    assert StreamResult(0, "enc", None, None)[4:] == (None,) * 8


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _one_hop(enc, anchor, weights=None, rows=8):
    ref = fn.FuseRef(rows, 0.5, INTR)
    T = enc.shape[0]
    return ref, ref.fuse(enc[None], list(range(T)), [1], [1], [anchor], None if weights is None else weights[None])


def test_one_hypothesis_gives_back_that_hypothesis():
    rng = np.random.default_rng(0)
    anchor = np.concatenate([fn.unit_pos(rng.normal(size=4)), [300.0, 250.0, 9.0]])
    enc = rng.normal(size=(4, 7)).astype(np.float32) * 0.3
    enc[:, 3:] = [fn.unit_pos(q) for q in rng.normal(size=(4, 4))]
    _, out = _one_hop(enc, anchor)
    assert np.array_equal(out["count"], [[1, 1, 1, 1]])
    assert np.abs(out["R"] - out["hyp_R"]).max() <= 2.0 ** -22
    assert np.abs(out["R"][0, 0] - anchor[:4]).max() <= 2.0 ** -22
    assert np.abs(out["T"] / out["hyp_T"] - 1.0).max() <= 1e-14
    assert np.array_equal(out["uvz"][0, 0], anchor[4:])
    for i in range(1, 4):
        q, x = fn.hypothesis(enc[i], anchor[:4], anchor[4:], 0.5)
        assert np.abs(out["hyp_R"][0, i] - q).max() <= 2.0 ** -23 and np.array_equal(out["uvz"][0, i], x)
    assert out["rot_spread"].max() <= 1e-7 and np.array_equal(out["trans_spread"], np.zeros((1, 4, 3), np.float32))


def test_q_and_minus_q_fuse_to_the_same_result():
    rng = np.random.default_rng(1)
    q, x = fn.unit_pos(rng.normal(size=4)), np.array([310.0, 200.0, 12.0])
    near = fn.unit_pos(fn.qmul(fn.axis_angle_quat([1.0, 2.0, 3.0], 0.1), q))
    rows = []
    for sign in (1.0, -1.0):
        row = np.zeros(fn.ROW)
        fn.add_hypothesis(row, 1.0, q, x)
        fn.add_hypothesis(row, 2.0, sign * near, x)
        rows.append(row)
    assert np.array_equal(rows[0], rows[1])
    fq, fu, lam, W = fn.fused(rows[1])
    assert fq[0] >= 0.0 and W == 3.0 and np.allclose(fu, x, rtol=1e-15)
    assert fn.rot_angle(fq, q) < 0.1 and fn.rot_angle(fq, near) < 0.1


@pytest.mark.parametrize("angles,symmetric", [
    ([0.1, 0.3, 0.8], False), ([-0.6, 0.2, 0.25, 0.7, 0.05], False), ([1.0, 1.4, 1.2, 0.9], False),
    ([0.2, 0.9], True), ([0.1, 0.4, 0.7], True), ([-0.55, -0.25, 0.05, 0.35, 0.65], True), ([0.3, 0.5, 1.1, 1.3], True)])
def test_coaxial_rotations_fuse_to_the_mean_angle(angles, symmetric):
    """K rotations about one axis by angles a_k, equal weights, spread below pi / 2. In the plane
    spanned by the base quaternion and axis (x) base the hypotheses are (cos a_k / 2, sin a_k / 2),
    and the principal axis of sum q q^T lies at half the angle atan2(sum sin a_k, sum cos a_k): the
    chordal mean of coaxial rotations is the circular mean of their angles, exactly. That is the
    arithmetic mean whenever the angles lie symmetrically about it (two angles; the last four sets);
    for the other sets it differs from it in second order of the spread (1e-3 rad at [0.1, 0.3, 0.8]),
    so those are held to the circular mean."""
    axis = np.array([0.3, -0.5, 0.8])
    base = fn.unit_pos([0.7, 0.1, -0.5, 0.4])
    row = np.zeros(fn.ROW)
    for a in angles:
        fn.add_hypothesis(row, 1.0, fn.unit_pos(fn.qmul(fn.axis_angle_quat(axis, a), base)), np.array([1.0, 2.0, 3.0]))
    fq, _, lam, W = fn.fused(row)
    mean = float(np.mean(angles))
    circular = math.atan2(sum(math.sin(a) for a in angles), sum(math.cos(a) for a in angles))
    want = fn.unit_pos(fn.qmul(fn.axis_angle_quat(axis, mean if symmetric else circular), base))
    assert np.abs(fq - want).max() <= 1e-14
    if symmetric:
        assert abs(circular - mean) <= 1e-15  # the two means coincide
    assert row[17] == len(angles) and W == len(angles)
    # the spread is the weighted RMS half-angle form: sin^2(spread / 2) = mean sin^2((a - fused angle) / 2)
    half = np.mean([math.sin(0.5 * (a - circular)) ** 2 for a in angles])
    assert abs(1.0 - lam / W - half) <= 1e-14


# ------------------------------------------------------------------------------------------------
# the drift property
# ------------------------------------------------------------------------------------------------
T, STRIDE, HOPS, SEEDS, RATIO = 8, 1, 40, 200, 0.5
SIG_ROT, SIG_UV, SIG_D = 0.02, 0.02, 0.005
BOUND = 0.5


def _drift(seed):
    """-> (RMS rotation error, RMS (u, v, z) error) of the final poses, fused and chained."""
    rng = np.random.default_rng(seed)
    frames = HOPS + T - 1
    q, x = fn.truth(rng, frames)
    anchor = np.concatenate([q[0], x[0]])
    ref = fn.FuseRef(T, RATIO, INTR)
    cq, cx = q[0], x[0]  # the chained reference
    err = {"fused": ([], []), "chained": ([], [])}
    for k in range(HOPS):
        enc = fn.window_encoding(rng, q, x, k, T, RATIO, SIG_ROT, SIG_UV, SIG_D)
        slots = [(k + i) % T for i in range(T)]
        last = k == HOPS - 1
        out = ref.fuse(enc[None], slots, [1 if k == 0 else T - STRIDE], [int(k == 0)], [anchor], want=last)
        fq, fu, _, _ = fn.fused(ref.acc[slots[0]])  # position 0 is final (stride 1)
        err["fused"][0].append(fn.rot_angle(fq, q[k]))
        err["fused"][1].append(np.linalg.norm(fu - x[k]))
        err["chained"][0].append(fn.rot_angle(cq, q[k]))
        err["chained"][1].append(np.linalg.norm(cx - x[k]))
        if last:  # the flush: the remaining frames of the last window
            for i in range(1, T):
                hq, hx = fn.hypothesis(enc[i], cq, cx, RATIO)
                err["fused"][0].append(fn.rot_angle(out["R"][0, i].astype(np.float64), q[k + i]))
                err["fused"][1].append(np.linalg.norm(out["uvz"][0, i] - x[k + i]))
                err["chained"][0].append(fn.rot_angle(hq, q[k + i]))
                err["chained"][1].append(np.linalg.norm(hx - x[k + i]))
        cq, cx = fn.chain_reference(enc[STRIDE], cq, cx, RATIO)
    rms = lambda v: math.sqrt(float(np.mean(np.square(v))))
    return [rms(err[a][b]) for a in ("fused", "chained") for b in (0, 1)]


def test_fusion_halves_the_drift_of_single_estimate_chaining():
    res = np.array([_drift(seed) for seed in range(SEEDS)])
    fr, fx, cr, cx = res.mean(0)
    better = ((res[:, 0] < res[:, 2]).sum(), (res[:, 1] < res[:, 3]).sum())
    print(f"drift, T={T} stride={STRIDE} hops={HOPS} seeds={SEEDS}: rotation fused {fr:.4e} rad chained {cr:.4e} rad "
          f"ratio {fr / cr:.3f} (better on {better[0]} seeds); (u, v, z) fused {fx:.4e} chained {cx:.4e} "
          f"ratio {fx / cx:.3f} (better on {better[1]} seeds)")
    assert fr <= BOUND * cr, f"rotation: fused {fr:.4e} > {BOUND} x chained {cr:.4e}"
    assert fx <= BOUND * cx, f"(u, v, z): fused {fx:.4e} > {BOUND} x chained {cx:.4e}"
