"""The landmark map without a GPU: the float64 restatement tests/landmark_numpy.py of
comet_landmark_update on synthetic rigid-body scenes, data.crop_intrinsics, the lm_gate_px score edit
and the constructor checks of PoseStream / StreamPool (DESIGN.md "Landmarks").

The restatement takes any float dtype; here tracks and quaternions are float64, so "exact projections"
are exact to double rounding (the kernel's f32 tracks would round a pixel to ~1e-5 px)."""
import numpy as np
import pytest
import torch

import landmark_numpy as ln

INTR = (300.0, 310.0, 63.5, 60.0)
P, T, S, HOPS = 40, 4, 1, 12


def _scene(inverse, hops=HOPS, step_deg=5.0, still=False, seed=0):
    """A rigid body of P points 6 units in front of the camera that turns `step_deg` per frame about a
    tilted axis and drifts slowly -> X [P, 3], per frame quaternions [F, 4], translations [F, 3] and
    exact pixels [F, P, 2], F = hops + T - 1 frames."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (P, 3))
    frames = hops * S + T - S
    q = np.stack([ln.quat_from_axis_angle((0.3, 1.0, 0.2), 0.0 if still else np.deg2rad(step_deg) * f)
                  for f in range(frames)])
    t = np.stack([np.array([0.1, -0.05, 6.0]) + (0.0 if still else 0.01 * f) * np.array([1.0, 0.5, 2.0])
                  for f in range(frames)])
    px = np.stack([ln.project(X, q[f], t[f], INTR, inverse)[0] for f in range(frames)])
    return X, q, t, px


def _run(q, t, px, inverse, hops=HOPS, min_pivot=1e-8, min_obs=3):
    """Chain `hops` single-stream hops of window T, stride S over the frames; slot j carries point j
    from the second hop on (born on the first) -> the outputs of every hop."""
    acc, acc_id = ln.new_state(1, P)
    ids = np.arange(P, dtype=np.int32)[None]
    outs = []
    for k in range(hops):
        f0 = k * S
        src = (-1 - np.arange(P, dtype=np.int32))[None] if k == 0 else ids
        outs.append(ln.update(px[f0:f0 + T][None], q[f0:f0 + T][None], t[f0:f0 + T][None], ids, src, [0],
                              np.array([INTR]), acc, acc_id, S, inverse_rotation=inverse, min_obs=min_obs,
                              min_pivot=min_pivot))
    return outs


@pytest.mark.parametrize("inverse", [0, 1])
def test_exact_projections_recover_the_body_points(inverse):
    X, q, t, px = _scene(inverse)
    outs = _run(q, t, px, inverse)
    assert (outs[0]["state"] == ln.NONE).all() and (outs[1]["state"] == ln.NONE).all(), "fewer than min_obs frames"
    last = outs[-1]
    assert (last["state"] == ln.VALID).all() and (last["n_obs"] == HOPS * S).all()
    err = np.abs(last["X"][0] - X).max(-1)
    bound = 1e-9 * (1.0 + np.linalg.norm(X, axis=-1))
    print(f"inverse={inverse}: max |X - X_true| {err.max():.3e}, max err_px {last['err_px'].max():.3e}")
    assert (err <= bound).all(), (err.max(), bound.min())
    assert (last["err_px"] <= 1e-6).all()
    # the other convention on the same pixels is a different problem: it must not recover the points
    other = _run(q, t, px, 1 - inverse)[-1]
    assert not (np.abs(other["X"][0] - X).max(-1) <= bound).all()


def test_no_relative_motion_is_ill_conditioned_everywhere():
    X, q, t, px = _scene(0, still=True)
    for out in _run(q, t, px, 0)[2:]:
        assert (out["state"] == ln.ILL).all()
        assert (out["X"] == 0).all() and np.isposinf(out["err_px"]).all()
        d = out["pivots"][0]
        assert (d[:, 2] <= 1e-12 * d[:, 0]).all(), "the third pivot of a rank-2 system is a rounding residue"


def test_more_committed_frames_reduce_the_error_under_pixel_noise():
    """sigma = 0.5 px on every pixel, seeds 0..49: the mean point error after 12 committed frames is below
    that after 3, in the mean over the seeds (the ratio is printed, not fixed)."""
    X, q, t, px = _scene(0)
    e3, e12 = [], []
    for seed in range(50):
        noisy = px + np.random.default_rng(seed).normal(0.0, 0.5, px.shape)
        outs = _run(q, t, noisy, 0)
        for k, sink in ((2, e3), (HOPS - 1, e12)):
            assert (outs[k]["state"] == ln.VALID).all() and (outs[k]["n_obs"] == (k + 1) * S).all()
            sink.append(np.linalg.norm(outs[k]["X"][0] - X, axis=-1).mean())
    m3, m12 = float(np.mean(e3)), float(np.mean(e12))
    print(f"mean |X - X_true|: 3 frames {m3:.4f}, 12 frames {m12:.4f}, ratio {m12 / m3:.3f}")
    assert m12 < m3


def test_reset_rule_pads_births_and_id_mismatch():
    X, q, t, px = _scene(0, hops=4)
    acc, acc_id = ln.new_state(2, P)
    ids = np.arange(P, dtype=np.int32)[None]
    born = (-1 - np.arange(P, dtype=np.int32))[None]
    kw = dict(intr=np.array([INTR]), acc=acc, acc_id=acc_id, s=S, min_obs=2)
    win = lambda k: (px[k:k + T][None], q[k:k + T][None], t[k:k + T][None])  # noqa: E731
    ln.update(*win(0), ids, born, [1], **kw)
    assert (acc[:P] == 0).all() and (acc_id[:P] == -1).all(), "stream 1 writes rows [P, 2 P) only"
    assert (acc[P:, 10] == 1).all() and (acc_id[P:] == ids[0]).all()
    ids2, src2 = ids.copy(), ids.copy()
    ids2[0, 0] = -1                 # a pad
    src2[0, 1] = -1 - 3             # a birth into a slot that held a track
    ids2[0, 2] = 99                 # carried by src, but the row belongs to another id
    out = ln.update(*win(1), ids2, src2, [1], **kw)
    assert (acc[P + 0] == 0).all() and acc_id[P + 0] == -1 and out["state"][0, 0] == ln.NONE and out["n_obs"][0, 0] == 0
    assert acc[P + 1, 10] == 1 and acc[P + 2, 10] == 1 and acc_id[P + 2] == 99
    assert (acc[P + 3:, 10] == 2).all() and (out["n_obs"][0, 3:] == 2).all()
    assert (acc[:, 11] == 0).all()


def test_frames_that_are_not_finite_or_have_no_weight_add_nothing():
    X, q, t, px = _scene(0, hops=3)
    px = np.repeat(px[:T][None], 1, 0).copy()
    w = np.ones((1, T, P), np.float32)
    px[0, 0, 0, 0] = np.nan
    px[0, 0, 1, 1] = np.inf
    w[0, 0, 2], w[0, 0, 3], w[0, 0, 4] = 0.0, -1.0, np.nan
    acc, acc_id = ln.new_state(1, P)
    ids = np.arange(P, dtype=np.int32)[None]
    out = ln.update(px, q[:T][None], t[:T][None], ids, -1 - ids, [0], np.array([INTR]), acc, acc_id, 1, weights=w)
    assert (out["n_obs"][0, :5] == 0).all() and (acc[:5] == 0).all() and (out["n_obs"][0, 5:] == 1).all()
    assert np.isfinite(acc).all()


def test_crop_intrinsics_maps_full_image_projections_into_the_crop():
    from comet_amd.data import crop_intrinsics
    full = (268.44444444, 268.44444444, 320.0, 240.0)
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1, 1, (50, 3)) + np.array([0.0, 0.0, 5.0])
    for box, size in (((100, 37, 420, 357), 256), ((-20, -5, 300, 315), 128), ((8, 0, 168, 160), (128, 96))):
        x0, y0, x1, y1 = box
        ow, oh = (size, size) if isinstance(size, int) else size
        u = full[0] * pts[:, 0] / pts[:, 2] + full[2]
        v = full[1] * pts[:, 1] / pts[:, 2] + full[3]
        # x_full = x0 + (x_crop + 0.5) * bw / size - 0.5, solved for x_crop
        uc = (u + 0.5 - x0) * ow / (x1 - x0) - 0.5
        vc = (v + 0.5 - y0) * oh / (y1 - y0) - 0.5
        fx, fy, cx, cy = crop_intrinsics(full, box, size)
        assert np.abs(fx * pts[:, 0] / pts[:, 2] + cx - uc).max() <= 1e-12 * (1 + np.abs(uc).max())
        assert np.abs(fy * pts[:, 1] / pts[:, 2] + cy - vc).max() <= 1e-12 * (1 + np.abs(vc).max())
    # the identity crop changes nothing; the convention is the resampler's: the centre of crop pixel 0 of
    # a 2 x reduction lies between full pixels 0 and 1
    assert crop_intrinsics(full, (0, 0, 640, 480), (640, 480)) == full
    fx, _, cx, _ = crop_intrinsics((1.0, 1.0, 0.0, 0.0), (0, 0, 64, 64), 32)
    assert fx == 0.5 and cx == -0.25  # full x = 0.5 (between pixels 0 and 1) -> crop x = 0


def test_gate_edits_only_row_s_of_valid_slots_over_the_gate():
    from comet_amd.stream import gate_scores
    g = torch.Generator().manual_seed(0)
    n, Tw, N, s = 2, 4, 16, 2
    score = torch.rand(n, Tw, N, generator=g)
    state = torch.randint(-1, 4, (n, N), generator=g, dtype=torch.int32)
    err = torch.rand(n, N, generator=g) * 10
    err[state != 1] = float("inf")
    state[0, 0], err[0, 0] = 1, 9.0
    state[0, 1], err[0, 1] = 1, 1.0
    state[0, 2], err[0, 2] = 1, 5.0   # exactly the gate: kept (the test is err > gate)
    before = score.clone()
    out = gate_scores(score, state, err, s, 5.0)
    assert torch.equal(score, before), "the input is left as it is"
    over = (state == 1) & (err > 5.0)
    assert bool(over[0, 0]) and not bool(over[0, 1]) and not bool(over[0, 2]) and bool((state != 1).any())
    assert bool(torch.isneginf(out[:, s][over]).all()) and torch.equal(out[:, s][~over], score[:, s][~over])
    rows = [i for i in range(Tw) if i != s]
    assert torch.equal(out[:, rows], score[:, rows])


def test_landmarks_need_fuse_carry_and_intrinsics():
    from comet_amd.stream import LandmarkMap, PoseStream, StreamPool
    intr = (100.0, 100.0, 64.0, 64.0)
    anchor = ([1.0, 0, 0, 0], [64.0, 64.0, 5.0], 1.0, 1.0, "YT")
    cand = lambda frame: None  # noqa: E731
    base = dict(window=4, stride=1, landmarks=True)
    carry = dict(carry=True, carry_tracks=8, carry_min_score=0.5, candidate_fn=cand)
    with pytest.raises(ValueError, match="landmarks=True needs fuse=True"):
        PoseStream(None, track_intr=intr, **base, **carry)
    with pytest.raises(ValueError, match="landmarks=True needs carry=True"):
        PoseStream(None, track_intr=intr, anchor=anchor, fuse=True, **base)
    with pytest.raises(ValueError, match="needs track_intr"):
        PoseStream(None, anchor=anchor, fuse=True, **base, **carry)
    with pytest.raises(ValueError, match="lm_weight"):
        PoseStream(None, anchor=anchor, fuse=True, track_intr=intr, lm_weight="age", **base, **carry)
    with pytest.raises(ValueError, match="lm_gate_px"):
        PoseStream(None, anchor=anchor, fuse=True, track_intr=intr, lm_gate_px=-1.0, **base, **carry)
    with pytest.raises(ValueError, match="landmarks=True needs fuse=True"):
        StreamPool(None, streams=2, track_intrs=[intr, intr], **base, **carry)
    with pytest.raises(ValueError, match="landmarks=True needs carry=True"):
        StreamPool(None, streams=2, track_intrs=[intr, intr], anchors=[anchor, anchor], fuse=True, **base)
    with pytest.raises(ValueError, match="one per stream"):
        StreamPool(None, streams=2, track_intrs=[intr], anchors=[anchor, anchor], fuse=True, **base, **carry)
    ok = PoseStream(None, anchor=anchor, fuse=True, track_intr=intr, **base, **carry)
    assert isinstance(ok.landmark_map, LandmarkMap) and ok.landmark_map.inverse_rotation == 0
    assert ok.landmark_map.min_obs == 3 and ok.landmark_map.min_pivot == 1e-8
    off = PoseStream(None, window=4, query_fn=cand)
    assert off.landmark_map is None and not off.landmarks
    ids, X, n_obs = ok.landmark_map.snapshot(0)
    assert ids.shape == (0,) and X.shape == (0, 3) and n_obs.shape == (0,)
    for bad in (dict(min_obs=1), dict(min_pivot=1.0), dict(stride=4), dict(intrs=[intr, intr])):
        with pytest.raises(ValueError):
            LandmarkMap(**dict(dict(window=4, stride=1, streams=1, tracks=8, intrs=[intr]), **bad))


def test_result_keeps_its_twelve_positions():
    from comet_amd.stream import StreamResult
    r = StreamResult(0, torch.zeros(4, 7), None, None)
    assert len(r) == 12 and r.landmarks is None and r.landmark_state is None
    from comet_amd.ops import LandmarkOut
    lo = LandmarkOut(torch.zeros(1, 3, 3, dtype=torch.float64), torch.ones(1, 3, dtype=torch.int32), torch.zeros(1, 3),
                     torch.ones(1, 3, dtype=torch.int32))
    r2 = r.with_tracks(torch.zeros(3), None, None).with_landmarks(lo, 0)._replace(final=1)
    assert len(r2) == 12 and r2.landmarks.shape == (3, 3) and r2.track_ids is not None and r2.final == 1
    assert r.landmarks is None


def test_crop_intrinsics_truncates_the_box_as_the_resampler_does():
    from comet_amd.data import crop_intrinsics
    full = (268.44444444, 268.44444444, 320.0, 240.0)
    assert crop_intrinsics(full, (100.9, 37.2, 420.7, 357.99), 256) == crop_intrinsics(full, (100, 37, 420, 357), 256)
    assert crop_intrinsics(full, (-20.5, -5.5, 300.5, 315.5), 128) == crop_intrinsics(full, (-20, -5, 300, 315), 128)
    with pytest.raises(ValueError, match="empty box"):
        crop_intrinsics(full, (10.2, 0, 10.9, 50), 64)


def test_config_plumbing_of_cfg_stream_landmarks():
    from comet_amd import loop
    from comet_amd.data import crop_intrinsics
    from comet_amd.models.utils import INTRINSICS
    carry = dict(carry=True)
    assert loop._stream_landmarks({}, True, carry) == {}
    assert loop._stream_landmarks({"stream": {"landmarks": False, "lm_gate_px": 3}}, False, {}) == {}
    assert loop._stream_landmarks({"stream": {"landmarks": True}}, True, carry) == dict(
        landmarks=True, lm_min_obs=3, lm_min_pivot=1e-8, lm_weight=None, lm_gate_px=None, lm_inverse_rotation=0)
    full = {"stream": {"landmarks": True, "lm_min_obs": 5, "lm_min_pivot": 1e-6, "lm_weight": "score", "lm_gate_px": 4,
                       "lm_inverse_rotation": 1}}
    kw = loop._stream_landmarks(full, True, carry)
    assert kw == dict(landmarks=True, lm_min_obs=5, lm_min_pivot=1e-6, lm_weight="score", lm_gate_px=4.0, lm_inverse_rotation=1)
    assert isinstance(kw["lm_gate_px"], float)
    for fuse, c in ((False, carry), (True, {})):
        with pytest.raises(ValueError, match="cfg.stream.landmarks needs cfg.stream.fuse and cfg.stream.carry"):
            loop._stream_landmarks(full, fuse, c)
    box = (100, 37, 420, 357)
    assert loop._track_intr("AMD", box, 256) == crop_intrinsics(INTRINSICS["AMD"], box, 256)
    assert loop._track_intr("spark", box, 256) != loop._track_intr("AMD", box, 256)
    # the keywords are the constructor's own
    from comet_amd.stream import PoseStream
    anchor = ([1.0, 0, 0, 0], [64.0, 64.0, 5.0], 1.0, 1.0, "AMD")
    st = PoseStream(None, window=4, stride=1, anchor=anchor, fuse=True, carry=True, carry_tracks=8, carry_min_score=0.5,
                    candidate_fn=lambda f: None, track_intr=loop._track_intr("AMD", box, 256), **kw)
    lm = st.landmark_map
    assert (lm.min_obs, lm.min_pivot, lm.inverse_rotation, st.lm_weight, st.lm_gate_px) == (5, 1e-6, 1, "score", 4.0)
    assert lm.intrs == [crop_intrinsics(INTRINSICS["AMD"], box, 256)]


def test_snapshot_csv_holds_one_row_per_landmark(tmp_path):
    import csv
    from comet_amd import loop

    class _Map:
        def snapshot(self, stream=0):
            assert stream == 2
            return (torch.tensor([7, 19], dtype=torch.int32), torch.tensor([[0.1, -0.2, 1 / 3], [1e-17, 2.0, -3.5]],
                    dtype=torch.float64), torch.tensor([3, 12], dtype=torch.int32))

    class _Empty:
        def snapshot(self, stream=0):
            return torch.empty(0, dtype=torch.int32), torch.empty(0, 3, dtype=torch.float64), torch.empty(0, dtype=torch.int32)
    path = str(tmp_path / "seq.csv")
    assert loop.landmarks_csv(path) == str(tmp_path / "seq_landmarks.csv")
    assert loop._log_landmarks(path, _Map(), 2) == 2
    rows = list(csv.DictReader(open(loop.landmarks_csv(path))))
    assert tuple(rows[0].keys()) == loop.LANDMARK_FIELDS == ("track_id", "x", "y", "z", "n_obs")
    assert [(int(r["track_id"]), float(r["x"]), float(r["y"]), float(r["z"]), int(r["n_obs"])) for r in rows] == [
        (7, 0.1, -0.2, 1 / 3, 3), (19, 1e-17, 2.0, -3.5, 12)]  # (floats are written so that they read back exactly)
    empty = str(tmp_path / "none.csv")
    assert loop._log_landmarks(empty, _Empty()) == 0
    assert open(loop.landmarks_csv(empty)).read().strip() == ",".join(loop.LANDMARK_FIELDS)


def test_pool_reset_takes_the_next_sequences_intrinsics():
    from comet_amd.stream import LandmarkMap, StreamPool
    a, b, c = (100.0, 100.0, 64.0, 64.0), (120.0, 110.0, 60.0, 66.0), (90.0, 95.0, 63.5, 63.5)
    lm = LandmarkMap(window=4, stride=1, streams=2, tracks=8, intrs=[a, b])
    lm._tables = {(0, 1): "cached"}
    lm.set_intr(1, b)
    assert lm._tables and lm.intrs == [a, b], "unchanged intrinsics keep the cached tables"
    lm.set_intr(1, c)
    assert lm.intrs == [a, c] and lm._tables == {}, "the tables hold the intrinsics by value: dropped on a change"
    for bad in (dict(stream=2, intr=c), dict(stream=0, intr=(1.0, 2.0)), dict(stream=0, intr=None)):
        with pytest.raises(ValueError):
            lm.set_intr(**bad)
    anchor = ([1.0, 0, 0, 0], [64.0, 64.0, 5.0], 1.0, 1.0, "AMD")
    kw = dict(window=4, stride=1, streams=2, anchors=[anchor, anchor], fuse=True, carry=True, carry_tracks=8,
              carry_min_score=0.5, candidate_fn=lambda f: None)
    pool = StreamPool(None, landmarks=True, track_intrs=[a, b], **kw)
    pool.reset(1, track_intr=c)
    assert pool.landmark_map.intrs == [a, c]
    with pytest.raises(ValueError, match="track_intr"):
        pool.reset(track_intr=c)
    with pytest.raises(ValueError, match="track_intr"):
        StreamPool(None, **kw).reset(0, track_intr=c)
