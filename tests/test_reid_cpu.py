"""The landmark archive without a GPU: the float64 restatement tests/reid_numpy.py of comet_landmark_reid,
chained with landmark_numpy.update, on a turning body whose points leave the view and return one revolution
later (DESIGN.md "Landmark archive"); the ordering and state rules on the constructed case of
tests/reid_cases.py; the constructor checks of LandmarkMap / PoseStream / StreamPool.

Tracks and quaternions are float64 here, so "exact projections" are exact to double rounding."""
import numpy as np
import pytest

import landmark_numpy as lmn
import reid_numpy as rn
from reid_cases import SHAPES, _case, _check_margins, _reference

INTR = (3000.0, 3100.0, 635.0, 600.0)
P, T, C = 8, 4, 16
STEP = np.deg2rad(6.0)
FRAMES = 150 + T            # 2.5 revolutions of 60 frames, and the last window
REID_PX, MIN_COS = 2.0, 0.5
VISIBLE = np.cos(np.deg2rad(24.0))  # tracked within 24 deg of facing: it leaves and returns <= 54 deg apart, cos > 0.5


def _body():
    """P points of the unit sphere at latitudes within 17 deg, spread in longitude; the normal is the point."""
    h = np.linspace(-0.3, 0.3, P)
    lon = np.arange(P) * (2 * np.pi / P) * 3 + 0.2
    r = np.sqrt(1.0 - h * h)
    return np.stack([r * np.sin(lon), h, r * np.cos(lon)], -1)


def _scene():
    X = _body()
    q = np.stack([lmn.quat_from_axis_angle((0.0, 1.0, 0.0), STEP * f) for f in range(FRAMES)])
    t = np.tile(np.array([0.0, 0.0, 6.0]), (FRAMES, 1))
    px = np.stack([lmn.project(X, q[f], t[f], INTR)[0] for f in range(FRAMES)])
    vis = np.zeros((FRAMES, P), bool)
    for f in range(FRAMES):
        c = rn.camera_centre(q[f], t[f], 0)
        v = c - X
        vis[f] = (X * v).sum(-1) / np.linalg.norm(v, axis=-1) > VISIBLE
    return X, q, t, px, vis


def _chain(px, q, t, vis, archive=True, capacity=C):
    """Hop k is the window of frames k .. k + T - 1; slot p holds point p while it is visible on frame k, pads
    when it is not and is born under a fresh id when it returns -> per hop (reid out or None, update out,
    ids [P])."""
    acc, acc_id = lmn.new_state(1, P)
    st = rn.new_state(1, P, capacity)
    intr = np.array([INTR])
    ids, nxt, hops = np.full(P, -1, np.int32), 0, []
    for k in range(FRAMES - T + 1):
        src = np.full(P, rn.INT_MIN, np.int32)
        for p in range(P):
            if not vis[k, p]:
                ids[p] = -1
            elif ids[p] < 0:
                ids[p], src[p], nxt = nxt, -1 - p, nxt + 1
            else:
                src[p] = p
        w = (px[k:k + T][None], q[k:k + T][None], t[k:k + T][None])
        ro = None
        if archive:
            ro = rn.reid(*w, ids[None], src[None], [0], intr, acc, acc_id, st, capacity, REID_PX, MIN_COS)
        lo = lmn.update(*w, ids[None], (ro["src_lm"] if archive else src[None]), [0], intr, acc, acc_id, 1)
        hops.append((ro, lo, ids.copy(), src.copy()))
        if ro is not None:
            ro["arch_ids"] = st["arch_id"].copy()  # (after the hop)
    return hops, st


def test_the_scene_keeps_its_points_apart():
    """The precondition of the matching tests: in every frame any two points project at least 3 reid_px
    apart (points on the far side included)."""
    X, q, t, px, vis = _scene()
    d = np.linalg.norm(px[:, :, None] - px[:, None, :], axis=-1) + 1e9 * np.eye(P)
    print(f"least projected separation over {FRAMES} frames: {d.min():.2f} px")
    assert d.min() >= 3 * REID_PX
    spans = vis.sum(0)
    assert (spans >= 2 * 4).all() and (~vis).any(0).all(), "every point is seen on each revolution and leaves the view"


def test_returning_points_get_their_landmark_and_identity_back():
    X, q, t, px, vis = _scene()
    hops, st = _chain(px, q, t, vis)
    name, returns = {}, 0  # point -> the identity of its landmark
    for k, (ro, lo, ids, src) in enumerate(hops):
        for p in range(P):
            if ids[p] < 0:
                assert ro["lm_id"][0, p] == -1
                continue
            if src[p] < 0:  # born: a return iff its landmark was archived when it left
                if p in name and name[p] in hops[k - 1][0]["arch_ids"]:
                    returns += 1
                    assert ro["reid_state"][0, p] == rn.MATCHED and ro["reid_dist"][0, p] <= 1e-6
                    assert ro["lm_id"][0, p] == name[p] != ids[p], "matched to its own earlier identity"
                    assert lo["state"][0, p] == lmn.VALID, "valid at the birth hop, without waiting min_obs frames"
                    assert lo["n_obs"][0, p] >= 3 + 1
                else:
                    assert ro["reid_state"][0, p] == rn.NO_CANDIDATE
                    name[p] = ids[p]
            assert ro["lm_id"][0, p] == name[p], "the landmark identity is stable across revolutions"
            if lo["state"][0, p] == lmn.VALID:
                err = np.abs(lo["X"][0, p] - X[p]).max()
                assert err <= 1e-9 * (1.0 + np.linalg.norm(X[p])), (k, p, err)
    assert returns >= P, "every point returned at least once"
    # without the archive the same births start from nothing
    plain, _ = _chain(px, q, t, vis, archive=False)
    for (ro, lo, ids, src), (_, lo0, _, _) in zip(hops, plain):
        born = (src < 0) & (ids >= 0)
        assert (lo0["state"][0][born] == lmn.NONE).all() and (lo0["n_obs"][0][born] == 1).all()


def test_a_point_on_the_far_side_is_never_a_candidate_and_a_fresh_entry_waits_a_hop():
    X, q, t, px, vis = _scene()
    hops, st = _chain(px, q, t, vis)
    owner, away_seen = {}, 0  # landmark identity -> the point it was born on
    for k, (ro, lo, ids, src) in enumerate(hops):
        for p in np.nonzero((ids >= 0) & (src < 0))[0]:
            owner[int(ids[p])] = p
        if k == 0:
            continue
        # from the scene's truth: the archive as the previous hop left it, every entry's point, and the angle
        # between the direction it was last seen from (frame k - 1 or earlier: its retirement frame) and now
        c = rn.camera_centre(q[k], t[k], 0)
        before = hops[k - 1][0]
        for e in np.nonzero(before["arch_ids"] >= 0)[0]:
            p = owner[int(before["arch_ids"][e])]
            now = (c - X[p]) / np.linalg.norm(c - X[p])
            facing = float(X[p] @ now)  # the point's normal is the point: cos of the angle to the camera
            if facing < 0.0:  # on the far side of the body: more than 90 deg from any direction it was tracked from
                away_seen += 1
                assert not ro["cand"][0, e], (k, e, p, facing)
                assert (lmn.project(X[p:p + 1], q[k], t[k], INTR)[1] > 0).all(), "in front of the camera all the same"
    assert away_seen > 100, "no archived point was ever on the far side"
    # an entry retired in a hop is not matched in that hop: a slot dies and is born again on the same pixel
    acc, acc_id = lmn.new_state(1, P)
    st = rn.new_state(1, P, C)
    k = int(np.nonzero(vis[:, 0])[0][0])
    acc[0], acc_id[0] = rn.rows_of(X[:1], q[k - 4:k], t[k - 4:k], INTR, 0)[0], 5
    ids, src = np.full((1, P), -1, np.int32), np.full((1, P), rn.INT_MIN, np.int32)
    ids[0, 0], src[0, 0] = 6, -1
    w = (px[k:k + T][None], q[k:k + T][None], t[k:k + T][None])
    out = rn.reid(*w, ids, src, [0], np.array([INTR]), acc, acc_id, st, C, REID_PX, MIN_COS)
    assert out["stats"][0].tolist() == [1, 0, 1, 0] and out["reid_state"][0, 0] == rn.NO_CANDIDATE
    lmn.update(*w, ids, out["src_lm"], [0], np.array([INTR]), acc, acc_id, 1)
    ids[0, 0], src[0, 0] = 7, -1  # killed and born once more, one hop later: now the entry is there
    w = (px[k + 1:k + 1 + T][None], q[k + 1:k + 1 + T][None], t[k + 1:k + 1 + T][None])
    out = rn.reid(*w, ids, src, [0], np.array([INTR]), acc, acc_id, st, C, REID_PX, MIN_COS)
    assert out["reid_state"][0, 0] == rn.MATCHED and out["lm_id"][0, 0] == 5
    assert out["stats"][0].tolist() == [0, 1, 0, 0], "the one-frame row of id 6 is below arch_min_obs: not retired"


@pytest.mark.parametrize("shape", SHAPES[:4])
def test_mutual_rule_ties_and_the_ring_on_the_constructed_case(shape):
    """The constructed case of tests/reid_cases.py: state 3, both tie rules, the wrap-around of the ring
    with fewer entries than deaths and its overwrite count."""
    n, N, Cc, Tw = shape
    c = _case(n, N, Cc, Tw, 0)
    out, acc, acc_id, st = _reference(c, Cc, 0)
    _check_margins(c, out, set() if N == 1 else {(h, j) for h in range(n) for j in (14, 15)})
    if N == 1:
        assert out["stats"][0].tolist() == [1, 1, 1, 0] and st["arch_id"][1] == 5 and st["arch_cursor"][1] == 0
        return
    for h, mk in enumerate(c["marks"]):
        s = mk["stream"]
        assert out["reid_state"][h, 12] == rn.MATCHED and out["reid_state"][h, 13] == rn.LOST, "the nearer slot is accepted"
        assert out["best"][h, 14] == out["best"][h, 15] and out["reid_state"][h, 14] == rn.MATCHED and \
            out["reid_state"][h, 15] == rn.LOST, "equal distances: the lower slot"
        assert out["best"][h, 14] == out["second"][h, 14] and out["lm_id"][h, 14] == 72, "equal distances: the lower entry"
        retired, matched, used, over = out["stats"][h]
        before = int((c["state"]["arch_id"][s * Cc:(s + 1) * Cc] >= 0).sum())
        assert st["arch_cursor"][s] == (3 + retired) % Cc
        assert used == min(Cc, before - matched + retired - over) and (used == Cc) == (retired >= Cc)
        if retired > Cc:
            assert over >= retired - Cc and (st["arch_id"][s * Cc:(s + 1) * Cc] >= 0).all()
            last = [j for j in range(N) if c["acc_id"][s * N + j] >= 0 and
                    (c["ids"][h, j] != c["acc_id"][s * N + j] or c["src"][h, j] != j)][-1]
            assert st["arch_id"][s * Cc + (3 + retired - 1) % Cc] == c["acc_id"][s * N + last], "the last retirement stays"


def test_reset_frees_a_stream_only():
    n, N, Cc, Tw = SHAPES[1]
    c = _case(n, N, Cc, Tw, 0)
    out, acc, acc_id, st = _reference(c, Cc, 0)
    keep = {k: v.copy() for k, v in st.items()}
    rn.reset(st, acc_id, 2, N, Cc)
    assert (st["arch_id"][2 * Cc:3 * Cc] == -1).all() and (st["alias"][2 * N:3 * N] == -1).all() and st["arch_cursor"][2] == 0
    assert rn.snapshot(st, 2, Cc)[0].size == 0 and (acc_id[2 * N:3 * N] == -1).all()
    for s in (1, 3):
        assert np.array_equal(st["arch_id"][s * Cc:(s + 1) * Cc], keep["arch_id"][s * Cc:(s + 1) * Cc])
        assert st["arch_cursor"][s] == keep["arch_cursor"][s] and rn.snapshot(st, s, Cc)[0].size > 0


def test_pixel_noise_gives_no_false_match():
    """sigma = 0.5 px on every pixel, seeds 0..49, under the separation precondition (>= 3 reid_px): no born
    slot is matched to another point's landmark. The matched fraction of the returns and the valid landmarks
    per hop on revolution 2, with and without the archive, are printed (DESIGN.md "Landmark archive")."""
    X, q, t, px, vis = _scene()
    false, matched, returns, valid_on, valid_off, hops_n = 0, 0, 0, 0, 0, 0
    for seed in range(50):
        noisy = px + np.random.default_rng(seed).normal(0.0, 0.5, px.shape)
        on, _ = _chain(noisy, q, t, vis)
        off, _ = _chain(noisy, q, t, vis, archive=False)
        first, owner = {}, {}  # point -> its newest landmark; landmark identity -> the point it was born on
        for k, ((ro, lo, ids, src), (_, lo0, _, _)) in enumerate(zip(on, off)):
            for p in np.nonzero(ids >= 0)[0]:
                if src[p] < 0:
                    owner[int(ids[p])] = p
                    if p in first and first[p] in on[k - 1][0]["arch_ids"]:
                        returns += 1
                    if ro["reid_state"][0, p] == rn.MATCHED:  # false: to a landmark of another point
                        matched += 1
                        false += owner[int(ro["lm_id"][0, p])] != p
                    else:
                        first[p] = ids[p]
            if 60 <= k < 120:
                hops_n += 1
                valid_on += int((lo["state"][0] == lmn.VALID).sum())
                valid_off += int((lo0["state"][0] == lmn.VALID).sum())
    print(f"noise 0.5 px, 50 seeds: {matched}/{returns} returns matched ({matched / returns:.3f}), {false} false; valid "
          f"landmarks per hop on revolution 2: archive on {valid_on / hops_n:.2f}, off {valid_off / hops_n:.2f}")
    assert false == 0 and matched > 0


def test_constructor_checks():
    from comet_amd.stream import LandmarkMap
    kw = dict(window=4, stride=1, streams=1, tracks=8, intrs=[INTR])
    lm = LandmarkMap(**kw)
    assert lm.archive == 0 and lm.archive_snapshot(0)[0].numel() == 0
    with pytest.raises(RuntimeError, match="archive > 0"):
        lm.reidentify([0], None, None, None, None, None)
    with pytest.raises(ValueError, match="reid_px"):
        LandmarkMap(archive=4, **kw)
    for bad in (dict(reid_px=0.0), dict(reid_px=float("inf")), dict(reid_px=2.0, reid_min_cos=1.5),
                dict(reid_px=2.0, arch_min_obs=1)):
        with pytest.raises(ValueError):
            LandmarkMap(archive=4, **bad, **kw)
    for bad in (-1, 4097):
        with pytest.raises(ValueError, match="archive must be"):
            LandmarkMap(archive=bad, reid_px=2.0, **kw)
    lm = LandmarkMap(archive=4, reid_px=2.0, min_obs=5, **kw)
    assert (lm.archive, lm.reid_px, lm.reid_min_cos, lm.arch_min_obs) == (4, 2.0, 0.5, 5)


def test_stream_keywords_need_landmarks():
    from comet_amd.stream import PoseStream, StreamPool
    with pytest.raises(ValueError, match="lm_archive > 0 needs landmarks=True"):
        StreamPool(None, 2, 4, lm_archive=8, reid_px=2.0)
    with pytest.raises(ValueError, match="lm_archive > 0 needs landmarks=True"):
        PoseStream(None, 4, lm_archive=8, reid_px=2.0)


def test_config_plumbing_of_cfg_stream_lm_archive():
    from comet_amd import loop
    carry = dict(carry=True)
    on = {"stream": {"landmarks": True, "lm_archive": 64, "reid_px": 3}}
    assert loop._stream_archive({}) == {} and loop._stream_archive({"stream": {"lm_archive": 0, "reid_px": 3}}) == {}
    base = loop._stream_landmarks({"stream": {"landmarks": True}}, True, carry)
    assert "lm_archive" not in base and "reid_px" not in base, "with the archive off the keywords are what they were"
    kw = loop._stream_landmarks(on, True, carry)
    assert {k: kw[k] for k in ("lm_archive", "reid_px", "reid_min_cos", "lm_arch_min_obs")} == dict(
        lm_archive=64, reid_px=3.0, reid_min_cos=0.5, lm_arch_min_obs=None)
    assert {k: v for k, v in kw.items() if k in base} == base
    full = {"stream": dict(on["stream"], reid_min_cos=0.25, lm_arch_min_obs=5)}
    kw = loop._stream_landmarks(full, True, carry)
    assert (kw["reid_min_cos"], kw["lm_arch_min_obs"]) == (0.25, 5)
    with pytest.raises(ValueError, match="reid_px"):
        loop._stream_landmarks({"stream": {"landmarks": True, "lm_archive": 8}}, True, carry)
    with pytest.raises(ValueError, match="lm_archive needs cfg.stream.landmarks"):
        loop._stream_landmarks({"stream": {"lm_archive": 8, "reid_px": 2}}, True, carry)
    # the keywords are the constructor's own
    from comet_amd.stream import PoseStream
    anchor = ([1.0, 0, 0, 0], [64.0, 64.0, 5.0], 1.0, 1.0, "AMD")
    st = PoseStream(None, window=4, stride=1, anchor=anchor, fuse=True, carry=True, carry_tracks=8, carry_min_score=0.5,
                    candidate_fn=lambda f: None, track_intr=INTR, **kw)
    lm = st.landmark_map
    assert (st.lm_archive, lm.archive, lm.reid_px, lm.reid_min_cos, lm.arch_min_obs) == (64, 64, 3.0, 0.25, 5)


def test_archive_csv_holds_one_row_per_entry(tmp_path):
    import csv
    import torch
    from comet_amd import loop

    class _Map:
        def archive_snapshot(self, stream=0):
            assert stream == 2
            return (torch.tensor([7, 19], dtype=torch.int32), torch.tensor([[0.1, -0.2, 1 / 3], [1e-17, 2.0, -3.5]],
                    dtype=torch.float64), torch.tensor([3, 12], dtype=torch.int32))

    path = str(tmp_path / "seq.csv")
    assert loop.archive_csv(path) == str(tmp_path / "seq_archive.csv")
    assert loop._log_archive(path, _Map(), 2) == 2
    rows = list(csv.DictReader(open(loop.archive_csv(path))))
    assert tuple(rows[0].keys()) == loop.LANDMARK_FIELDS
    assert [(int(r["track_id"]), float(r["x"]), float(r["y"]), float(r["z"]), int(r["n_obs"])) for r in rows] == [
        (7, 0.1, -0.2, 1 / 3, 3), (19, 1e-17, 2.0, -3.5, 12)]
    from comet_amd.stream import LandmarkMap
    empty = str(tmp_path / "none.csv")
    assert loop._log_archive(empty, LandmarkMap(4, 1, 1, 8, [INTR], archive=4, reid_px=2.0)) == 0
    assert open(loop.archive_csv(empty)).read().strip() == ",".join(loop.LANDMARK_FIELDS)


def test_snapshot_names_the_rows_of_the_update_it_reports():
    """snapshot() takes its identities from the reidentify() that preceded the update() it reports, on the same
    hops; an update() without one reports the carry's ids (host logic, checked on stand-in launches)."""
    import torch
    from comet_amd import ops, stream as sm
    lm = sm.LandmarkMap(4, 1, 2, 3, [INTR, INTR], archive=4, reid_px=2.0)
    lm.device = "cpu"
    lm._tables, lm._last, lm._pending = {}, {}, None
    lm._table = lambda sids: (None, None, None, None)
    for name in ("acc", "acc_id", "alias", "arch", "arch_id", "arch_cursor", "_ws"):
        setattr(lm, name, None)
    lm._ensure = lambda dev: None
    ids = torch.tensor([[5, 6, -1]], dtype=torch.int32)
    lo = ops.LandmarkOut(torch.zeros(1, 3, 3, dtype=torch.float64), torch.tensor([[4, 4, 0]], dtype=torch.int32),
                         torch.zeros(1, 3), torch.tensor([[1, 1, 0]], dtype=torch.int32))
    ro = ops.ReidOut(ids, torch.tensor([[2, 6, -1]], dtype=torch.int32), ids, torch.zeros(1, 3), torch.zeros(1, 4))
    real = ops.landmark_update, ops.landmark_reid
    ops.landmark_update, ops.landmark_reid = (lambda *a, **k: lo), (lambda *a, **k: ro)
    try:
        tr = torch.zeros(1, 4, 3, 2)
        lm.reidentify([1], tr, None, None, ids, ids)
        lm.update([1], tr, None, None, ids, ids)
        assert lm.snapshot(1)[0].tolist() == [2, 6], "the landmark identities"
        lm.update([1], tr, None, None, ids, ids)
        assert lm.snapshot(1)[0].tolist() == [5, 6], "no reidentify() before this update(): the carry's ids"
        lm.reidentify([0], tr, None, None, ids, ids)
        lm.update([1], tr, None, None, ids, ids)
        assert lm.snapshot(1)[0].tolist() == [5, 6], "a reidentify() of other hops does not name these rows"
    finally:
        ops.landmark_update, ops.landmark_reid = real


def test_drift_report_with_the_archive_on_and_off():
    """Report only (DESIGN.md "Landmark archive"): FuseRef, the landmark, PnP and archive restatements chained
    per hop with pnp_weight = 1 over two revolutions of the turning body, sigma 0.5 px on the tracks and the pose
    noise of test_fuse_cpu; the RMS rotation and (u, v, z) error of the final fused poses with the archive on
    and off. No direction is asserted."""
    import fuse_numpy as fn
    import pnp_numpy as pn
    from test_fuse_cpu import RATIO, SIG_D, SIG_ROT, SIG_UV
    fintr = (268.44444444, 268.44444444, 320.0, 240.0)
    frames, Pn, cap = 120 + T, 96, 256
    pose_T = lambda x: np.array([(x[0] - fintr[2]) * x[2] / fintr[0], (x[1] - fintr[3]) * x[2] / fintr[1], x[2]])  # noqa: E731
    h = np.linspace(-0.5, 0.5, Pn)
    lon = np.arange(Pn) * (2 * np.pi / Pn) * 7 + 0.2
    body = np.stack([np.sqrt(1 - h * h) * np.sin(lon), h, np.sqrt(1 - h * h) * np.cos(lon)], -1)
    q = np.stack([fn.unit_pos(lmn.quat_from_axis_angle((0.0, 1.0, 0.0), STEP * f)) for f in range(frames)])
    x = np.tile(np.array([320.0, 240.0, 3.0]), (frames, 1))
    vis = np.zeros((frames, Pn), bool)
    for f in range(frames):
        v = rn.camera_centre(q[f], pose_T(x[f]), 0) - body
        vis[f] = (body * v).sum(-1) / np.linalg.norm(v, axis=-1) > np.cos(np.deg2rad(50.0))  # (wider than the matching tests: PnP needs six landmarks in view)
    intr = np.array([fintr])

    def run(seed, archive, gate=3.0):
        rng = np.random.default_rng(seed)
        encs = [fn.window_encoding(rng, q, x, k, T, RATIO, SIG_ROT, SIG_UV, SIG_D) for k in range(frames - T + 1)]
        px = np.stack([lmn.project(body, q[f], pose_T(x[f]), fintr)[0] for f in range(frames)])
        px = (px + rng.normal(0.0, 0.5, px.shape)).astype(np.float32)
        ref = fn.FuseRef(T, RATIO, fintr)
        acc, acc_id = lmn.new_state(1, Pn)
        st = rn.new_state(1, Pn, cap)
        ids, nxt, er, ex, matched, valid = np.full(Pn, -1, np.int32), 0, [], [], 0, 0
        anchor = np.concatenate([q[0], x[0]])
        for k in range(frames - T + 1):
            src = np.full(Pn, rn.INT_MIN, np.int32)
            for p in range(Pn):
                if not vis[k, p]:
                    ids[p] = -1
                elif ids[p] < 0:
                    ids[p], src[p], nxt = nxt, -1 - p, nxt + 1
                else:
                    src[p] = p
            slots = [(k + i) % T for i in range(T)]
            out = ref.fuse(encs[k][None], slots, [1 if k == 0 else T - 1], [int(k == 0)], [anchor])
            fq, fu, _, _ = fn.fused(ref.acc[slots[0]])
            er.append(fn.rot_angle(fq, q[k]))
            ex.append(np.linalg.norm(fu - x[k]))
            tr, s2 = px[k:k + T][None], src[None]
            if archive:
                ro = rn.reid(tr, out["R"], out["T"], ids[None], s2, [0], intr, acc, acc_id, st, cap, gate, -0.3)  # (100 deg between leaving and returning)
                s2, matched = ro["src_lm"], matched + int(ro["stats"][0, 1])
            lo = lmn.update(tr, out["R"], out["T"], ids[None], s2, [0], intr, acc, acc_id, 1)
            valid += int((lo["state"] == lmn.VALID).sum())
            pn.pnp(tr, lo["X"], lo["state"], out["R"], out["T"], intr, 1, 3.0, fuse_acc=ref.acc, slots=slots, inject_w=1.0,
                   fuse_intr=fintr)
        rms = lambda v: float(np.sqrt(np.mean(np.square(v))))  # noqa: E731
        return rms(er), rms(ex), matched, valid / (frames - T + 1)

    seeds = range(3)
    off = np.array([run(s, False) for s in seeds])
    assert np.isfinite(off).all()
    print(f"drift over two revolutions, {len(seeds)} seeds, pnp_weight 1, archive off: rotation {off[:, 0].mean():.4e} rad, "
          f"(u, v, z) {off[:, 1].mean():.4e}, valid landmarks per hop {off[:, 3].mean():.2f}")
    for gate in (3.0, 15.0):
        on = np.array([run(s, True, gate) for s in seeds])
        assert np.isfinite(on).all()
        print(f"  archive on, reid_px {gate:g}: rotation {on[:, 0].mean():.4e} rad, (u, v, z) {on[:, 1].mean():.4e}, matches "
              f"per run {on[:, 2].mean():.1f}, valid landmarks per hop {on[:, 3].mean():.2f}")
