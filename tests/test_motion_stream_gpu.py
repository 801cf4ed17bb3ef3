"""The motion estimate through PoseStream and StreamPool on the GPU (DESIGN.md "Motion estimate").

The golden configuration of the landmark tests (T = 4, 128 x 128, N = 64, oracle.prng weights of seed 0 and
frames of seed 1, carried tracks, f32, 6 hops): motion=True changes nothing else the stream computes, and its
fields equal the restatement (tests/motion_numpy.py) chained on the recorded fused poses, within the bound of
tests/test_motion_gpu.py. Then a geometric stand-in for the model, a body that spins at a known constant
rate, on which the estimate has a truth."""
import numpy as np
import pytest
import torch

import fuse_numpy as fn
import motion_numpy as mn

pytestmark = pytest.mark.gpu

T, HW, N = 4, 128, 64
SEED_W, SEED_X, SEEDS = 0, 1, (4, 2, 6)
MIN_SCORE = 0.5
CAND_SEED, CAND_M = 7, 96
HOPS = 5
TOL = 1e-10
FIELDS = ("motion_omega", "motion_vel", "motion_q0", "motion_t0", "motion_rot_rms", "motion_trans_rms", "motion_frames",
          "motion_state", "motion_pred_R", "motion_pred_T", "motion_innov_rot", "motion_innov_trans")
REF = dict(motion_omega="omega", motion_vel="vel", motion_q0="q0", motion_t0="t0", motion_rot_rms="rot_rms",
           motion_trans_rms="trans_rms", motion_pred_R="pred_q", motion_pred_T="pred_t", motion_innov_rot="innov_rot",
           motion_innov_trans="innov_trans")
OTHERS = ("pred_pose_enc", "pred_tracks", "pred_score", "R", "T", "fused_R", "fused_T", "fused_count", "rot_spread",
          "trans_spread", "track_ids", "track_age", "track_src")


@pytest.fixture(scope="module")
def model():
    from comet_amd.config import instantiate, load_config
    from oracle import prng
    from oracle.weights import comet_shapes
    cfg = load_config()
    torch.manual_seed(0)
    m = instantiate(cfg.MODEL, _recursive_=False, cfg=cfg)
    m.load_state_dict(prng.make_state_dict(SEED_W, comet_shapes()), strict=True)
    return m.cuda().eval()


def _frames(seed, count):
    from oracle import prng
    img, _, _ = prng.synthetic_batch(seed, 1, count, HW, HW, N)
    return img[0].cuda()


class _Candidates:
    """A fixed seeded point set as candidate_fn."""

    def __init__(self):
        g = torch.Generator().manual_seed(CAND_SEED)
        self.points = (torch.rand(CAND_M, 2, generator=g) * (HW - 1)).cuda()

    def __call__(self, frame):
        assert frame.shape == (3, HW, HW)
        return self.points


def _anchor():
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device="cuda")
    return (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device="cuda"), 268.44,
            torch.tensor([0.5], dtype=torch.float64), "AMD")


def _kw(**kw):
    return dict(dict(window=T, stride=1, carry=True, carry_tracks=N, carry_cell=8, carry_border=0,
                     carry_min_score=MIN_SCORE, candidate_fn=_Candidates(), fuse=True, precision=torch.float32), **kw)


def _stream(model, **kw):
    from comet_amd.stream import PoseStream
    return PoseStream(model, anchor=_anchor(), **_kw(**kw))


def _run(st, frames):
    res = []
    for f in range(frames.shape[0]):
        res += st.push(frames[f])
    return res


def _np(t):
    return t.detach().cpu().numpy()


def _equal_restatement(r, ref, what):
    """A result's motion fields against row 0 of the restatement's outputs."""
    assert int(r.motion_state) == int(ref["state"][0]) and int(r.motion_frames) == int(ref["n_used"][0]), \
        (what, int(r.motion_state), int(ref["state"][0]), int(r.motion_frames), int(ref["n_used"][0]))
    worst = 0.0
    for name, key in REF.items():
        a, b = _np(getattr(r, name)).astype(np.float64), ref[key][0].astype(np.float64)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        fin = np.isfinite(b)
        assert (np.isfinite(a) == fin).all() and (a[~fin] == b[~fin]).all(), (what, name)
        if fin.any():
            err = float((np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))).max())
            assert err <= TOL, (what, name, err)
            worst = max(worst, err)
    return worst


@pytest.fixture(scope="module")
def plain(model):
    """The golden stream without the motion estimate, HOPS + 1 hops."""
    return _run(_stream(model), _frames(SEED_X, T + HOPS))


@pytest.fixture(scope="module")
def moved(model):
    """The same stream with motion=True (horizon 2, so that predictions past the window exist)."""
    st = _stream(model, motion=True, motion_horizon=2)
    return _run(st, _frames(SEED_X, T + HOPS)), st


def test_motion_changes_nothing_else_and_equals_the_restatement_chain(moved, plain):
    res, st = moved
    assert len(res) == len(plain) == HOPS + 1
    hist, hist_n = np.zeros((1, 16, 8)), np.zeros(1, np.int32)
    worst = 0.0
    for k, (r, p) in enumerate(zip(res, plain)):
        assert len(r) == 12 and all(getattr(p, name) is None for name in FIELDS)
        for name in OTHERS:  # the motion launch changes nothing the stream computes
            assert torch.equal(getattr(r, name), getattr(p, name)), (k, name)
        assert r.final == p.final == 1 and r.frame_index == p.frame_index == k
        ref = mn.motion_fit(_np(r.fused_R)[None], _np(r.fused_T)[None], [int(k == 0)], [0], hist, hist_n, 1, horizon=2)
        worst = max(worst, _equal_restatement(r, ref, f"hop {k}"))
        assert r.motion_omega.shape == (3,) and r.motion_omega.dtype == torch.float64 and r.motion_q0.shape == (4,)
        assert r.motion_pred_R.shape == (T - 1 + 2, 4) and r.motion_pred_T.shape == (T - 1 + 2, 3)
        assert r.motion_innov_rot.shape == (T - 1,) and r.motion_innov_trans.dtype == torch.float32
        assert int(r.motion_frames) == k + 1 and (int(r.motion_state) == 0) == (k < 2)
        print(f"hop {k}: state {int(r.motion_state)}, frames {int(r.motion_frames)}, |omega| "
              f"{float(r.motion_omega.norm()):.4f} rad/frame, rot_rms {float(r.motion_rot_rms):.4f}")
    print(f"max |stream - restatement| / max(1, |restatement|): {worst:.3e}")
    mt = st.motion_tracker
    assert (_np(mt.hist).view(np.int64) == hist.view(np.int64)).all() and _np(mt.hist_n).tolist() == [HOPS + 1]
    st.reset()
    assert mt._first == [True]


def test_pool_of_one_stream_equals_the_stream_bit_for_bit(model, moved):
    from comet_amd.stream import StreamPool
    base, _ = moved
    pool = StreamPool(model, streams=1, anchors=[_anchor()], **_kw(motion=True, motion_horizon=2))
    frames = _frames(SEED_X, T + HOPS)
    got = [r for f in range(frames.shape[0]) for _, r in pool.push(frames[f][None])]
    assert len(got) == len(base)
    for k, (g, b) in enumerate(zip(got, base)):
        for name in FIELDS:
            assert _np(getattr(g, name)).tobytes() == _np(getattr(b, name)).tobytes(), (k, name)


PUSHES, LATE, RESET_AT = 11, 1, 6  # stream 1 joins one push late and is reset before push 6


def test_pool_of_three_streams_out_of_phase_equals_the_restatement_per_stream(model):
    """warm_iters differs from the config's iterations, so a push in which stream 1's first hop falls together
    with later hops of streams 0 and 2 runs two model calls (first hops, then later hops); their rows are
    stacked in the order [1, 0, 2] for the fuse launch, and the motion launch runs on those rows in that order."""
    from comet_amd.stream import StreamPool
    seqs = [_frames(seed, PUSHES) for seed in SEEDS]
    pool = StreamPool(model, streams=3, anchors=[_anchor()] * 3, **_kw(motion=True, warm=True, warm_iters=2))
    assert int(model.cfg["track_trainit"]) != 2
    launches, inner = [], pool.motion_tracker.update
    pool.motion_tracker.update = lambda hops, fused, weights=None: (launches.append([s for s, _ in hops]),
                                                                    inner(hops, fused, weights))[1]
    hist, hist_n = np.zeros((3, 16, 8)), np.zeros(3, np.int32)
    hops, nxt, first = {0: 0, 1: 0, 2: 0}, {0: 0, 1: 0, 2: 0}, {0: True, 1: True, 2: True}
    since = {0: 0, 1: 0, 2: 0}  # frames committed since the stream's (re)start
    after_reset = None
    for p in range(PUSHES):
        if p == RESET_AT:
            pool.reset(1)
            after_reset, nxt[1], first[1], since[1] = hops[1], 0, True, 0
        ids = [s for s in range(3) if s != 1 or p >= LATE]
        out = pool.push(torch.stack([seqs[s][nxt[s]] for s in ids]), streams=ids)
        for s in ids:
            nxt[s] += 1
        for sid, r in out:
            ref = mn.motion_fit(_np(r.fused_R)[None], _np(r.fused_T)[None], [int(first[sid])], [sid], hist, hist_n, 1)
            _equal_restatement(r, ref, f"push {p} stream {sid}")
            first[sid] = False
            since[sid] += 1
            assert int(r.motion_frames) == since[sid], (p, sid)  # (every fused pose of the golden run is finite)
            if sid == 1 and after_reset == hops[1]:  # the first hop after the reset: the history starts over
                assert int(r.motion_frames) == 1 and int(r.motion_state) == 0
            hops[sid] += 1
        if pool.motion_tracker.device is not None:
            assert _np(pool.motion_tracker.hist_n).tolist() == hist_n.tolist(), p
            assert (_np(pool.motion_tracker.hist).view(np.int64) == hist.view(np.int64)).all(), p
    assert hops == {0: PUSHES - T + 1, 1: (RESET_AT - LATE - T + 1) + (PUSHES - RESET_AT - T + 1), 2: PUSHES - T + 1}, hops
    assert after_reset is not None and hops[1] > after_reset
    assert since == {0: PUSHES - T + 1, 1: PUSHES - RESET_AT - T + 1, 2: PUSHES - T + 1}, "streams 0 and 2 went on"
    split = [o for o in launches if o != sorted(o)]
    assert split == [[1, 0, 2], [1, 0, 2]], launches  # once when stream 1 joins late, once after its reset


# ------------------------------------------------------------------------------------------------
# a body with a known spin
# ------------------------------------------------------------------------------------------------
GHW, FRAMES, RATIO = 16, 11, 0.5
FINTR = (268.44444444, 268.44444444, 320.0, 240.0)  # models.utils.INTRINSICS["AMD"], the fuser's
SPIN = 0.05 * np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])  # rad / frame
# tests/test_motion_cpu.py test_noise_is_averaged_down_by_the_line_fit prints the rms omega error of the fit at
# sigma = 0.02 rad over 16 frames: 1.046e-3 rad / frame
CPU_SPREAD = 1.046e-3


class _Scene:
    """The truth per frame: q[f] = Exp(SPIN f) q[0], (u, v, z) on a line."""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        q0 = fn.unit_pos(np.array([1.0, 0.0, 0.0, 0.0]) + 0.2 * rng.normal(size=4))
        self.q = np.array([fn.unit_pos(fn.qmul(mn.qexp(SPIN * f), q0)) for f in range(FRAMES)])
        self.x = np.array([320.0, 240.0, 3.0]) + np.arange(FRAMES)[:, None] * np.array([0.5, -0.25, 0.01])
        self.seed = seed

    def enc(self, f0):
        rng = np.random.default_rng(1000 * self.seed + f0)
        return fn.window_encoding(rng, self.q, self.x, f0, T, RATIO, 5e-4, 1e-3, 1e-4)

    def anchor(self):
        return (torch.tensor(self.q[0], dtype=torch.float32).cuda(), torch.tensor(self.x[0], dtype=torch.float32).cuda(),
                FINTR[0], torch.tensor([RATIO], dtype=torch.float64), "AMD")

    def frames(self):
        fr = torch.zeros(FRAMES, 3, GHW, GHW)
        fr[:, 0] = torch.arange(FRAMES, dtype=torch.float32)[:, None, None]  # every frame carries its index
        return fr.cuda()


class _GeoModel:
    """The stand-in for COMET: frame_stages keeps the frame, the window call reads the frames' tags and
    returns the true relative encoding plus seeded noise."""

    def __init__(self, scene):
        self.scene = scene

    def frame_stages(self, frames):
        from comet_amd.models.E2Epose2 import FrameCache
        return FrameCache(fmaps=None, refine_frames=frames[None], tokens=None)

    def forward_all(self, images, training=False, tracks=None, frame_cache=None, **extra):
        fr = frame_cache.refine_frames
        n = fr.shape[0]
        tags = fr[:, :, 0, 0, 0].cpu().numpy()
        enc = []
        for b in range(n):
            f0 = int(tags[b, 0])
            assert [int(v) for v in tags[b]] == list(range(f0, f0 + T)), tags[b]
            enc.append(self.scene.enc(f0))
        return {"pred_pose_enc": torch.tensor(np.concatenate(enc), dtype=torch.float32).cuda(),
                "pred_tracks": tracks.clone(), "_track_predictions": {"pred_score": torch.ones(n, T, tracks.shape[2], device="cuda")}}

    __call__ = forward_all


def test_a_known_spin_is_recovered_through_the_stream():
    """8 hops of stride 1 commit 8 frames; the pose head's noise is 5e-4 rad per hypothesis, 40 x below the
    CPU noise test's sigma, so the estimate lies well inside that test's measured spread of the truth."""
    from comet_amd.stream import PoseStream
    scene = _Scene(31)
    st = PoseStream(_GeoModel(scene), window=T, stride=1, anchor=scene.anchor(), fuse=True, precision=torch.float32,
                    motion=True)
    frames, pts = scene.frames(), torch.rand(8, 2, device="cuda") * (GHW - 1)
    res = []
    for f in range(FRAMES):
        res += st.push(frames[f], query_points=pts)
    assert len(res) == 8
    last = res[-1]
    assert int(last.motion_state) == 1 and int(last.motion_frames) == 8
    err = _np(last.motion_omega) - SPIN
    print(f"known spin: omega {_np(last.motion_omega)} against {SPIN}, error {np.abs(err).max():.3e} rad/frame, "
          f"rot_rms {float(last.motion_rot_rms):.3e}, innovation {_np(last.motion_innov_rot)}")
    assert np.abs(err).max() <= CPU_SPREAD
    assert fn.rot_angle(_np(last.motion_q0), scene.q[last.frame_index]) <= 0.01
    # the prediction one frame ahead is the next frame's truth to the same accuracy
    assert fn.rot_angle(_np(last.motion_pred_R[0]), scene.q[last.frame_index + 1]) <= 0.01
    assert bool(torch.isfinite(last.motion_vel).all()) and bool((last.motion_innov_rot < 0.01).all())
