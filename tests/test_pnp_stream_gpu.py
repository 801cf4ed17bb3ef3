"""The PnP feedback through PoseStream and StreamPool on the GPU, on geometry (DESIGN.md "PnP refinement").

The golden configuration's random weights give tracks without geometry, so no position past 0 of a hop is
ever solved there and nothing would be injected. Here the model is replaced by a stand-in that returns what
a perfect tracker and a noisy pose head would: a rigid body of P points on a known trajectory, pred_tracks
= the exact projections (f32) of the body point each query sits on, pred_pose_enc = the true relative
encoding plus seeded noise, pred_score = 1. Every frame carries its index and its sequence in its pixels,
so the stand-in also checks that the rings hand it the right frames. Everything else is the real stream:
rings, comet_track_carry, comet_track_warm, comet_pose_fuse, comet_landmark_update, comet_landmark_pnp.

Reference, per stream: fuse_numpy.FuseRef on the recorded pred_pose_enc, landmark_numpy.update and
pnp_numpy.pnp on the recorded tracks and fused poses, the PnP restatement adding its poses to FuseRef's
accumulator. The PnP fields must equal the restatement (1e-10 relative, bit identity expected); the fused
poses of the later hops, which contain the injected hypotheses, must equal FuseRef's within the bounds of
tests/test_fuse_gpu.py (R 2^-22, T and (u, v, z) 1e-10 relative, counts equal)."""
import numpy as np
import pytest
import torch

import fuse_numpy as fn
import landmark_numpy as ln
import pnp_numpy as pn

pytestmark = pytest.mark.gpu

HW, N, T, P = 128, 64, 4, 40
TRACK_INTR = (150.0, 150.0, 63.5, 63.5)
FINTR = (268.44444444, 268.44444444, 320.0, 240.0)  # models.utils.INTRINSICS["AMD"], the fuser's
RATIO, HUBER, TOL, R_TOL = 0.5, 3.0, 1e-10, 2.0 ** -22
FRAMES = 16


class _Scene:
    """One sequence: the truth (q, (u, v, z)) per frame, the body, its exact pixels per frame."""

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        q = [fn.unit_pos(np.array([1.0, 0.0, 0.0, 0.0]) + 0.2 * rng.normal(size=4))]
        x = [np.array([320.0, 240.0, 3.0]) + rng.normal(size=3) * np.array([3.0, 3.0, 0.05])]
        for _ in range(FRAMES - 1):
            q.append(fn.unit_pos(fn.qmul(fn.axis_angle_quat(rng.normal(size=3), 0.06), q[-1])))
            x.append(x[-1] + rng.normal(size=3) * np.array([1.0, 1.0, 0.01]))
        self.seed, self.q, self.x = seed, np.array(q), np.array(x)
        self.body = rng.uniform(-0.8, 0.8, (P, 3))
        self.px = np.stack([ln.project(self.body, self.q[f], self.pose_T(f), TRACK_INTR)[0] for f in range(FRAMES)]).astype(np.float32)
        assert self.px.min() > 2.0 and self.px.max() < HW - 3.0

    def pose_T(self, f):
        u, v, z = self.x[f]
        return np.array([(u - FINTR[2]) * z / FINTR[0], (v - FINTR[3]) * z / FINTR[1], z])

    def enc(self, f0):
        rng = np.random.default_rng(1000 * self.seed + f0)
        return fn.window_encoding(rng, self.q, self.x, f0, T, RATIO, 0.01, 0.01, 0.002)

    def anchor(self):
        return (torch.tensor(self.q[0], dtype=torch.float32).cuda(), torch.tensor(self.x[0], dtype=torch.float32).cuda(),
                FINTR[0], torch.tensor([RATIO], dtype=torch.float64), "AMD")

    def anchor7(self):
        return np.concatenate([self.q[0].astype(np.float32), self.x[0].astype(np.float32)]).astype(np.float64)

    def frames(self, seq):
        fr = torch.zeros(FRAMES, 3, HW, HW)
        fr[:, 0] = torch.arange(FRAMES, dtype=torch.float32)[:, None, None]
        fr[:, 1] = float(seq)
        return fr.cuda()


class _GeoModel:
    """The stand-in for COMET: frame_stages keeps the frame, the window call reads the frames' tags."""
    cfg = {"track_trainit": 4}

    class track_predictor:
        coarse_down_ratio = 1

    def __init__(self, scenes):
        self.scenes, self.calls = scenes, []

    def frame_stages(self, frames):
        from comet_amd.models.E2Epose2 import FrameCache
        return FrameCache(fmaps=None, refine_frames=frames[None], tokens=None)

    def forward_all(self, images, training=False, tracks=None, frame_cache=None, **extra):
        fr = frame_cache.refine_frames
        n = fr.shape[0]
        tags = fr[:, :, :2, 0, 0].cpu().numpy()
        query = tracks[:, 0].cpu().numpy()
        enc, out = [], np.zeros((n, T, N, 2), np.float32)
        for b in range(n):
            seq, f0 = int(tags[b, 0, 1]), int(tags[b, 0, 0])
            assert [int(v) for v in tags[b, :, 0]] == list(range(f0, f0 + T)) and (tags[b, :, 1] == seq).all(), tags[b]
            sc = self.scenes[seq]
            d = np.linalg.norm(query[b][:, None] - sc.px[f0][None], axis=-1)
            idx = d.argmin(-1)
            assert d.min(-1).max() < 1e-3, "a query that sits on no body point"
            out[b] = sc.px[f0:f0 + T][:, idx]
            enc.append(sc.enc(f0))
        self.calls.append((n, extra.get("track_iters")))
        return {"pred_pose_enc": torch.tensor(np.concatenate(enc)).cuda(), "pred_tracks": torch.tensor(out).cuda(),
                "_track_predictions": {"pred_score": torch.ones(n, T, N, device="cuda")}}

    __call__ = forward_all


def _candidates(scenes):
    def cand(frame):
        f, seq = int(frame[0, 0, 0]), int(frame[1, 0, 0])
        return torch.tensor(scenes[seq].px[f]).cuda()
    return cand


def _kw(scenes, **kw):
    return dict(dict(window=T, stride=1, carry=True, carry_tracks=N, carry_cell=8, carry_border=0, carry_min_score=0.5,
                     candidate_fn=_candidates(scenes), fuse=True, precision=torch.float32, landmarks=True, lm_min_obs=2,
                     pnp=True, pnp_huber_px=HUBER, pnp_weight=1.0), **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _rel(a, b):
    return float((np.abs(a - b) / (1.0 + np.abs(b))).max()) if a.size else 0.0


def _chain(results, scene, intr, what):
    """The restatement chain of fuse, landmark and PnP over one stream's hops since its (re)start ->
    (hypotheses injected, hops whose fused poses contained an injected hypothesis)."""
    ref = fn.FuseRef(T, RATIO, FINTR)
    acc, acc_id = ln.new_state(1, N)
    injected, carried, has = 0, 0, set()
    for k, r in enumerate(results):
        f0 = r.frame_index
        assert f0 == k
        slots = [(f0 + i) % T for i in range(T)]
        out = ref.fuse(_np(r.pred_pose_enc)[None], slots, [1 if k == 0 else T - 1], [int(k == 0)], [scene.anchor7()])
        w = f"{what} hop {k}"
        assert (np.abs(_np(r.fused_R).astype(np.float64) - out["R"][0].astype(np.float64)).max() <= R_TOL), (w, "fused_R")
        assert _rel(_np(r.fused_T), out["T"][0]) <= TOL, (w, "fused_T", _rel(_np(r.fused_T), out["T"][0]))
        assert (_np(r.fused_count) == out["count"][0]).all(), (w, _np(r.fused_count), out["count"][0])
        carried += int(any(f0 + i in has for i in range(T)))
        tr, R, Tx = _np(r.pred_tracks)[None], _np(r.fused_R)[None], _np(r.fused_T)[None]
        lo = ln.update(tr, R, Tx, _np(r.track_ids)[None], _np(r.track_src)[None], [0], np.array([intr]), acc, acc_id, 1,
                       min_obs=2)
        assert (_np(r.landmark_state) == lo["state"][0]).all() and _rel(_np(r.landmarks), lo["X"][0]) <= TOL, w
        po = pn.pnp(tr, _np(r.landmarks)[None], _np(r.landmark_state)[None], R, Tx, np.array([intr]), 1, HUBER, fuse_acc=ref.acc, slots=slots, inject_w=1.0,
                    fuse_intr=FINTR)
        assert (_np(r.pnp_state) == po["state"][0]).all() and (_np(r.pnp_inliers) == po["n_in"][0]).all(), (w, po["state"])
        assert _rel(_np(r.pnp_T), po["t"][0]) <= TOL and _np(r.pnp_R).tobytes() == po["R"][0].tobytes(), w
        assert _np(r.pnp_rms_px).tobytes() == po["rms_px"][0].tobytes(), w
        for i in range(1, T):
            if po["state"][0, i] == 1:
                injected += 1
                has.add(f0 + i)
    return injected, carried


def test_stream_with_feedback_equals_the_restatement_chain():
    scenes = [_Scene(11)]
    from comet_amd.stream import PoseStream
    model = _GeoModel(scenes)
    st = PoseStream(model, anchor=scenes[0].anchor(), track_intr=TRACK_INTR, **_kw(scenes))
    off = PoseStream(model, anchor=scenes[0].anchor(), track_intr=TRACK_INTR, **_kw(scenes, pnp_weight=0.0))
    frames = scenes[0].frames(0)
    res, base = [], []
    for f in range(T + 7):
        res += st.push(frames[f])
        base += off.push(frames[f])
    assert len(res) == len(base) == 8
    injected, carried = _chain(res, scenes[0], TRACK_INTR, "stream")
    solved = [int((r.pnp_state == 1).sum()) for r in res]
    print(f"stream: solved positions per hop {solved}, {injected} hypotheses injected, {carried} hops fused with one")
    assert injected >= 6 and carried >= 3, "the feedback would show nothing"
    # the first hop is the run's without the feedback; a later one is not
    for name in ("pred_pose_enc", "fused_R", "fused_T", "fused_count", "pnp_R", "pnp_T", "pnp_state"):
        assert torch.equal(getattr(res[0], name), getattr(base[0], name)), name
    assert not torch.equal(res[-1].fused_T, base[-1].fused_T) and int(res[-1].fused_count[0]) > int(base[-1].fused_count[0])


PUSHES, LATE, RESET_AT = 11, 1, 6  # stream 1 joins one push late and is reset before push 6


def test_pool_of_three_streams_out_of_phase_with_a_split_push():
    """warm_iters differs from the config's iterations, so a push in which stream 1's first hop falls
    together with later hops of streams 0 and 2 runs two model calls; their rows are stacked in the order
    [1, 0, 2] for the fuse, landmark and PnP launches, and the injected rows follow that order."""
    from comet_amd.stream import StreamPool
    scenes = [_Scene(21), _Scene(22), _Scene(23)]
    intrs = [TRACK_INTR, (140.0, 160.0, 60.0, 66.0), (155.0, 150.0, 64.0, 63.0)]
    for sc, intr in zip(scenes, intrs):  # (each stream's tracks live in its own pixels)
        sc.px = np.stack([ln.project(sc.body, sc.q[f], sc.pose_T(f), intr)[0] for f in range(FRAMES)]).astype(np.float32)
        assert sc.px.min() > 2.0 and sc.px.max() < HW - 3.0
    model = _GeoModel(scenes)
    pool = StreamPool(model, streams=3, anchors=[sc.anchor() for sc in scenes],
                      **_kw(scenes, track_intrs=intrs, warm=True, warm_iters=2))
    launches, inner = [], pool._landmarks
    pool._landmarks = lambda order, results, co, later: (launches.append((list(order), len(later))),
                                                         inner(order, results, co, later))[1]
    seqs = [sc.frames(s) for s, sc in enumerate(scenes)]
    runs = {0: [[]], 1: [[]], 2: [[]]}
    nxt = {0: 0, 1: 0, 2: 0}
    for p in range(PUSHES):
        if p == RESET_AT:
            pool.reset(1)
            runs[1].append([])
            nxt[1] = 0
        ids = [s for s in range(3) if s != 1 or p >= LATE]
        out = pool.push(torch.stack([seqs[s][nxt[s]] for s in ids]), streams=ids)
        for s in ids:
            nxt[s] += 1
        for sid, r in out:
            runs[sid][-1].append(r)
    assert [len(v) for v in runs[0]] == [PUSHES - T + 1] and [len(v) for v in runs[2]] == [PUSHES - T + 1]
    assert [len(v) for v in runs[1]] == [RESET_AT - LATE - T + 1, PUSHES - RESET_AT - T + 1]
    split = [o for o, calls in launches if calls == 2]
    assert split == [[1, 0, 2], [1, 0, 2]], launches
    assert all(o == sorted(o) for o, calls in launches if calls == 1)
    assert (1, None) in model.calls and (2, 2) in model.calls, model.calls  # first hops cold, later hops at warm_iters
    total = {}
    for sid in range(3):
        for k, seg in enumerate(runs[sid]):
            total[(sid, k)] = _chain(seg, scenes[sid], intrs[sid], f"stream {sid} run {k}")
    print(f"pool: (hypotheses injected, hops fused with one) per stream and run {total}")
    assert total[(0, 0)][0] >= 6 and total[(0, 0)][1] >= 3 and total[(2, 0)][0] >= 6 and total[(2, 0)][1] >= 3
