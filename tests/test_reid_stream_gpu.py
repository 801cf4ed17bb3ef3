"""The landmark archive through PoseStream and StreamPool on the GPU, on geometry (DESIGN.md "Landmark
archive"), with the stand-in model of tests/test_pnp_stream_gpu.py: a perfect tracker on a rigid body. One body
point loses its score for a few frames, so its track dies by the carry's score test, and the detector offers
it again afterwards: the new track must get the old landmark and its identity back, and every archive field
must equal the restatement chained on the recorded outputs."""
import numpy as np
import pytest
import torch

import landmark_numpy as ln
import reid_numpy as rn
from test_landmark_gpu import model  # noqa: F401  (the golden model, a module-scoped fixture, for stream_eval)
from test_pnp_stream_gpu import FRAMES, HW, N, T, TRACK_INTR, _GeoModel, _Scene, _kw, _np

pytestmark = pytest.mark.gpu

HIDDEN, GONE = 3, range(5, 8)  # body point 3 scores 0 on the frames 5, 6, 7 and is no candidate there
C, REID_PX = 16, 4.0  # (the landmark is triangulated from noisy fused poses: it reprojects a pixel or two off)


class _HidingModel(_GeoModel):
    """The stand-in, with pred_score = 0 for the hidden point on the frames it is gone."""

    def __init__(self, scenes, gone=GONE):
        super().__init__(scenes)
        self.gone = gone

    def forward_all(self, images, training=False, tracks=None, frame_cache=None, **extra):
        out = super().forward_all(images, training, tracks, frame_cache, **extra)
        tags = frame_cache.refine_frames[:, :, :2, 0, 0].cpu().numpy()
        score = out["_track_predictions"]["pred_score"]
        for b in range(score.shape[0]):
            sc, f0 = self.scenes[int(tags[b, 0, 1])], int(tags[b, 0, 0])
            for i in range(T):
                if f0 + i in self.gone:
                    on = np.linalg.norm(_np(out["pred_tracks"][b, i]) - sc.px[f0 + i, HIDDEN], axis=-1) < 1e-3
                    score[b, i, torch.from_numpy(on).cuda()] = 0.0
        return out

    __call__ = forward_all


def _hiding_candidates(scenes, gone=GONE):
    def cand(frame):
        f, seq = int(frame[0, 0, 0]), int(frame[1, 0, 0])
        keep = [p for p in range(scenes[seq].px.shape[1]) if not (p == HIDDEN and f in gone)]
        return torch.tensor(scenes[seq].px[f][keep]).cuda()
    return cand


def _stream_kw(scenes, **kw):
    return _kw(scenes, pnp=False, pnp_huber_px=None, pnp_weight=0.0, candidate_fn=_hiding_candidates(scenes), **kw)


def _chain(results, what, intr=TRACK_INTR):
    """comet_landmark_reid and comet_landmark_update restated over one stream's recorded hops since its
    (re)start -> the restatement's archive state."""
    acc, acc_id = ln.new_state(1, N)
    st = rn.new_state(1, N, C)
    intr = np.array([intr])
    for k, r in enumerate(results):
        tr, R, Tx = _np(r.pred_tracks)[None], _np(r.fused_R)[None], _np(r.fused_T)[None]
        ids, src = _np(r.track_ids)[None], _np(r.track_src)[None]
        ro = rn.reid(tr, R, Tx, ids, src, [0], intr, acc, acc_id, st, C, REID_PX, 0.5, 2)
        lo = ln.update(tr, R, Tx, ids, ro["src_lm"], [0], intr, acc, acc_id, 1, min_obs=2)
        w = f"{what} hop {k}"
        assert np.array_equal(_np(r.landmark_ids), ro["lm_id"][0]) and np.array_equal(_np(r.reid_state), ro["reid_state"][0]), w
        assert _np(r.reid_dist).tobytes() == ro["reid_dist"][0].tobytes(), w
        assert np.array_equal(_np(r.landmark_state), lo["state"][0]) and np.array_equal(_np(r.landmark_obs), lo["n_obs"][0]), w
        assert (np.abs(_np(r.landmarks) - lo["X"][0]) <= 1e-10 * (1.0 + np.abs(lo["X"][0]))).all(), w
    return st


def _run(stream, frames, n=FRAMES):
    res = []
    for f in range(n):
        res += stream.push(frames[f])
    return res


def test_a_point_that_leaves_and_returns_gets_its_identity_back():
    from comet_amd.stream import PoseStream
    scenes = [_Scene(11)]
    st = PoseStream(_HidingModel(scenes), anchor=scenes[0].anchor(), track_intr=TRACK_INTR, lm_archive=C, reid_px=REID_PX,
                    **_stream_kw(scenes))
    res = _run(st, scenes[0].frames(0))
    assert len(res) == FRAMES - T + 1
    slot_of = lambda r: int(np.linalg.norm(_np(r.pred_tracks)[0] - scenes[0].px[r.frame_index, HIDDEN], axis=-1).argmin())  # noqa: E731
    j0 = slot_of(res[0])
    before = int(res[GONE[0] - 1].landmark_ids[j0])
    assert before == int(res[0].track_ids[j0]) >= 0
    back = [r for r in res if r.frame_index >= GONE[-1] + 1 and int((r.reid_state == 1).sum())]
    assert back, "no hop re-identified anything"
    r = back[0]
    j = int(torch.nonzero(r.reid_state == 1)[0])
    assert int(r.landmark_ids[j]) == before != int(r.track_ids[j]), "the new track carries the old landmark's identity"
    assert int(r.landmark_state[j]) == 1 and int(r.landmark_obs[j]) > 2, "valid at birth, with the archived frames"
    assert all(int(q.landmark_ids[j]) == before for q in res if q.frame_index > r.frame_index)
    ref = _chain(res, "stream")
    ids, X, n_obs = st.landmark_map.archive_snapshot(0)
    want = rn.snapshot(ref, 0, C)
    assert np.array_equal(_np(ids), want[0]) and np.array_equal(_np(n_obs), want[2]) and len(want[0]) > 0
    assert (np.abs(_np(X) - want[1]) <= 1e-10 * (1.0 + np.abs(want[1]))).all(), "X read back through archive_snapshot"
    # a pool of one stream equals the stream bit for bit
    from comet_amd.stream import StreamPool
    kw = _stream_kw(scenes)
    pool = StreamPool(_HidingModel(scenes), 1, anchors=[scenes[0].anchor()], track_intrs=[TRACK_INTR], lm_archive=C,
                      reid_px=REID_PX, **kw)
    frames, pres = scenes[0].frames(0), []
    for f in range(FRAMES):
        pres += [r for _, r in pool.push(frames[f][None])]
    assert len(pres) == len(res)
    for a, b in zip(res, pres):
        for name in ("fused_R", "fused_T", "landmarks", "landmark_state", "landmark_ids", "reid_state", "reid_dist", "track_ids"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_with_the_archive_off_nothing_changes():
    """lm_archive=0 against the keyword left out, with PnP and its feedback on: every field of every hop, the
    tuple's length and positions included, is bit-identical, and the archive fields stay None. (That the path
    without the keyword is the parent's is what the unchanged landmark, PnP and stream tests hold.)"""
    from comet_amd.stream import PoseStream, StreamResult
    scenes = [_Scene(11)]
    frames = scenes[0].frames(0)
    kw = _kw(scenes, candidate_fn=_hiding_candidates(scenes))
    a = _run(PoseStream(_HidingModel(scenes), anchor=scenes[0].anchor(), track_intr=TRACK_INTR, **kw), frames)
    b = _run(PoseStream(_HidingModel(scenes), anchor=scenes[0].anchor(), track_intr=TRACK_INTR, lm_archive=0, **kw), frames)
    attrs = ("track_ids", "track_age", "track_src", "track_warm", "landmarks", "landmark_obs", "landmark_err",
             "landmark_state", "pnp_R", "pnp_T", "pnp_inliers", "pnp_rms_px", "pnp_state")
    assert len(a) == len(b) == FRAMES - T + 1
    for x, y in zip(a, b):
        assert y.landmark_ids is None and y.reid_state is None and y.reid_dist is None
        assert len(x) == len(y) == len(StreamResult._fields) and x._fields == y._fields
        for name in StreamResult._fields + attrs:
            u, v = getattr(x, name), getattr(y, name)
            if torch.is_tensor(u):
                assert torch.is_tensor(v) and u.dtype == v.dtype and _np(u).tobytes() == _np(v).tobytes(), name
            else:
                assert u == v, name
        assert x.pnp_state is not None and x.track_age is not None


PUSHES, LATE, RESET_AT = FRAMES, 1, 12  # stream 1 joins one push late and is reset before push 12
SOON = range(5, 7)                      # the pool's point is gone on the frames 5, 6: it returns on hop 7


def test_pool_of_three_streams_out_of_phase_keeps_the_archives_apart():
    """Three streams with their own intrinsics, stream 1 one push late and reset mid-run (warm_iters splits the
    push in which its first hop falls together with later hops of the others into two model calls, whose rows
    are stacked out of stream order). Every stream's fields equal the restatement chained on its own recorded
    outputs since its (re)start, every run re-identifies its own returning point, and after the reset stream
    1's archive, cursor and aliases are those of a fresh stream while the others' live on."""
    from comet_amd.stream import StreamPool
    scenes = [_Scene(21), _Scene(22), _Scene(23)]
    intrs = [TRACK_INTR, (140.0, 160.0, 60.0, 66.0), (155.0, 150.0, 64.0, 63.0)]
    for sc, intr in zip(scenes, intrs):  # (each stream's tracks live in its own pixels)
        sc.px = np.stack([ln.project(sc.body, sc.q[f], sc.pose_T(f), intr)[0] for f in range(FRAMES)]).astype(np.float32)
        assert sc.px.min() > 2.0 and sc.px.max() < HW - 3.0
    kw = _kw(scenes, pnp=False, pnp_huber_px=None, pnp_weight=0.0, candidate_fn=_hiding_candidates(scenes, SOON),
             track_intrs=intrs, warm=True, warm_iters=2, lm_archive=C, reid_px=REID_PX)
    pool = StreamPool(_HidingModel(scenes, SOON), streams=3, anchors=[sc.anchor() for sc in scenes], **kw)
    launches, inner = [], pool._landmarks
    pool._landmarks = lambda order, results, co, later: (launches.append((list(order), len(later))),
                                                         inner(order, results, co, later))[1]
    seqs = [sc.frames(s) for s, sc in enumerate(scenes)]
    runs, nxt = {0: [[]], 1: [[]], 2: [[]]}, {0: 0, 1: 0, 2: 0}
    for p in range(PUSHES):
        if p == RESET_AT:
            assert pool.landmark_map.archive_snapshot(1)[0].numel() + int((pool.landmark_map.alias[N:2 * N] >= 0).sum()) > 0
            pool.reset(1)
            lm = pool.landmark_map
            assert lm.archive_snapshot(1)[0].numel() == 0 and int(lm.arch_cursor[1]) == 0 and (lm.alias[N:2 * N] == -1).all()
            assert lm.snapshot(1)[0].numel() == 0
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
    assert [o for o, calls in launches if calls == 2] == [[1, 0, 2], [1, 0, 2]], launches
    last = {}
    for sid in range(3):
        for k, seg in enumerate(runs[sid]):
            last[sid] = _chain(seg, f"stream {sid} run {k}", intrs[sid])
            matched = sum(int((r.reid_state == 1).sum()) for r in seg)
            if len(seg) > 5:
                assert matched >= 1, (sid, k, "the returning point was not re-identified")
    for sid in range(3):
        ids, X, n_obs = pool.landmark_map.archive_snapshot(sid)
        want = rn.snapshot(last[sid], 0, C)
        assert np.array_equal(_np(ids), want[0]) and np.array_equal(_np(n_obs), want[2]), sid
        assert (np.abs(_np(X) - want[1]) <= 1e-10 * (1.0 + np.abs(want[1]))).all(), sid
        assert int(pool.landmark_map.arch_cursor[sid]) == int(last[sid]["arch_cursor"][0])
        rows = slice(sid * N, (sid + 1) * N)
        assert np.array_equal(_np(pool.landmark_map.alias[rows]), last[sid]["alias"]), sid


def test_stream_eval_writes_the_archive_csv(model, tmp_path):  # noqa: F811
    """cfg.stream.lm_archive through stream_eval on the golden model (random weights: mechanics only): the hop
    CSV and the landmark CSV's header are what they are without it, no archive CSV is written with it off, and
    <stem>_archive.csv holds LandmarkMap.archive_snapshot of a PoseStream built by hand with the same settings
    on the same cropped frames."""
    import test_landmark_gpu as tl
    from comet_amd import loop
    from comet_amd.data import crop_intrinsics, crop_resize_normalize
    from comet_amd.models.utils import INTRINSICS
    from comet_amd.stream import PoseStream
    raw, box = tl._raw(3, tl.T + 6), (8, 0, 168, 160)
    on, off = str(tmp_path / "on.csv"), str(tmp_path / "off.csv")
    arch = dict(lm_archive=32, reid_px=3.0, lm_arch_min_obs=2)
    assert loop.stream_eval(model, iter(raw), tl._cfg(landmarks=True, lm_min_obs=2, **arch), box, on,
                            candidate_fn=tl._Candidates()) == 7
    assert loop.stream_eval(model, iter(raw), tl._cfg(landmarks=True, lm_min_obs=2), box, off, candidate_fn=tl._Candidates()) == 7
    assert loop.archive_csv(on) == str(tmp_path / "on_archive.csv") and not (tmp_path / "off_archive.csv").exists()
    rows_on, rows_off = tl._csv_rows(on), tl._csv_rows(off)
    assert len(rows_on) == len(rows_off) and tuple(rows_on[0].keys()) == tuple(rows_off[0].keys())
    with open(loop.landmarks_csv(on)) as f, open(loop.archive_csv(on)) as g:
        assert tuple(f.readline().strip().split(",")) == tuple(g.readline().strip().split(",")) == loop.LANDMARK_FIELDS
    fx, _, cx, cy = INTRINSICS["AMD"]
    intr = crop_intrinsics(INTRINSICS["AMD"], box, tl.HW)
    st = PoseStream(model, anchor=([1.0, 0.0, 0.0, 0.0], [cx, cy, 1.0], fx, 1.0, "AMD"),
                    **tl._kw(landmarks=True, track_intr=intr, lm_min_obs=2, **arch))
    for f in raw:
        st.push(crop_resize_normalize(torch.as_tensor(f)[None].cuda(), box, (tl.HW, tl.HW))[0])
    want = tl._snapshot_rows(st.landmark_map.archive_snapshot(0))
    got = tl._csv_rows(loop.archive_csv(on))
    print(f"stream_eval: {len(got)} archived landmarks, {len(tl._csv_rows(loop.landmarks_csv(on)))} live")
    assert got == want
    assert tl._csv_rows(loop.landmarks_csv(on)) == tl._snapshot_rows(st.landmark_map.snapshot(0))
