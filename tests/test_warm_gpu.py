"""Warm start of the coarse tracker on the GPU (comet_track_warm in csrc/warm.hip, ops.track_warm,
BaseTrackerPredictor coords_init, COMET track_init / track_iters, PoseStream / StreamPool warm=True,
loop.stream_eval; DESIGN.md "Warm start").

Kernel: every output is a copy of an input or f32 arithmetic both sides evaluate alike, so the kernel
must equal the numpy restatement tests/warm_numpy.py exactly, coordinates compared as bits.

End to end: the golden configuration of tests/test_carry_gpu.py (PRNG weights seed 0, T = 4, 128^2,
N = 64, its fixed seeded candidates, MIN_SCORE 0.5, oracle.prng frames of seed 1)."""
import copy

import numpy as np
import pytest
import torch

import carry_numpy as cn
import warm_numpy as wn

pytestmark = pytest.mark.gpu

INT32_MIN = cn.INT32_MIN


def _dev(a):
    return torch.as_tensor(a).cuda().contiguous()


def _gpu(prev, src, query, prev_valid, s, H, W, mode, div0, div1):
    from comet_amd import ops
    out = ops.track_warm(_dev(prev), _dev(src), _dev(query), _dev(prev_valid), s, H, W, mode, div0, div1)
    torch.cuda.synchronize()
    return out.coords.cpu().numpy(), out.warm.cpu().numpy()


def _both(prev, src, query, prev_valid, s, H, W, mode, div0, div1, what=""):
    ref = wn.warm(prev, src, query, prev_valid, s, H, W, mode, div0, div1)
    got = _gpu(prev, src, query, prev_valid, s, H, W, mode, div0, div1)
    for name, a, b in (("coords", got[0], ref[0]), ("warm", got[1], ref[1])):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        if name == "coords":
            a, b = a.view(np.int32), b.view(np.int32)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{what} {name}: {len(bad)} differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}"
    return ref


# ------------------------------------------------------------------------------------------------
# case a: every branch, by construction
# ------------------------------------------------------------------------------------------------
def _case_a():
    """Two hops, T = 4, N = 64, s = 1, a 128 x 96 frame (W != H, so a swapped clamp shows). Hop 0: slot 0
    carried. Hop 1: slot 0 born, so its lattice pad stays cold."""
    n, T, N, H, W = 2, 4, 64, 96, 128
    rng = np.random.default_rng(21)
    prev = (rng.random((n, T, N, 2)) * np.array([W - 1, H - 1])).astype(np.float32)
    src = np.tile(np.arange(N, dtype=np.int32), (n, 1))  # carried unless set below
    slots = dict(birth=1, pad_of_carried_0=2, pad_of_born=3, pad_of_carried_7=4, src_is_N=8, src_large=9,
                 pad_index_N=10, below_births=11, pad_index_large=12, nan_used=13, inf_used=14, nan_unused=15,
                 clamp_x_hi=16, clamp_x_lo=17, clamp_y_hi=18, clamp_y_lo=19, other_donor=20, pad_of_nan=21)
    src[0, 1] = -1 - 5
    src[0, 2] = INT32_MIN + 0
    src[0, 3] = INT32_MIN + 1
    src[0, 4] = INT32_MIN + 7
    src[0, 8], src[0, 9], src[0, 10], src[0, 11], src[0, 12] = N, 1000, INT32_MIN + N, -5000, INT32_MIN + 5000
    prev[0, 3, 13, 0] = np.nan    # the last row
    prev[0, 2, 14, 1] = np.inf    # row 1 + s: frame 1 of the new window
    prev[0, 0, 15, :] = np.nan    # row 0 < s: not used
    prev[0, 2:, 16] = [(100, 50), (120, 50)]   # x: 120 + 20 = 140 > 127
    prev[0, 2:, 17] = [(20, 50), (5, 50)]      # x: 5 - 15 = -10 < 0
    prev[0, 2:, 18] = [(50, 70), (50, 90)]     # y: 90 + 20 = 110 > 95
    prev[0, 2:, 19] = [(50, 30), (50, 10)]     # y: 10 - 20 = -10 < 0
    src[0, 20] = 7
    src[0, 21] = INT32_MIN + 13
    src[1, 0] = -1 - 2
    src[1, 5] = INT32_MIN  # the lattice pad: slot 0 is not carried
    src[1, 6] = INT32_MIN + 9
    query = (rng.random((n, N, 2)) * np.array([W - 1, H - 1])).astype(np.float32)
    for b in range(n):  # carried slots and pad copies have the query comet_track_carry gives them
        for j in range(N):
            k = wn.donor(src[b], j, N, 1)[0]
            if k is not None:
                query[b, j] = prev[b, 1, k]
    query[0, 13], query[0, 14], query[0, 21] = (3, 4), (5, 6), (3, 4)
    return dict(prev=prev, src=src, query=query, prev_valid=np.ones(n, np.int32), s=1, H=H, W=W), slots


@pytest.mark.parametrize("mode", [wn.HOLD, wn.VELOCITY])
def test_case_a_every_branch(mode):
    inp, sl = _case_a()
    coords, warm = _both(**inp, mode=mode, div0=2.0, div1=4.0, what=f"case a mode {mode}")
    px = coords * np.float32(8)
    prev, query = inp["prev"], inp["query"]
    w0 = warm[0]
    assert w0[0] == 1 and w0[7] == 1, "a carried slot"
    assert (px[0, 0, 1:3] == prev[0, 2:4, 0]).all() and (px[0, 0, 0] == query[0, 0]).all()
    assert w0[sl["birth"]] == 0 and (px[0, 1] == query[0, 1]).all(), "a birth"
    assert w0[sl["pad_of_carried_0"]] == 2 and (px[0, 2, 1:] == px[0, 0, 1:]).all(), "INT32_MIN + 0, slot 0 carried"
    assert w0[sl["pad_of_carried_7"]] == 2 and (px[0, 4, 1:] == px[0, 7, 1:]).all(), "a pad of a carried slot"
    assert w0[sl["pad_of_born"]] == 0 and (px[0, 3] == query[0, 3]).all(), "a pad of a born slot"
    assert warm[1, 0] == 0 and warm[1, 5] == 0 and (px[1, 5] == query[1, 5]).all(), "the lattice pad, slot 0 not carried"
    assert warm[1, 6] == 2
    for name in ("src_is_N", "src_large", "pad_index_N", "below_births", "pad_index_large"):
        assert w0[sl[name]] == 0 and (px[0, sl[name]] == query[0, sl[name]]).all(), name
    for name in ("nan_used", "inf_used", "pad_of_nan"):
        assert w0[sl[name]] == -1 and (px[0, sl[name]] == query[0, sl[name]]).all(), name
    assert w0[sl["nan_unused"]] == 1 and np.isfinite(coords).all(), "a NaN in a row that is not used"
    assert w0[sl["other_donor"]] == 1 and (px[0, 20, 1:] == px[0, 7, 1:]).all()
    clamps = (("clamp_x_hi", 0, 127.0, 120.0), ("clamp_x_lo", 0, 0.0, 5.0), ("clamp_y_hi", 1, 95.0, 90.0),
              ("clamp_y_lo", 1, 0.0, 10.0))
    for name, axis, clamped, last in clamps:
        assert w0[sl[name]] == 1 and px[0, sl[name], 3, axis] == (clamped if mode == wn.VELOCITY else last), name
        assert px[0, sl[name], 3, 1 - axis] == 50.0
    assert sorted(set(warm.ravel().tolist())) == [-1, 0, 1, 2]


# ------------------------------------------------------------------------------------------------
# case b: shapes, strides, modes, units
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T,N", [(1, 4, 64), (3, 5, 70), (1, 2, 1), (2, 4, 300)])
def test_case_b_shapes_strides_modes_and_units(n, T, N):
    """src and query come from the restatement of comet_track_carry on random tracks (16-px cells: carried
    slots, births and both kinds of pads), some tracks leave the frame (the clamp), some values are not
    finite. (3, 5, 70): hop 1 has prev_valid = 0 over a NaN-filled prev."""
    HW = 128
    for s in sorted({1, 2, T - 1} & set(range(1, T))):
        inp = cn.random_inputs(30 + s, n, T, N, 96, HW, HW, s=s)
        out = cn.carry(**inp, cell=16, border=0, min_score=0.3)
        prev, valid = inp["tracks"].copy(), inp["prev_valid"].copy()
        rng = np.random.default_rng(s)
        for _ in range(max(1, N // 16)):  # a few values that are not finite, anywhere
            prev[rng.integers(n), rng.integers(T), rng.integers(N), rng.integers(2)] = (np.nan, np.inf, -np.inf)[rng.integers(3)]
        if n == 3:
            valid[1] = 0
            prev[1] = np.nan
        if N == 1:  # one slot: carried, on a track that leaves the frame
            out["src"][:] = 0
            prev[0, :, 0] = [(100 + 20 * t, 5 - 4 * t) for t in range(T)]
        for mode in (wn.HOLD, wn.VELOCITY):
            for div in ((2.0, 4.0), (1.0, 1.0)):
                what = f"case b n={n} T={T} N={N} s={s} mode={mode} div={div}"
                coords, warm = _both(prev, out["src"], out["query"], valid, s, HW, HW, mode, *div, what=what)
                if N >= 64:
                    assert (warm == 1).any() and (warm == 0).any() and (warm == 2).any(), what
                if n == 3:
                    assert (warm[1] == 0).all() and np.isfinite(coords[1]).all()
                if N == 1:
                    assert warm[0, 0] == 1
                    if mode == wn.VELOCITY:
                        assert coords[0, 0, T - 1, 0] == np.float32(127) / np.float32(div[0]) / np.float32(div[1])
                        assert coords[0, 0, T - 1, 1] == 0


def test_track_warm_wrapper_rejects_bad_arguments():
    from comet_amd import _lib, ops
    inp, _ = _case_a()
    t = {k: _dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}

    def call(**kw):
        a = dict(dict(t, mode="hold", div0=2.0, div1=4.0), **kw)
        return ops.track_warm(a["prev"], a["src"], a["query"], a["prev_valid"], 1, 96, 128, a["mode"], a["div0"], a["div1"])
    for bad in (dict(prev=t["prev"].double()), dict(prev=t["prev"][..., :1]), dict(src=t["src"].long()),
                dict(src=t["src"][:, ::2]), dict(query=t["query"][:, :5]), dict(prev_valid=t["prev_valid"][:1]),
                dict(prev=t["prev"].cpu()), dict(mode=2), dict(div0=0.0), dict(div1=float("nan"))):
        with pytest.raises(_lib.CometHipError):
            call(**bad)
    out = call(mode="velocity")
    assert out.coords.shape == (2, 64, 4, 2) and out.warm.shape == (2, 64) and out.warm.dtype == torch.int32


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
T, HW, N = 4, 128, 64
SEED_W, SEED_X, SEEDS = 0, 1, (4, 2)
MIN_SCORE = 0.5
CAND_SEED, CAND_M = 7, 96
FACTOR = 4.0


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


def _carry_kw(**kw):
    return dict(dict(window=T, stride=1, carry=True, carry_tracks=N, carry_cell=8, carry_border=0,
                     carry_min_score=MIN_SCORE, candidate_fn=_Candidates()), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Coarse:
    """Records, for every call of the model's coarse predictor while active, its keyword arguments
    (iters, query_points, whether coords_init was given) and its last coarse prediction [B, T, N, 2]."""

    def __init__(self, model):
        self.pred, self.calls = model.track_predictor.coarse_predictor, []

    def __enter__(self):
        def before(mod, args, kw):
            assert not args
            self.calls.append(dict(iters=kw["iters"], query=kw["query_points"].clone(),
                                   init=None if kw.get("coords_init") is None else kw["coords_init"].clone()))

        def after(mod, args, out):
            self.calls[-1]["coarse"] = out[0][-1].clone()
        self.handles = [self.pred.register_forward_pre_hook(before, with_kwargs=True),
                        self.pred.register_forward_hook(after)]
        return self

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_predictor_with_the_broadcast_query_as_coords_init_equals_the_predictor_without(model, dtype):
    from comet_amd import functional as F
    tp = model.track_predictor
    frames = _frames(SEED_X, T)
    q = _Candidates().points[:N][None].contiguous()
    with F.precision(dtype), torch.no_grad():
        fmaps = tp.process_images_to_fmaps(frames[None], training=True)
        kw = dict(query_points=q, fmaps=fmaps, iters=2, down_ratio=tp.coarse_down_ratio, return_feat=True)
        base = tp.coarse_predictor(**kw)
        init = (q.reshape(1, N, 1, 2).repeat(1, 1, T, 1) / float(tp.coarse_down_ratio)
                / float(tp.coarse_predictor.stride)).contiguous()
        got = tp.coarse_predictor(**kw, coords_init=init)
        with pytest.raises(ValueError, match="coords_init"):
            tp.coarse_predictor(**kw, coords_init=init[:, :, :2])
    assert len(base[0]) == len(got[0]) == 2
    for a, b in zip(base[0], got[0]):
        assert torch.equal(a, b)
    for k in (1, 2, 3):
        assert torch.equal(base[k], got[k]), k
    assert base[4] is None and got[4] is None
    assert not torch.equal(base[0][-1][:, 1], base[0][-1][:, 0]), "the iterations moved nothing"


def _zero_flow(model):
    m = copy.deepcopy(model)
    head = m.track_predictor.coarse_predictor.updateformer.flow_head
    with torch.no_grad():
        head.weight.zero_()
        head.bias.zero_()
    return m


@pytest.fixture(scope="module")
def still_model(model):
    """The model with the coarse update former's flow head zeroed: the coarse iterations move nothing, so
    the coarse prediction is where the iterations started."""
    return _zero_flow(model)


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("mode", ["hold", "velocity"])
def test_zeroed_flow_head_shows_where_the_coarse_tracker_starts(still_model, s, mode):
    from comet_amd.stream import PoseStream
    m = still_model
    count = T + 3 * s
    frames = _frames(SEED_X, count)

    def run(**kw):
        st = PoseStream(m, precision=torch.float32, **_carry_kw(stride=s, **kw))
        res = []
        with _Coarse(m) as rec:
            for f in range(count):
                res += st.push(frames[f])
        assert len(res) == len(rec.calls) == 4
        return res, rec.calls

    res, calls = run(warm=True, warm_mode=mode)
    assert calls[0]["init"] is None and bool((res[0].track_warm == 0).all())
    coarse0 = calls[0]["coarse"][0]
    assert torch.equal(_bits(coarse0), _bits(coarse0[:1].expand(T, N, 2))), "the zeroed flow head moved a track"
    warm_total, moved = 0, False
    for k in (1, 2, 3):
        r, prev, c = res[k], res[k - 1], calls[k]
        coarse, query = c["coarse"][0], c["query"][0]  # [T, N, 2], [N, 2]
        assert c["init"] is not None and r.track_warm.shape == (N,) and r.track_warm.dtype == torch.int32
        w = r.track_warm
        n_warm = int((w == 1).sum())
        print(f"s={s} {mode} hop {k}: warm codes " + str({v: int((w == v).sum()) for v in (-1, 0, 1, 2)}))
        assert 1 <= n_warm <= N - 1, f"hop {k}: {n_warm} of {N} slots carried warm: the test would be vacuous"
        warm_total += n_warm
        assert torch.equal(w == 1, r.track_src == torch.arange(N, device="cuda", dtype=torch.int32))
        on = w == 1
        for i in range(T - s):  # the overlap: what the previous window refined, shifted by the stride
            assert torch.equal(_bits(coarse[i][on]), _bits(prev.pred_tracks[i + s][on])), (k, i)
        ref_c, ref_w = wn.warm(prev.pred_tracks.cpu().numpy()[None], r.track_src.cpu().numpy()[None],
                               query.cpu().numpy()[None], np.ones(1, np.int32), s, HW, HW, wn.HOLD if mode == "hold"
                               else wn.VELOCITY, 2.0, 4.0)
        assert (w.cpu().numpy() == ref_w[0]).all()
        ref_px = np.ascontiguousarray((ref_c[0] * np.float32(8)).transpose(1, 0, 2))  # [T, N, 2] pixels
        assert (_bits(coarse).cpu().numpy() == ref_px.view(np.int32)).all(), f"hop {k}: the coarse tracks"
        cold = w == 0
        assert torch.equal(_bits(coarse[:, cold]), _bits(query[cold][None].expand(T, -1, 2)))
        moved = moved or not torch.equal(coarse[1:, on], coarse[:1, on].expand(T - 1, -1, 2))
    assert moved, "no warm slot started anywhere but on its query point"
    assert 1 <= warm_total <= 3 * (N - 1)
    if mode == "hold":  # the same stream cold: every slot on its query in every frame
        res_c, calls_c = run()
        for k in range(4):
            coarse = calls_c[k]["coarse"][0]
            assert calls_c[k]["init"] is None and res_c[k].track_warm is None
            assert torch.equal(_bits(coarse), _bits(calls_c[k]["query"][0][None].expand(T, N, 2)))


def test_real_weights_first_hop_cold_later_hops_warm_with_fewer_iterations(model):
    from comet_amd.stream import PoseStream
    frames = _frames(SEED_X, 8)
    config_iters = int(model.cfg["track_trainit"])
    assert config_iters != 2

    def run(**kw):
        st = PoseStream(model, precision=torch.float32, **_carry_kw(**kw))
        res = []
        with _Coarse(model) as rec:
            for f in range(8):
                res += st.push(frames[f])
        return res, [c["iters"] for c in rec.calls]

    cold, cold_iters = run()
    warm, warm_iters = run(warm=True, warm_iters=2)
    assert len(cold) == len(warm) == 5
    assert cold_iters == [config_iters] * 5 and warm_iters == [config_iters, 2, 2, 2, 2]
    assert torch.equal(warm[0].pred_tracks, cold[0].pred_tracks) and torch.equal(warm[0].track_ids, cold[0].track_ids)
    differs = []
    for k, (w, c) in enumerate(zip(warm, cold)):
        d = float((w.pred_tracks - c.pred_tracks).abs().max()) if torch.equal(w.track_src, c.track_src) else float("nan")
        print(f"hop {k}: warm {int((w.track_warm > 0).sum())} slots, pred_tracks differ by {d:.3e} px, "
              f"pred_pose_enc by {float((w.pred_pose_enc - c.pred_pose_enc).abs().max()):.3e}")
        for t in (w.pred_tracks, w.pred_score.float(), w.pred_pose_enc):
            assert bool(torch.isfinite(t).all()), k
        differs.append(not torch.equal(w.pred_tracks, c.pred_tracks))
    assert not differs[0] and any(differs[1:]), "the warm start changed no later hop"
    assert bool((warm[0].track_warm == 0).all()) and any(bool((w.track_warm == 1).any()) for w in warm[1:])


PUSHES, LATE, RESET_AT = 10, 1, 6  # stream 1 joins one push late and is reset before push 6


def _pool_frame(s, p):
    return p - LATE if s == 1 and p >= LATE else (p if s == 0 else None)


class _Queries:
    """Records the query points (tracks[:, 0]) of every model.forward_all call while active."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __enter__(self):
        orig = self.model.forward_all

        def recorded(*a, **kw):
            self.seen.append((kw["tracks"][:, 0].clone(), kw.get("track_iters")))
            return orig(*a, **kw)
        self.model.forward_all = recorded
        return self

    def __exit__(self, *exc):
        del self.model.forward_all  # the instance attribute; the class's method is back


def test_pool_out_of_phase_equals_separate_streams_warm(model):
    """The schedule of tests/test_carry_gpu.py's pool test with warm=True, warm_iters=2, bf16: stream 1's
    first hops (pushes 4 and, after its reset, 9) fall together with later hops of stream 0, which run 2
    coarse iterations, so those pushes are two batched calls; push 5 is one call of two later hops.
    Identities, warm codes and queries: equality. pred_pose_enc: within 4 x floor, the floor measured as
    that test measures it (forward_all on the closed windows of the hops due in one push, stacked as one
    B = 2 batch against each window alone, with the queries the separate streams used)."""
    from comet_amd import functional as F
    from comet_amd.stream import PoseStream, StreamPool
    dtype = torch.bfloat16
    seqs = [_frames(seed, PUSHES) for seed in SEEDS]
    kw = dict(warm=True, warm_iters=2)
    singles = [PoseStream(model, precision=dtype, **_carry_kw(**kw)) for _ in range(2)]
    pool = StreamPool(model, streams=2, precision=dtype, **_carry_kw(**kw))
    alone, got, base = {}, {}, {0: 0, 1: 0}
    q_alone, q_got, pool_calls = {}, {}, {}
    for p in range(PUSHES):
        if p == RESET_AT:
            singles[1].reset()
            pool.reset(1)
            base[1] = _pool_frame(1, p)
        ids = [s for s in range(2) if _pool_frame(s, p) is not None]
        for s in ids:
            with _Queries(model) as rec:
                for r in singles[s].push(seqs[s][_pool_frame(s, p)]):
                    alone[(p, s)], q_alone[(p, s)] = r, rec.seen[0][0][0]
        with _Queries(model) as rec:
            out = pool.push(torch.stack([seqs[s][_pool_frame(s, p)] for s in ids]), streams=ids)
            rows = [q for qs, _ in rec.seen for q in qs]
            pool_calls[p] = [(qs.shape[0], it) for qs, it in rec.seen]
            assert [s for s, _ in out] == sorted(s for s, _ in out)
            # (two calls: first hops, then later hops; stream 1's first hop comes first then)
            order = [s for s, _ in out] if len(rec.seen) < 2 else [1, 0]
            for s, r in out:
                got[(p, s)], q_got[(p, s)] = r, rows[order.index(s)]
    assert sorted(got) == sorted(alone) and len(got) == 7 + 2 + 1, sorted(got)
    assert pool_calls[4] == [(1, None), (1, 2)] and pool_calls[9] == [(1, None), (1, 2)], pool_calls
    assert pool_calls[5] == [(2, 2)] and pool_calls[3] == [(1, None)] and pool_calls[6] == [(1, 2)], pool_calls
    floor = 0.0
    for p in range(PUSHES):
        due = [s for s in range(2) if (p, s) in alone]
        if len(due) < 2:
            continue
        wins = [seqs[s][base[s] + alone[(p, s)].frame_index:][:T] for s in due]
        trk = [q_alone[(p, s)][None].expand(T, -1, 2) for s in due]
        with F.precision(dtype), torch.no_grad():
            ob = model.forward_all(torch.stack(wins), training=False, tracks=torch.stack(trk))
            for b, (w, t) in enumerate(zip(wins, trk)):
                o1 = model(w[None], training=False, tracks=t[None])
                floor = max(floor, float((ob["pred_pose_enc"][b * T:(b + 1) * T].double() - o1["pred_pose_enc"].double()).abs().max()))
    print(f"floor bf16 pred_pose_enc {floor:.3e}")
    worst = 0.0
    for key in sorted(alone):  # (every figure is printed before anything is asserted)
        a, g = alone[key], got[key]
        print(f"pool (push, stream) {key}: pred_tracks {float((g.pred_tracks - a.pred_tracks).abs().max()):.3e} px, "
              f"pred_pose_enc {float((g.pred_pose_enc.double() - a.pred_pose_enc.double()).abs().max()):.3e}, "
              f"queries {float((q_got[key] - q_alone[key]).abs().max()):.3e} px, "
              f"warm {int((g.track_warm > 0).sum())} / {int((a.track_warm > 0).sum())} slots")
    for key in sorted(alone):
        a, g = alone[key], got[key]
        assert g.frame_index == a.frame_index
        for name in ("track_ids", "track_age", "track_src", "track_warm"):
            assert torch.equal(getattr(g, name), getattr(a, name)), (key, name)
        assert torch.equal(_bits(q_got[key]), _bits(q_alone[key])), (key, "queries")
        worst = max(worst, float((g.pred_pose_enc.double() - a.pred_pose_enc.double()).abs().max()))
    assert worst <= FACTOR * floor, f"pred_pose_enc {worst:.3e} > {FACTOR} x floor {floor:.3e}"
    assert bool((got[(4, 1)].track_warm == 0).all()) and bool((got[(9, 1)].track_warm == 0).all())
    assert bool((got[(5, 1)].track_warm == 1).any()) and bool((got[(9, 0)].track_warm == 1).any())


def test_stream_eval_writes_the_warm_column(model, tmp_path):
    import csv
    from comet_amd import loop
    from comet_amd.config import AttrDict
    g = torch.Generator().manual_seed(3)
    raw = [torch.randint(0, 256, (160, 176, 3), dtype=torch.uint8, generator=g).numpy() for _ in range(T + 2)]
    stream = {"enable": True, "window": T, "stride": 1, "carry": True, "carry_tracks": N, "carry_cell": 8,
              "carry_min_score": MIN_SCORE}
    on = AttrDict.wrap({"stream": dict(stream, warm=True, warm_mode="velocity", warm_iters=2),
                        "train": {"img_size": HW}, "mixed_precision": "bf16"})
    path = str(tmp_path / "warm.csv")
    with _Coarse(model) as rec:
        assert loop.stream_eval(model, iter(raw), on, (8, 0, 168, 160), path, candidate_fn=_Candidates()) == 3
    assert [c["iters"] for c in rec.calls] == [int(model.cfg["track_trainit"]), 2, 2]
    rows = list(csv.DictReader(open(path)))
    assert tuple(rows[0].keys()) == loop.STREAM_FIELDS + ("survivors", "born", "padded", "warm")
    for k, r in enumerate(rows):
        assert (int(r["warm"]) == 0) == (k == 0) and int(r["warm"]) >= int(r["survivors"]), (k, r)
    off = AttrDict.wrap({"stream": stream, "train": {"img_size": HW}, "mixed_precision": "bf16"})
    path = str(tmp_path / "carry.csv")
    assert loop.stream_eval(model, iter(raw), off, (8, 0, 168, 160), path, candidate_fn=_Candidates()) == 3
    assert tuple(next(csv.DictReader(open(path))).keys()) == loop.STREAM_FIELDS + ("survivors", "born", "padded")
    bad = AttrDict.wrap({"stream": {"enable": True, "window": T, "warm": True}, "train": {"img_size": HW}})
    with pytest.raises(ValueError, match="cfg.stream.warm needs cfg.stream.carry"):
        loop.stream_eval(model, iter(raw), bad, (8, 0, 168, 160), str(tmp_path / "bad.csv"), candidate_fn=_Candidates())
