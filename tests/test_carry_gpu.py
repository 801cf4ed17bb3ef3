"""Track carry on the GPU (comet_track_carry in csrc/carry.hip, ops.track_carry,
comet_amd.stream.TrackCarry, PoseStream / StreamPool carry=True, loop.stream_eval; DESIGN.md "Track
carry").

Kernel: every output is a copy of an input or an integer (the lattice pads: one f32 expression both
sides evaluate alike), so the kernel must equal the numpy restatement tests/carry_numpy.py exactly,
queries compared as bits.

End to end: the golden configuration of tests/test_stream_gpu.py (PRNG weights seed 0, T = 4, 128^2,
N = 64, oracle.prng frames), candidates from a fixed seeded point set (no detector weights needed).
MIN_SCORE and the frame seed are recorded at E2E below."""
import numpy as np
import pytest
import torch

import carry_numpy as cn

pytestmark = pytest.mark.gpu

OUT = ("query", "ids", "age", "src", "stats", "next_id")


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).cuda().contiguous()


def _gpu(inp, cell, border, min_score):
    """ops.track_carry on the numpy arguments of carry_numpy.carry -> the same dict of numpy arrays."""
    from comet_amd import ops
    next_id = _dev(inp["next_id"])
    out = ops.track_carry(_dev(inp["tracks"]), _dev(inp["score"]), _dev(inp["ids"]), _dev(inp["age"]), next_id,
                          _dev(inp["prev_valid"]), inp["s"], inp["H"], inp["W"], cell, border, min_score,
                          _dev(inp["cand"]), _dev(inp["cand_n"]), _dev(inp["mask"]))
    torch.cuda.synchronize()
    got = {k: getattr(out, k).cpu().numpy() for k in OUT[:5]}
    got["next_id"] = next_id.cpu().numpy()
    return got


def _same(got, ref, what=""):
    for k in OUT:
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if k == "query":
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.argwhere(a != b)
        assert bad.size == 0, f"{what} {k}: {len(bad)} differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]} != {b[tuple(bad[0])]}"


def _both(inp, cell, border, min_score, what=""):
    ref = cn.carry(**inp, cell=cell, border=border, min_score=min_score)
    got = _gpu(inp, cell, border, min_score)
    _same(got, ref, what)
    return ref


# ------------------------------------------------------------------------------------------------
# case a: every branch, by construction
# ------------------------------------------------------------------------------------------------
def _case_a():
    n, T, N, M, H, W = 1, 4, 64, 96, 128, 128
    tracks = np.full((n, T, N, 2), 200.0, np.float32)  # (rows other than s, and unused slots: outside the frame)
    score = np.ones((n, T, N), np.float32)
    ids = np.full((n, N), -1, np.int32)
    age = np.zeros((n, N), np.int32)
    rows = {  # slot: (x, y, score, id, age)
        0: (10, 10, 1, 100, 3), 1: (12, 12, 1, 101, 3),                       # two in one cell, equal ages: slot 0
        2: (20, 20, 1, 102, 1), 3: (21, 22, 1, 103, 5), 4: (22, 21, 1, 104, 2),  # three, unequal ages: slot 3
        5: (40, 40, 1, 105, 0),                                               # holds its cell against candidates 0 and 37
        6: (50, 10, 0.2, 106, 4),                                             # dead by score
        7: (70, 70, 1, 107, 4),                                               # dead by mask
        8: (2, 60, 1, 108, 4),                                                # dead by border
        9: (np.nan, 60, 1, 109, 4), 10: (60, np.inf, 1, 110, 4),              # dead by NaN / Inf position
        11: (90, 10, np.nan, 111, 4),                                         # dead by NaN score
        12: (100, 10, 1, -1, 4),                                              # id < 0: no track
        13: (10, 100, 1, 113, 1), 14: (11, 101, 1, 114, 2),                   # two, unequal ages: slot 14
        15: (20, 100, 1, 115, 2), 16: (21, 101, 1, 116, 2), 17: (22, 102, 1, 117, 2),  # three, equal ages: slot 15
        18: (36, 100, 1, 118, 7), 19: (44.5, 100.5, 1, 119, 0),
    }
    for j, (x, y, sc, i, a) in rows.items():
        tracks[0, 1, j] = (x, y)
        score[0, 1, j], ids[0, j], age[0, j] = sc, i, a
    mask = np.ones((n, H, W), np.uint8)
    mask[0, 64:96, 64:96] = 0
    cand = np.zeros((n, M, 2), np.float32)
    cand[0, 0] = (41, 41)                    # in the cell track 5 holds
    cand[0, 1], cand[0, 2] = (30, 50), (31, 51)  # two candidates in one cell: 1 wins
    cand[0, 3] = (80, 80)                    # outside the mask
    for c in range(4, M):                    # a lattice of distinct cells (some on the border, some in the mask hole)
        cand[0, c] = ((c % 16) * 8 + 4, 28 + (c // 16) * 8)
    return dict(tracks=tracks, score=score, ids=ids, age=age, mask=mask, cand=cand, cand_n=np.array([M], np.int32),
                next_id=np.array([500], np.int32), prev_valid=np.ones(n, np.int32), s=1, H=H, W=W)


def test_case_a_every_branch():
    inp = _case_a()
    ref = _both(inp, 8, 4, 0.5, "case a")
    src, idv, agev = ref["src"][0], ref["ids"][0], ref["age"][0]
    kept = [j for j in range(64) if src[j] == j]
    assert kept == [0, 3, 5, 14, 15, 18, 19], kept
    assert idv[kept].tolist() == [100, 103, 105, 114, 115, 118, 119] and agev[kept].tolist() == [4, 6, 1, 3, 3, 8, 1]
    born = {-1 - int(v): j for j, v in enumerate(src) if -96 <= v < 0}
    assert 0 not in born and 37 not in born, "a candidate took a cell that a track holds"
    assert 1 in born and 2 not in born and 51 not in born, "two candidates in one cell: the lower index wins"
    assert 3 not in born, "a candidate outside the mask was born"
    assert 15 not in born and 31 not in born, "a candidate on the border (x = 124 > W - 1 - border) was born"
    assert 72 not in born and 4 in born, "a candidate in the mask hole (68, 68) was born"
    stats = ref["stats"][0].tolist()
    assert stats == [7, 57, 0, 6], stats  # all 57 free slots are born into; the cell rule drops slots 1, 2, 4, 13, 16, 17
    # more kept candidates than free slots: the free slots take the first ones, in order
    assert sorted(born.values()) == [j for j in range(64) if j not in kept]
    order = [c for c, _ in sorted(born.items(), key=lambda kv: kv[1])]
    assert order == sorted(order) and max(order) < 94, "no kept candidate was left over (94 and 95 are alive)"
    assert idv[[born[c] for c in order]].tolist() == list(range(500, 557)) and ref["next_id"][0] == 557


# ------------------------------------------------------------------------------------------------
# case b: scans over several chunks of 256; N = 1; N no multiple of 64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(300, 700), (1, 5), (70, 100), (700, 300)])
def test_case_b_scans_span_chunks(N, M):
    inp = cn.random_inputs(11, 2, 4, N, M, 256, 256, s=2, fill=0.5)
    ref = _both(inp, 8, 3, 0.3, f"case b N={N} M={M}")
    if N >= 300:
        assert (ref["stats"][:, 0] > 0).all() and (ref["stats"][:, 1] > 0).all()
        if N == 300:  # candidates born from beyond the first chunk, into slots beyond the first chunk
            assert (ref["src"] < -256).any() and (ref["src"][:, 256:] < 0).any()
        else:
            assert (ref["stats"][:, 2] > 0).all(), "no pads"


# ------------------------------------------------------------------------------------------------
# case c: no candidates, nothing alive, first hop
# ------------------------------------------------------------------------------------------------
def test_case_c_duplicate_pads_lattice_pads_and_first_hop():
    base = cn.random_inputs(12, 1, 4, 70, 0, 128, 128, fill=0.6)
    assert base["cand"] is None
    ref = _both(base, 8, 0, 0.3, "case c, M = 0")
    assert ref["stats"][0, 1] == 0 and ref["stats"][0, 2] > 0 and ref["stats"][0, 0] > 0
    assert (ref["src"][0][ref["ids"][0] < 0] >= cn.INT32_MIN).all()
    dead = dict(base, score=np.zeros_like(base["score"]))
    ref = _both(dead, 8, 0, 0.3, "case c, all dead")
    assert ref["stats"][0].tolist() == [0, 0, 70, 0] and (ref["src"] == cn.INT32_MIN).all() and (ref["ids"] == -1).all()
    g = 9  # ceil(sqrt(70))
    assert ref["query"][0, 0].tolist() == [np.float32(0.5) * np.float32(128) / np.float32(g)] * 2
    assert len({tuple(q) for q in ref["query"][0].tolist()}) == 70
    first = cn.random_inputs(13, 2, 4, 70, 90, 128, 128)
    first["tracks"][:] = np.nan
    first["score"][:] = np.nan
    first["prev_valid"][:] = 0
    ref = _both(first, 8, 0, 0.3, "case c, prev_valid = 0")
    assert np.isfinite(ref["query"]).all() and (ref["stats"][:, 0] == 0).all() and (ref["stats"][:, 1] > 0).all()
    assert (ref["age"] == 0).all()


# ------------------------------------------------------------------------------------------------
# case d: three hops in one launch
# ------------------------------------------------------------------------------------------------
def test_case_d_three_hops_in_one_launch():
    inp = cn.random_inputs(14, 3, 4, 64, 96, 128, 128)
    inp["cand_n"][:] = (0, 50, 96)
    inp["prev_valid"][:] = (1, 1, 0)
    inp["next_id"][:] = (64, 1000, 0)
    assert not (inp["mask"][0] == inp["mask"][1]).all()
    ref = _both(inp, 8, 2, 0.3, "case d")
    assert ref["stats"][0, 1] == 0 and ref["stats"][1, 1] > 0 and ref["stats"][2, 0] == 0
    one = {k: (v[1:2] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
    one["mask"] = None
    nomask = _both(one, 8, 2, 0.3, "case d, mask NULL")
    assert not (nomask["src"] == ref["src"][1:2]).all(), "the mask made no difference"


# ------------------------------------------------------------------------------------------------
# case e: three chained calls
# ------------------------------------------------------------------------------------------------
def test_case_e_chained_calls_continue_ids():
    cur = cn.random_inputs(15, 2, 4, 64, 96, 128, 128)
    cur["prev_valid"][:] = 0
    cur["next_id"][:] = 0
    rng = np.random.default_rng(1)
    tops = []
    for k in range(3):
        ref = cn.carry(**cur, cell=8, border=2, min_score=0.3)
        got = _gpu(cur, 8, 2, 0.3)
        _same(got, ref, f"case e call {k}")
        tops.append(got["next_id"].copy())
        fresh = cn.random_inputs(16 + k, 2, 4, 64, 96, 128, 128)
        tracks = fresh["tracks"]
        tracks[:, 1] = got["query"] + rng.normal(0, 2, got["query"].shape).astype(np.float32)
        cur = dict(fresh, tracks=tracks, ids=got["ids"], age=got["age"], next_id=got["next_id"])
    assert (tops[0] > 0).all() and (tops[1] > tops[0]).all() and (tops[2] > tops[1]).all()
    assert (got["age"] == 2).any(), "no track lived through all three calls"


# ------------------------------------------------------------------------------------------------
# case f: a grid that does not divide the frame
# ------------------------------------------------------------------------------------------------
def test_case_f_grid_does_not_divide_the_frame():
    H, W, cell = 96, 80, 7  # 12 x 14 cells; the last column is 3 px wide, the last row 5 px high
    inp = cn.random_inputs(17, 1, 4, 64, 96, H, W, with_mask=False)
    edge = [(79, 95), (79, 10), (10, 95), (77, 91), (78.5, 94.5), (0, 0)]
    for j, p in enumerate(edge):
        inp["tracks"][0, 1, j] = p
        inp["score"][0, 1, j], inp["ids"][0, j], inp["age"][0, j] = 1, 900 + j, 50 - j
    inp["cand"][0, :3] = [(79, 95), (79, 50), (50, 95)]
    ref = _both(inp, cell, 0, 0.3, "case f")
    assert [j for j in range(6) if ref["src"][0, j] == j] == [0, 1, 2, 5]
    assert ref["src"][0, 3] != 3 and ref["src"][0, 4] != 4, "(77, 91) and (78.5, 94.5) share the last cell with slot 0"
    born = {-1 - int(v) for v in ref["src"][0] if -96 <= v < 0}
    assert 0 not in born and {1, 2} <= born, "candidates on the last row / column"


# ------------------------------------------------------------------------------------------------
# the wrapper
# ------------------------------------------------------------------------------------------------
def test_track_carry_wrapper_rejects_bad_arguments():
    from comet_amd import _lib, ops
    inp = cn.random_inputs(18, 1, 4, 64, 32, 128, 128)
    t = {k: _dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}

    def call(**kw):
        a = dict(t, **kw)
        return ops.track_carry(a["tracks"], a["score"], a["ids"], a["age"], a["next_id"], a["prev_valid"], 1, 128, 128,
                               a.get("cell", 8), 0, 0.3, a["cand"], a["cand_n"], a["mask"])
    for bad in (dict(tracks=t["tracks"].double()), dict(score=t["score"][:, :3]), dict(ids=t["ids"].long()),
                dict(cand=t["cand"][:, :, :1]), dict(cand_n=None), dict(mask=t["mask"].bool()),
                dict(tracks=t["tracks"].cpu()), dict(age=t["age"][:, ::2])):
        with pytest.raises(_lib.CometHipError):
            call(**bad)
    with pytest.raises(_lib.CometHipError, match="more than 8192 grid cells"):
        call(cell=1)
    assert call().query.shape == (1, 64, 2)


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
# E2E: frames of oracle.prng seed SEED_X; carried tracks need pred_score >= MIN_SCORE. With these two
# values the restatement alone, fed the recorded pred_tracks / pred_score of the 5 hops of the
# PoseStream test, carries more than no and fewer than all slots (asserted in the test itself; measured
# on an MI355X, f32: 60, 58, 58 and 60 of the 64 slots over hops 1 .. 4).
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
    """A fixed seeded point set as candidate_fn; counts its calls."""

    def __init__(self):
        g = torch.Generator().manual_seed(CAND_SEED)
        self.points = (torch.rand(CAND_M, 2, generator=g) * (HW - 1)).cuda()
        self.calls = 0

    def __call__(self, frame):
        assert frame.shape == (3, HW, HW)
        self.calls += 1
        return self.points


def _carry_kw(cand, **kw):
    return dict(dict(window=T, stride=1, carry=True, carry_tracks=N, carry_cell=8, carry_border=0,
                     carry_min_score=MIN_SCORE, candidate_fn=cand), **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Queries:
    """Records the query points (tracks[:, 0]) of every model.forward_all call while active."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __enter__(self):
        orig = self.model.forward_all

        def recorded(*a, **kw):
            self.seen.append(kw["tracks"][:, 0].clone())
            return orig(*a, **kw)
        self.model.forward_all = recorded
        return self

    def __exit__(self, *exc):
        del self.model.forward_all  # the instance attribute; the class's method is back


def test_pose_stream_carries_tracks_across_windows(model):
    from comet_amd.stream import PoseStream
    frames = _frames(SEED_X, 8)
    cand = _Candidates()
    s = PoseStream(model, precision=torch.float32, **_carry_kw(cand))
    res = []
    with _Queries(model) as rec:
        for f in range(8):
            res += s.push(frames[f])
    assert [r.frame_index for r in res] == [0, 1, 2, 3, 4] and cand.calls == 5
    queries = [q[0] for q in rec.seen]
    assert len(queries) == 5 and queries[0].shape == (N, 2)
    assert (res[0].track_age == 0).all() and not bool((res[0].track_src == torch.arange(N, device="cuda")).any())
    seen, carried, top = set(), 0, -1
    ar = torch.arange(N, device="cuda", dtype=torch.int32)
    # the restatement chained on the recorded outputs gives the same identities
    ids = np.full((1, N), -1, np.int32)
    age = np.zeros((1, N), np.int32)
    next_id = np.zeros(1, np.int32)
    pts = cand.points.cpu().numpy()[None]
    for k, r in enumerate(res):
        assert r.track_ids.shape == r.track_age.shape == r.track_src.shape == (N,) and r.track_ids.dtype == torch.int32
        prev = res[k - 1] if k else None
        ref = cn.carry(tracks=(prev.pred_tracks if k else torch.zeros(T, N, 2)).cpu().numpy()[None],
                       score=(prev.pred_score if k else torch.zeros(T, N)).float().cpu().numpy()[None], ids=ids, age=age,
                       mask=None, cand=pts, cand_n=np.array([CAND_M], np.int32), next_id=next_id,
                       prev_valid=np.array([int(k > 0)], np.int32), s=1, H=HW, W=HW, cell=8, border=0, min_score=MIN_SCORE)
        for name, field in (("ids", r.track_ids), ("age", r.track_age), ("src", r.track_src)):
            assert (field.cpu().numpy() == ref[name][0]).all(), (k, name)
        ids, age, next_id = ref["ids"], ref["age"], ref["next_id"]
        keep = r.track_src == ar
        print(f"hop {k}: carried {int(keep.sum())}, born {int(((r.track_src < 0) & (r.track_src >= -CAND_M)).sum())}, "
              f"pads {int((r.track_ids < 0).sum())}, stats {ref['stats'][0].tolist()}")
        if k >= 1:
            carried += int(keep.sum())
            assert torch.equal(_bits(queries[k][keep]), _bits(prev.pred_tracks[1][keep])), f"hop {k}: a carried query moved"
            assert (_bits(queries[k]).cpu().numpy() == ref["query"][0].view(np.int32)).all(), f"hop {k}: queries"
            assert torch.equal(r.track_ids[keep], prev.track_ids[keep]) and bool((r.track_ids[keep] >= 0).all())
            assert torch.equal(r.track_age[keep], prev.track_age[keep] + 1)
        born = (r.track_src < 0) & (r.track_src >= -CAND_M)
        new = r.track_ids[born].tolist()
        assert len(set(new)) == len(new) and not (set(new) & seen) and all(i > top for i in new)
        seen |= set(new)
        top = max([top] + new)
        live = r.track_ids[r.track_ids >= 0].tolist()
        assert len(set(live)) == len(live) and set(live) <= seen
    assert 0 < carried < 4 * N, f"{carried} of {4 * N} slots carried over hops 1 .. 4: the test would be vacuous"


def test_detect_every_two_calls_the_detector_on_even_hops(model):
    from comet_amd.stream import PoseStream
    frames = _frames(SEED_X, 8)
    cand = _Candidates()
    s = PoseStream(model, precision=torch.bfloat16, **_carry_kw(cand, detect_every=2))
    calls = []
    for f in range(8):
        got = s.push(frames[f])
        if got:
            calls.append(cand.calls)
            if len(calls) in (2, 4):  # hops 1 and 3: no detector, so nothing is born
                assert not bool(((got[0].track_src < 0) & (got[0].track_src >= -CAND_M)).any())
    assert calls == [1, 1, 2, 2, 3], calls


PUSHES, LATE, RESET_AT = 10, 1, 6  # stream 1 joins one push late and is reset before push 6


def _pool_frame(s, p):
    return p - LATE if s == 1 and p >= LATE else (p if s == 0 else None)


def test_pool_out_of_phase_equals_separate_streams(model):
    """Two streams, stream 1 one push late and reset before push 6, bf16 (hops: stream 0 in pushes 3 .. 9,
    stream 1 in pushes 4, 5 and, after its reset, 9). ids, ages, sources and
    queries: equality (the kernel is deterministic and, DESIGN.md section 14, tracks are bit-identical
    on every path). pred_pose_enc: within 4 x floor, the floor measured as tests/test_pool_gpu.py does:
    forward_all on the closed windows of the hops due in one push, with the queries the separate streams
    used, stacked as one B = 2 batch against each window alone, largest difference over the pushes."""
    from comet_amd import functional as F
    from comet_amd.stream import PoseStream, StreamPool
    dtype = torch.bfloat16
    seqs = [_frames(seed, PUSHES) for seed in SEEDS]
    cands = [_Candidates(), _Candidates(), _Candidates()]
    singles = [PoseStream(model, precision=dtype, **_carry_kw(cands[i])) for i in range(2)]
    pool = StreamPool(model, streams=2, precision=dtype, **_carry_kw(cands[2]))
    alone, got, base = {}, {}, {0: 0, 1: 0}
    q_alone, q_got = {}, {}
    for p in range(PUSHES):
        if p == RESET_AT:
            singles[1].reset()
            pool.reset(1)
            base[1] = _pool_frame(1, p)
        ids = [s for s in range(2) if _pool_frame(s, p) is not None]
        for s in ids:
            with _Queries(model) as rec:
                for r in singles[s].push(seqs[s][_pool_frame(s, p)]):
                    alone[(p, s)], q_alone[(p, s)] = r, rec.seen[0][0]
        with _Queries(model) as rec:
            for b, (s, r) in enumerate(pool.push(torch.stack([seqs[s][_pool_frame(s, p)] for s in ids]), streams=ids)):
                got[(p, s)], q_got[(p, s)] = r, rec.seen[0][b]
    assert sorted(got) == sorted(alone) and len(got) == 7 + 2 + 1, sorted(got)
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
              f"pred_score {float((g.pred_score.float() - a.pred_score.float()).abs().max()):.3e}, "
              f"queries {float((q_got[key] - q_alone[key]).abs().max()):.3e} px, "
              f"ids differ in {int((g.track_ids != a.track_ids).sum())} slots")
    for key in sorted(alone):
        a, g = alone[key], got[key]
        assert g.frame_index == a.frame_index
        for name in ("track_ids", "track_age", "track_src"):
            assert torch.equal(getattr(g, name), getattr(a, name)), (key, name)
        assert torch.equal(_bits(q_got[key]), _bits(q_alone[key])), (key, "queries")
        d = float((g.pred_pose_enc.double() - a.pred_pose_enc.double()).abs().max())
        worst = max(worst, d)
        print(f"pool (push, stream) {key}: pred_pose_enc {d:.3e} (floor {floor:.3e})")
    assert worst <= FACTOR * floor, f"pred_pose_enc {worst:.3e} > {FACTOR} x floor {floor:.3e}"
    # reset(1) restarted stream 1 only
    after, before = got[(PUSHES - 1, 1)], got[(RESET_AT - 1, 1)]
    assert bool((after.track_age == 0).all()) and int(after.track_ids.max()) < N and int(before.track_age.max()) > 0
    assert int(got[(PUSHES - 1, 0)].track_age.max()) > int(got[(RESET_AT - 1, 0)].track_age.max())
    assert int(got[(PUSHES - 1, 0)].track_ids.max()) >= N


def test_stream_eval_writes_the_carry_columns(model, tmp_path):
    import csv
    from comet_amd import loop
    from comet_amd.config import AttrDict
    g = torch.Generator().manual_seed(3)
    raw = [torch.randint(0, 256, (160, 176, 3), dtype=torch.uint8, generator=g).numpy() for _ in range(T + 2)]
    stream = {"enable": True, "window": T, "stride": 1}
    on = AttrDict.wrap({"stream": dict(stream, carry=True, carry_tracks=N, carry_cell=8, carry_min_score=MIN_SCORE,
                                       detect_every=2),
                        "train": {"img_size": HW}, "mixed_precision": "bf16"})
    cand = _Candidates()
    path = str(tmp_path / "carry.csv")
    assert loop.stream_eval(model, iter(raw), on, (8, 0, 168, 160), path, candidate_fn=cand) == 3 and cand.calls == 2
    rows = list(csv.DictReader(open(path)))
    assert tuple(rows[0].keys()) == loop.STREAM_FIELDS + ("survivors", "born", "padded")
    for k, r in enumerate(rows):
        sv, bn, pd = int(r["survivors"]), int(r["born"]), int(r["padded"])
        assert sv + bn + pd == N and (sv == 0) == (k == 0) and (bn == 0) == (k == 1)
    off = AttrDict.wrap({"stream": stream, "train": {"img_size": HW}, "mixed_precision": "bf16"})
    path = str(tmp_path / "plain.csv")
    q = cand.points[:N]
    assert loop.stream_eval(model, iter(raw), off, (8, 0, 168, 160), path, query_points=q) == 3
    assert tuple(next(csv.DictReader(open(path))).keys()) == loop.STREAM_FIELDS
    with pytest.raises(ValueError, match="query_points together with carry"):
        loop.stream_eval(model, iter(raw), on, (8, 0, 168, 160), str(tmp_path / "bad.csv"), query_points=q, candidate_fn=cand)
