"""Pose fusion on the GPU (comet_pose_fuse in csrc/stream.hip, comet_amd.stream.PoseFuser,
PoseStream / StreamPool with fuse=True, loop.stream_eval; DESIGN.md "Pose fusion") against the
float64 numpy restatement tests/fuse_numpy.py.

Shapes: T = 4, stride 1 and 3 (= T - 1), capacity 4 and 6 (slot reuse and wrap), S = 1 and 3,
3 x capacity hops. Encodings come from oracle.prng, not the model: a smooth trajectory, each window's
true relative encoding plus noise of at most 3 degrees / 0.03 per entry, so the hypotheses of a frame
lie within a few degrees of each other and the largest eigenvalue is simple (the tests check a gap of
at least 0.1 W): eigenvector conditioning is not what is tested.

Bounds against the restatement (derived, not measured): R within 2^-22 absolute (the f32 rounding of
a unit quaternion's entries, 2^-24, on both sides, doubled); float64 outputs within 1e-10 relative
(both sides accumulate in double; the translation arithmetic is the same operations in the same
order); counts equal; spreads within 1e-6 absolute (f32 outputs of a cancelling double expression).
Measured maxima: DESIGN.md "Pose fusion"."""
import csv

import numpy as np
import pytest
import torch

import fuse_numpy as fn

pytestmark = pytest.mark.gpu

T = 4
RATIO = 0.5
INTR = (268.44444444, 268.44444444, 320.0, 240.0)
R_TOL, F64_RTOL, SPREAD_TOL = 2.0 ** -22, 1e-10, 1e-6
F64 = ("uvz", "T", "hyp_T")


# ------------------------------------------------------------------------------------------------
# the scenario
# ------------------------------------------------------------------------------------------------
def _u(seed, name, shape):
    from oracle import prng
    return prng.uniform(seed, name, shape).astype(np.float64)


def _scenario(seed, frames):
    """Ground truth of `frames` frames and a function first frame -> the window's encoding [T, 7] f32."""
    dq, dx, q0 = _u(seed, "fuse.dq", (frames, 4)), _u(seed, "fuse.dx", (frames, 3)), _u(seed, "fuse.q0", (4,))
    q = [fn.unit_pos(q0 + np.array([1.5, 0.0, 0.0, 0.0]))]
    x = [np.array([331.25, 247.5, 11.375])]
    for f in range(1, frames):
        q.append(fn.unit_pos(fn.qmul(fn.axis_angle_quat(dq[f, :3] + 1e-3, 0.06 * dq[f, 3]), q[-1])))
        x.append(x[-1] + dx[f] * np.array([3.0, 3.0, 0.08]))

    def window(first):
        nz = _u(seed, f"fuse.noise.{first}", (T, 7))
        enc = np.zeros((T, 7), dtype=np.float32)
        enc[0, 3] = 1.0
        inv = q[first] * np.array([1.0, -1.0, -1.0, -1.0])
        for i in range(1, T):
            rel = fn.qmul(fn.axis_angle_quat(nz[i, 3:6] + 1e-3, 0.05 * nz[i, 6]), fn.qmul(q[first + i], inv))
            e = [(x[first + i][0] - x[first][0]) * RATIO / 128.0 + 0.03 * nz[i, 0],
                 (x[first + i][1] - x[first][1]) * RATIO / 128.0 + 0.03 * nz[i, 1],
                 (x[first + i][2] / x[first][2] - 1.0) * RATIO + 0.01 * nz[i, 2]]
            enc[i] = np.concatenate([e, fn.unit_pos(rel)])
        return enc
    return np.concatenate([q[0], x[0]]), window


def _stream_hops(stride, cap, count):
    """The first `count` hops of a stream: [Hop]."""
    from comet_amd.stream import RingSchedule
    ring, out = RingSchedule(T, stride, cap), []
    while len(out) < count:
        _, hop = ring.push()
        if hop is not None:
            out.append(hop)
    return out


def _np(out):
    return {k: getattr(out, k).cpu().numpy() for k in out._fields}


def _compare(got, ref, worst, what):
    d = {"R": float(np.abs(got["R"] - ref["R"]).max()), "hyp_R": float(np.abs(got["hyp_R"] - ref["hyp_R"]).max()),
         "rot_spread": float(np.abs(got["rot_spread"] - ref["rot_spread"]).max()),
         "trans_spread": float(np.abs(got["trans_spread"] - ref["trans_spread"]).max())}
    for k in F64:
        d[k] = float((np.abs(got[k] - ref[k]) / np.abs(ref[k])).max())
    for k, v in d.items():
        worst[k] = max(worst.get(k, 0.0), v)
    assert np.array_equal(got["count"], ref["count"]), what
    assert d["R"] <= R_TOL and d["hyp_R"] <= R_TOL, (what, d)
    assert all(d[k] <= F64_RTOL for k in F64), (what, d)
    assert d["rot_spread"] <= SPREAD_TOL and d["trans_spread"] <= SPREAD_TOL, (what, d)


def _gap_ok(acc, slots):
    """The eigen-gap of the rows just written is at least 0.1 W (the scenario's construction)."""
    for s in slots:
        row = acc[s]
        M = np.zeros((4, 4))
        for k, (i, j) in enumerate(fn._TRI):
            M[i, j] = M[j, i] = row[1 + k]
        lam = np.linalg.eigvalsh(M)
        if lam[3] - lam[2] < 0.1 * row[0]:
            return False
    return True


def _fuser(stride, cap, S, anchors, ratio=RATIO):
    from comet_amd.stream import PoseFuser
    return PoseFuser(T, stride, cap, S, [(a[:4], a[4:]) for a in anchors], ratio, INTR, "cuda")


# ------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement, at every hop
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,cap,S", [(1, 4, 1), (3, 6, 1), (1, 6, 3), (3, 4, 3)])
@pytest.mark.parametrize("weighted", [False, True])
def test_kernel_against_the_restatement_at_every_hop(stride, cap, S, weighted):
    """3 x capacity hops of S streams in phase, one launch per hop time (n = S), the ratio on the
    device for S = 1 and on the host for S = 3; `weighted`: a non-uniform weights tensor in
    [0.25, 1.75). Every output of every hop, and the accumulator ring at the end, within the bounds."""
    count = 3 * cap
    hops = _stream_hops(stride, cap, count)
    frames = hops[-1].frame_index + T
    scen = [_scenario(11 + s, frames) for s in range(S)]
    anchors = [a for a, _ in scen]
    ratio = torch.tensor([RATIO], dtype=torch.float64, device="cuda") if S == 1 else RATIO
    fuser = _fuser(stride, cap, S, anchors, ratio)
    ref = fn.FuseRef(S * cap, RATIO, INTR)
    worst = {}
    for k, hop in enumerate(hops):
        enc = np.stack([win(hop.frame_index) for _, win in scen])
        w = (1.0 + 0.75 * _u(5, f"fuse.w.{k}", (S, T))).astype(np.float32) if weighted else None
        slots = fuser.ring.table([(s, hop) for s in range(S)])
        assert sorted(slots) == sorted({*slots}) and all(0 <= v < S * cap for v in slots)
        got = fuser.fuse(torch.from_numpy(enc).cuda(), [(s, hop) for s in range(S)],
                         None if w is None else torch.from_numpy(w).cuda())
        want = ref.fuse(enc, slots, [1 if k == 0 else T - stride] * S, [int(k == 0)] * S, anchors, w)
        assert _gap_ok(ref.acc, slots), "the scenario must keep the largest eigenvalue simple"
        _compare(_np(got), want, worst, f"stride {stride} capacity {cap} S {S} hop {k}")
    acc = fuser.acc.cpu().numpy()
    scale = np.maximum(np.abs(ref.acc), ref.acc[:, :1])  # (the q q^T sums cancel: relative to the row's W)
    worst["acc"] = float((np.abs(acc - ref.acc) / scale).max())
    print(f"pose_fuse vs restatement, stride {stride} capacity {cap} S {S} weighted {weighted}, {count} hops: " +
          ", ".join(f"{k} {v:.3e}" for k, v in sorted(worst.items())))
    assert worst["acc"] <= F64_RTOL
    assert np.array_equal(acc[:, 18:], np.zeros((S * cap, 2)))
    assert ref.acc[:, 17].max() == (T - 1 if stride == 1 else 1)  # position 0 adds no hypothesis


# ------------------------------------------------------------------------------------------------
# 2. pool against separate, weights
# ------------------------------------------------------------------------------------------------
def _bits_equal(a, b, what):
    for k in a._fields:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (what, k)


def test_batched_launches_equal_single_stream_fusers_bit_for_bit():
    """S = 3 out of phase (stream 1 starts two pushes late, stream 2 is reset after its 5th frame),
    capacity 6, stride 1, 18 pushes: the batched launches of one PoseFuser against three single-stream
    fusers fed the same encodings. Same arithmetic per row in the same order: every output and every
    accumulator row bit-identical."""
    from comet_amd.stream import PoolSchedule, RingSchedule
    cap, pushes, late, reset_at = 6, 18, 2, 5
    scen = [_scenario(21 + s, pushes + T) for s in range(3)]
    anchors = [a for a, _ in scen]
    pool, sched = _fuser(1, cap, 3, anchors), PoolSchedule(3, T, 1, cap)
    singles = [_fuser(1, cap, 1, [a]) for a in anchors]
    rings = [RingSchedule(T, 1, cap) for _ in range(3)]
    launches = []
    for p in range(pushes):
        if p == reset_at:
            pool.reset(2)
            sched.reset(2)
            singles[2].reset()
            rings[2].reset()
        ids = [s for s in range(3) if not (s == 1 and p < late)]
        _, hops = sched.push(ids)
        if not hops:
            for s in ids:
                rings[s].push()
            continue
        enc = torch.from_numpy(np.stack([scen[s][1](hop.frame_index + (reset_at if s == 2 and p >= reset_at else 0))
                                         for s, hop in hops])).cuda()
        got = pool.fuse(enc, hops)
        launches.append(len(hops))
        due = {s: hop for s, hop in hops}
        for s in ids:
            _, hop = rings[s].push()
            assert (hop is not None) == (s in due) and (hop is None or hop == due[s])
        for b, (s, hop) in enumerate(hops):
            one = singles[s].fuse(enc[b:b + 1].contiguous(), [(0, hop)])
            _bits_equal(type(got)(*[t[b:b + 1] for t in got]), one, f"push {p} stream {s}")
    assert max(launches) == 3 and min(launches) < 3 and len(launches) >= 12
    torch.cuda.synchronize()
    for s in range(3):
        assert torch.equal(pool.acc[s * cap:(s + 1) * cap].view(torch.uint8), singles[s].acc.view(torch.uint8))


def test_no_weights_equals_all_ones_bit_for_bit():
    cap = 6
    hops = _stream_hops(1, cap, 2 * cap)
    anchor, win = _scenario(31, hops[-1].frame_index + T)
    a, b = _fuser(1, cap, 1, [anchor]), _fuser(1, cap, 1, [anchor])
    ones = torch.ones(1, T, device="cuda")
    for hop in hops:
        enc = torch.from_numpy(win(hop.frame_index)[None]).cuda()
        _bits_equal(a.fuse(enc, [(0, hop)]), b.fuse(enc, [(0, hop)], ones), f"hop {hop.frame_index}")
    assert torch.equal(a.acc.view(torch.uint8), b.acc.view(torch.uint8))


def test_wrapper_rejects_bad_arguments_and_leaves_the_ring_alone():
    from comet_amd import _lib
    hop = _stream_hops(1, 4, 1)[0]
    anchor, win = _scenario(41, 8)
    fuser = _fuser(1, 4, 2, [anchor, anchor])
    enc = torch.from_numpy(np.stack([win(0), win(0)])).cuda()
    with pytest.raises(ValueError, match="one hop per stream"):
        fuser.fuse(enc, [(0, hop), (0, hop)])
    with pytest.raises(ValueError, match="need enc"):
        fuser.fuse(enc[:1], [(0, hop), (1, hop)])
    with pytest.raises(_lib.CometHipError, match="f32"):
        fuser.fuse(enc.double(), [(0, hop), (1, hop)])
    with pytest.raises(_lib.CometHipError, match="weights"):
        fuser.fuse(enc, [(0, hop), (1, hop)], torch.ones(2, T + 1, device="cuda"))
    bad = _fuser(1, 4, 1, [anchor], ratio=-1.0)
    with pytest.raises(_lib.CometHipError, match="ratio must be finite and positive"):
        bad.fuse(enc[:1].contiguous(), [(0, hop)])
    torch.cuda.synchronize()
    assert bool((bad.acc == 0).all())


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
HW, N, SEED_W, SEED_X = 128, 64, 0, 1


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


@pytest.fixture(scope="module")
def seq():
    from oracle import prng
    img, tracks, _ = prng.synthetic_batch(SEED_X, 1, 10, HW, HW, N)
    return img[0].cuda(), tracks[0, 0].cuda()


def _anchor():
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device="cuda")
    return (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device="cuda"), 268.44,
            torch.tensor([0.5], dtype=torch.float64), "AMD")


def test_fusion_at_stride_window_minus_1_is_the_existing_chaining(model, seq):
    """stride = T - 1: every frame has one hypothesis, so fusion must reproduce the unfused stream.
    pred_pose_enc identical; at hop k (k + 1 hops chained so far) fused_R (and R) within
    (k + 1) x 2^-22 of the unfused R, fused_T (and T) within (k + 1) x 2^-22 x max |T|: the existing
    path rounds every reference (u, v, z) and quaternion to f32, the fused path keeps double."""
    from comet_amd.stream import PoseStream
    frames, q = seq
    res = {}
    for fuse in (False, True):
        st = PoseStream(model, window=T, stride=T - 1, anchor=_anchor(), precision=torch.float32, fuse=fuse)
        res[fuse] = [r for f in range(10) for r in st.push(frames[f], query_points=q)]
    assert len(res[True]) == len(res[False]) == 3
    for k, (a, b) in enumerate(zip(res[True], res[False])):
        assert a.frame_index == b.frame_index == k * (T - 1) and a.final == T - 1
        assert torch.equal(a.pred_pose_enc, b.pred_pose_enc) and torch.equal(a.pred_tracks, b.pred_tracks)
        assert b.fused_R is None and b.final is None
        assert a.fused_count.tolist() == [1] * T
        tol = (k + 1) * 2.0 ** -22
        scale = float(b.T.abs().max())
        dR = [float((x - b.R).abs().max()) for x in (a.fused_R, a.R)]
        dT = [float((x - b.T).abs().max()) / scale for x in (a.fused_T, a.T)]
        print(f"fused vs chained, stride T - 1, hop {k}: R {dR[0]:.3e} / {dR[1]:.3e}, T / max|T| {dT[0]:.3e} / {dT[1]:.3e} "
              f"(bound {tol:.3e})")
        assert a.fused_T.dtype == torch.float64 and a.fused_R.dtype == torch.float32
        assert max(dR) <= tol and max(dT) <= tol


@pytest.mark.parametrize("dtype,weight", [(torch.bfloat16, None), (torch.float32, "score")])
def test_pool_of_one_stream_equals_pose_stream_with_fusion_bit_for_bit(model, seq, dtype, weight):
    """S = 1, 7 frames, stride 1, capacity == window (the ring wraps): every field of every result."""
    from comet_amd.stream import PoseStream, StreamPool, StreamResult
    frames, q = seq
    one = PoseStream(model, window=T, stride=1, anchor=_anchor(), precision=dtype, fuse=True, fuse_weight=weight)
    pool = StreamPool(model, streams=1, window=T, stride=1, anchors=[_anchor()], precision=dtype, fuse=True,
                      fuse_weight=weight)
    n = 0
    for f in range(7):
        ref = one.push(frames[f], query_points=q)
        got = pool.push(frames[f:f + 1], query_points=q)
        assert [s for s, _ in got] == [0] * len(ref) and len(ref) == (1 if f >= T - 1 else 0)
        for (_, g), r in zip(got, ref):
            n += 1
            assert g.frame_index == r.frame_index and g.final == r.final == 1
            # (a window adds no hypothesis for its own first frame: that is its reference)
            assert r.fused_count.tolist() == [max(1, min(n - 1, T - 1))] + [min(n, T - i) for i in range(1, T)]
            for name in StreamResult._fields[1:-1]:
                a, b = getattr(g, name), getattr(r, name)
                assert a.shape == b.shape and a.dtype == b.dtype, name
                assert torch.equal(a, b), f"frame {f}, {name}"
    assert n == 4


def test_stream_eval_writes_the_fused_columns_and_a_flush(model, seq, tmp_path):
    """Fusion on: the STREAM_FIELDS columns, then the FUSE_FIELDS ones, one row per final frame and a
    flush of the last window's T - 1 remaining frames. Fusion off: the header and rows of before."""
    from comet_amd import loop
    from comet_amd.config import AttrDict
    _, q = seq
    g = torch.Generator().manual_seed(3)
    raw = [torch.randint(0, 256, (160, 176, 3), dtype=torch.uint8, generator=g).numpy() for _ in range(6)]
    box = (8, 0, 168, 160)
    base = {"enable": True, "window": T, "stride": 1}
    cfg = lambda extra: AttrDict.wrap({"stream": {**base, **extra}, "train": {"img_size": HW}, "mixed_precision": "bf16"})
    off, on = str(tmp_path / "off.csv"), str(tmp_path / "on.csv")
    assert loop.stream_eval(model, iter(raw), cfg({}), box, off, query_points=q) == 3
    assert loop.stream_eval(model, iter(raw), cfg({"fuse": True, "fuse_weight": "score"}), box, on, query_points=q) == 3
    rows_off, rows_on = list(csv.DictReader(open(off))), list(csv.DictReader(open(on)))
    assert open(off).readline().strip().split(",") == list(loop.STREAM_FIELDS)
    assert open(on).readline().strip().split(",") == list(loop.STREAM_FIELDS + loop.FUSE_FIELDS)
    assert len(rows_off) == 3 and len(rows_on) == 3 + (T - 1)
    assert [int(r["fused_frame"]) for r in rows_on] == list(range(6))
    assert [int(r["fused_count"]) for r in rows_on] == [1, 1, 2, 3, 2, 1]
    for r, e in zip(rows_on, rows_off):  # the hop's own columns do not depend on fusion
        assert all(r[k] == e[k] for k in loop.STREAM_FIELDS if k != "hop_ms")
    for r in rows_on:
        qn = sum(float(r[k]) ** 2 for k in ("fused_qw", "fused_qx", "fused_qy", "fused_qz"))
        assert abs(qn - 1.0) < 1e-6 and float(r["fused_qw"]) >= 0 and float(r["rot_spread"]) >= 0
        assert all(float(r[k]) >= 0 for k in ("spread_u", "spread_v", "spread_z"))
    assert [r["frame_index"] for r in rows_on[3:]] == [rows_on[2]["frame_index"]] * 3
