"""The stream pool on the GPU (comet_amd.stream.StreamPool, comet_ring_scatter in csrc/stream.hip,
loop.stream_eval_pool; DESIGN.md "Stream pool") at the golden configuration of
tests/test_stream_gpu.py: PRNG weights seed 0, T = 4, 128 x 128 frames, N = 64 query points, frames of
oracle.prng seed 1 for the single stream and seeds 4, 2 and 3 for the three streams (one sequence
per stream, so a result delivered to the wrong stream is a gross error).

Tolerances of the pool-vs-separate-streams comparisons. At S = 1 the pool executes the same kernels
on the same shapes as PoseStream: equality. With several streams the per-frame stages see k frames
per call instead of 1 and the cross-frame part runs at B = n instead of 1; only the row count of the
GEMMs changes, which changes their plans and summation order. The floor is what the same change does
on the closed path, existing code only: model.forward_all on the closed windows of the hops that fall
due in one push, stacked as one B = n batch, against each window alone -- per output and precision,
the largest difference over all pushes of the scenario (fixture `floors`, measured in the run and
printed). Every pool result must be within 4 x that floor of the separate stream's result (method
and margin of tests/test_stream_gpu.py).

Seeds. With seed 1 as stream 0 the floor itself (existing code: B = 3 against B = 1, bf16) holds a
discrete flip: in window 5 one refined track moves by exactly 1 px, because refine_track floors the
coarse track to an integer patch origin and the coarse coordinate crosses an integer when the
tracker's GEMMs change plan (seed 5 likewise, 1.055 px). Such a floor would allow 4 px. Seeds 4, 6
and 7 show no flip in either precision, in tracks or in compute_score_fn's 5 x 5 window; seed 4
takes the place of seed 1 for stream 0, streams 1 and 2 keep seeds 2 and 3. The single-stream test
compares for equality and keeps seed 1. Measured floors and worst differences: DESIGN.md
"Stream pool"."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

T, HW, N, CAP = 4, 128, 64, 6
SEED_W, SEED_ONE, SEEDS = 0, 1, (4, 2, 3)
PUSHES = 9
LATE, RESET_AT = 2, 5  # stream 1 joins two pushes late; stream 2 is reset after its 5th frame
FACTOR = 4.0
DTYPES = [torch.float32, torch.bfloat16]
NAMES = ("pred_pose_enc", "pred_tracks", "pred_score")


# ------------------------------------------------------------------------------------------------
# 1. - 2. the scatter kernel
# ------------------------------------------------------------------------------------------------
SCATTER_SLOTS = [5, 0, 7]


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("max_blocks", [1, 0])
def test_ring_scatter_is_exact(max_blocks):
    """Three tensors in one launch, f32 and bf16, rows of 16 B (one vector), 16 KiB + 16 B (one tile
    and a tail of one vector) and 48 KiB (three tiles); k = 3 rows to slots [5, 0, 7] of capacity 8.
    The three slots hold their sources bit for bit, every other slot and a guard slot on either side
    of the ring still hold the sentinel, and ring_gather of [5, 0, 7] returns the sources.
    max_blocks = 1: one workgroup walks every tile of every tensor (the grid-stride path)."""
    from comet_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(7)
    widths = [(torch.float32, 4), (torch.bfloat16, 8200), (torch.float32, 12288)]
    srcs, bigs = [], []
    for dtype, n in widths:
        srcs.append(torch.randn(3, n, device="cuda", generator=gen).to(dtype))
        bigs.append(torch.full((10, n), 7, device="cuda", dtype=dtype))  # guard, 8 slots, guard
    assert [s[0].numel() * s.element_size() for s in srcs] == [16, 16 * 1024 + 16, 48 * 1024]
    rings = [b[1:9] for b in bigs]
    dev = torch.tensor(SCATTER_SLOTS, dtype=torch.int32, device="cuda")
    host = (ctypes.c_int32 * 3)(*SCATTER_SLOTS)
    ops.ring_scatter(list(zip(srcs, rings)), dev, host, max_blocks=max_blocks)
    torch.cuda.synchronize()
    for src, ring, big in zip(srcs, rings, bigs):
        for j, slot in enumerate(SCATTER_SLOTS):
            assert torch.equal(_bits(ring[slot]), _bits(src[j])), (src.dtype, src.shape, slot)
        rest = [s for s in range(8) if s not in SCATTER_SLOTS]
        assert bool((ring[rest] == 7).all()), "a slot that is no target was written"
        assert bool((big[0] == 7).all()) and bool((big[9] == 7).all()), "written outside the ring"
    wins = [torch.zeros_like(s) for s in srcs]
    ops.ring_gather(list(zip(rings, wins)), dev, host, max_blocks=max_blocks)
    torch.cuda.synchronize()
    for src, win in zip(srcs, wins):
        assert torch.equal(_bits(win), _bits(src))


def test_ring_scatter_wrapper_rejects_bad_arguments():
    from comet_amd import _lib, ops
    ring = torch.zeros(8, 16, device="cuda")
    src = torch.zeros(3, 16, device="cuda")
    slots = torch.tensor(SCATTER_SLOTS, dtype=torch.int32, device="cuda")
    host = (ctypes.c_int32 * 3)(*SCATTER_SLOTS)
    with pytest.raises(_lib.CometHipError):
        ops.ring_scatter([(src.to(torch.bfloat16), ring)], slots, host)
    with pytest.raises(_lib.CometHipError):
        ops.ring_scatter([(torch.zeros(3, 8, device="cuda"), ring)], slots, host)
    with pytest.raises(_lib.CometHipError, match="duplicate slot"):
        ops.ring_scatter([(src, ring)], slots, (ctypes.c_int32 * 3)(5, 0, 5))
    with pytest.raises(_lib.CometHipError, match="outside the ring"):
        ops.ring_scatter([(src, ring)], slots, (ctypes.c_int32 * 3)(5, 0, 8))
    torch.cuda.synchronize()
    assert bool((ring == 0).all())


# ------------------------------------------------------------------------------------------------
# the model, the sequences, the scenario
# ------------------------------------------------------------------------------------------------
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


def _load_seqs(seeds):
    """[(frames [PUSHES, 3, H, W], query points [N, 2])] per stream."""
    from oracle import prng
    out = []
    for seed in seeds:
        img, tracks, _ = prng.synthetic_batch(seed, 1, PUSHES, HW, HW, N)
        out.append((img[0].cuda(), tracks[0, 0].cuda()))
    return out


@pytest.fixture(scope="module")
def seqs():
    return _load_seqs(SEEDS)


@pytest.fixture(scope="module")
def seq_one():
    return _load_seqs([SEED_ONE])[0]


def _frame_of(s, p):
    """Index, in stream s's sequence, of the frame it pushes in push p (None: absent)."""
    if s == 1:
        return p - LATE if p >= LATE else None
    return p


def _base(s, p):
    """Index, in stream s's sequence, of frame 0 of the stream as it runs in push p."""
    return RESET_AT if s == 2 and p >= RESET_AT else 0


def _fields(r):
    return (r.pred_pose_enc, r.pred_tracks, r.pred_score)


def _diff(a, b):
    return [float((x.double() - y.double()).abs().max()) for x, y in zip(a, b)]


class _Counter:
    """Counts the calls of model.<name> (and keeps the `tracks` shapes) while active."""

    def __init__(self, model, name):
        self.model, self.name, self.calls = model, name, []

    def __enter__(self):
        orig = getattr(self.model, self.name)

        def counted(*a, **kw):
            self.calls.append(tuple(kw["tracks"].shape) if "tracks" in kw else tuple(a[0].shape))
            return orig(*a, **kw)
        setattr(self.model, self.name, counted)
        return self

    def __exit__(self, *exc):
        delattr(self.model, self.name)  # the instance attribute; the class's method is back


def _run_alone(model, seqs, dtype):
    """Three independent PoseStream objects fed the scenario -> {(push, stream, frame_index): result}."""
    from comet_amd.stream import PoseStream
    streams = [PoseStream(model, window=T, stride=1, capacity=CAP, precision=dtype) for _ in SEEDS]
    out = {}
    for p in range(PUSHES):
        if p == RESET_AT:
            streams[2].reset()
        for s, (frames, q) in enumerate(seqs):
            f = _frame_of(s, p)
            if f is not None:
                for r in streams[s].push(frames[f], query_points=q):
                    out[(p, s, r.frame_index)] = r
    return out


def _run_pool(model, seqs, dtype):
    from comet_amd.stream import StreamPool
    pool = StreamPool(model, streams=3, window=T, stride=1, capacity=CAP, precision=dtype)
    qs = {s: q for s, (_, q) in enumerate(seqs)}
    out, per_push = {}, []
    for p in range(PUSHES):
        if p == RESET_AT:
            pool.reset(2)
        ids = [s for s in range(3) if _frame_of(s, p) is not None]
        got = pool.push(torch.stack([seqs[s][0][_frame_of(s, p)] for s in ids]), streams=ids, query_points=qs)
        assert [s for s, _ in got] == sorted(s for s, _ in got)
        per_push.append(len(got))
        for s, r in got:
            assert (p, s, r.frame_index) not in out
            out[(p, s, r.frame_index)] = r
    return out, per_push


@pytest.fixture(scope="module")
def alone(model, seqs):
    return {dtype: _run_alone(model, seqs, dtype) for dtype in DTYPES}


@pytest.fixture(scope="module")
def floors(model, seqs, alone):
    return _floors(model, seqs, alone)


def _floors(model, seqs, alone):
    """{dtype: [floor of pred_pose_enc, pred_tracks (pixels), pred_score]}: see the module docstring."""
    from comet_amd import functional as F
    out = {}
    for dtype in DTYPES:
        worst = [0.0, 0.0, 0.0]
        for p in range(PUSHES):
            due = sorted((s, k) for (pp, s, k) in alone[dtype] if pp == p)
            if len(due) < 2:
                continue  # a batch of one window is the window alone
            wins = [seqs[s][0][_base(s, p) + k:_base(s, p) + k + T] for s, k in due]
            trk = [seqs[s][1][None].expand(T, -1, 2) for s, _ in due]
            with F.precision(dtype), torch.no_grad():
                ob = model.forward_all(torch.stack(wins), training=False, tracks=torch.stack(trk))
                for b, (w, t) in enumerate(zip(wins, trk)):
                    o1 = model(w[None], training=False, tracks=t[None])
                    d = _diff((ob["pred_pose_enc"][b * T:(b + 1) * T], ob["pred_tracks"][b],
                               ob["_track_predictions"]["pred_score"][b]),
                              (o1["pred_pose_enc"], o1["pred_tracks"][0], o1["_track_predictions"]["pred_score"][0]))
                    print(f"floor {dtype} push {p} B={len(due)} window {due[b]}: " + ", ".join(
                        f"{n} {v:.3e}" for n, v in zip(NAMES, d)))
                    worst = [max(a, c) for a, c in zip(worst, d)]
        out[dtype] = worst
        print(f"floor {dtype}: " + ", ".join(f"{n} {v:.3e}" for n, v in zip(NAMES, worst)))
    return out


def _within(got, ref, floor, what):
    d = _diff(_fields(got), _fields(ref))
    print(f"{what}: " + ", ".join(f"{n} {v:.3e} (floor {f:.3e})" for n, v, f in zip(NAMES, d, floor)))
    for n, v, f in zip(NAMES, d, floor):
        assert v <= FACTOR * f, f"{what}, {n}: {v:.3e} > {FACTOR} x floor {f:.3e}"


# ------------------------------------------------------------------------------------------------
# 3. one stream: the pool is PoseStream
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_of_one_stream_equals_pose_stream_bit_for_bit(model, seq_one, dtype):
    """S = 1, 7 frames, stride 1, capacity == window (the ring wraps), with an anchor: every field of
    every result, the absolute R and T included, is equal to PoseStream's."""
    from comet_amd.stream import PoseStream, StreamPool
    frames, q = seq_one
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device="cuda")
    anchor = (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device="cuda"), 268.44,
              torch.tensor([0.5], dtype=torch.float64), "AMD")
    one = PoseStream(model, window=T, stride=1, anchor=anchor, precision=dtype)
    pool = StreamPool(model, streams=1, window=T, stride=1, anchors=[anchor], precision=dtype)
    n = 0
    for f in range(7):
        ref = one.push(frames[f], query_points=q)
        got = pool.push(frames[f:f + 1], query_points=q)
        assert [s for s, _ in got] == [0] * len(ref) and len(ref) == (1 if f >= T - 1 else 0)
        for (_, g), r in zip(got, ref):
            n += 1
            assert g.frame_index == r.frame_index
            for name in ("pred_pose_enc", "pred_tracks", "pred_score", "R", "T"):
                a, b = getattr(g, name), getattr(r, name)
                assert a.shape == b.shape and a.dtype == b.dtype, name
                assert torch.equal(a, b), f"frame {f}, {name}: max diff {float((a.double() - b.double()).abs().max()):.3e}"
    assert n == 4


# ------------------------------------------------------------------------------------------------
# 4. three streams out of phase
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_streams_out_of_phase(model, seqs, alone, floors, dtype):
    """Stream 1 joins two pushes late, stream 2 is reset after its 5th frame: the pool returns the
    results three independent PoseStream objects return, push by push and stream by stream, each
    within 4 x floor; and it does so with one frame_stages call per push and one forward_all call
    per push that completes a hop."""
    with _Counter(model, "frame_stages") as fs, _Counter(model, "forward_all") as fa:
        got, per_push = _run_pool(model, seqs, dtype)
    ref = alone[dtype]
    assert sorted(got) == sorted(ref)
    assert len(ref) == 13 and per_push == [0, 0, 0, 2, 2, 2, 2, 2, 3]
    assert [c[0] for c in fs.calls] == [2, 2, 3, 3, 3, 3, 3, 3, 3]
    assert fa.calls == [(n, T, N, 2) for n in per_push if n]
    for key in sorted(ref):
        _within(got[key], ref[key], floors[dtype], f"pool {dtype} (push, stream, window) {key}")


# ------------------------------------------------------------------------------------------------
# 5. query counts that differ
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_query_counts_are_grouped(model, seqs, floors, dtype):
    """Streams 0 and 2 with N = 64 and stream 1 with N = 48 fall due in one push: two batched calls
    (B = 2 and B = 1), three results, each within the bound of its single-stream result."""
    from comet_amd.stream import PoseStream, StreamPool
    qs = {0: seqs[0][1], 1: seqs[1][1][:48], 2: seqs[2][1]}
    pool = StreamPool(model, streams=3, window=T, precision=dtype)
    got = []
    with _Counter(model, "forward_all") as fa:
        for f in range(T):
            got += pool.push(torch.stack([seqs[s][0][f] for s in range(3)]), query_points=qs)
    assert fa.calls == [(2, T, 64, 2), (1, T, 48, 2)]
    assert [s for s, _ in got] == [0, 1, 2]
    for s, g in got:
        one = PoseStream(model, window=T, precision=dtype)
        ref = one.push(seqs[s][0][:T], query_points=qs[s])
        assert len(ref) == 1 and g.frame_index == ref[0].frame_index == 0
        assert g.pred_tracks.shape == (T, qs[s].shape[0], 2) and g.pred_score.shape == (T, qs[s].shape[0])
        _within(g, ref[0], floors[dtype], f"mixed counts {dtype} stream {s}")


# ------------------------------------------------------------------------------------------------
# 6. loop integration
# ------------------------------------------------------------------------------------------------
def test_stream_eval_pool_writes_one_csv_per_sequence(model, seqs, floors, tmp_path):
    """Two sequences of 6 and 9 frames on two streams: 3 and 6 rows, the pose columns within the
    bound of stream_eval run on each sequence alone (after the shorter one ends the pool goes on
    with one stream)."""
    import csv
    from comet_amd import loop
    from comet_amd.config import AttrDict
    q = seqs[0][1]
    g = torch.Generator().manual_seed(3)
    raw = {name: [torch.randint(0, 256, (160, 176, 3), dtype=torch.uint8, generator=g).numpy() for _ in range(n)]
           for name, n in (("a", 6), ("b", 9))}
    box = (8, 0, 168, 160)
    cfg = AttrDict.wrap({"stream": {"enable": True, "window": T, "stride": 1, "streams": 2},
                         "train": {"img_size": HW}, "mixed_precision": "bf16"})
    hops = loop.stream_eval_pool(model, [(name, iter(fr), box) for name, fr in raw.items()], cfg,
                                 str(tmp_path / "pool"), query_points=q)
    assert hops == {"a": 3, "b": 6}
    pose = ("du", "dv", "dd", "qw", "qx", "qy", "qz")
    floor = floors[torch.bfloat16][0]
    for name, fr in raw.items():
        path = str(tmp_path / f"{name}_alone.csv")
        assert loop.stream_eval(model, iter(fr), cfg, box, path, query_points=q) == hops[name]
        ref = list(csv.DictReader(open(path)))
        rows = list(csv.DictReader(open(tmp_path / "pool" / f"{name}.csv")))
        assert len(rows) == hops[name]
        assert [(r["frame_index"], r["newest_frame"]) for r in rows] == [(r["frame_index"], r["newest_frame"]) for r in ref]
        for r, e in zip(rows, ref):
            d = max(abs(float(r[k]) - float(e[k])) for k in pose)
            print(f"stream_eval_pool {name} window {r['frame_index']}: pose columns {d:.3e} (floor {floor:.3e})")
            assert d <= FACTOR * floor, f"{name}, window {r['frame_index']}: {d:.3e} > {FACTOR} x floor {floor:.3e}"
            assert float(r["hop_ms"]) > 0
    with pytest.raises(ValueError, match="opt-in"):
        loop.stream_eval_pool(model, [], AttrDict.wrap({"stream": {"enable": False}}), str(tmp_path / "off"))
