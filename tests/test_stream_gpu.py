"""The online path on the GPU (comet_amd/stream.py, csrc/stream.hip, DESIGN.md "Online / streaming
inference") at the golden model configuration of tests/test_model_gpu.py (PRNG weights seed 0),
T = 4, 128 x 128 frames, N = 64 query points, synthetic frames of oracle.prng seed SEED_X.

Tolerances of the stream-vs-closed-window comparisons. The stream runs the per-frame stages
(BasicEncoder, DINOv2, input_transform) on 1 (or k) frames per call instead of T, so their GEMMs and
convolutions take other plans (split-K at small M) and sum in another order; equality is not
expected. The floor is what a change of batch composition alone does on the closed path: a window's
per-frame stages evaluated inside a 2T-frame call (the window's T frames followed by T other
frames), the rest of the model unchanged, against the window evaluated alone -- per output and
precision mode, the largest difference over the windows the tests use (fixture `floors`, measured
in the run itself and printed). Every stream result must be within 4 x that floor (the factor the
SIFT tests use over their float floors, for the same reason). SEED_X = 1: none of its windows'
floors shows a flip of compute_score_fn's 5 x 5 window (a flip moves pred_score by ~1e-1 at once)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, HW, N = 4, 128, 64
SEED_W, SEED_X = 0, 1
NF = 2 * T + 1  # frames of the longest test: capacity == window, T + capacity + 1 pushes
FACTOR = 4.0
DTYPES = [torch.float32, torch.bfloat16]
NAMES = ("pred_pose_enc", "pred_tracks", "pred_score")


# ------------------------------------------------------------------------------------------------
# 1. the gather kernel
# ------------------------------------------------------------------------------------------------
def _rings(cap, T_, widths, gen):
    """[(ring [cap, ...], window [T_, ...] inside a buffer with one guard slot)] of the given dtypes."""
    out = []
    for dtype, n in widths:
        if dtype == torch.uint8:
            ring = torch.randint(0, 256, (cap, n), device="cuda", dtype=torch.uint8, generator=gen)
        else:
            ring = torch.randn(cap, n, device="cuda", generator=gen).to(dtype)
        big = torch.zeros(T_ + 1, n, device="cuda", dtype=dtype)
        big[T_] = 7
        out.append((ring, big))
    return out


GATHER_SLOTS = [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 0], [3, 4, 0, 1], [4, 0, 1, 2], [4, 1, 3, 0], [2, 2, 0, 4]]


@pytest.mark.parametrize("max_blocks", [0, 3])
def test_ring_gather_is_exact(max_blocks):
    """Three rings with slots of 16 B (one vector), 4 112 B (257 vectors: a tail below one
    workgroup's stride) and 1 048 592 B (65 537 vectors: 65 tiles per slot, the last with one
    vector), capacity 5, T 4, slot tables that wrap, skip and repeat: bit-identical to
    torch.index_select, nothing written behind the window. max_blocks = 3 makes every workgroup
    take many tiles (the grid-stride path) and adds a fourth ring."""
    import ctypes
    from comet_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    widths = [(torch.uint8, 16), (torch.bfloat16, 2056), (torch.float32, 262148)]
    if max_blocks:
        widths.append((torch.bfloat16, 8 * 1024 + 8))
    rings = _rings(5, 4, widths, gen)
    assert [r[0].numel() * r.element_size() for r, _ in rings][:3] == [16, 4112, 1048592]
    for slots in GATHER_SLOTS:
        dev = torch.tensor(slots, dtype=torch.int32, device="cuda")
        for _, big in rings:
            big[:4] = 0
        ops.ring_gather([(r, big[:4]) for r, big in rings], dev, (ctypes.c_int32 * 4)(*slots), max_blocks=max_blocks)
        torch.cuda.synchronize()
        for r, big in rings:
            ref = torch.index_select(r, 0, dev.long())
            assert torch.equal(big[:4].view(torch.uint8), ref.view(torch.uint8)), (slots, r.dtype)
            assert bool((big[4] == 7).all()), "guard slot behind the window was written"


def test_ring_gather_wrapper_rejects_mismatched_tensors():
    import ctypes
    from comet_amd import _lib, ops
    ring = torch.zeros(5, 16, device="cuda")
    slots = torch.zeros(4, dtype=torch.int32, device="cuda")
    host = (ctypes.c_int32 * 4)(0, 1, 2, 3)
    with pytest.raises(_lib.CometHipError):
        ops.ring_gather([(ring, torch.zeros(4, 8, device="cuda"))], slots, host)
    with pytest.raises(_lib.CometHipError):
        ops.ring_gather([(ring, torch.zeros(4, 16, device="cuda", dtype=torch.bfloat16))], slots, host)
    with pytest.raises(_lib.CometHipError, match="outside the ring"):
        ops.ring_gather([(ring, torch.zeros(4, 16, device="cuda"))], slots, (ctypes.c_int32 * 4)(0, 1, 2, 5))


# ------------------------------------------------------------------------------------------------
# the model, the frames, the closed-window results and the floors (computed once)
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


@pytest.fixture(scope="module")
def data():
    from oracle import prng
    img, tracks, _ = prng.synthetic_batch(SEED_X, 1, NF, HW, HW, N)
    return img[0].cuda(), tracks[0, 0].cuda()  # frames [NF, 3, H, W], query points [N, 2]


def _outs(o):
    return (o["pred_pose_enc"].clone(), o["pred_tracks"][0].clone(), o["_track_predictions"]["pred_score"][0].clone())


def _tracks(q):
    return q[None, None].expand(1, T, -1, 2)


class _Closed:
    """model(frames[k : k + T], training=False, tracks=q) per window and precision, computed once."""

    def __init__(self, model, frames, q):
        self.model, self.frames, self.q, self.memo = model, frames, q, {}

    def __call__(self, k, dtype):
        from comet_amd import functional as F
        if (k, dtype) not in self.memo:
            with F.precision(dtype):
                o = self.model(self.frames[None, k:k + T], training=False, tracks=_tracks(self.q))
            self.memo[(k, dtype)] = _outs(o)
        return self.memo[(k, dtype)]


@pytest.fixture(scope="module")
def closed(model, data):
    return _Closed(model, *data)


def _diff(a, b):
    return [float((x.double() - y.double()).abs().max()) for x, y in zip(a, b)]


@pytest.fixture(scope="module")
def floors(model, data, closed):
    """{dtype: [floor of pred_pose_enc, pred_tracks (pixels), pred_score]}: see the module docstring."""
    from comet_amd import functional as F
    from comet_amd.models.E2Epose2 import FrameCache
    frames, q = data
    out = {}
    for dtype in DTYPES:
        worst = [0.0, 0.0, 0.0]
        for k in range(NF - T + 1):
            idx = [(k + i) % NF for i in range(2 * T)]  # the window, then T other frames
            with F.precision(dtype), torch.no_grad():
                c = model.frame_stages(frames[idx])
                c = FrameCache(fmaps=c.fmaps[:, :T].contiguous(), refine_frames=c.refine_frames[:, :T].contiguous(),
                               tokens=c.tokens[:T].contiguous())
                o = model(frames[None, k:k + T], training=False, tracks=_tracks(q), frame_cache=c)
            d = _diff(_outs(o), closed(k, dtype))
            print(f"floor {dtype} window {k}: " + ", ".join(f"{n} {v:.3e}" for n, v in zip(NAMES, d)))
            worst = [max(a, b) for a, b in zip(worst, d)]
        out[dtype] = worst
        print(f"floor {dtype}: " + ", ".join(f"{n} {v:.3e}" for n, v in zip(NAMES, worst)))
    return out


def _check(results, first_frames, closed, floors, dtype, what):
    assert [r.frame_index for r in results] == first_frames, what
    for r in results:
        d = _diff((r.pred_pose_enc, r.pred_tracks, r.pred_score), closed(r.frame_index, dtype))
        print(f"{what} {dtype} window {r.frame_index}: " + ", ".join(
            f"{n} {v:.3e} (floor {f:.3e})" for n, v, f in zip(NAMES, d, floors[dtype])))
        for n, v, f in zip(NAMES, d, floors[dtype]):
            assert v <= FACTOR * f, f"{what}, window {r.frame_index}, {n}: {v:.3e} > {FACTOR} x floor {f:.3e}"


# ------------------------------------------------------------------------------------------------
# 2. the default path and the frame_cache path are the same computation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_frame_cache_of_the_whole_window_is_bit_identical(model, data, closed, dtype):
    """frame_cache built by the three per-frame stages on the whole [T] window at once: the same
    batch composition as the default path, so every output is equal bit for bit."""
    from comet_amd import functional as F
    frames, q = data
    with F.precision(dtype), torch.no_grad():
        cache = model.frame_stages(frames[:T])
        o = model(frames[None, :T], training=False, tracks=_tracks(q), frame_cache=cache)
    for n, a, b in zip(NAMES, _outs(o), closed(0, dtype)):
        assert torch.equal(a, b), f"{n}: max diff {float((a.double() - b.double()).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------
# 3. - 5. the stream against closed windows
# ------------------------------------------------------------------------------------------------
def _stream(model, dtype, **kw):
    from comet_amd.stream import PoseStream
    return PoseStream(model, window=T, precision=dtype, **kw)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stream_equals_closed_windows(model, data, closed, floors, dtype, stride):
    frames, q = data
    s = _stream(model, dtype, stride=stride, capacity=T + 2)
    results = []
    for f in range(T + 3):
        got = s.push(frames[f], query_points=q)
        assert len(got) == (1 if f >= T - 1 and (f - T + 1) % stride == 0 else 0)
        results += got
    _check(results, list(range(0, 4, stride)), closed, floors, dtype, f"stream stride {stride}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_push(model, data, closed, floors, dtype):
    """k = 3 frames per push: one batched call of the per-frame stages, hops for every window the
    push completes, within the same bound; the ring holds frame f in slot f % capacity, and two
    streams of different capacity that push the same frames with the same k hold the same bits."""
    frames, q = data
    a, b = _stream(model, dtype, capacity=T), _stream(model, dtype, capacity=T + 1)
    ra, rb = [], []
    for lo in (0, 3, 6):
        ra += a.push(frames[lo:min(lo + 3, T + 3)], query_points=q)
        rb += b.push(frames[lo:min(lo + 3, T + 3)], query_points=q)
    _check(ra, [0, 1, 2, 3], closed, floors, dtype, "batched push, capacity T")
    _check(rb, [0, 1, 2, 3], closed, floors, dtype, "batched push, capacity T + 1")
    for f in range(3, T + 3):  # the frames both rings still hold
        for x, y in zip(a._rings, b._rings):
            assert torch.equal(x[f % T], y[f % (T + 1)]), f"frame {f}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_around_never_reads_stale_slots(model, data, closed, floors, dtype):
    """capacity == window, T + capacity + 1 frames: every slot has been overwritten at least twice
    when the last window is gathered."""
    frames, q = data
    s = _stream(model, dtype, capacity=T, stride=1)
    results = []
    for f in range(NF):
        results += s.push(frames[f], query_points=q)
    assert len(results) == NF - T + 1
    _check(results[-1:], [NF - T], closed, floors, dtype, "wrap-around")
    s.reset()
    assert s.push(frames[:T - 1], query_points=q) == []
    _check(s.push(frames[T - 1], query_points=q), [0], closed, floors, dtype, "after reset")


def test_query_fn_gets_the_first_frame_of_the_window(model, data):
    frames, q = data
    seen = []

    def query_fn(frame):
        seen.append(frame.clone())
        return q
    s = _stream(model, torch.bfloat16, stride=2, query_fn=query_fn)
    n = sum(len(s.push(frames[f])) for f in range(T + 2))
    assert n == 2 and len(seen) == 2
    assert torch.equal(seen[0], frames[0]) and torch.equal(seen[1], frames[2])


# ------------------------------------------------------------------------------------------------
# 6. absolute poses
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
def test_anchor_chaining(model, data, stride):
    """Window k's first frame decodes to exactly the pose window k - 1 reported for that frame."""
    from comet_amd import ops
    from comet_amd.models.utils import INTRINSICS
    frames, q = data
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device="cuda")
    R0 = R0 / R0.norm()
    uvz0 = torch.tensor([331.25, 247.5, 11.375], device="cuda")
    ratio = torch.tensor([0.5], dtype=torch.float64)
    s = _stream(model, torch.float32, stride=stride, anchor=(R0, uvz0, 268.44, ratio, "AMD"))
    results = []
    for f in range(T + 3):
        results += s.push(frames[f], query_points=q)
    assert len(results) == len(range(0, 4, stride)) >= 2
    first = results[0]
    assert first.R.shape == (T, 4) and first.T.shape == (T, 3) and first.T.dtype == torch.float64
    R, Tx = ops.pose_decode(first.pred_pose_enc, R0.expand(T, 4).contiguous(), uvz0.expand(T, 3).contiguous(), ratio,
                            INTRINSICS["AMD"], 1, T)
    keep = [i for i in range(T) if i != stride]
    assert torch.equal(first.R[keep], R[keep]) and torch.equal(first.T[keep], Tx[keep])
    # the chained frame is reported with its (u, v, z) rounded to f32: within f32 rounding of the direct decode
    assert torch.allclose(first.R[stride], R[stride], rtol=0, atol=1e-6)
    assert torch.allclose(first.T[stride], Tx[stride], rtol=1e-6, atol=0)
    for a, b in zip(results, results[1:]):
        assert b.frame_index == a.frame_index + stride
        assert torch.equal(b.R[0], a.R[stride]), (a.frame_index, b.R[0], a.R[stride])
        assert torch.equal(b.T[0], a.T[stride]), (a.frame_index, b.T[0], a.T[stride])


# ------------------------------------------------------------------------------------------------
# loop integration
# ------------------------------------------------------------------------------------------------
def test_stream_eval_writes_one_row_per_hop(model, data, closed, tmp_path):
    import csv
    from comet_amd import loop
    from comet_amd.config import AttrDict
    _, q = data
    g = torch.Generator().manual_seed(3)
    raw = [torch.randint(0, 256, (160, 176, 3), dtype=torch.uint8, generator=g).numpy() for _ in range(T + 2)]
    cfg = AttrDict.wrap({"stream": {"enable": True, "window": T, "stride": 1}, "train": {"img_size": HW},
                         "mixed_precision": "bf16"})
    path = str(tmp_path / "stream.csv")
    assert loop.stream_eval(model, iter(raw), cfg, (8, 0, 168, 160), path, query_points=q) == 3
    rows = list(csv.DictReader(open(path)))
    assert [int(r["frame_index"]) for r in rows] == [0, 1, 2]
    assert [int(r["newest_frame"]) for r in rows] == [T - 1, T, T + 1]
    for r in rows:
        quat = torch.tensor([float(r[k]) for k in ("qw", "qx", "qy", "qz")])
        assert abs(float(quat.norm()) - 1) < 1e-3 and float(r["hop_ms"]) > 0


# ------------------------------------------------------------------------------------------------
# several hops inside one push
# ------------------------------------------------------------------------------------------------
class _FrameWise:
    """The model with frame_stages run one frame at a time and concatenated: what the rings hold then
    does not depend on how the frames were chunked into pushes."""

    def __init__(self, model):
        self.model = model

    def __getattr__(self, name):
        return getattr(self.model, name)

    def frame_stages(self, frames):
        from comet_amd.models.E2Epose2 import FrameCache
        cs = [self.model.frame_stages(frames[i:i + 1]) for i in range(frames.shape[0])]
        return FrameCache(fmaps=torch.cat([c.fmaps for c in cs], 1), refine_frames=torch.cat([c.refine_frames for c in cs], 1),
                          tokens=torch.cat([c.tokens for c in cs]))


def test_hops_inside_one_push_leave_their_state_to_the_next(model, data):
    """fuse + carry + warm + landmarks + pnp with feedback, stride 1, T + 5 frames pushed one at a time and
    in chunks of 3 (up to three hops complete inside one push): hop i is finished -- carried tracks, fused
    rows, landmark rows, the PnP poses fed back -- before frame i + 1 is stored, so every field of every
    result is the same bits."""
    from comet_amd.stream import StreamResult
    frames, _ = data
    cand = (torch.rand(96, 2, generator=torch.Generator().manual_seed(7)) * (HW - 1)).cuda()
    R0 = torch.tensor([0.8, 0.2, -0.4, 0.4], device="cuda")
    anchor = (R0 / R0.norm(), torch.tensor([331.25, 247.5, 11.375], device="cuda"), 268.44,
              torch.tensor([0.5], dtype=torch.float64), "AMD")

    def run(k):
        s = _stream(_FrameWise(model), torch.float32, stride=1, anchor=anchor, fuse=True, carry=True, carry_tracks=N,
                    carry_min_score=0.5, candidate_fn=lambda frame: cand, warm=True, landmarks=True,
                    track_intr=(150.0, 150.0, 63.5, 63.5), lm_min_obs=2, pnp=True, pnp_huber_px=3.0, pnp_weight=1.0)
        return [r for lo in range(0, T + 5, k) for r in s.push(frames[lo:lo + k])]

    one, three = run(1), run(3)
    assert [r.frame_index for r in one] == [r.frame_index for r in three] == list(range(6))
    assert all(bool((r.track_src >= 0).any()) for r in one[1:]), "no track was carried: the hops would share no state"
    for a, b in zip(one, three):
        for name in StreamResult._fields + tuple(StreamResult.__annotations__):
            x, y = getattr(a, name), getattr(b, name)
            assert x is not None and y is not None, name
            if torch.is_tensor(x):  # (the bits: an unsolved frame's +inf or a NaN compares as itself)
                x, y = x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)
                assert torch.equal(x, y), (a.frame_index, name)
            else:
                assert x == y, (a.frame_index, name)
