"""The landmark map on the GPU (comet_landmark_update in csrc/landmark.hip, ops.landmark_update,
stream.LandmarkMap, PoseStream / StreamPool landmarks=True; DESIGN.md "Landmarks").

Kernel: against the float64 restatement tests/landmark_numpy.py, which performs the same IEEE operations
in the same order. Bounds: X within 1e-10 (1 + |X|), accumulator rows within 1e-10 of the row's trace
(the f64 bound of the fusion tests), n_obs / state / acc_id equal, err_px within 1e-4 px. Every input
set is first checked on the CPU: no pivot of a solved slot lies between 1e-12 and 1e-3 of the diagonal,
so no case sits near min_pivot.

End to end: the golden configuration of tests/test_carry_gpu.py (PRNG weights seed 0, T = 4, 128^2,
N = 64, its fixed seeded candidates, carry_min_score 0.5, f32, oracle.prng frames of seed 1). Random
weights give arbitrary geometry, so only the mechanics are asserted there, never accuracy."""
import numpy as np
import pytest
import torch

import landmark_numpy as ln

pytestmark = pytest.mark.gpu

INT32_MIN = -2 ** 31
INTR = (300.0, 310.0, 63.5, 60.0)
X_TOL, ROW_TOL, ERR_TOL = 1e-10, 1e-10, 1e-4
WORST = {"X": 0.0, "row": 0.0, "err": 0.0}  # measured maxima over the module, printed by the last kernel test


# ------------------------------------------------------------------------------------------------
# the kernel against the restatement
# ------------------------------------------------------------------------------------------------
class _Device:
    """The landmark state on the device, updated from numpy inputs."""

    def __init__(self, streams, N):
        self.acc = torch.zeros(streams * N, ln.LM_ROW, dtype=torch.float64, device="cuda")
        self.acc_id = torch.full((streams * N,), -1, dtype=torch.int32, device="cuda")

    def update(self, inp, s, **kw):
        import ctypes
        from comet_amd import ops
        d = {k: None if v is None else torch.as_tensor(v).cuda().contiguous() for k, v in inp.items()}
        idx = [int(v) for v in inp["stream_idx"]]
        flat = [float(v) for v in np.asarray(inp["intr"]).ravel()]
        out = ops.landmark_update(d["tracks"], d["R"], d["T"], d["ids"], d["src"], d["stream_idx"],
                                  (ctypes.c_int32 * len(idx))(*idx), d["intr"], (ctypes.c_double * len(flat))(*flat),
                                  self.acc, self.acc_id, s, d["weights"], **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out._asdict().items()}


def _pivots_clear_of_the_bound(ref, what):
    """Every pivot that decides a solved slot's state is at least 1e-3 of max(diag M), the scale of the
    kernel's threshold, or at most 1e-12 of it: the pivots in elimination order up to and including the
    first one at or below 1e-12 (the later ones are quotients by it and decide nothing)."""
    piv, diag = ref["pivots"].reshape(-1, 3), ref["diag"].reshape(-1)
    for d, m in zip(piv, diag):
        if not m > 0.0:  # nothing solved (NaN), or an all-zero M whose pivots are at the threshold's 0
            continue
        for p in d:
            assert p >= 1e-3 * m or p <= 1e-12 * m, f"{what}: a pivot at {p / m:.3e} of max(diag M)"
            if p <= 1e-12 * m:
                break


def _compare(got, ref, acc, acc_id, dev, what):
    _pivots_clear_of_the_bound(ref, what)
    for name in ("n_obs", "state"):
        assert got[name].dtype == ref[name].dtype == np.int32 and (got[name] == ref[name]).all(), (what, name)
    assert (dev.acc_id.cpu().numpy() == acc_id).all(), (what, "acc_id")
    dx = np.abs(got["X"] - ref["X"]).max(-1) / (1.0 + np.linalg.norm(ref["X"], axis=-1))
    on = ref["state"] == ln.VALID
    assert (got["X"][~on] == 0).all() and np.isposinf(got["err_px"][~on]).all(), (what, "states other than 1")
    de = np.abs(got["err_px"][on].astype(np.float64) - ref["err_px"][on]) if on.any() else np.zeros(1)
    rows = dev.acc.cpu().numpy()
    trace = rows[:, 0] + rows[:, 3] + rows[:, 5]
    dr = np.abs(rows - acc).max(-1) / np.where(trace > 0, trace, 1.0)
    assert np.isfinite(rows).all() == np.isfinite(acc).all()
    WORST["X"], WORST["row"], WORST["err"] = max(WORST["X"], dx.max()), max(WORST["row"], np.nanmax(dr)), max(WORST["err"], de.max())
    assert dx.max() <= X_TOL, (what, "X", dx.max())
    assert np.nanmax(dr) <= ROW_TOL, (what, "rows", np.nanmax(dr))
    assert de.max() <= ERR_TOL, (what, "err_px", de.max())


def _poses(seed, frames, still=False):
    """A body 6 units in front of the camera that turns 0.4 rad per frame and drifts -> q [F, 4] f32,
    t [F, 3] f64."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    q = np.stack([ln.quat_from_axis_angle(axis, 0.0 if still else 0.4 * f + 0.1) for f in range(frames)])
    t = np.stack([np.array([0.1, -0.05, 6.0]) + (0.0 if still else 0.05 * f) * np.array([1.0, 0.5, 2.0])
                  for f in range(frames)])
    return q.astype(np.float32), t


def _window(X, q, t, f0, Tw, inverse):
    """Exact projections of the body points on the frames [f0, f0 + Tw), rounded to f32 -> [Tw, N, 2]."""
    return np.stack([ln.project(X, q[f].astype(np.float64), t[f], INTR, inverse)[0] for f in range(f0, f0 + Tw)]).astype(np.float32)


def case_a():
    """Two hops per launch (T = 4, N = 64, s = 1, min_obs = 2), two chained launches. Hop 0 (stream 2)
    watches a turning body, hop 1 (stream 0) one that does not move relative to the camera. Named slots
    of hop 0 take every branch in the second launch."""
    n, Tw, N, s = 2, 4, 64, 1
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (N, 3))
    slots = dict(carried=0, birth=1, pad=2, mismatch=3, nan_x=4, inf_y=5, zero_w=6, negative_w=7, nan_w=8, behind=9)
    X[slots["behind"]] = (0.2, -0.1, -30.0)  # behind the camera in every frame; its pixels are still finite
    poses = [_poses(1, 8), _poses(2, 8, still=True)]
    calls = []
    for c in range(2):
        tracks = np.stack([_window(X, q, t, c * s, Tw, 0) for q, t in poses])
        R = np.stack([q[c * s:c * s + Tw] for q, _ in poses])
        T = np.stack([t[c * s:c * s + Tw] for _, t in poses])
        ids = np.tile(np.arange(N, dtype=np.int32), (n, 1))
        src = ids.copy() if c else -1 - ids
        w = rng.uniform(0.5, 1.5, (n, Tw, N)).astype(np.float32)
        if c:
            ids[0, slots["birth"]], src[0, slots["birth"]] = 100, -1 - 7
            ids[0, slots["pad"]], src[0, slots["pad"]] = -1, INT32_MIN + 0
            ids[0, slots["mismatch"]] = 101
            tracks[0, 0, slots["nan_x"], 0] = np.nan
            tracks[0, 0, slots["inf_y"], 1] = np.inf
            w[0, 0, slots["zero_w"]], w[0, 0, slots["negative_w"]], w[0, 0, slots["nan_w"]] = 0.0, -1.0, np.nan
        calls.append(dict(tracks=tracks, R=R, T=T, ids=ids, src=src, stream_idx=np.array([2, 0], np.int32),
                          intr=np.array([INTR, INTR]), weights=w))
    return calls, slots, dict(n=n, Tw=Tw, N=N, s=s, streams=3)


def test_case_a_every_branch_occurs_and_matches():
    calls, sl, m = case_a()
    N, s = m["N"], m["s"]
    acc, acc_id = ln.new_state(m["streams"], N)
    dev = _Device(m["streams"], N)
    kw = dict(min_obs=2, min_pivot=1e-8)
    refs = []
    for c, inp in enumerate(calls):
        refs.append(ln.update(**inp, acc=acc, acc_id=acc_id, s=s, **kw))
        got = dev.update(inp, s, **kw)
        _compare(got, refs[-1], acc, acc_id, dev, f"case a launch {c}")
    first, ref = refs
    row = lambda j: acc[2 * N + j]  # noqa: E731  (hop 0 is stream 2)
    assert (first["n_obs"] == 1).all() and (first["state"] == ln.NONE).all(), "n_obs < min_obs on the first launch"
    assert ref["n_obs"][0, sl["carried"]] == 2 and ref["state"][0, sl["carried"]] == ln.VALID, "a carried add"
    assert ref["err_px"][0, sl["carried"]] < 1e-2
    for name in ("birth", "mismatch"):
        assert ref["n_obs"][0, sl[name]] == 1 and ref["state"][0, sl[name]] == ln.NONE, name
    assert acc_id[2 * N + sl["birth"]] == 100 and acc_id[2 * N + sl["mismatch"]] == 101
    assert (row(sl["pad"]) == 0).all() and acc_id[2 * N + sl["pad"]] == -1 and ref["n_obs"][0, sl["pad"]] == 0, "a pad"
    for name in ("nan_x", "inf_y", "zero_w", "negative_w", "nan_w"):
        assert ref["n_obs"][0, sl[name]] == 1 and np.isfinite(row(sl[name])).all(), name
    assert ref["n_obs"][0, sl["behind"]] == 2 and ref["state"][0, sl["behind"]] == ln.BEHIND, "behind the camera"
    assert (ref["n_obs"][1] == 2).all() and (ref["state"][1] == ln.ILL).all(), "no relative motion: state 2"
    assert (acc[N:2 * N] == 0).all() and (acc_id[N:2 * N] == -1).all(), "stream 1 took no hop"
    assert sorted(set(ref["state"].ravel().tolist())) == [ln.NONE, ln.VALID, ln.ILL, ln.BEHIND]


def shape_case(n, Tw, N, s, weighted, inverse, launches=3):
    """`launches` chained launches of n hops: every stream watches its own turning body; slots are
    carried, reborn, padded or handed a foreign id at random, a few pixels and weights are not usable."""
    rng = np.random.default_rng(1000 * n + 100 * Tw + N + s)
    streams = n + 1
    order = np.array(rng.permutation(streams)[:n], np.int32)
    X = rng.uniform(-1, 1, (n, N, 3))
    poses = [_poses(10 + h, launches * s + Tw) for h in range(n)]
    ids = np.tile(np.arange(N, dtype=np.int32), (n, 1))
    next_id = N
    calls = []
    for c in range(launches):
        tracks = np.stack([_window(X[h], *poses[h], c * s, Tw, inverse) for h in range(n)])
        R = np.stack([q[c * s:c * s + Tw] for q, _ in poses])
        T = np.stack([t[c * s:c * s + Tw] for _, t in poses])
        src = np.tile(np.arange(N, dtype=np.int32), (n, 1)) if c else -1 - ids
        ids = ids.copy()
        if c and N > 1:
            u = rng.random((n, N))
            for h, j in np.argwhere(u < 0.15):      # reborn: a new id, src a candidate
                ids[h, j], src[h, j] = next_id, -1 - int(rng.integers(50))
                next_id += 1
            for h, j in np.argwhere((u >= 0.15) & (u < 0.25)):  # a pad
                ids[h, j], src[h, j] = -1, INT32_MIN + int(rng.integers(N))
            for h, j in np.argwhere((u >= 0.25) & (u < 0.3)):   # carried by src, under a foreign id
                if ids[h, j] >= 0:
                    ids[h, j] = next_id
                    next_id += 1
            for h, j in np.argwhere(u >= 0.3):      # a slot that was a pad and is carried: it comes back born
                if ids[h, j] < 0:
                    ids[h, j], src[h, j] = next_id, -1
                    next_id += 1
        if N > 1:
            for _ in range(max(1, N // 16)):
                tracks[rng.integers(n), rng.integers(Tw), rng.integers(N), rng.integers(2)] = (np.nan, np.inf, -np.inf)[rng.integers(3)]
        w = None
        if weighted:
            w = rng.uniform(0.5, 1.5, (n, Tw, N)).astype(np.float32)
            if N > 1:
                w[rng.random((n, Tw, N)) < 0.05] = 0.0
        calls.append(dict(tracks=tracks, R=R, T=T, ids=ids, src=src, stream_idx=order,
                          intr=np.tile(np.array(INTR), (n, 1)), weights=w))
    return calls, streams


SHAPES = [(1, 4, 64, 1), (3, 5, 70, 2), (1, 2, 1, 1), (2, 4, 300, 3)]


@pytest.mark.parametrize("n,Tw,N,s", SHAPES)
def test_case_b_shapes_weights_and_both_rotation_conventions(n, Tw, N, s):
    seen = set()
    for weighted in (False, True):
        for inverse in (0, 1):
            calls, streams = shape_case(n, Tw, N, s, weighted, inverse)
            acc, acc_id = ln.new_state(streams, N)
            dev = _Device(streams, N)
            kw = dict(inverse_rotation=inverse, min_obs=2, min_pivot=1e-8)
            for c, inp in enumerate(calls):
                ref = ln.update(**inp, acc=acc, acc_id=acc_id, s=s, **kw)
                got = dev.update(inp, s, **kw)
                _compare(got, ref, acc, acc_id, dev, f"case b n={n} T={Tw} N={N} s={s} w={weighted} inv={inverse} launch {c}")
                seen |= set(ref["state"].ravel().tolist())
            assert (ref["state"] == ln.VALID).any() and ref["err_px"][ref["state"] == ln.VALID].max() < 1e-2
            assert ref["n_obs"].max() == 3 * s
    if N >= 64:
        assert {ln.NONE, ln.VALID} <= seen
    print(f"measured maxima so far: X {WORST['X']:.3e} rel, rows {WORST['row']:.3e} of the trace, err_px {WORST['err']:.3e} px")


def test_three_hops_in_one_launch_equal_three_single_hop_launches():
    n, Tw, N, s = 3, 5, 70, 2
    calls, streams = shape_case(n, Tw, N, s, True, 0)
    together, apart = _Device(streams, N), _Device(streams, N)
    for c, inp in enumerate(calls):
        a = together.update(inp, s, min_obs=2)
        parts = [apart.update({k: None if v is None else v[h:h + 1] for k, v in inp.items()}, s, min_obs=2) for h in range(n)]
        for name in a:
            b = np.concatenate([p[name] for p in parts])
            assert a[name].tobytes() == b.tobytes(), (c, name)
        assert torch.equal(together.acc.view(torch.int64), apart.acc.view(torch.int64)), c
        assert torch.equal(together.acc_id, apart.acc_id), c
    assert bool((together.acc_id >= 0).any())


def test_landmark_update_wrapper_rejects_bad_arguments():
    import ctypes
    from comet_amd import _lib, ops
    calls, _, m = case_a()
    t = {k: torch.as_tensor(v).cuda() for k, v in calls[0].items()}
    acc = torch.zeros(3 * 64, 12, dtype=torch.float64, device="cuda")
    acc_id = torch.full((3 * 64,), -1, dtype=torch.int32, device="cuda")
    host = ((ctypes.c_int32 * 2)(2, 0), (ctypes.c_double * 8)(*(list(INTR) * 2)))

    def call(**kw):
        a = dict(dict(t, acc=acc, acc_id=acc_id, idx_host=host[0], intr_host=host[1], s=1), **kw)
        return ops.landmark_update(a["tracks"], a["R"], a["T"], a["ids"], a["src"], a["stream_idx"], a["idx_host"],
                                   a["intr"], a["intr_host"], a["acc"], a["acc_id"], a["s"], a["weights"])
    for bad in (dict(tracks=t["tracks"].double()), dict(R=t["R"].double()), dict(T=t["T"].float()),
                dict(ids=t["ids"].long()), dict(src=t["src"][:, ::2]), dict(weights=t["weights"][:, :2]),
                dict(acc=acc[:, :10]), dict(acc_id=acc_id[:5]), dict(tracks=t["tracks"].cpu()),
                dict(idx_host=(ctypes.c_int32 * 1)(0)), dict(s=4), dict(idx_host=(ctypes.c_int32 * 2)(1, 1)),
                dict(idx_host=(ctypes.c_int32 * 2)(0, 3))):
        with pytest.raises(_lib.CometHipError):
            call(**bad)
    assert bool((acc_id == -1).all()), "a rejected call launched"
    out = call()
    assert out.X.shape == (2, 64, 3) and out.X.dtype == torch.float64 and out.err_px.dtype == torch.float32
    assert out.n_obs.dtype == out.state.dtype == torch.int32


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
T, HW, N = 4, 128, 64
SEED_W, SEED_X, SEEDS = 0, 1, (4, 2, 6)
MIN_SCORE = 0.5
CAND_SEED, CAND_M = 7, 96
HOPS = 5
TRACK_INTR = (150.0, 150.0, 63.5, 63.5)


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


@pytest.fixture(scope="module")
def plain(model):
    """The golden stream without landmarks, HOPS + 1 hops."""
    return _run(_stream(model), _frames(SEED_X, T + HOPS))


@pytest.fixture(scope="module")
def mapped(model):
    """The same stream with landmarks=True (min_obs 2, so that landmarks exist from the second hop on)."""
    st = _stream(model, landmarks=True, track_intr=TRACK_INTR, lm_min_obs=2)
    return _run(st, _frames(SEED_X, T + HOPS)), st


def _np(t):
    return t.detach().cpu().numpy()


def _restate(results, intr, s=1, acc=None, acc_id=None, stream=0, streams=1, **kw):
    """The restatement chained on the recorded outputs of one stream's hops -> its outputs per hop."""
    if acc is None:
        acc, acc_id = ln.new_state(streams, N)
    outs = []
    for r in results:
        outs.append(ln.update(_np(r.pred_tracks)[None], _np(r.fused_R)[None], _np(r.fused_T)[None],
                              _np(r.track_ids)[None], _np(r.track_src)[None], [stream], np.array([intr]), acc, acc_id, s,
                              **kw))
    return outs


def _equal_restatement(r, ref, what):
    got = dict(X=_np(r.landmarks)[None], n_obs=_np(r.landmark_obs)[None], err_px=_np(r.landmark_err)[None],
               state=_np(r.landmark_state)[None])
    _pivots_clear_of_the_bound(ref, what)
    assert (got["n_obs"] == ref["n_obs"]).all() and (got["state"] == ref["state"]).all(), what
    dx = np.abs(got["X"] - ref["X"]).max(-1) / (1.0 + np.linalg.norm(ref["X"], axis=-1))
    on = ref["state"] == ln.VALID
    assert dx.max() <= X_TOL, (what, dx.max())
    assert (got["X"][~on] == 0).all() and np.isposinf(got["err_px"][~on]).all(), what
    if on.any():
        assert np.abs(got["err_px"][on].astype(np.float64) - ref["err_px"][on]).max() <= ERR_TOL, what


def test_stream_landmarks_equal_the_restatement_on_the_recorded_outputs(mapped, plain):
    res, st = mapped
    assert len(res) == len(plain) == HOPS + 1
    refs = _restate(res, TRACK_INTR, min_obs=2)
    arange = torch.arange(N, device="cuda", dtype=torch.int32)
    oldest = 0
    for k, (r, ref, p) in enumerate(zip(res, refs, plain)):
        hist = {v: int((r.landmark_state == v).sum()) for v in (-1, 0, 1, 2, 3)}
        valid = r.landmark_err[r.landmark_state == 1]
        print(f"hop {k}: states {hist}, n_obs max {int(r.landmark_obs.max())}, err_px of the valid "
              f"{[round(float(v), 3) for v in valid.sort().values[:6]]}")
        assert r.landmarks.shape == (N, 3) and r.landmarks.dtype == torch.float64 and len(r) == 12
        _equal_restatement(r, ref, f"hop {k}")
        live = r.track_ids >= 0
        assert bool(live.any())
        # a slot carried over `age` hops holds its first hop's frames plus one stride per hop since
        assert torch.equal(r.landmark_obs[live], (r.track_age[live] + 1) * 1), k
        assert bool((r.landmark_obs[~live] == 0).all())
        assert torch.equal(r.track_src[live & (r.track_age > 0)], arange[live & (r.track_age > 0)])
        oldest = max(oldest, int(r.track_age.max()))
        # the landmark launch changes nothing the stream computes
        for name in ("pred_pose_enc", "pred_tracks", "pred_score", "fused_R", "fused_T", "track_ids", "track_age", "track_src"):
            assert torch.equal(getattr(r, name), getattr(p, name)), (k, name)
    assert oldest >= 2, "no track was carried over two hops: the add path would be untested"
    ids, X, n_obs = st.landmark_map.snapshot(0)
    last = res[-1]
    on = last.landmark_state == 1
    assert torch.equal(ids, last.track_ids[on]) and torch.equal(X, last.landmarks[on]) and torch.equal(n_obs, last.landmark_obs[on])
    st.reset()
    assert st.landmark_map.snapshot(0)[0].numel() == 0 and bool((st.landmark_map.acc_id == -1).all())


def test_gate_kills_exactly_the_gated_slots_at_the_next_hop(model, mapped):
    """lm_gate_px between two measured err_px values of the ungated run: up to and including the first
    hop that gates a slot both runs are the same stream; at the next hop every gated slot has lost its
    track, and every other slot the ungated stream carried is carried."""
    base, _ = mapped
    k0 = next((k for k, r in enumerate(base[:-1]) if int((r.landmark_state == 1).sum()) >= 2
               and float(r.landmark_err[r.landmark_state == 1].max()) > float(r.landmark_err[r.landmark_state == 1].min())), None)
    assert k0 is not None, "no hop of the run has two valid landmarks with different errors: nothing to gate between"
    errs = base[k0].landmark_err[base[k0].landmark_state == 1].sort().values
    gate = 0.5 * (float(errs[0]) + float(errs[-1]))
    assert float(errs[0]) < gate < float(errs[-1])
    got = _run(_stream(model, landmarks=True, track_intr=TRACK_INTR, lm_min_obs=2, lm_gate_px=gate), _frames(SEED_X, T + HOPS))
    first = next(k for k, r in enumerate(base) if bool(((r.landmark_state == 1) & (r.landmark_err > gate)).any()))
    assert first <= k0
    for k in range(first + 1):  # the same stream so far
        for name in ("pred_pose_enc", "pred_tracks", "pred_score", "landmark_err", "landmark_state", "track_ids"):
            assert torch.equal(getattr(got[k], name), getattr(base[k], name)), (k, name)
    gated = (base[first].landmark_state == 1) & (base[first].landmark_err > gate)
    arange = torch.arange(N, device="cuda", dtype=torch.int32)
    kept_base = base[first + 1].track_src == arange
    kept_got = got[first + 1].track_src == arange
    print(f"gate {gate:.3f} px at hop {first}: {int(gated.sum())} gated, {int((gated & kept_base).sum())} of them carried "
          f"without the gate; carried next hop {int(kept_got.sum())} with / {int(kept_base.sum())} without")
    assert not bool((kept_got & gated).any()), "a gated slot kept its track"
    assert bool((kept_got | gated)[kept_base].all()), "a slot that was not gated lost a track the ungated stream kept"
    died = kept_base & ~kept_got
    assert bool(gated[died].all()), "a slot died that was not gated"
    assert bool((gated & kept_base).any()), "no gated slot would have been carried: the gate would show nothing"
    ids_before = base[first].track_ids
    assert bool((got[first + 1].track_ids[gated & kept_base] != ids_before[gated & kept_base]).all())


PUSHES, LATE, RESET_AT = 11, 1, 6  # stream 1 joins one push late and is reset before push 6


def test_pool_of_one_stream_equals_the_stream_bit_for_bit(model, mapped):
    from comet_amd.stream import StreamPool
    base, _ = mapped
    pool = StreamPool(model, streams=1, anchors=[_anchor()], **_kw(landmarks=True, track_intrs=[TRACK_INTR], lm_min_obs=2))
    frames = _frames(SEED_X, T + HOPS)
    got = [r for f in range(frames.shape[0]) for _, r in pool.push(frames[f][None])]
    assert len(got) == len(base)
    for k, (g, b) in enumerate(zip(got, base)):
        assert torch.equal(g.landmarks.view(torch.int64), b.landmarks.view(torch.int64)), k
        assert torch.equal(g.landmark_err.view(torch.int32), b.landmark_err.view(torch.int32)), k
        assert torch.equal(g.landmark_obs, b.landmark_obs) and torch.equal(g.landmark_state, b.landmark_state), k
    on = base[-1].landmark_state == 1
    for a, b in zip(pool.landmark_map.snapshot(0), (base[-1].track_ids[on], base[-1].landmarks[on], base[-1].landmark_obs[on])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("warm", [{}, dict(warm=True, warm_iters=2)], ids=["cold", "warm-split"])
def test_pool_of_three_streams_out_of_phase_equals_the_restatement_per_stream(model, warm):
    """warm-split: warm_iters differs from the config's iterations, so a push in which stream 1's first hop
    falls together with later hops of streams 0 and 2 runs two model calls (first hops, then later hops);
    their rows are stacked in the order [1, 0, 2] for the one landmark launch, and ids / src follow them."""
    from comet_amd.stream import StreamPool
    intrs = [TRACK_INTR, (140.0, 160.0, 60.0, 66.0), (155.0, 150.0, 64.0, 63.0)]
    seqs = [_frames(seed, PUSHES) for seed in SEEDS]
    pool = StreamPool(model, streams=3, anchors=[_anchor()] * 3,
                      **_kw(landmarks=True, track_intrs=intrs, lm_min_obs=2, lm_weight="score", **warm))
    launches, inner = [], pool._landmarks
    pool._landmarks = lambda order, results, co, later: (launches.append((list(order), len(later))),
                                                         inner(order, results, co, later))[1]
    acc, acc_id = ln.new_state(3, N)
    hops, nxt = {0: 0, 1: 0, 2: 0}, {0: 0, 1: 0, 2: 0}
    after_reset = None
    for p in range(PUSHES):
        if p == RESET_AT:
            pool.reset(1)
            acc_id[N:2 * N] = -1
            after_reset, nxt[1] = hops[1], 0
        ids = [s for s in range(3) if s != 1 or p >= LATE]
        out = pool.push(torch.stack([seqs[s][nxt[s]] for s in ids]), streams=ids)
        for s in ids:
            nxt[s] += 1
        for sid, r in out:
            ref = ln.update(_np(r.pred_tracks)[None], _np(r.fused_R)[None], _np(r.fused_T)[None], _np(r.track_ids)[None],
                            _np(r.track_src)[None], [sid], np.array([intrs[sid]]), acc, acc_id, 1,
                            weights=_np(r.pred_score.float())[None], min_obs=2)
            _equal_restatement(r, ref, f"push {p} stream {sid}")
            if sid == 1 and after_reset == hops[1]:  # the first hop after the reset: every row fresh
                live = r.track_ids >= 0
                assert bool(live.any()) and bool((r.landmark_obs[live] <= 1).all()) and bool((r.landmark_state == 0).all())
                assert bool((r.track_age == 0).all())
            hops[sid] += 1
        if pool.landmark_map.device is None:  # (no hop yet: the state is allocated by the first)
            continue
        rows = pool.landmark_map.acc.cpu().numpy()
        trace = rows[:, 0] + rows[:, 3] + rows[:, 5]
        assert (np.abs(rows - acc).max(-1) <= ROW_TOL * np.where(trace > 0, trace, 1.0)).all(), p
        assert (pool.landmark_map.acc_id.cpu().numpy() == acc_id).all(), p
    assert hops == {0: PUSHES - T + 1, 1: (RESET_AT - LATE - T + 1) + (PUSHES - RESET_AT - T + 1), 2: PUSHES - T + 1}, hops
    assert after_reset is not None and hops[1] > after_reset
    split = [o for o, calls in launches if calls == 2]
    if warm:  # once when stream 1 joins late, once after its reset; every other push is one call in stream order
        assert int(model.cfg["track_trainit"]) != warm["warm_iters"]
        assert split == [[1, 0, 2], [1, 0, 2]], launches
    else:
        assert not split
    assert all(o == sorted(o) for o, calls in launches if calls == 1)


# ------------------------------------------------------------------------------------------------
# the evaluation loop: cfg.stream.landmarks
# ------------------------------------------------------------------------------------------------
def _cfg(**stream):
    from comet_amd.config import AttrDict
    base = {"enable": True, "window": T, "stride": 1, "fuse": True, "carry": True, "carry_tracks": N, "carry_cell": 8,
            "carry_min_score": MIN_SCORE}
    return AttrDict.wrap({"stream": dict(base, **stream), "train": {"img_size": HW}, "mixed_precision": "no"})


def _raw(seed, count):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (160, 176, 3), dtype=torch.uint8, generator=g).numpy() for _ in range(count)]


def _csv_rows(path):
    import csv
    with open(path) as f:
        return list(csv.DictReader(f))


def _snapshot_rows(snap):
    ids, X, n_obs = snap
    return [dict(track_id=str(int(i)), x=repr(float(x[0])), y=repr(float(x[1])), z=repr(float(x[2])), n_obs=str(int(k)))
            for i, x, k in zip(ids.tolist(), X.tolist(), n_obs.tolist())]


def test_stream_eval_writes_the_final_snapshot_with_the_crop_intrinsics(model, tmp_path):
    """cfg.stream.landmarks: the stream runs with the dataset's intrinsics mapped into the sequence's box,
    the hop CSV is what it is without landmarks, and <stem>_landmarks.csv is the final snapshot: the rows
    of a PoseStream built by hand with the same settings on the same cropped frames."""
    from comet_amd import loop
    from comet_amd.data import crop_intrinsics, crop_resize_normalize
    from comet_amd.models.utils import INTRINSICS
    from comet_amd.stream import PoseStream
    raw, box = _raw(3, T + 4), (8, 0, 168, 160)
    on, off = str(tmp_path / "on.csv"), str(tmp_path / "off.csv")
    assert loop.landmarks_csv(on) == str(tmp_path / "on_landmarks.csv")
    cfg = _cfg(landmarks=True, lm_min_obs=2, lm_weight="score")
    assert loop.stream_eval(model, iter(raw), cfg, box, on, candidate_fn=_Candidates()) == 5
    assert loop.stream_eval(model, iter(raw), _cfg(), box, off, candidate_fn=_Candidates()) == 5
    assert not (tmp_path / "off_landmarks.csv").exists()
    rows_on, rows_off = _csv_rows(on), _csv_rows(off)
    assert len(rows_on) == len(rows_off) and tuple(rows_on[0].keys()) == tuple(rows_off[0].keys())
    for a, b in zip(rows_on, rows_off):
        assert {k: v for k, v in a.items() if k != "hop_ms"} == {k: v for k, v in b.items() if k != "hop_ms"}
    fx, _, cx, cy = INTRINSICS["AMD"]
    intr = crop_intrinsics(INTRINSICS["AMD"], box, HW)
    st = PoseStream(model, anchor=([1.0, 0.0, 0.0, 0.0], [cx, cy, 1.0], fx, 1.0, "AMD"),
                    **_kw(landmarks=True, track_intr=intr, lm_min_obs=2, lm_weight="score"))
    for f in raw:
        st.push(crop_resize_normalize(torch.as_tensor(f)[None].cuda(), box, (HW, HW))[0])
    want = _snapshot_rows(st.landmark_map.snapshot(0))
    got = _csv_rows(loop.landmarks_csv(on))
    print(f"stream_eval: {len(got)} landmarks in the final snapshot")
    with open(loop.landmarks_csv(on)) as f:
        assert tuple(f.readline().strip().split(",")) == loop.LANDMARK_FIELDS
    assert got == want
    for bad in (dict(fuse=False), dict(carry=False)):
        with pytest.raises(ValueError, match="cfg.stream.landmarks needs"):
            loop.stream_eval(model, iter(raw), _cfg(landmarks=True, **bad), box, str(tmp_path / "bad.csv"),
                             candidate_fn=_Candidates(), query_points=None if bad.get("carry", True) else torch.zeros(N, 2).cuda())


def test_stream_eval_pool_gives_every_sequence_its_own_intrinsics_and_snapshot(model, tmp_path, monkeypatch):
    """Two streams, three sequences with three boxes: the third takes over stream 0 when the first ends.
    Every landmark launch must read, for each stream, the intrinsics of the box of the sequence that
    stream is running, and every sequence's <name>_landmarks.csv is the snapshot taken when it ended."""
    from comet_amd import loop
    from comet_amd.data import crop_intrinsics
    from comet_amd.models.utils import INTRINSICS
    from comet_amd.stream import LandmarkMap
    boxes = {"a": (8, 0, 168, 160), "b": (0, 0, 150, 150), "c": (16, 10, 166, 160)}
    seqs = [("a", _raw(4, T + 1), boxes["a"]), ("b", _raw(5, T + 5), boxes["b"]), ("c", _raw(6, T + 1), boxes["c"])]
    used, snaps = [], []
    update, snapshot = LandmarkMap.update, LandmarkMap.snapshot

    def rec_update(self, sids, *a, **k):
        used.append({int(s): self.intrs[int(s)] for s in sids})
        return update(self, sids, *a, **k)

    def rec_snapshot(self, stream=0):
        snaps.append((int(stream), _snapshot_rows(snapshot(self, stream))))
        return snapshot(self, stream)
    monkeypatch.setattr(LandmarkMap, "update", rec_update)
    monkeypatch.setattr(LandmarkMap, "snapshot", rec_snapshot)
    hops = loop.stream_eval_pool(model, [(n, iter(f), b) for n, f, b in seqs], _cfg(streams=2, landmarks=True, lm_min_obs=2),
                                 str(tmp_path), candidate_fn=_Candidates())
    assert hops == {"a": 2, "b": 6, "c": 2}
    intr = {n: crop_intrinsics(INTRINSICS["AMD"], b, HW) for n, b in boxes.items()}
    assert len({intr["a"], intr["b"], intr["c"]}) == 3
    assert [u[0] for u in used if 0 in u] == [intr["a"]] * 2 + [intr["c"]] * 2
    assert [u[1] for u in used if 1 in u] == [intr["b"]] * 6
    assert [s for s, _ in snaps] == [0, 1, 0]  # a ends, then b, then c
    for name, (_, want) in zip(("a", "b", "c"), snaps):
        got = _csv_rows(str(tmp_path / f"{name}_landmarks.csv"))
        print(f"stream_eval_pool {name}: {len(got)} landmarks in the final snapshot")
        assert got == want
