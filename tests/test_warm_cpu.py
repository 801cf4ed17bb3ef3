"""Warm start without a GPU: the ValueErrors of the PoseStream / StreamPool constructors and
properties of the numpy restatement of comet_track_warm (tests/warm_numpy.py), also on the `src` that
the restatement of comet_track_carry produces (comet_amd/stream.py, DESIGN.md "Warm start")."""
import numpy as np
import pytest

import carry_numpy as cn
import warm_numpy as wn

# cn.random_inputs(SEED, 2, 4, 64, 96, 128, 128) carried with cell CELL, border 2, min_score 0.3: with 16-px
# cells the frame has 64 cells and fewer live tracks than slots, so pads copy carried and born slots alike and
# the warm values 0, 1 and 2 all occur in both hops (hold, s = 1: 42 / 16 / 6 and 30 / 21 / 13 slots; with
# 8-px cells every free slot is born into and seeds 0 .. 3 give almost no pads)
SEED, CELL = 0, 16


def _make(kind, **kw):
    from comet_amd.stream import PoseStream, StreamPool
    args = dict(window=4, stride=1, carry=True, carry_tracks=64, carry_min_score=0.5, candidate_fn=lambda f: None)
    args.update(kw)
    return PoseStream(None, **args) if kind == "stream" else StreamPool(None, streams=2, **args)


@pytest.mark.parametrize("kind", ["stream", "pool"])
def test_constructors_reject_bad_warm_arguments(kind):
    on = _make(kind, warm=True, warm_mode="velocity", warm_iters=2)
    assert on.warm and on.warm_iters == 2 and on._carry.warm_mode == "velocity"
    off = _make(kind)
    assert not off.warm and off.warm_iters is None and off._carry.warm_mode is None
    with pytest.raises(ValueError, match="warm=True needs carry=True"):
        _make(kind, warm=True, carry=False)
    with pytest.raises(ValueError, match="warm_mode"):
        _make(kind, warm=True, warm_mode="linear")
    with pytest.raises(ValueError, match="warm_iters"):
        _make(kind, warm=True, warm_iters=0)
    with pytest.raises(ValueError, match="warm_iters"):
        _make(kind, warm=True, warm_iters=-2)


def test_stream_result_gains_track_warm():
    from comet_amd.stream import StreamResult
    r = StreamResult(0, "enc", None, None)
    assert r.track_warm is None and len(r) == 12
    c = r.with_tracks("ids", "age", "src")
    assert c.track_warm is None
    w = r.with_tracks("ids", "age", "src", "warm")._replace(R="R")
    assert (w.track_ids, w.track_warm, w.R) == ("ids", "warm", "R") and len(w) == 12


def test_pool_groups_first_and_later_hops_only_when_their_iterations_differ():
    class _Model:
        cfg = {"track_trainit": 4}
    from comet_amd.stream import StreamPool
    kw = dict(window=4, stride=1, carry=True, carry_tracks=64, carry_min_score=0.5, candidate_fn=lambda f: None)
    pool = StreamPool(_Model(), streams=3, warm=True, warm_iters=2, **kw)
    assert pool._warm_groups([True, False, True]) == [([0, 2], False, None), ([1], True, 2)]
    assert pool._warm_groups([False, False, False]) == [([0, 1, 2], True, 2)]
    assert pool._warm_groups([True, True, True]) == [([0, 1, 2], False, None)]
    for iters in (None, 4):
        same = StreamPool(_Model(), streams=3, warm=True, warm_iters=iters, **kw)
        assert same._warm_groups([True, False, True]) == [([0, 1, 2], True, None)]
        assert same._warm_groups([False, False, False]) == [([0, 1, 2], True, iters)]
    cold = StreamPool(_Model(), streams=3, **kw)
    assert cold._warm_groups([True, False, True]) == [([0, 1, 2], False, None)]


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _carried(seed=SEED, n=2, T=4, N=64, M=96, HW=128, s=1):
    inp = cn.random_inputs(seed, n, T, N, M, HW, HW, s=s)
    out = cn.carry(**inp, cell=CELL, border=2, min_score=0.3)
    return inp, out


@pytest.fixture(scope="module")
def case():
    inp, out = _carried()
    res = {mode: wn.warm(inp["tracks"], out["src"], out["query"], inp["prev_valid"], 1, 128, 128, mode, 2.0, 4.0)
           for mode in (wn.HOLD, wn.VELOCITY)}
    return inp, out, res


def test_carry_src_gives_every_warm_value(case):
    inp, out, res = case
    for mode, (coords, warm) in res.items():
        assert coords.shape == (2, 64, 4, 2) and coords.dtype == np.float32 and warm.dtype == np.int32
        for b in range(2):
            counts = {v: int((warm[b] == v).sum()) for v in (-1, 0, 1, 2)}
            assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0 and counts[-1] == 0, (mode, b, counts)
            assert 0 < counts[1] + counts[2] < 64, "all warm or all cold"
            carried = out["src"][b] == np.arange(64)
            assert ((warm[b] == 1) == carried).all()
            born = (out["src"][b] < 0) & (out["src"][b] >= -96)
            assert (warm[b][born] == 0).all()


def test_frame_zero_is_the_query_for_every_slot(case):
    inp, out, res = case
    q = (out["query"] / np.float32(2.0) / np.float32(4.0)).astype(np.float32)
    for coords, warm in res.values():
        assert (coords[:, :, 0].view(np.uint32) == q.view(np.uint32)).all()
        cold = warm == 0
        assert (coords[cold].view(np.uint32) == np.repeat(q[cold][:, None], 4, 1).view(np.uint32)).all()


@pytest.mark.parametrize("s", [1, 2, 3])
def test_a_carried_slots_overlap_is_the_shifted_previous_rows(s):
    inp, out = _carried(s=s)
    T = 4
    for mode in (wn.HOLD, wn.VELOCITY):
        coords, warm = wn.warm(inp["tracks"], out["src"], out["query"], inp["prev_valid"], s, 128, 128, mode, 1.0, 1.0)
        assert (warm == 1).any()
        for b, j in np.argwhere(warm == 1):
            for i in range(1, T - s):
                assert (coords[b, j, i].view(np.uint32) == inp["tracks"][b, i + s, j].view(np.uint32)).all()
            if mode == wn.HOLD:
                for i in range(T - s, T):
                    assert (coords[b, j, i].view(np.uint32) == inp["tracks"][b, T - 1, j].view(np.uint32)).all()
            else:
                tail = coords[b, j, T - s:]
                assert (tail >= 0).all() and (tail <= 127).all()
        for b, j in np.argwhere(warm == 2):  # a pad copy has its donor's row after frame 0
            l = int(out["src"][b, j]) - cn.INT32_MIN
            assert warm[b, l] == 1 and (coords[b, j, 1:].view(np.uint32) == coords[b, l, 1:].view(np.uint32)).all()


def test_hold_and_velocity_agree_when_the_track_stands_still():
    inp, out = _carried()
    prev = inp["tracks"].copy()
    prev[:, 2] = prev[:, 3]  # last == before (inside or outside the frame)
    prev[:, 3] = np.clip(prev[:, 3], 0, 127)  # (inside the frame, so that the clamp changes nothing)
    prev[:, 2] = prev[:, 3]
    hold = wn.warm(prev, out["src"], out["query"], inp["prev_valid"], 1, 128, 128, wn.HOLD, 2.0, 4.0)
    vel = wn.warm(prev, out["src"], out["query"], inp["prev_valid"], 1, 128, 128, wn.VELOCITY, 2.0, 4.0)
    assert (hold[1] == vel[1]).all() and (hold[1] > 0).any()
    assert (hold[0].view(np.uint32) == vel[0].view(np.uint32)).all()
    moved = wn.warm(inp["tracks"], out["src"], out["query"], inp["prev_valid"], 1, 128, 128, wn.VELOCITY, 2.0, 4.0)
    assert (moved[0] != hold[0]).any(), "the velocity term made no difference on moving tracks"


def test_a_value_that_is_not_finite_falls_back_only_where_it_is_used():
    inp, out = _carried()
    j = int(np.argwhere(out["src"][0] == np.arange(64))[0, 0])
    for row, mode, s, want in ((3, wn.HOLD, 1, -1), (2, wn.HOLD, 1, -1), (1, wn.HOLD, 1, 1), (0, wn.VELOCITY, 1, 1),
                               (2, wn.HOLD, 3, 1), (2, wn.VELOCITY, 3, -1)):
        prev = inp["tracks"].copy()
        prev[0, row, j, 1] = np.nan
        query = out["query"].copy()  # (for s = 3 the query is not prev[s]; frame 0 is the query either way)
        coords, warm = wn.warm(prev, out["src"], query, inp["prev_valid"], s, 128, 128, mode, 2.0, 4.0)
        assert warm[0, j] == want, (row, mode, s)
        assert np.isfinite(coords).all()
        if want == -1:
            assert (coords[0, j] == coords[0, j, 0]).all()
    big = inp["tracks"].copy()
    big[0, 3, j], big[0, 2, j] = (3e38, 5), (-3e38, 5)  # finite inputs, an extrapolation that overflows
    assert wn.warm(big, out["src"], out["query"], inp["prev_valid"], 1, 128, 128, wn.VELOCITY, 2.0, 4.0)[1][0, j] == -1
    assert wn.warm(big, out["src"], out["query"], inp["prev_valid"], 1, 128, 128, wn.HOLD, 2.0, 4.0)[1][0, j] == 1


def test_prev_valid_zero_is_cold_and_reads_nothing():
    inp, out = _carried()
    prev = np.full_like(inp["tracks"], np.nan)
    coords, warm = wn.warm(prev, out["src"], out["query"], np.zeros(2, np.int32), 1, 128, 128, wn.VELOCITY, 2.0, 4.0)
    assert (warm == 0).all() and np.isfinite(coords).all()
