"""Track carry without a GPU: properties of the numpy restatement of comet_track_carry
(tests/carry_numpy.py) on random inputs, the host-only CarrySchedule, and the ValueErrors of the
PoseStream / StreamPool constructors (comet_amd/stream.py, DESIGN.md "Track carry")."""
import numpy as np
import pytest

import carry_numpy as cn

CELL, BORDER, MIN_SCORE = 8, 2, 0.3
SHAPE = dict(n=2, T=4, N=70, M=150, H=96, W=80)


def _run(inp, **kw):
    return cn.carry(**inp, **dict(dict(cell=CELL, border=BORDER, min_score=MIN_SCORE), **kw))


@pytest.fixture(scope="module", params=[0, 1, 2])
def case(request):
    inp = cn.random_inputs(request.param, **SHAPE, spread=0.6 if request.param == 2 else 1.0)
    return inp, _run(inp)


def test_at_most_one_live_track_per_cell(case):
    inp, out = case
    for b in range(SHAPE["n"]):
        live = out["ids"][b] >= 0
        assert live.sum() > 0
        q = out["query"][b][live]
        cells = list(zip(np.floor(q[:, 0] / np.float32(CELL)).astype(int), np.floor(q[:, 1] / np.float32(CELL)).astype(int)))
        assert len(set(cells)) == len(cells)
        assert (q >= BORDER).all() and (q[:, 0] <= SHAPE["W"] - 1 - BORDER).all() and (q[:, 1] <= SHAPE["H"] - 1 - BORDER).all()
        assert all(inp["mask"][b][int(np.rint(y)), int(np.rint(x))] for x, y in q)


def test_kept_tracks_keep_slot_and_id_and_age_grows_by_one(case):
    inp, out = case
    N = SHAPE["N"]
    for b in range(SHAPE["n"]):
        kept = out["src"][b] == np.arange(N)
        assert 0 < kept.sum() < N and kept.sum() == out["stats"][b, 0]
        assert (out["ids"][b][kept] == inp["ids"][b][kept]).all() and (inp["ids"][b][kept] >= 0).all()
        assert (out["age"][b][kept] == inp["age"][b][kept] + 1).all()
        assert (out["query"][b][kept].view(np.uint32) == inp["tracks"][b, inp["s"]][kept].view(np.uint32)).all()
        assert (inp["score"][b, inp["s"]][kept] >= np.float32(MIN_SCORE)).all()
        born = (out["src"][b] < 0) & (out["src"][b] >= -SHAPE["M"])
        assert born.sum() == out["stats"][b, 1] and (out["age"][b][born] == 0).all()
        assert kept.sum() + born.sum() + out["stats"][b, 2] == N
        assert out["next_id"][b] == inp["next_id"][b] + born.sum()


def _chain(inp, calls=3, seed=9):
    """`calls` chained calls: the outputs' ids / age / next_id and fresh random tracks at the queries."""
    rng = np.random.default_rng(seed)
    outs, cur = [], dict(inp)
    for k in range(calls):
        out = _run(cur)
        outs.append(out)
        tracks = cur["tracks"].copy()
        tracks[:, cur["s"]] = out["query"] + rng.normal(0, 3, out["query"].shape).astype(np.float32)
        fresh = cn.random_inputs(seed + k + 1, **SHAPE)
        cur = dict(cur, tracks=tracks, score=fresh["score"], cand=fresh["cand"], cand_n=fresh["cand_n"],
                   ids=out["ids"], age=out["age"], next_id=out["next_id"])
    return outs


def test_ids_are_unique_and_increase_across_three_chained_calls():
    inp = cn.random_inputs(3, **SHAPE)
    inp["ids"][:] = -1  # a first hop in all but prev_valid
    inp["next_id"][:] = 0
    outs = _chain(inp)
    for b in range(SHAPE["n"]):
        seen, top = set(), -1
        for out in outs:
            live = out["ids"][b][out["ids"][b] >= 0]
            assert len(set(live.tolist())) == len(live)
            new = set(live.tolist()) - seen
            assert all(i > top for i in new), "a fresh id is not above every earlier id"
            born = (out["src"][b] < 0) & (out["src"][b] >= -SHAPE["M"])
            assert new == set(out["ids"][b][born].tolist())
            seen |= new
            top = max([top] + list(new))
            assert out["next_id"][b] == top + 1
        assert len(outs[2]["ids"][b][outs[2]["age"][b] >= 2]) > 0, "no track lived through all three calls"


def test_pads_have_id_minus_one_and_are_free_on_the_next_call():
    inp = cn.random_inputs(4, **dict(SHAPE, M=20))
    out = _run(inp)
    N = SHAPE["N"]
    for b in range(SHAPE["n"]):
        pad = out["src"][b] < -SHAPE["M"]
        assert pad.sum() == out["stats"][b, 2] > 0
        assert (out["ids"][b][pad] == -1).all() and (out["age"][b][pad] == 0).all()
        k = out["src"][b][pad].astype(np.int64) - cn.INT32_MIN
        assert ((k >= 0) & (k < N)).all() and (out["ids"][b][k] >= 0).all()
        assert (out["query"][b][pad] == out["query"][b][k]).all()
    # next call: tracks exactly at the queries, all scores high, no candidates -> no pad slot is carried
    tracks = inp["tracks"].copy()
    tracks[:, inp["s"]] = out["query"]
    nxt = _run(dict(inp, tracks=tracks, score=np.ones_like(inp["score"]), ids=out["ids"], age=out["age"],
                    next_id=out["next_id"], cand=None, cand_n=None))
    for b in range(SHAPE["n"]):
        carried = nxt["src"][b] == np.arange(N)
        assert (carried == (out["ids"][b] >= 0)).all()


def test_permuting_candidates_of_different_cells_changes_nothing():
    """Candidates are reordered so that the relative order inside every cell is kept. The selection is
    the same: the same candidates are born, into the same set of slots (births go by candidate index,
    so which of those slots a candidate takes follows the new order), the kept tracks, the set of live
    query points and the statistics are unchanged."""
    inp = cn.random_inputs(5, **dict(SHAPE, n=1, N=200, M=60), fill=0.2)
    inp["cand_n"][:] = 60
    base = _run(inp)
    cand = inp["cand"][0]
    cells = [cn.alive(x, y, SHAPE["H"], SHAPE["W"], CELL, BORDER, None)[1] for x, y in cand]
    cells = [c if c is not None else ("dead", i) for i, c in enumerate(cells)]
    # a stable sort by a random rank of the cell keeps the order within each cell
    rng = np.random.default_rng(0)
    rank = {c: rng.random() for c in set(cells)}
    order = sorted(range(len(cand)), key=lambda i: rank[cells[i]])
    assert order != list(range(len(cand)))
    perm = _run(dict(inp, cand=cand[order][None]))
    N = 200
    kept = base["src"][0] == np.arange(N)
    for k in ("query", "ids", "age", "src"):
        assert (perm[k][0][kept] == base[k][0][kept]).all()
    assert (perm["stats"] == base["stats"]).all() and base["stats"][0, 1] > 0 and base["stats"][0, 2] > 0
    born_b = sorted(-1 - base["src"][0][(base["src"][0] < 0) & (base["src"][0] >= -60)])
    born_p = sorted(order[c] for c in -1 - perm["src"][0][(perm["src"][0] < 0) & (perm["src"][0] >= -60)])
    assert born_b == born_p, "another set of candidates was selected"
    live_b, live_p = base["ids"][0] >= 0, perm["ids"][0] >= 0
    assert (live_b == live_p).all(), "the live slots moved"
    assert sorted(map(tuple, perm["query"][0][live_p].tolist())) == sorted(map(tuple, base["query"][0][live_b].tolist()))


# ------------------------------------------------------------------------------------------------
# CarrySchedule
# ------------------------------------------------------------------------------------------------
def test_schedule_detects_every_k_and_always_on_the_first_hop():
    from comet_amd.stream import CarrySchedule
    s = CarrySchedule(window=4, stride=1, streams=1, detect_every=3)
    assert s.is_first() and s.detects()
    assert [s.hop() for _ in range(7)] == [(True, True), (False, False), (False, False), (False, True),
                                           (False, False), (False, False), (False, True)]
    one = CarrySchedule(window=4, stride=2)
    assert [one.hop() for _ in range(3)] == [(True, True), (False, True), (False, True)]


def test_schedule_resets_one_stream_and_keeps_streams_out_of_phase():
    from comet_amd.stream import CarrySchedule
    s = CarrySchedule(window=4, stride=1, streams=3, detect_every=2)
    assert s.hop(0) == (True, True) and s.hop(0) == (False, False)
    assert s.hop(1) == (True, True)  # stream 1 starts later: its own phase
    assert s.detects(0) and not s.detects(1) and s.is_first(2)
    assert s.hop(0) == (False, True) and s.hop(1) == (False, False)
    s.reset(1)
    assert s.is_first(1) and s.detects(1) and not s.is_first(0) and not s.detects(0)
    assert s.hop(1) == (True, True) and s.hop(0) == (False, False) and s.hop(2) == (True, True)
    s.reset()
    assert all(s.is_first(i) for i in range(3))
    with pytest.raises(ValueError, match="unknown stream"):
        s.hop(3)


@pytest.mark.parametrize("kw", [dict(window=4, stride=4), dict(window=4, stride=5), dict(window=4, stride=0),
                                dict(window=4, streams=0), dict(window=4, detect_every=0)])
def test_schedule_rejects_bad_arguments(kw):
    from comet_amd.stream import CarrySchedule
    with pytest.raises(ValueError):
        CarrySchedule(**kw)


# ------------------------------------------------------------------------------------------------
# constructors
# ------------------------------------------------------------------------------------------------
def _make(kind, **kw):
    from comet_amd.stream import PoseStream, StreamPool
    args = dict(window=4, stride=1, carry=True, carry_tracks=64, carry_min_score=0.5, candidate_fn=lambda f: None)
    args.update(kw)
    return PoseStream(None, **args) if kind == "stream" else StreamPool(None, streams=2, **args)


@pytest.mark.parametrize("kind", ["stream", "pool"])
def test_constructors_reject_bad_carry_arguments(kind):
    assert _make(kind).carry
    with pytest.raises(ValueError, match="stride < window"):
        _make(kind, stride=4)
    with pytest.raises(ValueError, match="candidate_fn"):
        _make(kind, candidate_fn=None)
    with pytest.raises(ValueError, match="carry_min_score"):
        _make(kind, carry_min_score=None)
    with pytest.raises(ValueError, match="carry_tracks"):
        _make(kind, carry_tracks=5000)
    off = _make(kind, carry=False, candidate_fn=None, carry_min_score=None, stride=4)  # carry off: none of it is checked
    assert not off.carry and off._carry is None


@pytest.mark.parametrize("kind", ["stream", "pool"])
def test_query_points_with_carry_is_an_error(kind):
    import torch
    obj = _make(kind)
    frames = torch.zeros(3, 8, 8) if kind == "stream" else torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="query_points together with carry"):
        obj.push(frames, query_points=torch.zeros(64, 2))


def test_stream_result_gains_the_track_fields():
    """None with carry off; they follow the tuple as attributes (its positions are what they were) and
    survive _replace, which the anchor and fusion code applies after the carry fields are set."""
    from comet_amd.stream import StreamResult
    r = StreamResult(0, "enc", None, None)
    assert r.track_ids is None and r.track_age is None and r.track_src is None and len(r) == 12
    c = r.with_tracks("ids", "age", "src")
    assert (c.track_ids, c.track_age, c.track_src) == ("ids", "age", "src") and r.track_ids is None and c == r
    d = c._replace(R="R", final=1)
    assert isinstance(d, StreamResult) and (d.R, d.final, d.pred_pose_enc) == ("R", 1, "enc")
    assert (d.track_ids, d.track_age, d.track_src) == ("ids", "age", "src")
