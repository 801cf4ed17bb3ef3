"""Host-side logic of comet_amd.stream.PoolSchedule (no GPU): the pooled slot layout, which streams
complete a hop in a push, the concatenated slot table, the grouping by query count and the argument
errors of a push."""
import pytest

S, T, CAP = 3, 4, 6
PUSHES = 14
LATE, RESET_AFTER = 2, 5  # stream 1 joins two pushes late; stream 2 is reset after its 5th frame


def _ids(p):
    return [s for s in range(S) if not (s == 1 and p < LATE)]


def _replay(stride):
    """The scenario on a PoolSchedule and on S independent RingSchedule objects ->
    [(push, ids, slots, hops of the pool, {stream: (slot, Hop or None)} of the independent ones)]."""
    from comet_amd.stream import PoolSchedule, RingSchedule
    pool = PoolSchedule(S, T, stride, CAP)
    alone = [RingSchedule(T, stride, CAP) for _ in range(S)]
    out = []
    for p in range(PUSHES):
        if p == RESET_AFTER:
            pool.reset(2)
            alone[2].reset()
        ids = _ids(p)
        due = pool.due(ids)
        slots, hops = pool.push(ids)
        assert due == [s for s, _ in hops], "due() must predict the hops of the push"
        out.append((p, ids, slots, hops, {s: alone[s].push() for s in ids}))
    return pool, out


@pytest.mark.parametrize("stride", [1, 2])
def test_hops_fall_due_where_independent_schedules_say(stride):
    pool, log = _replay(stride)
    seen = 0
    for p, ids, slots, hops, ref in log:
        assert slots == [s * CAP + ref[s][0] for s in ids]
        assert hops == [(s, ref[s][1]) for s in sorted(ids) if ref[s][1] is not None], f"push {p}"
        seen += len(hops)
    assert seen > 0
    # stream 0 from push T - 1, stream 1 two pushes later, stream 2 twice from frame 0
    firsts = {s: [h.frame_index for _, _, _, hops, _ in log for x, h in hops if x == s] for s in range(S)}
    assert firsts[0] == list(range(0, PUSHES - T + 1, stride))
    assert firsts[1] == list(range(0, PUSHES - LATE - T + 1, stride))
    assert firsts[2] == list(range(0, RESET_AFTER - T + 1, stride)) + list(range(0, PUSHES - RESET_AFTER - T + 1, stride))


@pytest.mark.parametrize("stride", [1, 2])
def test_slots_of_different_streams_never_coincide(stride):
    from comet_amd.stream import PoolSchedule
    pool, log = _replay(stride)
    for p, ids, slots, hops, _ in log:
        assert len(set(slots)) == len(slots)
        for s, slot in zip(ids, slots):
            assert s * CAP <= slot < (s + 1) * CAP
    sched = PoolSchedule(S, T, stride, CAP)
    owner = {}
    for s in range(S):
        for f in range(3 * CAP):
            slot = sched.slot(s, f)
            assert slot == s * CAP + f % CAP and 0 <= slot < S * CAP
            assert owner.setdefault(slot, s) == s


@pytest.mark.parametrize("stride", [1, 2])
def test_window_slots_are_the_streams_own_shifted_by_its_offset(stride):
    from comet_amd.stream import RingSchedule
    pool, log = _replay(stride)
    one = RingSchedule(T, stride, CAP)
    for s in range(S):
        for head in range(CAP):
            assert pool.window_slots(s, head) == [s * CAP + x for x in one.window_slots(head)]
    content = {}  # absolute slot -> (stream, frame) held, replayed alongside the hops
    frame = [0] * S
    for p, ids, slots, hops, _ in log:
        if p == RESET_AFTER:
            frame[2] = 0
        for s, slot in zip(ids, slots):
            content[slot] = (s, frame[s])
            frame[s] += 1
        table = pool.table(hops)
        assert len(table) == len(hops) * T
        assert table == [x for s, h in hops for x in pool.window_slots(s, h.head)]
        for i, (s, h) in enumerate(hops):
            # every window holds its own stream's T newest frames, oldest first
            assert [content[x] for x in table[i * T:(i + 1) * T]] == [(s, h.frame_index + j) for j in range(T)]


def test_grouping_by_query_count_keeps_the_stream_order():
    from comet_amd.stream import PoolSchedule
    assert PoolSchedule.group([64, 64, 64]) == [(64, [0, 1, 2])]
    assert PoolSchedule.group([64, 48, 64]) == [(64, [0, 2]), (48, [1])]
    assert PoolSchedule.group([48, 64, 56, 64, 48]) == [(48, [0, 4]), (64, [1, 3]), (56, [2])]
    assert PoolSchedule.group([]) == []


def test_push_ids_are_checked():
    from comet_amd.stream import PoolSchedule
    pool = PoolSchedule(S, T, 1, CAP)
    assert pool.ids(S) == [0, 1, 2]
    assert pool.ids(2, [2, 0]) == [2, 0]
    with pytest.raises(ValueError, match="one frame per push"):
        pool.ids(2, [1, 1])
    with pytest.raises(ValueError, match="unknown stream"):
        pool.ids(2, [0, 3])
    with pytest.raises(ValueError, match="unknown stream"):
        pool.ids(1, [-1])
    with pytest.raises(ValueError, match="pass `streams`"):
        pool.ids(2)
    with pytest.raises(ValueError):
        pool.ids(3, [0, 1])
    with pytest.raises(ValueError, match="unknown stream"):
        pool.reset(7)
    assert all(s.frames_seen == 0 for s in pool.scheds), "a rejected call changes nothing"


def test_constructor_errors_are_those_of_the_ring_schedule():
    from comet_amd.stream import PoolSchedule
    with pytest.raises(ValueError):
        PoolSchedule(0, T)
    with pytest.raises(ValueError):
        PoolSchedule(2, T, capacity=T - 1)
    with pytest.raises(ValueError):
        PoolSchedule(2, T, stride=0)


def test_stream_pool_rejects_bad_pushes_before_any_launch():
    """StreamPool.push on CPU tensors with a model that must not be reached."""
    import torch
    from comet_amd.stream import StreamPool

    class NoModel:
        cfg = None

        def frame_stages(self, frames):
            raise AssertionError("launched")

    q = torch.zeros(8, 2)
    pool = StreamPool(NoModel(), streams=S, window=T, capacity=CAP)
    f = torch.zeros(S, 3, 32, 32)
    with pytest.raises(ValueError, match="no query source"):
        pool.push(f)
    with pytest.raises(ValueError, match="one frame per push"):
        pool.push(f, streams=[0, 1, 1], query_points=q)
    with pytest.raises(ValueError, match="unknown stream"):
        pool.push(f, streams=[0, 1, 3], query_points=q)
    with pytest.raises(ValueError, match="pass `streams`"):
        pool.push(f[:2], query_points=q)
    with pytest.raises(ValueError, match=r"\[k, 3, H, W\]"):
        pool.push(f[0], query_points=q)
    pool._hw = (64, 64)
    with pytest.raises(ValueError, match="frame size changed"):
        pool.push(f, query_points=q)
    pool._hw = None
    for sch in pool.sched.scheds:
        sch.frames_seen = T - 1  # the next frame of every stream completes a hop
    with pytest.raises(ValueError, match=r"streams \[1\]"):
        pool.push(f, query_points={0: q, 2: q})
    with pytest.raises(ValueError, match="anchors must name every stream"):
        StreamPool(NoModel(), streams=2, window=T, anchors={0: (None, None, 1.0, 1.0, "AMD")})
    with pytest.raises(ValueError, match="stride < window"):
        StreamPool(NoModel(), streams=1, window=T, stride=T, anchors=[(None, None, 1.0, 1.0, "AMD")])
