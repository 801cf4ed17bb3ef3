"""Host-side logic of comet_amd.stream (no GPU): the ring's slot arithmetic, the hop schedule,
the anchor-chaining index and the argument errors."""
import pytest
import torch


def _run(window, stride, capacity, n):
    """Push n frames -> (slot of every frame, [(push number, Hop)] of the pushes that emit)."""
    from comet_amd.stream import RingSchedule
    s = RingSchedule(window, stride, capacity)
    slots, hops = [], []
    for i in range(n):
        slot, hop = s.push()
        slots.append(slot)
        if hop is not None:
            hops.append((i, hop))
    return s, slots, hops


@pytest.mark.parametrize("window,capacity", [(4, 4), (4, 5), (4, 9), (1, 1), (3, 7)])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_slots_wrap_and_windows_hold_the_right_frames(window, stride, capacity):
    n = 3 * capacity + window + 2
    s, slots, hops = _run(window, stride, capacity, n)
    assert slots == [f % capacity for f in range(n)]
    assert s.frames_seen == n
    content = {}  # slot -> frame held, replayed alongside the hops
    it = iter(hops)
    nxt = next(it, None)
    for f in range(n):
        content[slots[f]] = f
        if nxt is not None and nxt[0] == f:
            hop = nxt[1]
            ws = s.window_slots(hop.head)
            assert len(ws) == window and all(0 <= x < capacity for x in ws)
            assert len(set(ws)) == window
            # the window is the `window` newest frames, oldest first: no stale slot is read
            assert [content[x] for x in ws] == list(range(f - window + 1, f + 1))
            assert hop.frame_index == f - window + 1 and hop.head == hop.frame_index % capacity
            nxt = next(it, None)
    assert nxt is None


@pytest.mark.parametrize("window,stride,expect", [
    (4, 1, [3, 4, 5, 6, 7, 8, 9]),
    (4, 2, [3, 5, 7, 9]),
    (4, 3, [3, 6, 9]),
    (4, 4, [3, 7]),
    (4, 6, [3, 9]),
    (1, 1, list(range(10))),
])
def test_hop_schedule(window, stride, expect):
    """Which of 10 pushes (numbered from 0) emit a result: the first full window, then every
    `stride` frames."""
    _, _, hops = _run(window, stride, window + 3, 10)
    assert [i for i, _ in hops] == expect
    assert [h.frame_index for _, h in hops] == [i - window + 1 for i in expect]


def test_reset_restarts_the_schedule():
    from comet_amd.stream import RingSchedule
    s = RingSchedule(3, 2, 4)
    first = [s.push() for _ in range(9)]
    s.reset()
    assert s.frames_seen == 0
    assert [s.push() for _ in range(9)] == first


def test_anchor_chain_index():
    """The next window starts `stride` frames into the current one, so its reference is the pose at
    window position `stride`; with stride >= window that frame has no estimate."""
    from comet_amd.stream import RingSchedule
    for window, stride in [(4, 1), (4, 2), (4, 3), (16, 15)]:
        s = RingSchedule(window, stride)
        assert s.chain_index() == stride
        hops = [h for h in (s.push()[1] for _ in range(3 * window)) if h is not None]
        for a, b in zip(hops, hops[1:]):
            assert b.frame_index == a.frame_index + s.chain_index()
    for window, stride in [(4, 4), (4, 5), (1, 1)]:
        with pytest.raises(ValueError, match="stride < window"):
            RingSchedule(window, stride).chain_index()


def test_schedule_argument_errors():
    from comet_amd.stream import RingSchedule
    with pytest.raises(ValueError, match="capacity"):
        RingSchedule(4, 1, 3)
    with pytest.raises(ValueError, match="stride"):
        RingSchedule(4, 0)
    with pytest.raises(ValueError, match="window"):
        RingSchedule(0)
    assert RingSchedule(4).capacity == 4


class _Model:
    """Stands in for COMET where PoseStream must fail before it touches the model."""
    cfg = {"mixed_precision": "bf16"}

    def frame_stages(self, frames):
        raise AssertionError("argument errors must be raised before any model call")


def test_stream_argument_errors():
    from comet_amd.stream import PoseStream
    m = _Model()
    with pytest.raises(ValueError, match="capacity"):
        PoseStream(m, window=4, capacity=3)
    with pytest.raises(ValueError, match="stride"):
        PoseStream(m, window=4, stride=0)
    anchor = (torch.tensor([1.0, 0, 0, 0]), torch.tensor([320.0, 240.0, 10.0]), 268.44, 0.5, "AMD")
    with pytest.raises(ValueError, match="stride < window"):
        PoseStream(m, window=4, stride=4, anchor=anchor, query_fn=lambda f: None)
    s = PoseStream(m, window=4)
    assert s.precision == torch.bfloat16
    with pytest.raises(ValueError, match="no query source"):
        s.push(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="frames"):
        s.push(torch.zeros(8, 8), query_points=torch.zeros(2, 2))
    with pytest.raises(ValueError, match="frames"):
        s.push(torch.zeros(2, 4, 8, 8), query_points=torch.zeros(2, 2))


def test_stream_rejects_a_changed_frame_size():
    from comet_amd.stream import PoseStream
    s = PoseStream(_Model(), window=4, query_fn=lambda f: None)
    s._hw = (8, 8)  # as after a first push of 8 x 8 frames
    with pytest.raises(ValueError, match="frame size changed"):
        s.push(torch.zeros(3, 8, 12))
    s.reset()
    assert s._hw is None and s.sched.frames_seen == 0


def test_stream_eval_is_opt_in():
    from comet_amd import loop
    with pytest.raises(ValueError, match="opt-in"):
        loop.stream_eval(_Model(), iter(()), {"stream": {"enable": False}}, (0, 0, 8, 8), "unused.csv")
    with pytest.raises(ValueError, match="opt-in"):
        loop.stream_eval(_Model(), iter(()), {}, (0, 0, 8, 8), "unused.csv")


def test_sequence_stream_yields_every_frame_in_order_and_one_box(tmp_path):
    import numpy as np
    from PIL import Image
    from comet_amd import loop
    seq = tmp_path / "model1" / "seq_0"
    (seq / "frames").mkdir(parents=True)
    (seq / "Mask").mkdir()
    for i in range(5):
        Image.fromarray(np.full((40, 60, 3), i, dtype=np.uint8)).save(seq / "frames" / f"frame_{i:04d}.png")
        m = np.zeros((40, 60), dtype=np.uint8)
        m[10:20, 20 + i:30 + i] = 255  # the object drifts right
        Image.fromarray(m).save(seq / "Mask" / f"mask_{i:04d}.png")
    frames, box = loop.sequence_stream(str(seq))
    frames = list(frames)
    assert [int(f[0, 0, 0]) for f in frames] == [0, 1, 2, 3, 4]
    assert frames[0].shape == (40, 60, 3) and frames[0].dtype == np.uint8
    x0, y0, x1, y1 = box
    assert x1 - x0 == y1 - y0 > 0, "square box"
    assert x0 <= 20 and x1 >= 33 and y0 <= 10 and y1 >= 19, "covers the object in every frame"
