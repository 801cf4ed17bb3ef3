"""Online pose estimation: a sliding window over a frame stream with a per-frame cache
(DESIGN.md "Online / streaming inference").

COMET.forward takes a closed [1, T, 3, H, W] sequence. Fed one frame at a time, a caller would run
it on every window and recompute the DINOv2 backbone and the tracker's BasicEncoder on T - 1 frames
it has already seen. Those stages see one frame at a time (COMET.frame_stages); PoseStream runs
them once per frame, keeps their outputs in device rings, and for every hop gathers the window
(comet_ring_gather, one launch) and runs only the part of the model that mixes frames
(model(..., frame_cache=...)).

  RingSchedule   the slot / hop arithmetic, host only (no tensors)
  PoseStream     push(frame | frames) -> one StreamResult per completed hop
  keypoint_query query_fn from the SuperPoint / SIFT detectors of comet_amd.keypoints
"""
import ctypes
from typing import NamedTuple, Optional

import torch

from . import functional as F
from . import ops


class Hop(NamedTuple):
    frame_index: int  # global index of the window's first frame
    head: int         # ring slot of that frame; the window is slots (head + i) % capacity, i < window


class RingSchedule:
    """Which ring slot a frame lands in and which pushes complete a hop. Frame f (global index,
    from 0) is stored in slot f % capacity, overwriting frame f - capacity. A hop is due when a full
    window ends at the newest frame and (frames_seen - window) % stride == 0; its window is the
    frames [frames_seen - window, frames_seen), which are always still in the ring because
    capacity >= window."""

    def __init__(self, window, stride=1, capacity=None):
        capacity = window if capacity is None else capacity
        if window < 1:
            raise ValueError(f"window must be at least 1, got {window}")
        if stride < 1:
            raise ValueError(f"stride must be at least 1, got {stride}")
        if capacity < window:
            raise ValueError(f"capacity {capacity} is below the window length {window}")
        self.window, self.stride, self.capacity = int(window), int(stride), int(capacity)
        self.frames_seen = 0

    def reset(self):
        self.frames_seen = 0

    def slot(self, frame_index):
        return frame_index % self.capacity

    def window_slots(self, head):
        return [(head + i) % self.capacity for i in range(self.window)]

    def push(self):
        """Account for one new frame -> (its slot, the Hop it completes or None)."""
        slot = self.slot(self.frames_seen)
        self.frames_seen += 1
        first = self.frames_seen - self.window
        if first >= 0 and first % self.stride == 0:
            return slot, Hop(first, self.slot(first))
        return slot, None

    def chain_index(self):
        """Anchor chaining: the position, inside a window, of the frame that is the next window's
        first frame (= stride). Only a frame of the current window has an estimated pose."""
        if self.stride >= self.window:
            raise ValueError(f"anchor chaining needs stride < window (stride {self.stride}, window {self.window}): "
                             "the next window's first frame must lie inside the current window")
        return self.stride


class StreamResult(NamedTuple):
    frame_index: int                   # global index of the window's first frame
    pred_pose_enc: torch.Tensor        # [T, 7], relative to the window's first frame
    pred_tracks: Optional[torch.Tensor]  # [T, N, 2]
    pred_score: Optional[torch.Tensor]   # [T, N]
    R: Optional[torch.Tensor] = None   # [T, 4] absolute quaternions (anchor given)
    T: Optional[torch.Tensor] = None   # [T, 3] absolute translations, float64 (anchor given)


class Anchor(NamedTuple):
    R: torch.Tensor        # [4] quaternion of the stream's first frame
    T_uvz: torch.Tensor    # [3] (u, v, z) of the stream's first frame
    focal: float           # kept for the caller; the pose codec's decode does not read it
    ratio: object          # as gt_cameras.ratio: host float or float64 tensor
    dataset: str           # key of models.utils.INTRINSICS


def _model_precision(model):
    cfg = getattr(model, "cfg", None)
    mp = cfg.get("mixed_precision", "no") if cfg is not None and hasattr(cfg, "get") else "no"
    return torch.bfloat16 if mp == "bf16" else torch.float32


class PoseStream:
    """Sliding-window pose estimation over a frame stream.

        stream = PoseStream(model, window=16, stride=1, query_fn=keypoint_query(sp))
        for frame in camera:                       # [3, H, W] f32, normalised as the model expects
            for r in stream.push(frame):           # one result per completed hop
                use(r.frame_index, r.pred_pose_enc)

    push() runs the per-frame stages on the new frame(s) (k frames pushed together are one batched
    call) under torch.no_grad() and the model's precision (cfg.mixed_precision, or `precision`),
    stores them in the ring, and whenever a full window ends at a frame with
    (frames_seen - window) % stride == 0 gathers that window and calls
    model(..., training=False, tracks=..., frame_cache=...). The window's query points are
    `query_points` [N, 2] of the push, else query_fn(first frame of the window [3, H, W]).

    Results are relative to each window's first frame, as the model defines its encoding. With
    anchor=(R0 quaternion [4], T_uvz0 [3], focal, ratio, dataset) every result also carries absolute
    R [T, 4] and T [T, 3] from ops.pose_decode: the first window is decoded against the anchor, each
    later window against the pose already estimated for the frame that is now its first frame (so
    stride < window is required). That frame's (u, v, z) is rounded to the codec's f32 before it
    becomes the reference, and the earlier window's result reports the rounded pose, so a frame that
    is a window's first frame has one pose in both results. Errors of successive references add up:
    the drift accumulates over the stream and is not corrected.

    One stream (batch 1). The model is used as is (its eval / train mode included)."""

    def __init__(self, model, window, stride=1, capacity=None, query_fn=None, anchor=None, precision=None):
        self.model = model
        self.sched = RingSchedule(window, stride, capacity)
        self.query_fn = query_fn
        self.precision = precision if precision is not None else _model_precision(model)
        self.anchor = None
        if anchor is not None:
            self.sched.chain_index()  # raises unless stride < window
            self.anchor = Anchor(*anchor)
        self.reset()

    def reset(self):
        """Forget every frame (the next push starts a new stream at frame 0, at the anchor)."""
        self.sched.reset()
        self._rings = None   # FrameCache-ordered list of [capacity, ...] tensors (None where unused)
        self._wins = None    # the gathered window, same order, [window, ...]
        self._hw = None
        self._ref = None     # (R [4] f32, T_uvz [3] f32) the next hop is decoded against

    # -- ring -------------------------------------------------------------------------------------
    @staticmethod
    def _per_frame(cache):
        """FrameCache of one k-frame sequence -> its tensors as [k, ...] (None where unused)."""
        return [None if cache.fmaps is None else cache.fmaps[0], cache.refine_frames[0], cache.tokens]

    def _allocate(self, per, dev):
        cap, T = self.sched.capacity, self.sched.window
        self._rings, self._wins = [], []
        for t in per:
            if t is None:
                self._rings.append(None)
                self._wins.append(None)
                continue
            slot = t.shape[1:]
            if (slot.numel() * t.element_size()) % 16 != 0:
                raise ValueError(f"frame size not supported by the ring: a slot of {tuple(slot)} {t.dtype} is no "
                                 "multiple of 16 bytes")
            self._rings.append(torch.empty(cap, *slot, device=dev, dtype=t.dtype))
            self._wins.append(torch.empty(T, *slot, device=dev, dtype=t.dtype))
        # the slot table of every possible head, on the device and on the host
        rows = [self.sched.window_slots(h) for h in range(cap)]
        self._tables = torch.tensor(rows, dtype=torch.int32, device=dev)
        self._tables_host = [(ctypes.c_int32 * T)(*r) for r in rows]

    def _store(self, per, i, slot):
        for ring, t in zip(self._rings, per):
            if ring is not None:
                ring[slot].copy_(t[i])

    def _gather(self, head):
        """The window whose first frame sits in slot `head`, contiguous, as a FrameCache (B = 1)."""
        pairs = [(r, w) for r, w in zip(self._rings, self._wins) if r is not None]
        ops.ring_gather(pairs, self._tables[head], self._tables_host[head])
        from .models.E2Epose2 import FrameCache
        fm, fr, tok = self._wins
        return FrameCache(fmaps=None if fm is None else fm[None], refine_frames=fr[None], tokens=tok)

    # -- hops -------------------------------------------------------------------------------------
    def _decode(self, enc, T):
        from .models.utils import INTRINSICS
        a = self.anchor
        Rref, uvz = self._ref
        intr = INTRINSICS[a.dataset]
        R, Tx = ops.pose_decode(enc, Rref.expand(T, 4).contiguous(), uvz.expand(T, 3).contiguous(), a.ratio, intr, 1, T)
        # the next window's reference: this window's frame `stride`, its (u, v, z) in the codec's f32
        s = self.sched.chain_index()
        ratio = self._ratio
        e = enc[s].double()
        u0 = uvz.double()
        nxt = torch.stack([u0[0] + e[0] / ratio * 128.0, u0[1] + e[1] / ratio * 128.0,
                           u0[2] * (e[2] / ratio + 1.0)]).float()
        self._ref = (R[s].clone(), nxt)
        # report frame `stride` as the next window will see it (its first frame decodes to exactly this)
        ident = torch.zeros(1, 7, device=enc.device)
        ident[0, 3] = 1.0
        Rs, Ts = ops.pose_decode(ident, self._ref[0][None], nxt[None], a.ratio, intr, 1, 1)
        R[s], Tx[s] = Rs[0], Ts[0]
        return R, Tx

    def _hop(self, hop, query_points):
        T = self.sched.window
        cache = self._gather(hop.head)
        if query_points is None:
            query_points = self.query_fn(cache.refine_frames[0, 0])
        q = query_points.to(self._tables.device, torch.float32)
        tracks = q[None, None].expand(1, T, -1, 2)
        # (with a frame_cache the model reads only the shape of its image argument)
        out = self.model(cache.refine_frames, training=False, tracks=tracks, frame_cache=cache)
        enc = out["pred_pose_enc"]
        tr = out.get("pred_tracks")
        sc = out.get("_track_predictions", {}).get("pred_score")
        R = Tx = None
        if self.anchor is not None:
            R, Tx = self._decode(enc, T)
        return StreamResult(hop.frame_index, enc, None if tr is None else tr[0], None if sc is None else sc[0], R, Tx)

    @torch.no_grad()
    def push(self, frames, query_points=None):
        """frames [3, H, W] or [k, 3, H, W] f32 on the model's device -> list of StreamResult, one
        per hop the new frames complete (often empty)."""
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f"push takes [3, H, W] or [k, 3, H, W] frames, got {tuple(frames.shape)}")
        hw = tuple(frames.shape[-2:])
        if self._hw is not None and hw != self._hw:
            raise ValueError(f"frame size changed from {self._hw} to {hw}; reset() starts a new stream")
        if query_points is None and self.query_fn is None:
            raise ValueError("no query source: pass query_points to push() or query_fn to PoseStream")
        results = []
        with F.precision(self.precision):
            per = self._per_frame(self.model.frame_stages(frames.float()))
            if self._rings is None:
                self._allocate(per, frames.device)
                self._hw = hw
                if self.anchor is not None:
                    a, dev = self.anchor, frames.device
                    self._ref = (torch.as_tensor(a.R, dtype=torch.float32).to(dev).reshape(4),
                                 torch.as_tensor(a.T_uvz, dtype=torch.float32).to(dev).reshape(3))
                    self._ratio = torch.as_tensor(a.ratio, dtype=torch.float64).reshape(-1)[0].to(dev)
            for i in range(frames.shape[0]):
                slot, hop = self.sched.push()
                self._store(per, i, slot)
                if hop is not None:
                    results.append(self._hop(hop, query_points))
        return results


def keypoint_query(sp, sift=None, mask_fn=None, track_num=512, min_required=256):
    """query_fn for PoseStream from the detectors of comet_amd.keypoints: SuperPoint.extract (plus
    SIFT.extract when given) on the window's first frame, then filter_and_pad against
    mask_fn(frame [3, H, W]) -> bool [H, W] (all true when mask_fn is None) -> [N, 2],
    min_required <= N <= track_num, as the evaluation loop initialises its tracks."""
    from .keypoints import filter_and_pad

    def query(frame):
        pts = sp.extract(frame)["keypoints"][0]
        if sift is not None:
            pts = torch.cat([pts, sift.extract(frame)["keypoints"][0]], 0)
        H, W = frame.shape[-2:]
        mask = torch.ones(H, W, dtype=torch.bool, device=frame.device) if mask_fn is None else mask_fn(frame).bool()
        return filter_and_pad(pts, mask, min(min_required, track_num), track_num)
    return query
