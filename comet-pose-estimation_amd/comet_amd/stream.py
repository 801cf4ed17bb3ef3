"""Online pose estimation: a sliding window over a frame stream with a per-frame cache
(DESIGN.md "Online / streaming inference").

COMET.forward takes a closed [1, T, 3, H, W] sequence. Fed one frame at a time, a caller would run
it on every window and recompute the DINOv2 backbone and the tracker's BasicEncoder on T - 1 frames
it has already seen. Those stages see one frame at a time (COMET.frame_stages); PoseStream runs
them once per frame, keeps their outputs in device rings, and for every hop gathers the window
(comet_ring_gather, one launch) and runs only the part of the model that mixes frames
(model(..., frame_cache=...)).

  RingSchedule   the slot / hop arithmetic, host only (no tensors)
  PoseStream     push(frame | frames) -> one StreamResult per completed hop; a StreamPool of one stream
  PoolSchedule   the same arithmetic for S streams over pooled rings, host only
  StreamPool     S streams on one model: push(one frame per stream) runs the per-frame stages, the
                 ring store (comet_ring_scatter) and the hops that fall due as one batch each
  FuseSchedule   which hop is a stream's first, which window positions are new / final, host only
  PoseFuser      one fused pose per frame from the overlapping windows (comet_pose_fuse, one launch
                 per push); usable on its own with any [n, T, 7] encodings
  CarrySchedule  which hop is a stream's first and on which hops the detector runs, host only
  TrackCarry     persistent track ids: the next window's queries are this window's tracks on the frame
                 that becomes first (comet_track_carry, one launch per push); with warm_mode also where
                 the coarse tracker starts in the new window (comet_track_warm, one launch per push)
  LandmarkMap    one 3-D point per carried track, triangulated from the frames whose fused pose is final
                 (comet_landmark_update, one launch per push)
  MotionTracker  the target's angular and linear velocity from the final fused poses, with predictions for the
                 next frames (comet_motion_fit, one launch per push)
  keypoint_query query_fn from the SuperPoint / SIFT detectors of comet_amd.keypoints
  keypoint_candidates  candidate_fn of the same detectors for carry=True: raw detections, no padding
"""
import ctypes
import math
from typing import NamedTuple, Optional

import torch

from . import _lib as L
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


class _StreamFields(NamedTuple):
    frame_index: int                   # global index of the window's first frame
    pred_pose_enc: torch.Tensor        # [T, 7], relative to the window's first frame
    pred_tracks: Optional[torch.Tensor]  # [T, N, 2]
    pred_score: Optional[torch.Tensor]   # [T, N]
    R: Optional[torch.Tensor] = None   # [T, 4] absolute quaternions (anchor given)
    T: Optional[torch.Tensor] = None   # [T, 3] absolute translations, float64 (anchor given)
    # fuse=True only: one pose per frame from every window that has seen it so far (PoseFuser)
    fused_R: Optional[torch.Tensor] = None       # [T, 4]
    fused_T: Optional[torch.Tensor] = None       # [T, 3] float64
    fused_count: Optional[torch.Tensor] = None   # [T] int32, hypotheses fused
    rot_spread: Optional[torch.Tensor] = None    # [T] radians
    trans_spread: Optional[torch.Tensor] = None  # [T, 3], of (u, v, z)
    final: Optional[int] = None  # the leading positions whose fused pose will not change again


class StreamResult(_StreamFields):
    """The tuple above, followed by four fields that are attributes only (the tuple keeps its twelve
    positions, so code that unpacks or slices a result sees what it saw): with carry=True the identity
    of the track in every query slot (TrackCarry), else None; with warm=True also how the coarse
    tracker started in every slot, else None."""
    track_ids: Optional[torch.Tensor] = None  # [N] int32, -1: a pad
    track_age: Optional[torch.Tensor] = None  # [N] int32 hops the track has lived
    track_src: Optional[torch.Tensor] = None  # [N] int32: j carried, -1 - c born from candidate c, else a pad
    track_warm: Optional[torch.Tensor] = None  # [N] int32: 0 cold, 1 carried, 2 pad of a carried slot, -1 fallen back
    # landmarks=True only (LandmarkMap; attributes too, the tuple keeps its twelve positions)
    landmarks: Optional[torch.Tensor] = None       # [N, 3] float64, body frame; 0 where landmark_state != 1
    landmark_obs: Optional[torch.Tensor] = None    # [N] int32 frames the landmark has been seen in
    landmark_err: Optional[torch.Tensor] = None    # [N] f32 reprojection error in pixels on position `stride`
    landmark_state: Optional[torch.Tensor] = None  # [N] int32: 1 valid, 0 none, 2 ill-conditioned, 3 behind, -1 not finite
    # pnp=True only (LandmarkMap.pnp): every frame of the window posed against the landmark map
    pnp_R: Optional[torch.Tensor] = None        # [T, 4] f32 quaternion (fused_R where pnp_state != 1)
    pnp_T: Optional[torch.Tensor] = None        # [T, 3] float64 (fused_T where pnp_state != 1)
    pnp_inliers: Optional[torch.Tensor] = None  # [T] int32 landmarks within pnp_huber_px at the refined pose
    pnp_rms_px: Optional[torch.Tensor] = None   # [T] f32 weighted rms reprojection error (+inf where pnp_state != 1)
    pnp_state: Optional[torch.Tensor] = None    # [T] int32: 1 solved, 0 too few landmarks, 2 degenerate, -1 not finite
    # motion=True only (MotionTracker; attributes too): a constant-rate fit to the final fused poses so far.
    # (Plain class attributes: the annotated fields above end with the PnP ones.)
    motion_omega = None      # [3] float64 rad / frame, camera frame: R(tau) = Exp(omega tau) R0
    motion_vel = None        # [3] float64 per frame
    motion_q0 = None         # [4] float64 fitted rotation at the newest final frame
    motion_t0 = None         # [3] float64 fitted translation at the newest final frame
    motion_rot_rms = None    # [] f32 rad (+inf where motion_state != 1)
    motion_trans_rms = None  # [3] f32 (+inf where motion_state != 1)
    motion_frames = None     # [] int32 frames the fit used
    motion_state = None      # [] int32: 1 fitted, 0 too few, 2 degenerate, 3 too fast, -1 not finite
    motion_pred_R = None     # [T - stride + horizon, 4] float64, 1, 2, .. frames past the newest final one
    motion_pred_T = None     # [T - stride + horizon, 3] float64
    motion_innov_rot = None    # [T - stride] f32 rad: fused against predicted, positions [stride, T)
    motion_innov_trans = None  # [T - stride] f32
    # lm_archive > 0 only (LandmarkMap.reidentify; attributes too)
    landmark_ids = None  # [N] int32 landmark identity: the archived id of a restored landmark, else track_ids
    reid_state = None    # [N] int32: 0 not born, 1 matched to the archive, 2 no candidate, 3 its pick took another slot
    reid_dist = None     # [N] f32 pixel distance of a match (+inf where reid_state != 1)

    def _replace(self, **kw):
        r = super()._replace(**kw)
        r.__dict__.update(self.__dict__)
        return r

    def with_tracks(self, track_ids, track_age, track_src, track_warm=None):
        r = self._replace()
        r.track_ids, r.track_age, r.track_src, r.track_warm = track_ids, track_age, track_src, track_warm
        return r

    def with_landmarks(self, lo, b):
        """The result with row b of an ops.LandmarkOut."""
        r = self._replace()
        r.landmarks, r.landmark_obs, r.landmark_err, r.landmark_state = lo.X[b], lo.n_obs[b], lo.err_px[b], lo.state[b]
        return r

    def with_reid(self, ro, b):
        """The result with row b of an ops.ReidOut."""
        r = self._replace()
        r.landmark_ids, r.reid_state, r.reid_dist = ro.lm_id[b], ro.reid_state[b], ro.reid_dist[b]
        return r

    def with_pnp(self, po, b):
        """The result with row b of an ops.PnpOut."""
        r = self._replace()
        r.pnp_R, r.pnp_T, r.pnp_inliers, r.pnp_rms_px, r.pnp_state = po.R[b], po.T[b], po.inliers[b], po.rms_px[b], po.state[b]
        return r

    def with_motion(self, mo, b):
        """The result with row b of an ops.MotionOut."""
        r = self._replace()
        r.motion_omega, r.motion_vel, r.motion_q0, r.motion_t0 = mo.omega[b], mo.vel[b], mo.q0[b], mo.t0[b]
        r.motion_rot_rms, r.motion_trans_rms, r.motion_frames, r.motion_state = (mo.rot_rms[b], mo.trans_rms[b],
                                                                                 mo.n_used[b], mo.state[b])
        r.motion_pred_R, r.motion_pred_T = mo.pred_q[b], mo.pred_t[b]
        r.motion_innov_rot, r.motion_innov_trans = mo.innov_rot[b], mo.innov_trans[b]
        return r


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


def _anchor_ref(anchor, dev):
    """Anchor -> ((R [4] f32, T_uvz [3] f32) the first hop is decoded against, ratio as a float64
    device scalar)."""
    ref = (torch.as_tensor(anchor.R, dtype=torch.float32).to(dev).reshape(4),
           torch.as_tensor(anchor.T_uvz, dtype=torch.float32).to(dev).reshape(3))
    return ref, torch.as_tensor(anchor.ratio, dtype=torch.float64).reshape(-1)[0].to(dev)


def _decode_chained(a, ref, ratio, s, enc, T):
    """One window's absolute poses: enc [T, 7] decoded against ref = (R [4], T_uvz [3]) of its first
    frame -> (R [T, 4], T [T, 3] float64, the next window's ref). s: the position in this window of
    the next window's first frame (RingSchedule.chain_index)."""
    from .models.utils import INTRINSICS
    Rref, uvz = ref
    intr = INTRINSICS[a.dataset]
    R, Tx = ops.pose_decode(enc, Rref.expand(T, 4).contiguous(), uvz.expand(T, 3).contiguous(), a.ratio, intr, 1, T)
    # the next window's reference: this window's frame `stride`, its (u, v, z) in the codec's f32
    e = enc[s].double()
    u0 = uvz.double()
    nxt = torch.stack([u0[0] + e[0] / ratio * 128.0, u0[1] + e[1] / ratio * 128.0,
                       u0[2] * (e[2] / ratio + 1.0)]).float()
    ref = (R[s].clone(), nxt)
    # report frame `stride` as the next window will see it (its first frame decodes to exactly this)
    ident = torch.zeros(1, 7, device=enc.device)
    ident[0, 3] = 1.0
    Rs, Ts = ops.pose_decode(ident, ref[0][None], nxt[None], a.ratio, intr, 1, 1)
    R[s], Tx[s] = Rs[0], Ts[0]
    return R, Tx, ref


class FuseSchedule:
    """The host-only arithmetic of pose fusion for `streams` streams of one window / stride. A
    stream's first hop (after construction or reset) is decoded against its anchor and every
    position of it is new: fresh_from = 1. In a later hop the positions [window - stride, window)
    are frames no earlier window has seen (fresh_from = window - stride; their accumulator rows are
    overwritten, the others added to). The first `final` = stride positions of any hop appear in no
    later window: their fused pose will not change again."""

    def __init__(self, window, stride=1, streams=1):
        if stride < 1 or stride >= window:
            raise ValueError(f"pose fusion needs 1 <= stride < window (stride {stride}, window {window}): the next "
                             "window's first frame must lie inside the current window")
        if streams < 1:
            raise ValueError(f"at least 1 stream, got {streams}")
        self.window, self.stride, self.streams = int(window), int(stride), int(streams)
        self._first = [True] * self.streams

    @property
    def final(self):
        return self.stride

    def reset(self, stream=None):
        for s in (range(self.streams) if stream is None else [self._id(stream)]):
            self._first[s] = True

    def _id(self, stream):
        s = int(stream)
        if not 0 <= s < self.streams:
            raise ValueError(f"unknown stream {s}: the schedule has streams 0 .. {self.streams - 1}")
        return s

    def is_first(self, stream=0):
        """Whether the next hop of the stream is its first (nothing is advanced)."""
        return self._first[self._id(stream)]

    def hop(self, stream=0):
        """Account for one hop of the stream -> (first, fresh_from)."""
        s = self._id(stream)
        first = self._first[s]
        self._first[s] = False
        return first, (1 if first else self.window - self.stride)


class PoseFuser:
    """One pose per frame from overlapping windows (DESIGN.md "Pose fusion").

        fuser = PoseFuser(window=T, stride=1, anchors=[(R0 [4], T_uvz0 [3])], ratio=ratio, intr=(fx, fy, cx, cy))
        out = fuser.fuse(enc, [(0, hop)])        # enc [1, T, 7]; hop: the Hop RingSchedule.push gave

    Owns the accumulator ring acc [streams * capacity, 20] float64 on the device (row of frame f of
    stream s: s * capacity + f % capacity, the slot numbering of the frame rings) and a FuseSchedule.
    fuse() is one comet_pose_fuse launch for all the hops given (at most one per stream): each hop is
    referenced to the fused pose of its first frame (its anchor for a stream's first hop), every
    frame's row takes the hop's hypothesis, and the fused pose, count and spread of every frame of
    every hop come back (ops.FuseOut, [n, T, ...]). The small per-hop int32 tables are cached on the
    device by their values, so a steady-state call uploads nothing. Fusion reduces the drift of
    single-estimate chaining, it does not remove it: there is no loop closure and no global
    optimisation, and as stride approaches window / 2 the chained frame has one hypothesis only and
    nothing is gained."""

    _TABLES_MAX = 1024

    def __init__(self, window, stride=1, capacity=None, streams=1, anchors=None, ratio=1.0, intr=None, device="cuda"):
        self.ring = PoolSchedule(streams, window, stride, capacity)
        self.sched = FuseSchedule(window, stride, streams)
        if intr is None or len(intr) != 4:
            raise ValueError("PoseFuser needs intr = (fx, fy, cx, cy)")
        self.ratio, self.intr = ratio, tuple(float(v) for v in intr)
        self.device = torch.device(device)
        self.acc = torch.zeros(self.ring.streams * self.ring.capacity, 20, dtype=torch.float64, device=self.device)
        self._anchors = torch.zeros(self.ring.streams, 7, dtype=torch.float64)  # host; rows go up by stream tuple
        self._anchors[:, 0] = 1.0
        self._set = [False] * self.ring.streams
        self._tables, self._anchor_rows = {}, {}
        if anchors is not None:
            for s, a in (anchors.items() if isinstance(anchors, dict) else enumerate(anchors)):
                self.set_anchor(s, a[0], a[1])

    def set_anchor(self, stream, R, T_uvz):
        """The pose of the stream's first frame: R [4] quaternion, T_uvz [3]; read by its next first hop."""
        s = self.sched._id(stream)
        row = torch.cat([torch.as_tensor(R).detach().double().reshape(4).cpu(),
                         torch.as_tensor(T_uvz).detach().double().reshape(3).cpu()])
        self._anchors[s] = row
        self._set[s] = True
        self._anchor_rows.clear()

    def reset(self, stream=None):
        """The next hop of `stream` (default: of every stream) is a first hop again, at its anchor.
        Its rows need no clearing: a first hop overwrites every row it touches."""
        self.sched.reset(stream)

    def _table(self, values):
        key = tuple(values)
        hit = self._tables.get(key)
        if hit is None:
            if len(self._tables) >= self._TABLES_MAX:
                self._tables.clear()
            hit = (torch.tensor(key, dtype=torch.int32, device=self.device), (ctypes.c_int32 * len(key))(*key))
            self._tables[key] = hit
        return hit

    def fuse(self, enc, hops, weights=None):
        """enc [n, T, 7] f32 (or [n * T, 7]) of the n hops `hops` = [(stream, Hop)], weights [n, T]
        f32 or None -> ops.FuseOut. The streams must be distinct."""
        T = self.ring.window
        ids = tuple(self.sched._id(s) for s, _ in hops)
        n = len(ids)
        if n == 0 or len(set(ids)) != n:
            raise ValueError(f"fuse takes at least one hop and one hop per stream, got the streams {list(ids)}")
        if enc.numel() != n * T * 7:
            raise ValueError(f"{n} hops of window {T} need enc [{n}, {T}, 7], got {tuple(enc.shape)}")
        missing = [s for s in ids if self.sched.is_first(s) and not self._set[s]]
        if missing:
            raise ValueError(f"no anchor for the streams {missing}, whose first hop this is")
        flags = [(self.sched.is_first(s), 1 if self.sched.is_first(s) else T - self.sched.stride) for s in ids]
        slots, slots_host = self._table(self.ring.table(list(hops)))
        fresh, fresh_host = self._table([f for _, f in flags])
        first, first_host = self._table([int(f) for f, _ in flags])
        rows = self._anchor_rows.get(ids)
        if rows is None:
            rows = self._anchor_rows[ids] = self._anchors[list(ids)].contiguous().to(self.device)
        out = ops.pose_fuse(enc.view(n, T, 7), self.acc, slots, slots_host, fresh, fresh_host, first, first_host, rows,
                            self.ratio, self.intr, weights)
        for s in ids:  # (only a launch that went out advances the schedule)
            self.sched.hop(s)
        return out


def _score_weights(sc):
    """fuse_weight="score": pred_score [n, T, N] -> weights [n, T], the mean over the tracks, at least 1e-6."""
    if sc is None:
        raise RuntimeError('fuse_weight="score" needs the model\'s pred_score output')
    return sc.float().mean(-1).clamp_min(1e-6).contiguous()


def _check_fuse(fuse, fuse_weight, anchored):
    if fuse_weight not in (None, "score"):
        raise ValueError(f'fuse_weight must be None or "score", got {fuse_weight!r}')
    if fuse and not anchored:
        raise ValueError("fuse=True needs an anchor: fused poses are absolute")


def _fused_fields(out, b, final):
    return dict(R=out.hyp_R[b], T=out.hyp_T[b], fused_R=out.R[b], fused_T=out.T[b], fused_count=out.count[b],
                rot_spread=out.rot_spread[b], trans_spread=out.trans_spread[b], final=final)


class CarrySchedule:
    """The host-only arithmetic of track carry for `streams` streams of one window / stride: which hop
    of a stream is its first (after construction or reset: nothing to carry, prev_valid = 0) and on
    which hops the detector runs (hop index % detect_every == 0, so always on the first). The next
    window's first frame must lie inside the current one: stride < window."""

    def __init__(self, window, stride=1, streams=1, detect_every=1):
        if stride < 1 or stride >= window:
            raise ValueError(f"track carry needs 1 <= stride < window (stride {stride}, window {window}): the next "
                             "window's first frame must lie inside the current window")
        if streams < 1:
            raise ValueError(f"at least 1 stream, got {streams}")
        if detect_every < 1:
            raise ValueError(f"detect_every must be at least 1, got {detect_every}")
        self.window, self.stride, self.streams = int(window), int(stride), int(streams)
        self.detect_every = int(detect_every)
        self._hops = [0] * self.streams

    def _id(self, stream):
        s = int(stream)
        if not 0 <= s < self.streams:
            raise ValueError(f"unknown stream {s}: the schedule has streams 0 .. {self.streams - 1}")
        return s

    def reset(self, stream=None):
        for s in (range(self.streams) if stream is None else [self._id(stream)]):
            self._hops[s] = 0

    def is_first(self, stream=0):
        """Whether the next hop of the stream is its first (nothing is advanced)."""
        return self._hops[self._id(stream)] == 0

    def detects(self, stream=0):
        """Whether the detector runs on the next hop of the stream (nothing is advanced)."""
        return self._hops[self._id(stream)] % self.detect_every == 0

    def hop(self, stream=0):
        """Account for one hop of the stream -> (first, detect)."""
        s = self._id(stream)
        out = (self._hops[s] == 0, self._hops[s] % self.detect_every == 0)
        self._hops[s] += 1
        return out


class TrackCarry:
    """Persistent track identities across windows (DESIGN.md "Track carry").

        carry = TrackCarry(window=T, stride=1, tracks=512, min_score=0.5)
        out = carry.step([0], H, W, cands=[detections [M, 2]], masks=[None])   # ops.CarryOut, [1, N, ...]
        ... run the model with out.query[0] as the window's query points ...
        carry.update([0], pred_tracks [1, T, N, 2], pred_score [1, T, N])

    Holds, per stream, the ids and ages of the N query slots and the id counter on the device, and a
    reference to the stream's last pred_tracks / pred_score. step() is one comet_track_carry launch
    for all the hops given (at most one per stream): a track that is still alive on the frame that
    is now first (inside the frame and the mask, score >= min_score) and holds its grid cell keeps
    its slot and id, free slots take candidates in detector order, the rest is padded (id -1). On a
    hop where the detector does not run pass no candidates (CarrySchedule.detects).

    warm_mode "hold" or "velocity" (default None: off): step() also launches comet_track_warm, right
    after comet_track_carry and on the same previous tracks, and leaves its outputs in `warm`
    (ops.WarmOut: the coarse tracker's starting coordinates [n, N, T, 2] in the units warm_div =
    (down_ratio, stride) gives, and per slot how it starts; DESIGN.md "Warm start"). The CarryOut is
    what it is without."""

    _TABLES_MAX = 1024

    def __init__(self, window, stride=1, streams=1, tracks=512, cell=8, border=0, min_score=None, detect_every=1,
                 warm_mode=None, warm_div=(1.0, 1.0)):
        self.sched = CarrySchedule(window, stride, streams, detect_every)
        if warm_mode is not None and warm_mode not in ops.WARM_MODES:
            raise ValueError(f'warm_mode must be "hold" or "velocity", got {warm_mode!r}')
        self.warm_mode, self.warm_div = warm_mode, (float(warm_div[0]), float(warm_div[1]))
        self.warm = None  # ops.WarmOut of the last step (warm_mode given)
        if min_score is None:
            raise ValueError("track carry needs carry_min_score: the lowest pred_score a carried track may have "
                             "(there is no default; DESIGN.md \"Track carry\" records the value the benchmark used)")
        if not 1 <= int(tracks) <= L.CARRY_MAX_TRACKS:
            raise ValueError(f"carry_tracks must lie in [1, {L.CARRY_MAX_TRACKS}], got {tracks}")
        if int(cell) < 1 or int(border) < 0:
            raise ValueError(f"carry_cell must be at least 1 and carry_border at least 0, got {cell} and {border}")
        self.tracks, self.cell, self.border, self.min_score = int(tracks), int(cell), int(border), float(min_score)
        self.device = None
        self._last = {}  # stream -> (pred_tracks [n, T, N, 2], pred_score [n, T, N], row)

    def _ensure(self, dev):
        if self.device == dev:
            return
        S, N, T = self.sched.streams, self.tracks, self.sched.window
        self.device = dev
        self.ids = torch.full((S, N), -1, dtype=torch.int32, device=dev)
        self.age = torch.zeros(S, N, dtype=torch.int32, device=dev)
        self.next_id = torch.zeros(S, dtype=torch.int32, device=dev)
        self._blank = (torch.zeros(T, N, 2, device=dev), torch.zeros(T, N, device=dev))
        self._tables, self._last = {}, {}
        self.sched.reset()

    def _table(self, values, dtype=torch.int32):
        key = (dtype, tuple(values))
        hit = self._tables.get(key)
        if hit is None:
            if len(self._tables) >= self._TABLES_MAX:
                self._tables.clear()
            hit = self._tables[key] = torch.tensor(key[1], dtype=dtype, device=self.device)
        return hit

    def reset(self, stream=None):
        """The next hop of `stream` (default: of every stream) is a first hop again: no track is
        carried into it and its ids start at 0."""
        self.sched.reset(stream)
        if self.device is None:
            return
        if stream is None:
            self._last.clear()
            self.next_id.zero_()
        else:
            self._last.pop(int(stream), None)
            self.next_id[int(stream)] = 0

    def detects(self, stream=0):
        return self.sched.detects(stream)

    def _previous(self, sids):
        """pred_tracks [n, T, N, 2] and pred_score [n, T, N] of the streams' last windows: the batched
        outputs themselves when the same streams ran as one batch, else stacked."""
        refs = [None if self.sched.is_first(s) else self._last.get(s) for s in sids]
        r0 = refs[0]
        if r0 is not None and r0[0].shape[0] == len(sids) and all(
                r is not None and r[0] is r0[0] and r[2] == i for i, r in enumerate(refs)):
            return r0[0], r0[1]
        rows = [self._blank if r is None else (r[0][r[2]], r[1][r[2]]) for r in refs]
        if len(rows) == 1:
            return rows[0][0][None], rows[0][1][None]
        return torch.stack([t for t, _ in rows]), torch.stack([s for _, s in rows])

    def step(self, sids, H, W, cands=None, masks=None):
        """The queries of the next hop of every stream in `sids` (distinct) -> ops.CarryOut [n, N, ...].
        cands: per hop the detections [M, 2] in detector order, or None; masks: per hop [H, W] bool /
        uint8 or None (no mask at all when every entry is None)."""
        sids = [self.sched._id(s) for s in sids]
        n = len(sids)
        if n == 0 or len(set(sids)) != n:
            raise ValueError(f"step takes at least one hop and one hop per stream, got the streams {sids}")
        cands = list(cands) if cands is not None else [None] * n
        masks = list(masks) if masks is not None else [None] * n
        if len(cands) != n or len(masks) != n:
            raise ValueError(f"{n} hops need {n} candidate sets and masks")
        dev = next((t.device for t in cands + masks if t is not None), self.device)
        if dev is None:
            raise ValueError("the first step needs a candidate set or a mask (they give the device)")
        self._ensure(dev)
        N, S = self.tracks, self.sched.streams
        tr, sc = self._previous(sids)
        prev_valid = self._table([0 if self.sched.is_first(s) else 1 for s in sids])
        # candidates, padded to a common M
        cands = [None if c is None else c.to(dev, torch.float32).reshape(-1, 2)[:L.CARRY_MAX_CANDIDATES] for c in cands]
        counts = [0 if c is None else c.shape[0] for c in cands]
        M = max(counts)
        cand = cand_n = None
        if M > 0:
            cand_n = self._table(counts)
            if n == 1:
                cand = cands[0].contiguous()[None]
            else:
                cand = torch.zeros(n, M, 2, device=dev)
                for b, c in enumerate(cands):
                    if c is not None:
                        cand[b, :counts[b]] = c
        mask = None
        if any(m is not None for m in masks):
            ms = [torch.ones(H, W, dtype=torch.uint8, device=dev) if m is None else
                  (m if m.dtype in (torch.bool, torch.uint8) else m != 0).to(dev).contiguous().view(torch.uint8)
                  for m in masks]
            mask = ms[0][None] if n == 1 else torch.stack(ms)
        whole = sids == list(range(S))
        if whole:
            ids, age, next_id = self.ids, self.age, self.next_id
        else:
            idx = self._table(sids, torch.int64)
            ids, age, next_id = self.ids.index_select(0, idx), self.age.index_select(0, idx), self.next_id.index_select(0, idx)
        out = ops.track_carry(tr, sc, ids, age, next_id, prev_valid, self.sched.stride, H, W, self.cell, self.border,
                              self.min_score, cand, cand_n, mask)
        if self.warm_mode is not None:
            self.warm = ops.track_warm(tr, out.src, out.query, prev_valid, self.sched.stride, H, W, self.warm_mode,
                                       *self.warm_div)
        if whole:
            self.ids, self.age = out.ids, out.age  # (new tensors: results handed out earlier stay as they were)
        else:
            # (out of place: a whole-batch step's outputs are the state and are also views of results handed out)
            self.ids = self.ids.index_copy(0, idx, out.ids)
            self.age = self.age.index_copy(0, idx, out.age)
            self.next_id.index_copy_(0, idx, next_id)
        for s in sids:  # (only a launch that went out advances the schedule)
            self.sched.hop(s)
        return out

    def update(self, sids, pred_tracks, pred_score):
        """Keep the windows' outputs for the next step: pred_tracks [n, T, N, 2], pred_score [n, T, N]
        of the hops of `sids`, in their order."""
        if pred_tracks is None or pred_score is None:
            raise RuntimeError("track carry needs the model's pred_tracks and pred_score outputs")
        tr, sc = pred_tracks.float().contiguous(), pred_score.float().contiguous()
        for b, s in enumerate(sids):
            self._last[int(s)] = (tr, sc, b)


def _check_carry(carry, candidate_fn, query_points=None):
    if carry and candidate_fn is None:
        raise ValueError("carry=True needs a candidate_fn (keypoint_candidates): free slots take its detections")
    if carry and query_points is not None:
        raise ValueError("explicit query_points together with carry=True: the carried tracks are the query points")


def _carry_fields(co, b, wo=None):
    return co.ids[b], co.age[b], co.src[b], None if wo is None else wo.warm[b]


def _check_warm(warm, carry, warm_mode, warm_iters):
    if warm_mode not in ops.WARM_MODES:
        raise ValueError(f'warm_mode must be "hold" or "velocity", got {warm_mode!r}')
    if warm_iters is not None and int(warm_iters) < 1:
        raise ValueError(f"warm_iters must be at least 1, got {warm_iters}")
    if warm and not carry:
        raise ValueError("warm=True needs carry=True: the warm start follows the carried tracks")


def _warm_div(model):
    """The two divisions of the model's coarse predictor, (down_ratio, stride), or (1, 1) where it
    divides by nothing (BaseTrackerPredictor.forward)."""
    tp = model.track_predictor
    if tp.coarse_down_ratio > 1:
        return float(tp.coarse_down_ratio), float(tp.coarse_predictor.stride)
    return 1.0, 1.0


def _check_landmarks(landmarks, fuse, carry, intrs, streams, lm_weight, lm_gate_px):
    if lm_weight not in (None, "score"):
        raise ValueError(f'lm_weight must be None or "score", got {lm_weight!r}')
    if not landmarks:
        return
    if not fuse:
        raise ValueError("landmarks=True needs fuse=True: a landmark is triangulated from the final fused poses")
    if not carry:
        raise ValueError("landmarks=True needs carry=True: a landmark is the 3-D point of a carried track")
    if intrs is None or len(intrs) != streams or any(i is None or len(i) != 4 for i in intrs):
        raise ValueError("landmarks=True needs track_intr = (fx, fy, cx, cy) of the pixels the tracks live in, one "
                         "per stream (data.crop_intrinsics)")
    if lm_gate_px is not None and not float(lm_gate_px) >= 0.0:
        raise ValueError(f"lm_gate_px must be None or a distance in pixels >= 0, got {lm_gate_px}")


def _check_pnp(pnp, landmarks, pnp_iters, pnp_huber_px, pnp_min_pts, pnp_weight):
    """-> the keywords of LandmarkMap.pnp, or None with pnp off."""
    if not pnp:
        return None
    if not landmarks:
        raise ValueError("pnp=True needs landmarks=True: a frame is posed against the landmark map")
    if pnp_huber_px is None or not 0.0 < float(pnp_huber_px) < float("inf"):
        raise ValueError(f"pnp=True needs pnp_huber_px, a finite distance in pixels > 0 (nothing here derives one), got "
                         f"{pnp_huber_px}")
    if not 1 <= int(pnp_iters) <= L.PNP_MAX_ITERS:
        raise ValueError(f"pnp_iters must be 1 to {L.PNP_MAX_ITERS}, got {pnp_iters}")
    if int(pnp_min_pts) < 4:
        raise ValueError(f"pnp_min_pts must be at least 4, got {pnp_min_pts}")
    if not 0.0 <= float(pnp_weight) < float("inf"):
        raise ValueError(f"pnp_weight must be finite and >= 0, got {pnp_weight}")
    return dict(iters=int(pnp_iters), huber_px=float(pnp_huber_px), min_pts=int(pnp_min_pts), weight=float(pnp_weight))


def gate_scores(score, state, err_px, s, gate_px):
    """lm_gate_px: pred_score [n, T, N] -> a copy whose row s is -inf where the slot's landmark is valid
    (state == 1) and its reprojection error exceeds gate_px; every other entry is the input's. The track
    then fails comet_track_carry's score test at the next hop."""
    out = score.clone()
    over = (state == 1) & (err_px > gate_px)
    out[:, s] = torch.where(over, torch.full_like(out[:, s], float("-inf")), out[:, s])
    return out


def _landmark_step(lm, sids, tr, sc, fo, ids, src, lm_weight, lm_gate_px, pnp=None, fuser=None, hops=None):
    """The landmark launch of a push: the hops of `sids` with pred_tracks tr [n, T, N, 2], pred_score sc
    [n, T, N], their ops.FuseOut rows fo and the carry's ids / src [n, N] -> (ops.LandmarkOut, the score
    TrackCarry.update takes: sc itself, or its gated copy when lm_gate_px is given, the ops.PnpOut or None, the
    ops.ReidOut of the archive launch that precedes the landmark launch, or None with the archive off).
    pnp (_check_pnp): the PnP launch follows on the same rows, with the landmark launch's weights; with
    pnp["weight"] > 0 it adds its poses to the accumulator of `fuser`, on the rows of `hops` = [(stream, Hop)],
    the hops fo was fused from, in its order."""
    if tr is None or sc is None:
        raise RuntimeError("landmarks need the model's pred_tracks and pred_score outputs")
    n, T = tr.shape[:2]
    w = sc.float().contiguous() if lm_weight == "score" else None
    trf, R, Tx = tr.float().contiguous(), fo.R.view(n, T, 4), fo.T.view(n, T, 3)
    ro = None
    if lm.archive:  # dying rows retire, born slots on an archived landmark get its row back: update() then adds
        ro = lm.reidentify(sids, trf, R, Tx, ids, src)
        src = ro.src_lm
    lo = lm.update(sids, trf, R, Tx, ids, src, w)
    po = None
    if pnp is not None:
        po = lm.pnp(sids, trf, R, Tx, lo, w, fuser if pnp["weight"] > 0.0 else None, hops, iters=pnp["iters"],
                    huber_px=pnp["huber_px"], min_pts=pnp["min_pts"], weight=pnp["weight"])
    if lm_gate_px is not None:
        sc = gate_scores(sc, lo.state, lo.err_px, lm.stride, lm_gate_px)
    return lo, sc, po, ro


def _check_archive(archive, reid_px, reid_min_cos, arch_min_obs, min_obs):
    """-> (capacity, reid_px, reid_min_cos, arch_min_obs) of a LandmarkMap; capacity 0: the archive is off."""
    archive = int(archive)
    if not 0 <= archive <= L.LM_ARCH_MAX:
        raise ValueError(f"archive must be 0 (off) or a capacity of 1 to {L.LM_ARCH_MAX} entries per stream, got {archive}")
    if not archive:
        return 0, None, float(reid_min_cos), int(min_obs if arch_min_obs is None else arch_min_obs)
    if reid_px is None or not 0.0 < float(reid_px) < float("inf"):
        raise ValueError(f"archive > 0 needs reid_px, a finite distance in pixels > 0 (nothing here derives one), got "
                         f"{reid_px}")
    if not -1.0 <= float(reid_min_cos) <= 1.0:
        raise ValueError(f"reid_min_cos must lie in [-1, 1], got {reid_min_cos}")
    arch_min_obs = int(min_obs if arch_min_obs is None else arch_min_obs)
    if arch_min_obs < 2:
        raise ValueError(f"arch_min_obs must be at least 2, got {arch_min_obs}")
    return archive, float(reid_px), float(reid_min_cos), arch_min_obs


class LandmarkMap:
    """One 3-D point per carried track (DESIGN.md "Landmarks").

        lm = LandmarkMap(window=T, stride=1, streams=1, tracks=N, intrs=[(fx, fy, cx, cy)])
        out = lm.update([0], pred_tracks [1, T, N, 2], fused_R [1, T, 4], fused_T [1, T, 3], ids [1, N], src [1, N])
        ids, X, n_obs = lm.snapshot(0)

    Owns the normal equations acc [streams * N, 12] float64 and acc_id [streams * N] int32 on the device
    (row of slot j of stream s: s * N + j). update() is one comet_landmark_update launch for all the hops
    given (at most one per stream; ids / src as ops.track_carry returned them for these hops, R / T as
    ops.pose_fuse): the first `stride` positions of every window, whose fused pose is final, are added to
    the rows of the slots that carried their track, born slots start over, pads are cleared, and every
    slot's point, observation count, reprojection error on position `stride` and state come back
    (ops.LandmarkOut [n, N, ...]). intrs: per stream (fx, fy, cx, cy) of the pixels the tracks live in
    (data.crop_intrinsics for a cropped, resized frame). The stream-index and intrinsics tables are cached
    on the device by their values, so a steady-state call uploads nothing.

    min_pivot = 1e-8 is a guard against dividing by a rounding residue, not a tuned value: a pivot of the
    LDL^T at or below min_pivot * max(diag M) marks the slot ill-conditioned (no parallax yet).
    inverse_rotation = 0: x_cam = R(q) X + T, the way the dataset labels are produced and consumed
    (DESIGN.md "Landmarks"); 1 uses the transpose. With archive = 0 a landmark lives as long as its slot
    carries its track and nothing is kept after the track dies. With archive = C > 0 (DESIGN.md "Landmark
    archive") the row of a dying track is kept in a ring of C entries per stream, and reidentify(), one
    comet_landmark_reid launch before update(), hands it back with its identity to a track born within reid_px
    pixels of its projection (required: nothing here derives one) while it still faces the camera
    (reid_min_cos = 0.5 is a stated value, not a tuned one); arch_min_obs (None: min_obs) frames make a row
    worth keeping."""

    _TABLES_MAX = 1024

    def __init__(self, window, stride=1, streams=1, tracks=512, intrs=None, min_obs=3, min_pivot=1e-8,
                 inverse_rotation=0, archive=0, reid_px=None, reid_min_cos=0.5, arch_min_obs=None):
        if stride < 1 or stride >= window:
            raise ValueError(f"landmarks need 1 <= stride < window (stride {stride}, window {window})")
        if streams < 1 or not 1 <= int(tracks) <= L.CARRY_MAX_TRACKS:
            raise ValueError(f"at least 1 stream and 1 to {L.CARRY_MAX_TRACKS} tracks, got {streams} and {tracks}")
        if intrs is None or len(intrs) != streams:
            raise ValueError("LandmarkMap needs intrs: one (fx, fy, cx, cy) per stream")
        if int(min_obs) < 2 or not 0.0 <= float(min_pivot) < 1.0:
            raise ValueError(f"min_obs must be at least 2 and min_pivot in [0, 1), got {min_obs} and {min_pivot}")
        self.window, self.stride, self.streams, self.tracks = int(window), int(stride), int(streams), int(tracks)
        self.intrs = [tuple(float(v) for v in i) for i in intrs]
        self.min_obs, self.min_pivot, self.inverse_rotation = int(min_obs), float(min_pivot), int(bool(inverse_rotation))
        self.archive, self.reid_px, self.reid_min_cos, self.arch_min_obs = _check_archive(
            archive, reid_px, reid_min_cos, arch_min_obs, self.min_obs)
        self.device = None
        self._last = {}  # stream -> (LandmarkOut, row, ids [n, N])

    def _id(self, stream):
        s = int(stream)
        if not 0 <= s < self.streams:
            raise ValueError(f"unknown stream {s}: the map has streams 0 .. {self.streams - 1}")
        return s

    def _ensure(self, dev):
        if self.device == dev:
            return
        self.device = dev
        self.acc = torch.zeros(self.streams * self.tracks, L.LM_ROW, dtype=torch.float64, device=dev)
        self.acc_id = torch.full((self.streams * self.tracks,), -1, dtype=torch.int32, device=dev)
        self._tables, self._last = {}, {}
        if self.archive:
            i32 = dict(dtype=torch.int32, device=dev)
            self.arch = torch.zeros(self.streams * self.archive, L.LM_ARCH_ROW, dtype=torch.float64, device=dev)
            self.arch_id = torch.full((self.streams * self.archive,), -1, **i32)
            self.arch_cursor = torch.zeros(self.streams, **i32)
            self.alias = torch.full((self.streams * self.tracks,), -1, **i32)
            self._ws = torch.empty(self.streams, self.tracks, L.LM_ROW, dtype=torch.float64, device=dev)
            self._pending = None  # (sids, lm_id [n, N]) of a reidentify() whose update() has not come yet

    def _table(self, sids):
        hit = self._tables.get(sids)
        if hit is None:
            if len(self._tables) >= self._TABLES_MAX:
                self._tables.clear()
            flat = [v for s in sids for v in self.intrs[s]]
            hit = self._tables[sids] = (torch.tensor(sids, dtype=torch.int32, device=self.device),
                                        (ctypes.c_int32 * len(sids))(*sids),
                                        torch.tensor(flat, dtype=torch.float64, device=self.device).view(len(sids), 4),
                                        (ctypes.c_double * len(flat))(*flat))
        return hit

    def set_intr(self, stream, intr):
        """The intrinsics (fx, fy, cx, cy) of the stream's track pixels from now on (a new sequence with
        its own crop; reset(stream) goes with it: the rows already added were built with the old ones)."""
        s = self._id(stream)
        if intr is None or len(intr) != 4:
            raise ValueError("set_intr takes (fx, fy, cx, cy)")
        intr = tuple(float(v) for v in intr)
        if intr != self.intrs[s]:
            self.intrs[s] = intr
            self._tables = {}

    def reset(self, stream=None):
        """The rows of `stream` (default: of every stream) hold no landmark any more. A stream's first
        hop has only births and pads, which overwrite their rows, so nothing else is cleared. With the
        archive on, the stream's entries, cursor and aliases are freed too."""
        if stream is not None:
            self._id(stream)
        if self.device is None:
            return
        if stream is None:
            self._last.clear()
            self.acc_id.fill_(-1)
            if self.archive:
                self._pending = None
                self.arch_id.fill_(-1)
                self.arch_cursor.zero_()
                self.alias.fill_(-1)
        else:
            s = int(stream)
            self._last.pop(s, None)
            self.acc_id[s * self.tracks:(s + 1) * self.tracks] = -1
            if self.archive:
                self.arch_id[s * self.archive:(s + 1) * self.archive] = -1
                self.arch_cursor[s:s + 1] = 0
                self.alias[s * self.tracks:(s + 1) * self.tracks] = -1

    def reidentify(self, sids, tracks, R, T, ids, src):
        """The archive step of the hops of the streams `sids` (distinct), before update() on the same hops
        and arguments: the rows update() is about to overwrite or clear are retired to the archive, and the
        born slots are matched against it -> ops.ReidOut; hand its src_lm to update() in place of src."""
        if not self.archive:
            raise RuntimeError("reidentify needs a LandmarkMap with archive > 0")
        sids = tuple(self._id(s) for s in sids)
        if len(sids) == 0 or len(set(sids)) != len(sids):
            raise ValueError(f"reidentify takes at least one hop and one hop per stream, got the streams {list(sids)}")
        self._ensure(tracks.device)
        idx, idx_host, intr, intr_host = self._table(sids)
        out = ops.landmark_reid(tracks, R, T, ids, src, idx, idx_host, intr, intr_host, self.acc, self.acc_id,
                                self.alias, self.arch, self.arch_id, self.arch_cursor, self._ws, self.reid_px,
                                self.reid_min_cos, self.arch_min_obs, self.inverse_rotation, self.min_pivot)
        self._pending = (sids, out.lm_id)
        return out

    def archive_snapshot(self, stream=0):
        """(ids [A] int32, X [A, 3] float64, n_obs [A] int32) of the stream's archive entries in use, in
        entry order (empty with the archive off, before the first hop and after a reset)."""
        s = self._id(stream)
        if not self.archive or self.device is None:
            dev = self.device if self.device is not None else "cpu"
            return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, 3, dtype=torch.float64, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev))
        sl = slice(s * self.archive, (s + 1) * self.archive)
        on = self.arch_id[sl] >= 0
        a = self.arch[sl][on]
        return self.arch_id[sl][on], a[:, 12:15].contiguous(), a[:, 10].to(torch.int32)

    def update(self, sids, tracks, R, T, ids, src, weights=None):
        """The hops of the streams `sids` (distinct), in their order: tracks [n, T, N, 2] f32, R [n, T, 4]
        f32, T [n, T, 3] f64, ids / src [n, N] int32, weights [n, T, N] f32 or None -> ops.LandmarkOut."""
        sids = tuple(self._id(s) for s in sids)
        if len(sids) == 0 or len(set(sids)) != len(sids):
            raise ValueError(f"update takes at least one hop and one hop per stream, got the streams {list(sids)}")
        self._ensure(tracks.device)
        idx, idx_host, intr, intr_host = self._table(sids)
        out = ops.landmark_update(tracks, R, T, ids, src, idx, idx_host, intr, intr_host, self.acc, self.acc_id,
                                  self.stride, weights, self.inverse_rotation, self.min_obs, self.min_pivot)
        if self.archive:  # the identities of these rows: the lm_id of the reidentify() of the same hops, if there was one
            pending, self._pending = self._pending, None
            if pending is not None and pending[0] == sids:
                ids = pending[1]
        for b, s in enumerate(sids):
            self._last[s] = (out, b, ids)
        return out

    def pnp(self, sids, tracks, R, T, lo, weights=None, fuser=None, hops=None, iters=4, huber_px=None, min_pts=6,
            weight=0.0):
        """Every frame of the hops of `sids` posed against the landmarks of the same push (DESIGN.md "PnP
        refinement"): tracks [n, T, N, 2] f32, R [n, T, 4] f32 / T [n, T, 3] f64 the fused poses, lo the
        ops.LandmarkOut update() returned for these hops, weights [n, T, N] f32 or None -> ops.PnpOut, one
        comet_landmark_pnp launch. `iters` Gauss-Newton steps with the Huber threshold huber_px (required;
        nothing here derives one); fewer than min_pts usable landmarks leave a frame's pose as it came.
        With a PoseFuser and weight > 0 the solved poses of the positions [stride, T) are added to the
        fuser's accumulator as one hypothesis of that weight each; `hops` = [(stream, Hop)], the hops of
        that push's fuser.fuse() call in its order, then name the rows (the fuser's own slot table)."""
        sids = tuple(self._id(s) for s in sids)
        if len(sids) == 0 or len(set(sids)) != len(sids):
            raise ValueError(f"pnp takes at least one hop and one hop per stream, got the streams {list(sids)}")
        if huber_px is None:
            raise ValueError("pnp needs huber_px, the Huber threshold in pixels")
        if lo.X.shape[0] != len(sids):
            raise ValueError(f"{len(sids)} hops need the LandmarkOut of the same {len(sids)} hops, got {lo.X.shape[0]} rows")
        self._ensure(tracks.device)
        _, _, intr, intr_host = self._table(sids)
        kw = {}
        if fuser is not None and weight > 0.0:
            if hops is None or tuple(int(s) for s, _ in hops) != sids:
                raise ValueError(f"the feedback needs hops, the (stream, Hop) pairs of the streams {list(sids)} in this "
                                 f"order, got {None if hops is None else [int(s) for s, _ in hops]}")
            slots, slots_host = fuser._table(fuser.ring.table(list(hops)))
            kw = dict(fuse_acc=fuser.acc, slots=slots, slots_host=slots_host, inject_w=weight, fuse_intr=fuser.intr)
        return ops.landmark_pnp(tracks, lo.X, lo.state, R, T, intr, intr_host, self.stride, huber_px, weights,
                                self.inverse_rotation, iters, min_pts, self.min_pivot, **kw)

    def snapshot(self, stream=0):
        """(ids [L] int32, X [L, 3] float64, n_obs [L] int32) of the stream's valid live landmarks, as its
        last hop left them (empty before the first hop and after a reset). With the archive on the ids are
        the landmark identities (ReidOut.lm_id) of the reidentify() that preceded that update() on the same
        hops; an update() that no reidentify() of the same hops preceded reports the carry's ids."""
        last = self._last.get(self._id(stream))
        if last is None:
            dev = self.device if self.device is not None else "cpu"
            return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, 3, dtype=torch.float64, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev))
        out, b, ids = last
        on = out.state[b] == 1
        return ids[b][on], out.X[b][on], out.n_obs[b][on]


def _check_motion(motion, fuse, motion_len, motion_min_frames, motion_iters, motion_horizon, motion_max_angle,
                  motion_inverse_rotation):
    """-> the keywords of MotionTracker, or None with motion off."""
    if not motion:
        return None
    if not fuse:
        raise ValueError("motion=True needs fuse=True: the motion is fitted to the final fused poses")
    if not 2 <= int(motion_len) <= L.MOTION_MAX_CAP:
        raise ValueError(f"motion_len must be 2 to {L.MOTION_MAX_CAP} frames, got {motion_len}")
    if not 2 <= int(motion_min_frames) <= int(motion_len):
        raise ValueError(f"motion_min_frames must be 2 to motion_len = {motion_len}, got {motion_min_frames}")
    if not 1 <= int(motion_iters) <= L.MOTION_MAX_ITERS:
        raise ValueError(f"motion_iters must be 1 to {L.MOTION_MAX_ITERS}, got {motion_iters}")
    if not 0 <= int(motion_horizon) <= L.MOTION_MAX_HORIZON:
        raise ValueError(f"motion_horizon must be 0 to {L.MOTION_MAX_HORIZON}, got {motion_horizon}")
    if not 0.0 < float(motion_max_angle) < math.pi:
        raise ValueError(f"motion_max_angle must lie in (0, pi) radians, got {motion_max_angle}")
    if motion_inverse_rotation not in (0, 1, False, True):
        raise ValueError(f"motion_inverse_rotation must be 0 or 1, got {motion_inverse_rotation}")
    return dict(fit_len=int(motion_len), min_frames=int(motion_min_frames), iters=int(motion_iters),
                horizon=int(motion_horizon), max_angle=float(motion_max_angle),
                inverse_rotation=int(motion_inverse_rotation))


class MotionTracker:
    """The target's angular and linear velocity from the final fused poses (DESIGN.md "Motion estimate").

        mt = MotionTracker(window=T, stride=1, streams=1)
        fo = fuser.fuse(enc, [(0, hop)])
        mo = mt.update([(0, hop)], fo)            # ops.MotionOut: omega, vel, q0, t0, predictions, innovations

    Owns the history hist [streams, fit_len, 8] float64 and hist_n [streams] int32 on the device. update() is
    one comet_motion_fit launch for all the hops given (at most one per stream): `hops` = [(stream, Hop)], the
    pairs of that push's PoseFuser.fuse() call in its order, and `fused` its ops.FuseOut (or any object with
    R [n, T, 4] f32 and T [n, T, 3] f64). The first `stride` positions of every window, whose fused pose is
    final, are appended to the stream's history, and a constant angular velocity (a weighted line through the
    rotation vectors about a reference the fit re-centres `iters` times) and a constant linear velocity are
    fitted to its newest fit_len frames. A stream's hops must follow one another: a hop whose first frame is
    not the stride-th after the previous hop's raises, since the history's time axis is the frame count.
    reset(stream) forgets that stream's history (its next hop starts a new one).

    fit_len = 16, min_frames = 3, iters = 2, horizon = 1 and max_angle = 2.0 rad are stated values, not tuned
    ones: nothing here has been measured on real imagery. max_angle bounds the rotation between a frame and the
    reference inside the fitted span, where a rotation vector stops being a usable coordinate; a faster tumble
    reports state 3 and no rate. inverse_rotation: as LandmarkMap's. The estimate is reported and fed back
    into nothing."""

    _TABLES_MAX = 1024

    def __init__(self, window, stride=1, streams=1, fit_len=16, min_frames=3, iters=2, horizon=1, max_angle=2.0,
                 inverse_rotation=0):
        if stride < 1 or stride >= window:
            raise ValueError(f"the motion estimate needs 1 <= stride < window (stride {stride}, window {window})")
        if streams < 1:
            raise ValueError(f"at least 1 stream, got {streams}")
        self._kw = _check_motion(True, True, fit_len, min_frames, iters, horizon, max_angle, inverse_rotation)
        self.window, self.stride, self.streams = int(window), int(stride), int(streams)
        self.device = None
        self._first = [True] * self.streams
        self._next = [None] * self.streams  # the frame index a stream's next hop must start at
        self._tables = {}

    def _id(self, stream):
        s = int(stream)
        if not 0 <= s < self.streams:
            raise ValueError(f"unknown stream {s}: the tracker has streams 0 .. {self.streams - 1}")
        return s

    def _ensure(self, dev):
        if self.device == dev:
            return
        self.device = dev
        self.hist = torch.zeros(self.streams, self._kw["fit_len"], L.MOTION_ROW, dtype=torch.float64, device=dev)
        self.hist_n = torch.zeros(self.streams, dtype=torch.int32, device=dev)
        self._first = [True] * self.streams
        self._next = [None] * self.streams
        self._tables = {}

    def _table(self, values):
        hit = self._tables.get(values)
        if hit is None:
            if len(self._tables) >= self._TABLES_MAX:
                self._tables.clear()
            hit = self._tables[values] = (torch.tensor(values, dtype=torch.int32, device=self.device),
                                          (ctypes.c_int32 * len(values))(*values))
        return hit

    def reset(self, stream=None):
        """The history of `stream` (default: of every stream) is forgotten: its next hop starts a new one
        (first = 1 in its launch, which sets hist_n = 0 before it appends; no row needs clearing)."""
        for s in (range(self.streams) if stream is None else [self._id(stream)]):
            self._first[s], self._next[s] = True, None

    def update(self, hops, fused, weights=None):
        """hops = [(stream, Hop)] of distinct streams, fused.R [n, T, 4] f32 / fused.T [n, T, 3] f64 in their
        order, weights [n, T] f32 or None -> ops.MotionOut."""
        sids = tuple(self._id(s) for s, _ in hops)
        n, T = len(sids), self.window
        if n == 0 or len(set(sids)) != n:
            raise ValueError(f"update takes at least one hop and one hop per stream, got the streams {list(sids)}")
        for s, (_, hop) in zip(sids, hops):
            if not self._first[s] and hop.frame_index != self._next[s]:
                raise ValueError(f"stream {s}: the hop at frame {hop.frame_index} does not follow the last one (frame "
                                 f"{self._next[s]} expected): every frame is committed exactly once; reset({s}) "
                                 "starts a new history")
        R, Tx = fused.R, fused.T
        if R.numel() != n * T * 4:
            raise ValueError(f"{n} hops of window {T} need fused poses [{n}, {T}, ...], got R {tuple(R.shape)}")
        self._ensure(R.device)
        idx, idx_host = self._table(sids)
        first, _ = self._table(tuple(int(self._first[s]) for s in sids))
        out = ops.motion_fit(R.view(n, T, 4), Tx.view(n, T, 3), first, idx, idx_host, self.hist, self.hist_n,
                             self.stride, weights, **self._kw)
        for s, (_, hop) in zip(sids, hops):  # (only a launch that went out advances the bookkeeping)
            self._first[s], self._next[s] = False, hop.frame_index + self.stride
        return out


def _per_frame(cache):
    """FrameCache of one k-frame sequence -> its tensors as [k, ...] (None where unused)."""
    return [None if cache.fmaps is None else cache.fmaps[0], cache.refine_frames[0], cache.tokens]


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
    every hop adds a full single-window error to the reference, and without fusion nothing reduces it.

    fuse=True (needs an anchor, so stride < window) makes use of the overlap: with stride < window a
    frame lies in up to ceil(window / stride) windows, and one comet_pose_fuse launch per hop
    (PoseFuser) keeps a running weighted mean of all its hypotheses. Each window is then referenced
    to the fused pose of its first frame, not to one earlier estimate, and every result carries
    fused_R / fused_T (one pose per frame so far), fused_count, rot_spread (radians) and trans_spread
    (of u, v, z); the first `final` = stride positions will not change again. R / T are still this
    window's own hypothesis, against the fused reference. fuse_weight="score" weights position i by
    the mean of pred_score[i] over the tracks (at least 1e-6); None weights every hypothesis 1. Fusion
    reduces the drift (DESIGN.md "Pose fusion": to about 0.2 - 0.35 of chaining at stride <= window / 4)
    and does not remove it: there is no loop closure and no global optimisation, and the gain
    vanishes as stride approaches window / 2, where the chained frame has a single hypothesis.
    _decode_chained is not called when fuse is on; with fuse=False nothing changes.

    carry=True (needs stride < window, a candidate_fn and carry_min_score; query_points / query_fn are
    then not used) keeps tracks alive from window to window (TrackCarry, DESIGN.md "Track carry"): every
    window has carry_tracks query slots; a track whose refined position on the frame that becomes the
    next window's first frame is inside the frame (carry_border), inside mask_fn(frame) -> [H, W] bool
    when given, has pred_score >= carry_min_score and holds its carry_cell x carry_cell pixel cell
    keeps its slot and id, and that position is the next query. Free slots take candidate_fn(frame)
    -> [M, 2] (keypoint_candidates) in detector order on the hops where the detector runs (every
    detect_every-th hop of the stream, always the first), the rest is padded. Results then carry
    track_ids, track_age and track_src. carry_min_score has no default: the model was trained with
    detector keypoints on frame 0, and what carried queries do to pose accuracy is unmeasured beyond
    DESIGN.md "Track carry" (whose benchmark used 0.0). With carry=False nothing changes.

    warm=True (needs carry=True) also starts the coarse tracker of every hop but the stream's first where
    the tracks already are (comet_track_warm, DESIGN.md "Warm start"): a carried slot starts on the previous
    window's refined track shifted by the stride; the `stride` frames the previous window has not seen
    repeat its last position (warm_mode="hold") or continue its last step, clamped to the frame
    ("velocity"); born slots, pads of born slots and slots whose previous track is not finite start on
    their query point as always. warm_iters (None: cfg.track_trainit) is the number of coarse iterations
    of those hops; the first hop after construction or reset is cold and runs cfg.track_trainit. Results
    then carry track_warm. What a warm start and fewer iterations do to pose accuracy on real sequences is
    unmeasured, so the option is off by default. With warm=False nothing changes.

    landmarks=True (needs fuse=True, carry=True and track_intr = (fx, fy, cx, cy) of the pixels the tracks
    live in: data.crop_intrinsics for a cropped, resized frame) triangulates every carried track into a 3-D
    point on the body (LandmarkMap, DESIGN.md "Landmarks"): one comet_landmark_update launch per hop, after
    the fuse launch, adds the window's first `stride` frames, whose fused pose is final, to the slot's normal
    equations. Results then carry landmarks [N, 3] float64, landmark_obs, landmark_err (pixels, on the frame
    that becomes the next window's first) and landmark_state; stream.landmark_map.snapshot() gives the valid
    ones with their ids. lm_min_obs: frames a landmark needs; lm_min_pivot = 1e-8 is a guard against
    dividing by a rounding residue, not a tuned value; lm_weight="score" weights an observation by its
    pred_score; lm_inverse_rotation: LandmarkMap. lm_gate_px (default None: no gate; nothing here derives
    a value) makes the landmark a test of the track: the score the carry sees on the next window's first
    frame is -inf where the landmark is valid and its reprojection error exceeds lm_gate_px, so the track
    dies at the next hop by the carry's own score test. Landmark accuracy on real imagery and the effect
    of the gate on pose accuracy are unmeasured. With landmarks=False nothing changes.

    lm_archive = C > 0 (needs landmarks=True and reid_px, a gate in pixels that nothing here derives) keeps the
    landmark of a track that dies in a ring of C entries and gives it back, with its identity and its
    observations, to a track born within reid_px of its projection while it still faces the camera (DESIGN.md
    "Landmark archive"): one comet_landmark_reid launch per hop, before the landmark launch. reid_min_cos =
    0.5 is a stated value, not a tuned one; lm_arch_min_obs (None: lm_min_obs) frames make a landmark worth
    keeping. Results then carry landmark_ids (the landmark's identity, stable across re-identifications),
    reid_state and reid_dist; stream.landmark_map.archive_snapshot() gives the archived landmarks. The accuracy
    of re-identification on real imagery, every default, and whether archived landmarks improve pose drift are
    unmeasured. With lm_archive=0 nothing changes.

    pnp=True (needs landmarks=True and pnp_huber_px, a Huber threshold in pixels that nothing here derives)
    poses every frame of the window against the landmark map (LandmarkMap.pnp, DESIGN.md "PnP refinement"):
    one comet_landmark_pnp launch per hop, after the landmark launch, runs pnp_iters Gauss-Newton steps from
    the fused pose (4: a stated number of steps, not a tuned value). Results then carry pnp_R [T, 4], pnp_T
    [T, 3] float64, pnp_inliers, pnp_rms_px and pnp_state (1 solved; else the pose is the fused one);
    fewer than pnp_min_pts usable landmarks leave a frame unsolved. pnp_weight = 0 reports only;
    pnp_weight > 0 adds the solved poses of the positions [stride, T) to the fusion accumulator as one
    hypothesis of that weight each, which the next hop's fused poses then include. On a synthetic
    trajectory that feedback lowers the (u, v, z) drift and raises the rotation drift; accuracy on real
    imagery is unmeasured and no value of these keywords is recommended. With pnp=False nothing changes.

    motion=True (needs fuse=True) estimates how the target moves (MotionTracker, DESIGN.md "Motion estimate"):
    one comet_motion_fit launch per hop, after the fuse launch, appends the window's first `stride` frames,
    whose fused pose is final, to a history of motion_len frames and fits a constant angular velocity and a
    constant linear velocity to it. Results then carry motion_omega [3] (rad / frame, camera frame: R(tau) =
    Exp(omega tau) R0), motion_vel [3] (per frame), motion_q0 / motion_t0 (the fitted pose at the newest final
    frame), motion_rot_rms, motion_trans_rms, motion_frames, motion_state (1 fitted; else no rate: omega = vel
    = 0 and the predictions repeat the newest final pose), motion_pred_R / motion_pred_T (the poses 1 ..
    window - stride + motion_horizon frames past the newest final frame; the first window - stride of them are
    the positions [stride, window) of this window) and motion_innov_rot / motion_innov_trans (fused against
    predicted on those positions). motion_len = 16, motion_min_frames = 3, motion_iters = 2, motion_horizon = 1
    and motion_max_angle = 2.0 rad are stated values, not tuned ones; motion_inverse_rotation: as
    lm_inverse_rotation. The estimate is reported only and feeds nothing back; its accuracy on real imagery
    is unmeasured. With motion=False nothing changes.

    One stream (batch 1): a PoseStream is a StreamPool of one stream. push() runs the per-frame stages on
    its k frames as one batch and hands them, frame by frame, to the pool's hop pipeline
    (StreamPool._advance), which is the only implementation of everything above. The model is used as is
    (its eval / train mode included)."""

    def __init__(self, model, window, stride=1, capacity=None, query_fn=None, anchor=None, precision=None,
                 fuse=False, fuse_weight=None, carry=False, carry_tracks=512, carry_cell=8, carry_border=0,
                 carry_min_score=None, detect_every=1, candidate_fn=None, mask_fn=None, warm=False, warm_mode="hold",
                 warm_iters=None, landmarks=False, track_intr=None, lm_min_obs=3, lm_min_pivot=1e-8, lm_weight=None,
                 lm_gate_px=None, lm_inverse_rotation=0, pnp=False, pnp_iters=4, pnp_huber_px=None, pnp_min_pts=6,
                 pnp_weight=0.0, motion=False, motion_len=16, motion_min_frames=3, motion_iters=2, motion_horizon=1,
                 motion_max_angle=2.0, motion_inverse_rotation=0, lm_archive=0, reid_px=None, reid_min_cos=0.5,
                 lm_arch_min_obs=None):
        self._pool = StreamPool(
            model, 1, window, stride, capacity, query_fn, None if anchor is None else [anchor], precision, fuse=fuse,
            fuse_weight=fuse_weight, carry=carry, carry_tracks=carry_tracks, carry_cell=carry_cell,
            carry_border=carry_border, carry_min_score=carry_min_score, detect_every=detect_every,
            candidate_fn=candidate_fn, mask_fn=mask_fn, warm=warm, warm_mode=warm_mode, warm_iters=warm_iters,
            landmarks=landmarks, track_intrs=None if track_intr is None else [track_intr], lm_min_obs=lm_min_obs,
            lm_min_pivot=lm_min_pivot, lm_weight=lm_weight, lm_gate_px=lm_gate_px,
            lm_inverse_rotation=lm_inverse_rotation, pnp=pnp, pnp_iters=pnp_iters, pnp_huber_px=pnp_huber_px,
            pnp_min_pts=pnp_min_pts, pnp_weight=pnp_weight, motion=motion, motion_len=motion_len,
            motion_min_frames=motion_min_frames, motion_iters=motion_iters, motion_horizon=motion_horizon,
            motion_max_angle=motion_max_angle, motion_inverse_rotation=motion_inverse_rotation, lm_archive=lm_archive,
            reid_px=reid_px, reid_min_cos=reid_min_cos, lm_arch_min_obs=lm_arch_min_obs)
        self.sched = self._pool.sched.scheds[0]  # the stream's own RingSchedule
        self.anchor = None if anchor is None else self._pool.anchors[0]
        self._hw = None  # the frame size push() holds the stream to

    # what a caller reads off a stream is the pool's (landmark_map: the LandmarkMap, motion_tracker: the
    # MotionTracker, or None)
    _POOLED = frozenset(("model", "query_fn", "precision", "fuse", "fuse_weight", "carry", "candidate_fn", "mask_fn",
                         "warm", "warm_mode", "warm_iters", "landmarks", "lm_weight", "lm_gate_px", "lm_archive", "pnp", "landmark_map",
                         "_pnp", "_carry", "_lm", "_fuser", "_rings", "_wins", "motion", "motion_tracker", "_motion"))

    def __getattr__(self, name):
        if name in self._POOLED:
            return getattr(self._pool, name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def reset(self):
        """Forget every frame (the next push starts a new stream at frame 0, at the anchor; a new frame
        size may follow)."""
        self._hw = None
        self._pool.reset()

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
        pool = self._pool
        _check_carry(pool.carry, pool.candidate_fn, query_points)
        if query_points is None and pool.query_fn is None and not pool.carry:
            raise ValueError("no query source: pass query_points to push() or query_fn to PoseStream")
        results = []
        with F.precision(pool.precision):
            per = _per_frame(pool.model.frame_stages(frames.float()))  # one batched call for the k frames
            self._hw = hw
            for i in range(frames.shape[0]):  # (frame i's hop is complete before frame i + 1 is stored)
                rows = [None if t is None else t[i:i + 1] for t in per]
                results += [r for _, r in pool._advance(rows, [0], query_points)]
        return results


class PoolSchedule:
    """The host-only arithmetic of a StreamPool (no tensors): `streams` RingSchedule objects over
    pooled rings of streams * capacity slots. Frame f of stream s lives in slot
    s * capacity + f % capacity, so slots of different streams never coincide; a stream's hops fall
    due exactly where its own RingSchedule says."""

    def __init__(self, streams, window, stride=1, capacity=None):
        if streams < 1:
            raise ValueError(f"a pool needs at least 1 stream, got {streams}")
        self.streams = int(streams)
        self.scheds = [RingSchedule(window, stride, capacity) for _ in range(self.streams)]
        s0 = self.scheds[0]
        self.window, self.stride, self.capacity = s0.window, s0.stride, s0.capacity

    def reset(self, stream=None):
        for s in (range(self.streams) if stream is None else self.ids(1, [stream])):
            self.scheds[s].reset()

    def ids(self, k, streams=None):
        """The stream ids of a push of k frames: `streams` (k distinct known ids), default
        range(streams), which needs k == streams."""
        if streams is None:
            if k != self.streams:
                raise ValueError(f"push of {k} frames into a pool of {self.streams} streams: pass `streams`, the id "
                                 "of each frame's stream")
            return list(range(self.streams))
        ids = [int(s) for s in streams]
        if len(ids) != k:
            raise ValueError(f"{k} frames for {len(ids)} stream ids")
        for s in ids:
            if not 0 <= s < self.streams:
                raise ValueError(f"unknown stream {s}: the pool has streams 0 .. {self.streams - 1}")
        if len(set(ids)) != len(ids):
            raise ValueError(f"a stream takes one frame per push, got the ids {ids}")
        return ids

    def slot(self, stream, frame_index):
        return stream * self.capacity + self.scheds[stream].slot(frame_index)

    def window_slots(self, stream, head):
        """RingSchedule.window_slots(head) of the stream, shifted by stream * capacity."""
        return [stream * self.capacity + s for s in self.scheds[stream].window_slots(head)]

    def due(self, ids):
        """The streams among `ids` whose next frame completes a hop (nothing is advanced)."""
        out = []
        for s in ids:
            first = self.scheds[s].frames_seen + 1 - self.window
            if first >= 0 and first % self.stride == 0:
                out.append(s)
        return sorted(out)

    def push(self, ids):
        """Account for one new frame of every stream in `ids` -> (the absolute slot of each frame, in
        the order of `ids`; [(stream, Hop)] of the hops this completes, ordered by stream id)."""
        slots, hops = [], []
        for s in ids:
            slot, hop = self.scheds[s].push()
            slots.append(s * self.capacity + slot)
            if hop is not None:
                hops.append((s, hop))
        return slots, sorted(hops)

    def table(self, hops):
        """The concatenated slot table of the windows of `hops` [(stream, Hop)]: len(hops) * window
        absolute slots, a valid comet_ring_gather table over the pooled ring."""
        return [s for stream, hop in hops for s in self.window_slots(stream, hop.head)]

    @staticmethod
    def group(counts):
        """Due hops with the query counts `counts` (one per hop, hops ordered by stream id) ->
        [(N, [positions of the hops with N query points, ascending])], in the order each N first
        appears: every group is one batched call."""
        groups = {}
        for i, n in enumerate(counts):
            groups.setdefault(int(n), []).append(i)
        return list(groups.items())


class StreamPool:
    """Several streams that share one model and batch their work: the hop pipeline of this module
    (PoseStream is a pool of one stream; its docstring describes every keyword).

        pool = StreamPool(model, streams=S, window=16, query_fn=keypoint_query(sp))
        for frames in cameras:                       # [S, 3, H, W], one new frame per stream
            for sid, r in pool.push(frames):         # r: StreamResult, as PoseStream returns
                use(sid, r.frame_index, r.pred_pose_enc)

    One push takes at most one frame per stream (`streams`: the k distinct ids of the k frames;
    default all S in order). The k frames go through the per-frame stages as one batch
    (model.frame_stages), one comet_ring_scatter launch stores their outputs in pooled rings
    [S * capacity, ...] (PoolSchedule: stream s, frame f -> slot s * capacity + f % capacity), and
    the n hops that fall due in the push are gathered by one comet_ring_gather launch and run as one
    model.forward_all with B = n. Streams need not be in phase: one can be absent from a push, start
    later, or be restarted with reset(stream).

    Query points of a due hop: `query_points` of the push ([N, 2] shared by all streams, or a dict
    by stream id), else query_fn(first frame of the window). Hops whose query counts differ
    (filter_and_pad returns between min_required and track_num points) are grouped by N, one
    batched call per group. anchors: a dict or list giving every stream the 5-tuple PoseStream
    takes; each stream chains its absolute poses on its own (_decode_chained, per stream). fuse /
    fuse_weight: as PoseStream's; all the hops due in a push, of every query-count group, are fused
    by one comet_pose_fuse launch. With
    fuse=True every anchor must carry the same ratio and dataset (one launch takes one ratio and one
    set of intrinsics). carry / carry_* / detect_every / candidate_fn / mask_fn: as PoseStream's; every
    carried hop has carry_tracks queries, so the hops due in a push are one group, and one
    comet_track_carry launch serves them all; reset(stream) restarts that stream's ids and ages.
    warm / warm_mode / warm_iters: as PoseStream's; one comet_track_warm launch serves all the hops
    due. A stream's first hop runs cfg.track_trainit coarse iterations and a later one warm_iters, so
    when both fall in one push and the two counts differ they run as two batched calls (first hops,
    then later hops); otherwise the hops due stay one group. The result order is unchanged.
    landmarks / track_intrs (one (fx, fy, cx, cy) per stream) / lm_*: as PoseStream's; one
    comet_landmark_update launch, after the fuse launch, serves all the hops due in a push (the rows of two
    warm-start calls are stacked first); reset(stream) forgets that stream's landmarks. pnp / pnp_*: as
    PoseStream's; one comet_landmark_pnp launch per push, on the rows of the landmark launch in its order.
    lm_archive / reid_px / reid_min_cos / lm_arch_min_obs: as PoseStream's; one comet_landmark_reid launch per
    push, before the landmark launch, on its rows in its order; reset(stream) frees that stream's archive.
    motion / motion_*: as PoseStream's; one comet_motion_fit launch per push, on the rows of the fuse launch in
    its order; reset(stream) forgets that stream's history.

    push() -> [(stream id, StreamResult)] ordered by stream id. The tensors of a result are views
    of the batched outputs. The model is used as is (its eval / train mode included)."""

    _TABLES_MAX = 1024  # cached device slot tables (periodic in capacity for streams in phase)

    def __init__(self, model, streams, window, stride=1, capacity=None, query_fn=None, anchors=None, precision=None,
                 fuse=False, fuse_weight=None, carry=False, carry_tracks=512, carry_cell=8, carry_border=0,
                 carry_min_score=None, detect_every=1, candidate_fn=None, mask_fn=None, warm=False, warm_mode="hold",
                 warm_iters=None, landmarks=False, track_intrs=None, lm_min_obs=3, lm_min_pivot=1e-8, lm_weight=None,
                 lm_gate_px=None, lm_inverse_rotation=0, pnp=False, pnp_iters=4, pnp_huber_px=None, pnp_min_pts=6,
                 pnp_weight=0.0, motion=False, motion_len=16, motion_min_frames=3, motion_iters=2, motion_horizon=1,
                 motion_max_angle=2.0, motion_inverse_rotation=0, lm_archive=0, reid_px=None, reid_min_cos=0.5,
                 lm_arch_min_obs=None):
        self.model = model
        self.sched = PoolSchedule(streams, window, stride, capacity)
        _check_landmarks(landmarks, fuse, carry, track_intrs, self.sched.streams, lm_weight, lm_gate_px)
        self._pnp = _check_pnp(pnp, landmarks, pnp_iters, pnp_huber_px, pnp_min_pts, pnp_weight)
        self.pnp = self._pnp is not None
        self.landmarks, self.lm_weight = bool(landmarks), lm_weight
        self.lm_gate_px = None if lm_gate_px is None else float(lm_gate_px)
        self._lm = None
        if self.landmarks:
            self._lm = LandmarkMap(window, stride, streams, carry_tracks, list(track_intrs), lm_min_obs, lm_min_pivot,
                                   lm_inverse_rotation, lm_archive, reid_px, reid_min_cos, lm_arch_min_obs)
        elif int(lm_archive):
            raise ValueError("lm_archive > 0 needs landmarks=True: the archive keeps the landmarks of dead tracks")
        self.lm_archive = int(lm_archive)
        self.query_fn = query_fn
        self.carry, self.candidate_fn, self.mask_fn = bool(carry), candidate_fn, mask_fn
        _check_warm(warm, self.carry, warm_mode, warm_iters)
        self.warm, self.warm_mode = bool(warm), warm_mode
        self.warm_iters = None if warm_iters is None else int(warm_iters)
        self._carry = None
        if self.carry:
            self.sched.scheds[0].chain_index()  # raises unless stride < window
            _check_carry(True, candidate_fn)
            self._carry = TrackCarry(window, stride, streams, carry_tracks, carry_cell, carry_border, carry_min_score,
                                     detect_every, warm_mode if self.warm else None)
        self.precision = precision if precision is not None else _model_precision(model)
        _check_fuse(fuse, fuse_weight, anchors is not None)
        self.fuse, self.fuse_weight = bool(fuse), fuse_weight
        self._fuser = None
        self.anchors = None
        if anchors is not None:
            self.sched.scheds[0].chain_index()  # raises unless stride < window
            items = anchors.items() if isinstance(anchors, dict) else enumerate(anchors)
            self.anchors = {int(s): Anchor(*a) for s, a in items}
            if sorted(self.anchors) != list(range(self.sched.streams)):
                raise ValueError(f"anchors must name every stream 0 .. {self.sched.streams - 1}, got "
                                 f"{sorted(self.anchors)}")
        mkw = _check_motion(motion, self.fuse, motion_len, motion_min_frames, motion_iters, motion_horizon,
                            motion_max_angle, motion_inverse_rotation)
        self.motion = mkw is not None
        self._motion = None
        if self.motion:
            self._motion = MotionTracker(window, stride, streams, **mkw)
        self._ratios = {}
        if self.fuse:
            self._fuse_key = self._anchor_key(self.anchors[0])
            for a in self.anchors.values():
                self._same_key(a)
        self.reset()

    @staticmethod
    def _anchor_key(a):
        return float(torch.as_tensor(a.ratio, dtype=torch.float64).reshape(-1)[0]), a.dataset

    def _same_key(self, a):
        if self._anchor_key(a) != self._fuse_key:
            raise ValueError(f"fuse=True needs one ratio and one dataset for all anchors, got {self._anchor_key(a)} "
                             f"and {self._fuse_key}")

    def reset(self, stream=None, anchor=None, track_intr=None):
        """reset(s): stream s forgets its frames (its next frame is frame 0, at its anchor, or at
        `anchor` when one is given); the other streams go on. reset(): every stream, and the rings are
        dropped (a new frame size may follow). track_intr (landmarks=True): the (fx, fy, cx, cy) of the
        track pixels of the sequence that stream s takes next."""
        self.sched.reset(stream)
        if track_intr is not None:
            if stream is None or self._lm is None:
                raise ValueError("reset(stream, track_intr=...) replaces the intrinsics of one stream of a pool with "
                                 "landmarks=True")
            self._lm.set_intr(stream, track_intr)
        if anchor is not None:
            if stream is None or self.anchors is None:
                raise ValueError("reset(stream, anchor=...) replaces the anchor of one stream of an anchored pool")
            a = Anchor(*anchor)
            if self.fuse:
                self._same_key(a)
                if self._fuser is not None:
                    self._fuser.set_anchor(stream, a.R, a.T_uvz)
            self.anchors[int(stream)] = a
        if self._fuser is not None:
            self._fuser.reset(stream)
        if self._carry is not None:
            self._carry.reset(stream)
        if self._lm is not None:
            self._lm.reset(stream)
        if self._motion is not None:
            self._motion.reset(stream)
        if stream is None:
            self._rings = self._wins = self._hw = self._dev = None
            self._tables = {}
            self._refs = {}
        else:
            self._refs.pop(int(stream), None)

    @property
    def landmark_map(self):
        """The LandmarkMap (landmarks=True), else None."""
        return self._lm

    @property
    def motion_tracker(self):
        """The MotionTracker (motion=True), else None."""
        return self._motion

    # -- rings ------------------------------------------------------------------------------------
    def _allocate(self, per):
        S, cap, T = self.sched.streams, self.sched.capacity, self.sched.window
        dev, self._hw = per[1].device, tuple(per[1].shape[-2:])  # (refine_frames: the frames themselves)
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
            self._rings.append(torch.empty(S * cap, *slot, device=dev, dtype=t.dtype))
            self._wins.append(torch.empty(S * T, *slot, device=dev, dtype=t.dtype))
        self._dev = dev
        if self.fuse and (self._fuser is None or self._fuser.device != dev):
            from .models.utils import INTRINSICS
            ratio, dataset = self._fuse_key
            self._fuser = PoseFuser(T, self.sched.stride, cap, S, {s: (a.R, a.T_uvz) for s, a in self.anchors.items()},
                                    ratio, INTRINSICS[dataset], dev)

    def _table(self, values):
        """A slot table on the device (int32) and on the host (ctypes), cached by its values."""
        key = tuple(values)
        hit = self._tables.get(key)
        if hit is None:
            if len(self._tables) >= self._TABLES_MAX:
                self._tables.clear()
            hit = (torch.tensor(key, dtype=torch.int32, device=self._dev), (ctypes.c_int32 * len(key))(*key))
            self._tables[key] = hit
        return hit

    def _query(self, sid, hop, query_points):
        q = query_points.get(sid) if isinstance(query_points, dict) else query_points
        if q is None:
            q = self.query_fn(self._rings[1][self.sched.slot(sid, hop.frame_index)])
        return q.to(self._dev, torch.float32)

    def _decode(self, sid, enc, T):
        a = self.anchors[sid]
        if sid not in self._refs:
            self._refs[sid], self._ratios[sid] = _anchor_ref(a, enc.device)
        R, Tx, self._refs[sid] = _decode_chained(a, self._refs[sid], self._ratios[sid],
                                                 self.sched.scheds[sid].chain_index(), enc, T)
        return R, Tx

    # -- hops -------------------------------------------------------------------------------------
    def _carried(self, hops):
        """carry=True: the queries of all the hops due, one comet_track_carry launch -> ops.CarryOut."""
        firsts = [self._rings[1][self.sched.slot(sid, hop.frame_index)] for sid, hop in hops]
        cands = [self.candidate_fn(f) if self._carry.detects(sid) else None for f, (sid, _) in zip(firsts, hops)]
        masks = [self.mask_fn(f) if self.mask_fn is not None else None for f in firsts]
        if self.warm:
            self._carry.warm_div = _warm_div(self.model)
        return self._carry.step([sid for sid, _ in hops], self._hw[0], self._hw[1], cands, masks)

    def _warm_groups(self, firsts):
        """carry=True: the hops due (firsts[i]: hop i is its stream's first) -> [(positions, warm start
        given, coarse iterations or None for the config's)], one batched call each. One group unless
        warm=True and first and later hops fall together whose iteration counts differ."""
        every = list(range(len(firsts)))
        if not self.warm or all(firsts):
            return [(every, False, None)]
        iters = self.warm_iters
        if iters is None or iters == int(self.model.cfg["track_trainit"]) or not any(firsts):
            return [(every, True, None if any(firsts) else iters)]
        return [([i for i in every if firsts[i]], False, None), ([i for i in every if not firsts[i]], True, iters)]

    def _hops(self, hops, qs, pos, fused=None, co=None, wo=None, warm=False, iters=None, later=None):
        """The hops hops[i], i in pos (all with N query points) as one batched call ->
        [(stream, StreamResult)] in the order of pos. fused (fuse=True): a list that takes the
        group's (pred_pose_enc, pred_score); the absolute poses are then left to _fuse. co
        (carry=True): the ops.CarryOut whose rows are the queries of all the hops due; wo (warm=True):
        the ops.WarmOut of the same hops, whose coordinates start the coarse tracker when `warm`;
        iters: the coarse iterations of this call (None: the config's). later (landmarks=True): a list
        that takes the group's (pred_tracks, pred_score); TrackCarry.update is then left to _landmarks."""
        from .models.E2Epose2 import FrameCache
        T, n = self.sched.window, len(pos)
        rows = None if co is None or n == len(hops) else self._table(pos)[0].long()
        table, table_host = self._table(self.sched.table([hops[i] for i in pos]))
        wins = [None if w is None else w[:n * T] for w in self._wins]
        ops.ring_gather([(r, w) for r, w in zip(self._rings, wins) if r is not None], table, table_host)
        fm, fr, tok = wins
        cache = FrameCache(fmaps=None if fm is None else fm.view(n, T, *fm.shape[1:]),
                           refine_frames=fr.view(n, T, *fr.shape[1:]), tokens=tok)
        if co is not None:
            q = co.query if rows is None else co.query.index_select(0, rows)
        else:
            q = torch.stack([qs[i] for i in pos])
        tracks = q[:, None].expand(n, T, -1, 2)
        extra = {}
        if warm:  # (the predictor updates its starting coordinates in place: wo.coords, or the copy, is this call's)
            extra["track_init"] = wo.coords if rows is None else wo.coords.index_select(0, rows)
        if iters is not None:
            extra["track_iters"] = iters
        # (with a frame_cache the model reads only the shape of its image argument)
        out = self.model.forward_all(cache.refine_frames, training=False, tracks=tracks, frame_cache=cache, **extra)
        enc = out["pred_pose_enc"]  # [n * T, 7]
        tr = out.get("pred_tracks")
        sc = out.get("_track_predictions", {}).get("pred_score")
        results = []
        if fused is not None:
            fused.append((enc, sc))
        if later is not None:
            later.append((tr, sc))
        elif co is not None:
            self._carry.update([hops[i][0] for i in pos], tr, sc)
        for b, i in enumerate(pos):
            sid, hop = hops[i]
            e = enc[b * T:(b + 1) * T]
            R = Tx = None
            if self.anchors is not None and fused is None:
                R, Tx = self._decode(sid, e, T)
            results.append((sid, StreamResult(hop.frame_index, e, None if tr is None else tr[b],
                                              None if sc is None else sc[b], R, Tx)))
            if co is not None:
                results[-1] = (sid, results[-1][1].with_tracks(*_carry_fields(co, i, wo)))
        return results

    def _fuse(self, hops, results, fused):
        """One comet_pose_fuse launch for all the hops of a push: hops in the order of `results`,
        fused = [(pred_pose_enc, pred_score)] per query-count group."""
        enc = fused[0][0] if len(fused) == 1 else torch.cat([e for e, _ in fused])
        w = None
        if self.fuse_weight == "score":
            ws = [_score_weights(sc) for _, sc in fused]
            w = ws[0] if len(ws) == 1 else torch.cat(ws)
        out = self._fused = self._fuser.fuse(enc, hops, w)
        self._fused_hops = list(hops)  # (the rows of `out`, for the PnP feedback of _landmarks)
        final = self._fuser.sched.final
        results = [(sid, r._replace(**_fused_fields(out, b, final))) for b, (sid, r) in enumerate(results)]
        if self.motion:  # (on the rows of the fuse launch, in its order)
            mo = self._motion.update(self._fused_hops, out)
            results = [(sid, r.with_motion(mo, b)) for b, (sid, r) in enumerate(results)]
        return results

    def _landmarks(self, order, results, co, later):
        """One comet_landmark_update launch for all the hops of a push, after _fuse: results and the
        FuseOut are in the order `order` (positions in the hops due), co's rows in the order of the hops
        due, later = [(pred_tracks, pred_score)] per batched call. Then the carry takes the scores."""
        tr = later[0][0] if len(later) == 1 else torch.cat([t for t, _ in later])
        sc = later[0][1] if len(later) == 1 else torch.cat([s for _, s in later])
        ids, src = co.ids, co.src
        if order != list(range(len(order))):
            rows = self._table(order)[0].long()
            ids, src = ids.index_select(0, rows), src.index_select(0, rows)
        sids = [sid for sid, _ in results]
        lo, sc, po, ro = _landmark_step(self._lm, sids, tr, sc, self._fused, ids, src, self.lm_weight, self.lm_gate_px,
                                    self._pnp, self._fuser, self._fused_hops)
        self._carry.update(sids, tr, sc)
        results = [(sid, r.with_landmarks(lo, b)) for b, (sid, r) in enumerate(results)]
        if po is not None:
            results = [(sid, r.with_pnp(po, b)) for b, (sid, r) in enumerate(results)]
        if ro is not None:
            results = [(sid, r.with_reid(ro, b)) for b, (sid, r) in enumerate(results)]
        return results

    @torch.no_grad()
    def push(self, frames, streams=None, query_points=None):
        """frames [k, 3, H, W] f32 on the model's device, one per stream of `streams` (k distinct
        ids; default: all streams in order) -> [(stream id, StreamResult)] of the hops the frames
        complete, ordered by stream id (often empty). Bad arguments raise ValueError before anything
        is launched."""
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f"push takes [k, 3, H, W] frames, got {tuple(frames.shape)}")
        ids = self.sched.ids(frames.shape[0], streams)
        hw = tuple(frames.shape[-2:])
        if self._hw is not None and hw != self._hw:
            raise ValueError(f"frame size changed from {self._hw} to {hw}; reset() starts new streams")
        _check_carry(self.carry, self.candidate_fn, query_points)
        if self.query_fn is None and not self.carry:
            if query_points is None:
                raise ValueError("no query source: pass query_points to push() or query_fn to StreamPool")
            if isinstance(query_points, dict):
                missing = [s for s in self.sched.due(ids) if query_points.get(s) is None]
                if missing:
                    raise ValueError(f"no query source for the streams {missing}, whose hop is due in this push")
        with F.precision(self.precision):
            return self._advance(_per_frame(self.model.frame_stages(frames.float())), ids, query_points)

    def _advance(self, per, ids, query_points):
        """The part of a push behind the per-frame stages, called under F.precision and no_grad: per, the
        FrameCache-ordered tensors with one row per stream of `ids` (_per_frame), go into the rings and
        the hops that fall due run -> [(stream id, StreamResult)] ordered by stream id. Everything a
        hop leaves behind (carried tracks, accumulator rows, the chained reference) is in place when
        this returns, so the stream's next frame may be stored."""
        if self._rings is None:
            self._allocate(per)
        results = []
        slots, hops = self.sched.push(ids)
        slot_table, slot_host = self._table(slots)
        ops.ring_scatter([(t.contiguous(), r) for t, r in zip(per, self._rings) if r is not None],
                         slot_table, slot_host)
        if hops:
            fused, order = ([] if self.fuse else None), []
            later = [] if self.landmarks else None
            if self.carry:  # every hop has carry_tracks queries: one group, unless the coarse iterations differ
                firsts = [self._carry.sched.is_first(sid) for sid, _ in hops]
                co = self._carried(hops)
                wo = self._carry.warm if self.warm else None
                for pos, warm, iters in self._warm_groups(firsts):
                    results += self._hops(hops, None, pos, fused, co, wo, warm, iters, later)
                    order += pos
            else:
                qs = [self._query(sid, hop, query_points) for sid, hop in hops]
                for _, pos in self.sched.group([q.shape[0] for q in qs]):
                    results += self._hops(hops, qs, pos, fused)
                    order += pos
            if self.fuse:
                results = self._fuse([hops[i] for i in order], results, fused)
            if self.landmarks:
                results = self._landmarks(order, results, co, later)
        return sorted(results, key=lambda r: r[0])


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


def keypoint_candidates(sp, sift=None):
    """candidate_fn for carry=True from the detectors of comet_amd.keypoints: the raw detections of
    SuperPoint.extract (then SIFT.extract when given) on a frame [3, H, W] -> [M, 2] in detector
    order, neither filtered nor padded: comet_track_carry applies the mask, the border and the
    one-per-cell rule and pads to the fixed track count."""
    def candidates(frame):
        pts = sp.extract(frame)["keypoints"][0]
        if sift is not None:
            pts = torch.cat([pts, sift.extract(frame)["keypoints"][0]], 0)
        return pts
    return candidates
