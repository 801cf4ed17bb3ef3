"""COMET (mirror of comet/models/E2Epose2.py:59-266): tracker (no_grad) -> score inversion ->
camera predictor. Same constructor (TRACK, CAMERA, cfg) and forward signature."""
from typing import Dict, NamedTuple, Optional

import torch
import torch.nn as nn

from ..config import instantiate
from .refine_track import refine_frame_input, refine_track


class FrameCache(NamedTuple):
    """Outputs of the per-frame stages for B x T frames (COMET.frame_stages, comet_amd.stream)."""
    fmaps: Optional[torch.Tensor]          # [B, T, h, w, 128] (process_images_to_fmaps)
    refine_frames: Optional[torch.Tensor]  # [B, T, 3, H, W] f32 (refine_frame_input)
    tokens: Optional[torch.Tensor]         # [B*T, P, C] (CameraPredictor.frame_tokens)


class COMET(nn.Module):
    def __init__(self, TRACK: Dict, CAMERA: Dict, cfg=None):
        super().__init__()
        if cfg is None:
            raise ValueError("cfg must be provided")
        self.cfg = cfg
        self.enable_track = cfg["enable_track"]
        self.enable_pose = cfg["enable_pose"]
        self.window_len = cfg.get("window_len", 8) if hasattr(cfg, "get") else 8
        if not (self.enable_track or self.enable_pose):
            raise ValueError("You have to enable at least tracking or pose estimation.")
        if self.enable_track:
            self.track_predictor = instantiate(TRACK, _recursive_=False, cfg=cfg)
            self._freeze_tracker_params()
        if self.enable_pose:
            self.camera_predictor = instantiate(CAMERA, _recursive_=False, cfg=cfg)

    def _freeze_tracker_params(self):
        if self.cfg.get("freeze_track", False):
            for p in self.track_predictor.parameters():
                p.requires_grad = False

    def forward(self, image, gt_cameras=None, training=True, tracks=None, tracks_visibility=None, crop_params=None,
                epoch=-1, frame_cache=None, track_init=None, track_iters=None):
        if training:
            return self.forward_all(image, gt_cameras=gt_cameras, training=training, tracks=tracks,
                                    tracks_visibility=tracks_visibility, frame_cache=frame_cache,
                                    track_init=track_init, track_iters=track_iters)
        assert image.shape[0] == 1, f"evaluation processes one sequence at a time, got batch {image.shape[0]}"
        with torch.no_grad():
            return self.forward_all(image, gt_cameras=gt_cameras, training=training, tracks=tracks,
                                    tracks_visibility=tracks_visibility, frame_cache=frame_cache,
                                    track_init=track_init, track_iters=track_iters)

    @torch.no_grad()
    def frame_stages(self, frames):
        """The stages that see one frame at a time, for frames [n, 3, H, W] f32 -> FrameCache with a
        batch of one n-frame sequence: the tracker's feature maps, the frames as refine_track reads
        them, and the camera head's per-frame tokens. forward_all(..., frame_cache=...) skips these
        stages and uses the tensors (DESIGN.md "Online / streaming inference")."""
        fmaps = tokens = None
        refine_frames = refine_frame_input(frames[None])
        if self.enable_track:
            fmaps = self.track_predictor.process_images_to_fmaps(frames[None], training=True)
        if self.enable_pose:
            tokens = self.camera_predictor.frame_tokens(frames)
        return FrameCache(fmaps=fmaps, refine_frames=refine_frames, tokens=tokens)

    def forward_all(self, image, preliminary_cameras=None, gt_cameras=None, training=True, tracks=None,
                    tracks_visibility=None, frame_cache=None, track_init=None, track_iters=None):
        """E2Epose2.py:151-266 (fine_tracker=True, softmax_refine=False, track_conf=False).
        frame_cache (FrameCache, optional): the per-frame stages' outputs for these B x T frames,
        computed earlier; `image` then only supplies the shape.
        track_init (optional): the coarse predictor's coords_init, f32 [B, N, T, 2] in its grid units,
        updated in place; track_iters (optional): the coarse iterations of this call instead of
        cfg.track_trainit (DESIGN.md "Warm start"). Both None: the call runs as it always has."""
        B, T, C, H, W = image.shape
        cfg = self.cfg
        predictions = {}
        pred_track = inverted_score = None
        with torch.no_grad():
            if self.enable_track:
                tp = self.track_predictor
                if frame_cache is None:
                    fmaps = tp.process_images_to_fmaps(image, training=True)
                else:
                    fmaps = frame_cache.fmaps
                coarse_lists, vis_e, _, _, _ = tp.coarse_predictor(query_points=tracks[:, 0], fmaps=fmaps,
                                                                   iters=cfg["track_trainit"] if track_iters is None
                                                                   else int(track_iters),
                                                                   down_ratio=tp.coarse_down_ratio, return_feat=True,
                                                                   coords_init=track_init)
                coarse = coarse_lists[-1]
                if cfg["fine_tracker"]:
                    refined, score, inverted_score = refine_track(
                        image if frame_cache is None else frame_cache.refine_frames, tp.fine_fnet, tp.fine_predictor,
                        coarse, compute_score=True)
                    predictions["coarse_pred_track"] = coarse
                    predictions["refine_pred_track"] = refined
                    predictions["pred_score"] = inverted_score
                    pred_track = refined
                else:
                    pred_track = coarse
                    predictions["refine_pred_track"] = coarse
        pose_predictions = {}
        if self.enable_pose and frame_cache is None:
            pose_predictions = self.camera_predictor(image.reshape(-1, C, H, W), preliminary_cameras=None,
                                                     batch_size=B, gt_cameras=gt_cameras, iters=cfg["camera_iter"],
                                                     pred_trajectories=pred_track, track_confidence=inverted_score)
        elif self.enable_pose:
            pose_predictions = self.camera_predictor(None, preliminary_cameras=None, batch_size=B,
                                                     gt_cameras=gt_cameras, iters=cfg["camera_iter"],
                                                     pred_trajectories=pred_track, track_confidence=inverted_score,
                                                     tokens=frame_cache.tokens)
        if self.enable_track:
            pose_predictions["pred_tracks"] = predictions["refine_pred_track"]
            pose_predictions["_track_predictions"] = predictions
        return pose_predictions
