"""Keypoint initialisation of the training loop (train_eval_func_new_cp5.py:527-595).

The reference builds `lightglue.SuperPoint(max_num_keypoints=cfg.train.track_num,
detection_threshold=0.005)` and `lightglue.SIFT(max_num_keypoints=track_num)`, runs `.extract()` on
frame 0 of every sequence, concatenates both keypoint sets and keeps / pads them with
`filter_and_pad` against the sequence's first object mask (train_eval_func_new_cp5.py:249-314);
the result, broadcast over the T frames, is the `tracks` input of COMET.

Here:
  * SuperPoint: LightGlue's network (magicleap SuperPoint v1: VGG encoder conv1a..conv4b, detector
    convPa/convPb, descriptor convDa/convDb -- same parameter names, so `superpoint_v1.pth` loads)
    and its extract() pipeline (resize to `resize` on the long side, grayscale, simple_nms radius 4,
    4-px border removal, threshold, top-k, keypoints rescaled to the input). Every dense stage runs
    on libcomet_hip.so (comet_sp_preprocess, comet_conv2d_nhwc with fused ReLU,
    comet_maxpool2_nhwc, comet_sp_scores, comet_maxfilt2d); candidate selection / top-k are device
    torch ops. The descriptor head is not evaluated: COMET uses only the keypoints.
  * filter_and_pad: the reference's rules, on the device, with the same torch RNG calls
    (torch.randint / torch.randperm on the keypoints' device) -- so a run seeded like the reference
    on the same device draws the same padding points -- and the 3x3 dilation on comet_maxfilt2d.
  * SIFT: LightGlue's SIFT wraps OpenCV's CPU detector (neither OpenCV nor pycolmap exists here).
    `SIFT` is that detector's algorithm on the device (csrc/sift.hip: comet_sift_base,
    comet_gauss_blur, comet_downsample2, comet_sift_detect -- Gaussian scale space, DoG extrema,
    sub-pixel refinement, contrast and edge tests, orientation-peak count), followed by OpenCV's
    keep-best-n and the wrapper's filter_dog_point / top-k as device torch ops; the loop builds it
    when `train.track_by_sift` is set. `sift=None` uses the SuperPoint keypoints alone.
Parity: the NMS and filter_and_pad are pinned to fixtures generated from the reference tree
(glue-factory's batched_nms = LightGlue's simple_nms; the reference's filter_and_pad), and the
network + keypoint selection to the reference tree's copy of the same magicleap network
(gluefactory_nonfree/superpoint.py) run with PRNG weights (the trained superpoint_v1.pth is a
download that is not available here); SIFT is pinned to a float64 restatement of OpenCV's rules
(tests/sift_numpy.py) and an analytic blob check -- parity with OpenCV itself is unmeasured.
"""
import math

import torch
import torch.nn as nn

from . import _lib as L
from . import functional as F
from . import ops


def _maxfilt(x, r):
    """(2r+1)^2 stride-1 max filter of [B, H, W] f32 (comet_maxfilt2d)."""
    x = x.contiguous().float()
    B, H, W = x.shape
    y = torch.empty_like(x)
    tmp = torch.empty_like(x)
    L.check(L.load().comet_maxfilt2d(x.data_ptr(), y.data_ptr(), tmp.data_ptr(), B, H, W, r, ops.stream()),
            "comet_maxfilt2d")
    return y


def simple_nms(scores, nms_radius):
    """LightGlue superpoint.simple_nms (= glue-factory batched_nms, superpoint_open.py:34-48):
    local maxima of a (2r+1)^2 window, two rounds of re-admitting maxima outside suppressed areas."""
    zeros = torch.zeros_like(scores)
    max_mask = scores == _maxfilt(scores, nms_radius)
    for _ in range(2):
        supp_mask = _maxfilt(max_mask.float(), nms_radius) > 0
        supp_scores = torch.where(supp_mask, zeros, scores)
        new_max_mask = supp_scores == _maxfilt(supp_scores, nms_radius)
        max_mask = max_mask | (new_max_mask & (~supp_mask))
    return torch.where(max_mask, scores, zeros)


def sp_scores(logits_nhwc):
    """Detector logits [B, h, w, 65] -> dense keypoint scores [B, 8h, 8w] (softmax, dustbin dropped,
    depth-to-space; comet_sp_scores)."""
    lg = logits_nhwc.contiguous().float()
    B, h, w, _ = lg.shape
    out = torch.empty(B, 8 * h, 8 * w, device=lg.device, dtype=torch.float32)
    L.check(L.load().comet_sp_scores(lg.data_ptr(), out.data_ptr(), B, h, w, ops.stream()), "comet_sp_scores")
    return out


class SuperPoint(nn.Module):
    """LightGlue's SuperPoint (superpoint_v1 architecture and parameter names) with extract()."""

    default_conf = {"descriptor_dim": 256, "nms_radius": 4, "max_num_keypoints": None,
                    "detection_threshold": 0.0005, "remove_borders": 4, "resize": 1024}

    def __init__(self, **conf):
        super().__init__()
        self.conf = {**self.default_conf, **conf}
        mk = self.conf["max_num_keypoints"]
        if mk is not None and mk <= 0:
            raise ValueError("max_num_keypoints must be positive or None")
        c1, c2, c3, c4, c5 = 64, 64, 128, 128, 256
        self.conv1a = nn.Conv2d(1, c1, 3, 1, 1)
        self.conv1b = nn.Conv2d(c1, c1, 3, 1, 1)
        self.conv2a = nn.Conv2d(c1, c2, 3, 1, 1)
        self.conv2b = nn.Conv2d(c2, c2, 3, 1, 1)
        self.conv3a = nn.Conv2d(c2, c3, 3, 1, 1)
        self.conv3b = nn.Conv2d(c3, c3, 3, 1, 1)
        self.conv4a = nn.Conv2d(c3, c4, 3, 1, 1)
        self.conv4b = nn.Conv2d(c4, c4, 3, 1, 1)
        self.convPa = nn.Conv2d(c4, c5, 3, 1, 1)
        self.convPb = nn.Conv2d(c5, 65, 1, 1, 0)
        self.convDa = nn.Conv2d(c4, c5, 3, 1, 1)
        self.convDb = nn.Conv2d(c5, self.conf["descriptor_dim"], 1, 1, 0)

    def _conv(self, x, conv, relu=True, out_dtype=None):
        k, pad = conv.kernel_size[0], conv.padding[0]
        if x.dtype == torch.bfloat16:  # implicit GEMM with the bias + ReLU epilogue
            w = F.wcast_conv(conv.weight, cin_pad=x.shape[-1])
            return ops.conv2d_nhwc(x, w, k, k, 1, pad, bias=conv.bias,
                                   act=L.ACT_RELU if relu else L.ACT_NONE, out_dtype=out_dtype or x.dtype)
        from .models.modules import conv2d_nhwc  # f32: im2col + GEMM
        y = conv2d_nhwc(x, conv, 1, pad, out_dtype=out_dtype or x.dtype)
        return torch.relu_(y) if relu else y

    def _pool(self, x):
        n, H, W, C = x.shape
        y = torch.empty(n, H // 2, W // 2, C, device=x.device, dtype=x.dtype)
        L.check(L.load().comet_maxpool2_nhwc(ops.dt(x), x.data_ptr(), y.data_ptr(), n, H, W, C, ops.stream()),
                "comet_maxpool2_nhwc")
        return y

    @torch.no_grad()
    def dense_probs(self, x):
        """Preprocessed NHWC image [B, H, W, 8] -> dense keypoint probabilities [B, H, W] (encoder,
        detector head, softmax with the dustbin dropped, depth-to-space; superpoint.py:202-233)."""
        for a, b in (("conv1a", "conv1b"), ("conv2a", "conv2b"), ("conv3a", "conv3b")):
            x = self._conv(self._conv(x, getattr(self, a)), getattr(self, b))
            x = self._pool(x)
        x = self._conv(self._conv(x, self.conv4a), self.conv4b)
        logits = self._conv(self._conv(x, self.convPa), self.convPb, relu=False, out_dtype=torch.float32)
        return sp_scores(logits)

    @torch.no_grad()
    def dense_scores(self, x):
        """Preprocessed NHWC image [B, H, W, 8] -> keypoint scores [B, H', W'] after the NMS and the
        border removal (LightGlue SuperPoint.forward up to the candidate selection)."""
        scores = simple_nms(self.dense_probs(x), self.conf["nms_radius"])
        pad = self.conf["remove_borders"]
        if pad:
            scores[:, :pad] = -1
            scores[:, :, :pad] = -1
            scores[:, -pad:] = -1
            scores[:, :, -pad:] = -1
        return scores

    def _preprocess(self, image, OH, OW):
        B, _, H, W = image.shape
        dt = F.compute_dtype()
        y = torch.empty(B, OH, OW, 8, device=image.device, dtype=dt)
        L.check(L.load().comet_sp_preprocess(ops.dt(y), image.contiguous().float().data_ptr(), y.data_ptr(), B, H, W,
                                             OH, OW, 8, ops.stream()), "comet_sp_preprocess")
        return y

    @torch.no_grad()
    def extract(self, img):
        """LightGlue Extractor.extract: img [3, H, W] or [1, 3, H, W] -> {"keypoints" [1, K, 2]
        (x, y in input pixels), "keypoint_scores" [1, K]}."""
        if img.dim() == 3:
            img = img[None]
        if img.dim() != 4 or img.shape[0] != 1:
            raise ValueError("extract takes one image")
        _, _, H, W = img.shape
        r = self.conf["resize"]
        if r is not None:  # resize so that the long side is `resize` (ImagePreprocessor side="long")
            s = r / max(H, W)
            OH, OW = int(round(H * s)), int(round(W * s))
        else:
            OH, OW = H, W
        scores = self.dense_scores(self._preprocess(img, OH, OW))
        idx = torch.nonzero(scores[0] > self.conf["detection_threshold"])  # (i, j), row-major
        sc = scores[0][idx[:, 0], idx[:, 1]]
        mk = self.conf["max_num_keypoints"]
        if mk is not None and mk < idx.shape[0]:
            sc, order = torch.topk(sc, mk, dim=0, sorted=True)
            idx = idx[order]
        kp = torch.flip(idx, [1]).float()
        scale = torch.tensor([OW / W, OH / H], device=kp.device, dtype=kp.dtype)
        kp = (kp + 0.5) / scale - 0.5
        return {"keypoints": kp[None], "keypoint_scores": sc[None]}


class SIFT(nn.Module):
    """LightGlue's SIFT extractor (`backend="opencv"`: cv2.SIFT_create + detectAndCompute behind a
    device-to-host copy) as a device-side difference-of-Gaussians detector on libcomet_hip.so
    (csrc/sift.hip). No parameters, no descriptors, no orientation angles: COMET reads only the
    keypoint coordinates.

    The wrapper hands its `num_octaves` to OpenCV as nOctaveLayers (gluefactory sift.py:129); that is
    reproduced on purpose: `num_octaves` (default 4) is the number of layers per octave, and the
    number of octaves is OpenCV's own, round(log2(min(H, W)) - 2) + 1 with H, W the size of the 2x
    up-sampled base image (first octave -1).

    The steps follow OpenCV's detector rule by rule; they are pinned to a float64
    restatement of those rules (tests/sift_numpy.py), not to OpenCV itself, which cannot be run where
    this is built and tested."""

    default_conf = {"max_num_keypoints": 4096, "detection_threshold": 0.0066667, "edge_threshold": 10,
                    "num_octaves": 4, "nms_radius": 0, "resize": 1024, "candidate_capacity": 32768}
    sigma = 1.6

    def __init__(self, **conf):
        super().__init__()
        unknown = set(conf) - set(self.default_conf)
        if unknown:
            raise ValueError(f"unknown SIFT options {sorted(unknown)}")
        self.conf = {**self.default_conf, **conf}
        mk = self.conf["max_num_keypoints"]
        if mk is not None and mk <= 0:
            raise ValueError("max_num_keypoints must be positive or None")
        if not 1 <= self.conf["num_octaves"] <= 8:
            raise ValueError("num_octaves (layers per octave) must be in 1..8")

    def layer_sigmas(self):
        """The blur that takes layer i - 1 of an octave to layer i (i = 1 .. layers + 2)."""
        nl = self.conf["num_octaves"]
        k = 2.0 ** (1.0 / nl)
        return [((self.sigma * k ** i) ** 2 - (self.sigma * k ** (i - 1)) ** 2) ** 0.5 for i in range(1, nl + 3)]

    @torch.no_grad()
    def pyramid(self, gray):
        """gray uint8 [B, H, W] -> one [B, layers + 3, h, w] f32 buffer of Gaussian images per octave.
        Octaves without a pixel inside the detector's 5-px border are not built: nothing reads them."""
        gray = gray.contiguous()
        B, H, W = gray.shape
        lib, st = L.load(), ops.stream()
        nl = self.conf["num_octaves"]
        n_oct = int(round(math.log2(min(2 * H, 2 * W)) - 2)) + 1
        sig = self.layer_sigmas()
        octaves = []
        h, w = 2 * H, 2 * W
        for o in range(n_oct):
            if min(h, w) <= 10:
                break
            buf = torch.empty(B, nl + 3, h, w, device=gray.device, dtype=torch.float32)
            layers = [torch.empty(B, h, w, device=gray.device, dtype=torch.float32) for _ in range(nl + 3)]
            if o == 0:
                L.check(lib.comet_sift_base(gray.data_ptr(), layers[0].data_ptr(), B, H, W, st), "comet_sift_base")
            else:
                ph, pw = prev.shape[-2:]
                L.check(lib.comet_downsample2(prev.data_ptr(), layers[0].data_ptr(), B, ph, pw, st), "comet_downsample2")
            for i in range(1, nl + 3):
                L.check(lib.comet_gauss_blur(layers[i - 1].data_ptr(), layers[i].data_ptr(), B, h, w, sig[i - 1], st),
                        "comet_gauss_blur")
            torch.stack(layers, 1, out=buf)
            octaves.append(buf)
            prev = layers[nl]
            h, w = h // 2, w // 2
        return octaves

    @torch.no_grad()
    def detect(self, gray):
        """gray uint8 [B, H, W] -> per image the candidate list before any cut: [n, 7] f32 rows
        (x, y, size, response, orientation count, octave, layer), x / y / size in pixels of `gray`,
        sorted by (response descending, octave, layer, y, x) -- the kernel appends candidates in the
        order its atomic adds arrive, the sort makes the list independent of that."""
        if gray.dtype != torch.uint8 or gray.dim() != 3:
            raise ValueError("detect takes a uint8 [B, H, W] batch")
        B = gray.shape[0]
        lib, st = L.load(), ops.stream()
        cap = int(self.conf["candidate_capacity"])
        cand = torch.empty(B, cap, 8, device=gray.device, dtype=torch.float32)
        count = torch.zeros(B + 1, device=gray.device, dtype=torch.int32)  # [B] counters, then the overflow flag
        for o, buf in enumerate(self.pyramid(gray)):
            h, w = buf.shape[-2:]
            L.check(lib.comet_sift_detect(buf.data_ptr(), B, self.conf["num_octaves"], h, w, o,
                                          float(self.conf["detection_threshold"]), float(self.conf["edge_threshold"]),
                                          self.sigma, cand.data_ptr(), cap, count.data_ptr(),
                                          count.data_ptr() + 4 * B, st), "comet_sift_detect")
        n = count.tolist()
        if n[B] != 0:
            raise L.CometHipError(f"SIFT: more than candidate_capacity={cap} keypoints in one image "
                                  f"(counts {n[:B]}); raise candidate_capacity")
        out = []
        for b in range(B):
            c = cand[b, :n[b], :7]
            order = torch.arange(c.shape[0], device=c.device)
            for col, desc in ((0, False), (1, False), (6, False), (5, False), (3, True)):  # least significant key first
                order = order[torch.sort(c[order, col], stable=True, descending=desc)[1]]
            c = c[order].clone()
            c[:, :3] *= 0.5  # the base image is the 2x up-sample (first octave -1)
            out.append(c)
        return out

    def select(self, cand, H, W):
        """Indices into a detect() list (sorted by response) of the keypoints extract() returns:
        OpenCV's keep-best-n over the list with every candidate repeated once per orientation peak
        (all ties with the last kept response stay), then the wrapper's filter_dog_point (one
        keypoint per rounded pixel -- the best; equal scores: the first of the sorted list -- and the
        (2 nms_radius + 1)^2 max filter), then the top max_num_keypoints by score."""
        mk = self.conf["max_num_keypoints"]
        resp, nori = cand[:, 3], cand[:, 4]
        idx = torch.nonzero(nori > 0)[:, 0]
        if mk is not None and idx.numel() > 0:
            cum = torch.cumsum(nori[idx], 0)
            if cum[-1] > mk:
                last = resp[idx][torch.searchsorted(cum, torch.tensor([float(mk)], device=cum.device))[0]]
                idx = idx[resp[idx] >= last]
        if idx.numel() == 0:
            return idx
        ij = torch.round(cand[idx, :2] - 0.5).long()
        pix = ij[:, 1].clamp(0, H - 1) * W + ij[:, 0].clamp(0, W - 1)
        ps, perm = torch.sort(pix, stable=True)
        first = torch.ones_like(ps, dtype=torch.bool)
        first[1:] = ps[1:] != ps[:-1]
        keep = torch.sort(perm[first])[0]
        idx, pix = idx[keep], pix[keep]
        r = int(self.conf["nms_radius"] or 0)
        if r > 0:
            buf = torch.zeros(H * W, device=cand.device, dtype=torch.float32)
            buf[pix] = resp[idx]
            idx = idx[buf[pix] == _maxfilt(buf.view(1, H, W), r).view(-1)[pix]]
        if mk is not None and idx.numel() > mk:
            idx = idx[:mk]
        return idx

    @torch.no_grad()
    def extract(self, img):
        """LightGlue Extractor.extract for a batch: img [3, H, W] or [B, 3, H, W] in [0, 1] ->
        {"keypoints" [B, N, 2] (x, y in input pixels), "keypoint_scores" [B, N], "scales" [B, N],
        "num_keypoints" [B]}, best response first. N is the largest count of the batch; the rows
        past an image's own count hold keypoints -1 and zeros."""
        if img.dim() == 3:
            img = img[None]
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError("extract takes [3, H, W] or [B, 3, H, W]")
        B, _, H, W = img.shape
        r = self.conf["resize"]
        if r is not None:  # resize so that the long side is `resize` (ImagePreprocessor side="long")
            s = r / max(H, W)
            OH, OW = int(round(H * s)), int(round(W * s))
        else:
            OH, OW = H, W
        g = torch.empty(B, OH, OW, 1, device=img.device, dtype=torch.float32)
        L.check(L.load().comet_sp_preprocess(L.F32, img.contiguous().float().data_ptr(), g.data_ptr(), B, H, W, OH, OW,
                                             1, ops.stream()), "comet_sp_preprocess")
        gray = (g.view(B, OH, OW) * 255.0).clamp_(0, 255).to(torch.uint8)  # sift.py:156, truncating
        sel = []
        for c in self.detect(gray):
            sel.append(c[self.select(c, OH, OW)])
        n = max(c.shape[0] for c in sel)
        scale = torch.tensor([OW / W, OH / H], device=img.device, dtype=torch.float32)
        kp = torch.full((B, n, 2), -1.0, device=img.device)
        sc = torch.zeros(B, n, device=img.device)
        sz = torch.zeros(B, n, device=img.device)
        for b, c in enumerate(sel):
            kp[b, :c.shape[0]] = (c[:, :2] + 0.5) / scale - 0.5
            sc[b, :c.shape[0]] = c[:, 3]
            sz[b, :c.shape[0]] = c[:, 2] / scale.mean()
        num = torch.tensor([c.shape[0] for c in sel], device=img.device)
        return {"keypoints": kp, "keypoint_scores": sc, "scales": sz, "num_keypoints": num}


def sample_extra_points(mask, need_extra, device):
    """need_extra random pixels (x, y) of a bool mask (train_eval_func_new_cp5.py:249-259)."""
    ys, xs = torch.where(mask)
    if ys.numel() == 0:
        return None
    idx = torch.randint(0, ys.shape[0], (need_extra,), device=device)
    return torch.stack([xs[idx], ys[idx]], dim=1).float().to(device)


def filter_and_pad(pts, mask0, min_pts, max_pts, sel_first_name=None):
    """Keypoints inside the first object mask, padded to at least min_pts with random mask pixels,
    then pixels of the mask's 1-px dilation ring, then any pixel; at most max_pts (random subset)
    (train_eval_func_new_cp5.py:261-314, same RNG calls in the same order)."""
    H, W = mask0.shape
    device = pts.device
    xs = pts[:, 0].round().clamp(0, W - 1).long()
    ys = pts[:, 1].round().clamp(0, H - 1).long()
    region = mask0.to(device).bool()
    keep = pts[region[ys, xs]]
    if keep.shape[0] < min_pts:
        need = min_pts - keep.shape[0]
        extra = sample_extra_points(region, need, device)
        if extra is None or extra.shape[0] < need:
            ring = (_maxfilt(region.float()[None], 1)[0] > 0) & (~region)
            remain = need if extra is None else need - extra.shape[0]
            extra2 = sample_extra_points(ring, remain, device)
            if extra2 is not None:
                extra = extra2 if extra is None else torch.cat([extra, extra2], 0)
        if extra is None or extra.shape[0] < need:
            gy, gx = torch.meshgrid(torch.arange(H, device=device), torch.arange(W, device=device), indexing="ij")
            grid = torch.stack([gx.flatten(), gy.flatten()], dim=1).float()
            remain = need if extra is None else need - extra.shape[0]
            extra3 = grid[torch.randint(0, grid.shape[0], (remain,), device=device)]
            extra = extra3 if extra is None else torch.cat([extra, extra3], 0)
        keep = torch.cat([keep, extra], 0)
    if keep.shape[0] > max_pts:
        keep = keep[torch.randperm(keep.shape[0], device=device)[:max_pts]]
    return keep


@torch.no_grad()
def keypoint_tracks(sp, images, mask, track_num, sift=None, min_required=256, names=None):
    """train_eval_func_new_cp5.py:560-592: frame-0 keypoints of every sequence (SuperPoint, plus
    SIFT when given), filtered / padded against the first mask, broadcast over the T frames ->
    (tracks [B, T, N, 2], tracks_visibility [B, T, N] bool). images [B, T, 3, H, W]; mask [B, H, W]."""
    B, T = images.shape[:2]
    sel = []
    for i in range(B):
        pts = sp.extract(images[i, 0])["keypoints"][0]
        if sift is not None:
            pts = torch.cat([pts, sift.extract(images[i, 0])["keypoints"][0]], 0)
        sel.append(filter_and_pad(pts, mask[i].bool(), min_required, track_num, names))
    kp0 = torch.stack(sel, 0)  # the reference stacks too: equal counts per sequence required
    tracks = kp0.unsqueeze(1).expand(B, T, -1, -1)
    vis = torch.ones(B, T, kp0.shape[1], device=images.device, dtype=torch.bool)
    return tracks, vis
