"""Plain float64 restatements of the tracker and camera-head glue operations of csrc/tracker.hip
and csrc/head.hip: the pins for tests/test_tracker_ops_gpu.py. Torch on the CPU only; nothing here
imports comet_amd.

Every helper is written from the kernel's header comment and the reference site it cites, with
loops where the kernel has index arithmetic, and is itself tied to oracle/comet_oracle.py (or to
torch's own interpolate / grid_sample) by tests/test_tracker_ref_cpu.py at the shapes the GPU tests
use. Layouts are the kernels': feature maps NHWC, track state [B, N, S, .] with row
t = (b*N + n)*S + s, coarse tracks / topleft / preds / scores [B, S, N, .]."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def dyadic(t, den=64, bound=1024.0):
    """True when every value is a multiple of 1/den below `bound` in magnitude: then float32 and
    float64 agree on floor() and on the fraction, and on every product with a small integer."""
    t = t.double()
    return bool(((t * den) == (t * den).round()).all() and (t.abs() < bound).all())


def bf16_round(x):
    """float64 -> nearest bfloat16 (ties to even), back in float64. Rounds through float32 first, as
    every kernel does (its value is formed in float32 and then converted)."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def bf16_ulp(x):
    """Spacing of bfloat16 (8 significand bits) at |x|, float64; the smallest normal's below it."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


# ---- samplers and image preparation ------------------------------------------------------------
def sample_bilinear(fmap, coords, border):
    """comet_sample_bilinear = sample_features4d / bilinear_sampler (utils.py:874-974): fmap
    [B, H, W, C] (channels last), coords [B, R, 2] pixel (x, y) -> [B, R, C]. grid_sample in float64
    after bilinear_sampler's normalisation x * 2 / max(size - 1, 1) - 1, align_corners=True, border
    or zeros padding."""
    B, H, W, C = fmap.shape
    inp = fmap.double().permute(0, 3, 1, 2)
    scale = torch.tensor([2.0 / max(W - 1, 1), 2.0 / max(H - 1, 1)], dtype=F64)
    grid = coords.double().unsqueeze(2) * scale - 1.0  # [B, R, 1, 2]
    out = F.grid_sample(inp, grid, mode="bilinear", align_corners=True, padding_mode="border" if border else "zeros")
    return out[..., 0].permute(0, 2, 1).contiguous()  # [B, C, R, 1] -> [B, R, C]


def images_nhwc(images, oh, ow, cpad):
    """comet_images_nhwc: [n, 3, H, W] -> [n, oh, ow, cpad]; bilinear align_corners resize
    (track_predictor.py:137) when the size changes, channels 3.. exactly zero."""
    n, _, H, W = images.shape
    x = images.double()
    if (oh, ow) != (H, W):
        x = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=True)
    out = torch.zeros(n, oh, ow, cpad, dtype=F64)
    out[..., :3] = x.permute(0, 2, 3, 1)
    return out


def dino_prep(images, R, patch, ldc, mean, std):
    """comet_dino_prep (camera_predictor10.py:622-634 + the DINOv2 patch_embed im2col): [BS, 3, H, W]
    -> resize to R x R (align_corners) -> (x - mean) / std -> rows (f, py, px), columns
    ci*p*p + ky*p + kx (the conv weight's flatten order), columns 3*p*p.. exactly zero."""
    BS = images.shape[0]
    x = F.interpolate(images.double(), size=(R, R), mode="bilinear", align_corners=True)
    x = (x - mean.double().view(1, 3, 1, 1)) / std.double().view(1, 3, 1, 1)
    g = R // patch
    kk = 3 * patch * patch
    cols = torch.zeros(BS * g * g, ldc, dtype=F64)
    for f in range(BS):
        for py in range(g):
            for px in range(g):
                blk = x[f, :, py * patch:(py + 1) * patch, px * patch:(px + 1) * patch]  # [ci, ky, kx]
                cols[(f * g + py) * g + px, :kk] = blk.reshape(-1)
    return cols


# ---- fine refinement glue ----------------------------------------------------------------------
def patch_gather(images, coarse, pradius, cpad):
    """comet_patch_gather (refine_track.py:74-131): images [B, S, 3, H, W], coarse [B, S, N, 2] ->
    patches [B*N*S, P, P, cpad] in (b, n, s) order (copies of image values, channels 3.. zero),
    topleft [B, S, N, 2] = floor(coarse) - pradius (int, unclamped), query [B*N, 2] =
    frac(coarse[:, 0]) + pradius. The patch origin is topleft clamped to [0, H - P] on BOTH axes
    (the reference uses H for x as well)."""
    B, S, _, H, W = images.shape
    N = coarse.shape[2]
    P = 2 * pradius + 1
    img = images.double()
    c = coarse.double()
    patches = torch.zeros(B * N * S, P, P, cpad, dtype=F64)
    topleft = torch.zeros(B, S, N, 2, dtype=torch.int32)
    query = torch.zeros(B * N, 2, dtype=F64)
    for b in range(B):
        for s in range(S):
            for n in range(N):
                ix, iy = math.floor(c[b, s, n, 0].item()), math.floor(c[b, s, n, 1].item())
                tlx, tly = ix - pradius, iy - pradius
                topleft[b, s, n, 0], topleft[b, s, n, 1] = tlx, tly
                x0 = min(max(tlx, 0), H - P)
                y0 = min(max(tly, 0), H - P)
                assert x0 + P <= W, "patch outside the frame: the H-for-both-axes clamp needs W >= H"
                patches[(b * N + n) * S + s, :, :, :3] = img[b, s, :, y0:y0 + P, x0:x0 + P].permute(1, 2, 0)
                if s == 0:
                    query[b * N + n, 0] = (c[b, s, n, 0] - ix) + pradius
                    query[b * N + n, 1] = (c[b, s, n, 1] - iy) + pradius
    return patches, topleft, query


def refine_combine(fine, topleft, coarse):
    """comet_refine_combine (refine_track.py:143-153): fine [B*N, S, 2] (patch coordinates, (b n, s)
    order), topleft [B, S, N, 2] int, coarse [B, S, N, 2] -> refined [B, S, N, 2] = fine + topleft in
    (b, s, n) order, frame 0 = the coarse query point. Computed in fine's dtype (pass float32 for
    the kernel's own sum)."""
    B, S, N, _ = coarse.shape
    out = torch.zeros(B, S, N, 2, dtype=fine.dtype)
    for b in range(B):
        for s in range(S):
            for n in range(N):
                if s == 0:
                    out[b, s, n] = coarse[b, 0, n].to(fine.dtype)
                else:
                    out[b, s, n] = fine[b * N + n, s] + topleft[b, s, n].to(fine.dtype)
    return out


def coords_update(coords, delta2, scale):
    """comet_coords_update (base_track_predictor.py:247-254): coords [B, N, S, 2], delta2 [B*N*S, 2]
    (the first two columns of the update former's output, row (b*N + n)*S + s) -> (new coords with
    frame 0 pinned, preds [B, S, N, 2] = new coords * scale)."""
    B, N, S, _ = coords.shape
    new = coords.double().clone()
    d = delta2.double().reshape(B, N, S, 2)
    new[:, :, 1:] += d[:, :, 1:]
    preds = torch.zeros(B, S, N, 2, dtype=F64)
    for b in range(B):
        for s in range(S):
            for n in range(N):
                preds[b, s, n] = new[b, n, s] * scale
    return new, preds


# ---- update former tokens ----------------------------------------------------------------------
def tracker_tokens(coords, feats, latent, corr, corrdim, pos, tdim, S):
    """comet_tracker_tokens (base_track_predictor.py:170-221, utils.py:835-871): row t of
    [flow embedding (2E, E = latent/2) | flow (2) | corr | feats | zeros] + pos[t // S], tdim columns.

    The flow (coords[t] - coords[frame 0 of t]) and the embedding's argument a * div,
    div = float32(k & ~1) * (float32(1000) / float32(E)), are formed in float32 exactly as the kernel
    and the reference form them; sin / cos are then evaluated in float64 ON that float32 argument
    (arguments reach ~2e4, where the rounding of the argument alone moves sin by ~2e-3: a float64
    argument would measure that, not the kernel)."""
    f32 = np.float32
    c = coords.detach().cpu().numpy().astype(f32).reshape(-1, 2)
    rows = c.shape[0]
    E = latent // 2
    flow = (c - c[(np.arange(rows) // S) * S]).astype(f32)  # one float32 subtraction
    k = np.arange(E)
    div = ((k & ~1).astype(f32) * (f32(1000.0) / f32(E))).astype(f32)
    out = torch.zeros(rows, tdim, dtype=F64)
    for axis in range(2):
        arg = (flow[:, axis:axis + 1] * div[None, :]).astype(f32).astype(np.float64)  # float32 product
        emb = np.where((k & 1)[None, :] == 1, np.cos(arg), np.sin(arg))
        out[:, axis * E:(axis + 1) * E] = torch.from_numpy(emb)
    out[:, 2 * E:2 * E + 2] = torch.from_numpy(flow.astype(np.float64))
    o = 2 * E + 2
    out[:, o:o + corrdim] = corr.double()[:, :corrdim]
    out[:, o + corrdim:o + corrdim + latent] = feats.double()
    return out + pos.double()[torch.arange(rows) // S]


# ---- track score -------------------------------------------------------------------------------
def track_score(qfeat, pfeat, fine, B, S, N, sradius):
    """comet_track_score = compute_score_fn (refine_track.py:174-278) + the inversion of
    E2Epose2.py:232-236. qfeat [B*N, C], pfeat [B*N, S, P, P, C] (b n, s order, channels last),
    fine [B*N, S, 2] -> (score [B, S, N], inv_score [B, S, N], var [B, S-1, N, 2]).

    The reference's indexing, reproduced: for output (b, s, n) the feature map is always patch
    (s = 0, n = 0) of sequence b; the window origin is read from `fine` at FLAT position
    m = (b*S + s)*N + n of its (b n, s) memory; window row = clamp(floor(y) - r, 0, P - ss), column
    = clamp(floor(x) - r, 0, P - ss). score = sqrt(max(var_x, 1e-10)) + sqrt(max(var_y, 1e-10)) of
    the softmax heat map over a [-1, 1] grid, 1 for frame 0; inv = 1 / (score + 1e-6), divided by
    its maximum over s."""
    P, C = pfeat.shape[2], pfeat.shape[4]
    ss = 2 * sradius + 1
    q = qfeat.double()
    pf = pfeat.double()
    fl = fine.double().reshape(-1, 2)
    lin = torch.linspace(-1.0, 1.0, ss, dtype=F64)
    score = torch.ones(B, S, N, dtype=F64)
    var = torch.zeros(B, S - 1, N, 2, dtype=F64)
    for b in range(B):
        fm = pf[b * N, 0]  # [P, P, C]: patch (b, n = 0), frame 0
        for s in range(1, S):
            for n in range(N):
                m = (b * S + s) * N + n
                tx = min(max(math.floor(fl[m, 0].item()) - sradius, 0), P - ss)
                ty = min(max(math.floor(fl[m, 1].item()) - sradius, 0), P - ss)
                sim = (fm[ty:ty + ss, tx:tx + ss] @ q[b * N + n]) / math.sqrt(C)  # [row, col]
                heat = torch.softmax(sim.reshape(-1), 0).reshape(ss, ss)
                px, py = heat.sum(0), heat.sum(1)  # marginals over columns (x) and rows (y)
                vx = (px * lin * lin).sum() - (px * lin).sum() ** 2
                vy = (py * lin * lin).sum() - (py * lin).sum() ** 2
                var[b, s - 1, n, 0], var[b, s - 1, n, 1] = vx, vy
                score[b, s, n] = math.sqrt(max(vx.item(), 1e-10)) + math.sqrt(max(vy.item(), 1e-10))
    inv = 1.0 / (score + 1e-6)
    inv = inv / inv.max(dim=1, keepdim=True)[0]
    return score, inv, var


# ---- camera head -------------------------------------------------------------------------------
def rowscale(x, w):
    """comet_rowscale_fwd: y[r, c] = x[r, c] * w[r]."""
    return x.double() * w.double().reshape(-1, 1)


def rowscale_bwd(x, w, dy):
    """comet_rowscale_bwd: dx = dy * w[r], dw[r] = sum_c dy * x."""
    return dy.double() * w.double().reshape(-1, 1), (dy.double() * x.double()).sum(-1)


def gapr(rot, uv, d, gt, B, S, w_trans=1.0, w_rot=2.0):
    """The GAPR tail (camera_predictor10.py:385-460), differentiable in whatever dtype it is given:
    rot [B*S, 4] raw, uv [B*S, 2], d [B*S, 1], gt [B*S, >= 7] -> (enc [B*S, 7], losses [3]).
    qn = F.normalize(rot, eps=1e-8); per sequence, over frames 1.., trans = 100 * mse((u, v, d),
    gt[:, :3]), rot = 100 * mse(qn, gt[:, 3:7]); losses = mean over sequences of
    (w_trans*trans + w_rot*rot, trans, rot); enc = (u, v, d, qn) with frame 0 forced to
    (0, 0, 0, 1, 0, 0, 0)."""
    qn = F.normalize(rot, p=2, dim=-1, eps=1e-8)
    uvd = torch.cat([uv, d], -1)
    tot = lt = lr = 0.0
    for b in range(B):
        r = slice(b * S + 1, (b + 1) * S)
        tl = ((uvd[r] - gt[r, :3]) ** 2).mean() * 100
        rl = ((qn[r] - gt[r, 3:7]) ** 2).mean() * 100
        tot, lt, lr = tot + (w_trans * tl + w_rot * rl), lt + tl, lr + rl
    enc = torch.cat([uvd, qn], -1).detach().clone()
    ident = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=enc.dtype)
    for b in range(B):
        enc[b * S] = ident
    return enc, torch.stack([tot / B, lt / B, lr / B])


def quat_raw_mul(a, b):
    """Hamilton product, (w, x, y, z) (rotation_conversions.py:398-417)."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def quat_mul(a, b):
    """quaternion_multiply: the raw product with w made non-negative. -> (product, raw w)."""
    ab = quat_raw_mul(a, b)
    return torch.where(ab[..., :1] < 0, -ab, ab), ab[..., 0]


def _conj(q):
    return q * torch.tensor([1, -1, -1, -1], dtype=q.dtype)


def pose_encode(R, T_uvz, focal, ratio, B, S):
    """comet_pose_encode = camera_to_pose_encoding2 (utils.py:631-688) for every sequence against its
    own frame 0: R [B*S, 4], T_uvz [B*S, 3], focal [B*S, 2] -> (enc [B*S, 8], raw product w)."""
    R, T, fl = R.double().reshape(B, S, 4), T_uvz.double().reshape(B, S, 3), focal.double().reshape(B, S, 2)
    ratio = float(ratio)
    q, w = quat_mul(R, _conj(R[:, :1]).expand(B, S, 4))
    enc = torch.zeros(B, S, 8, dtype=F64)
    enc[..., 0] = (T[..., 0] - T[:, :1, 0]) * ratio / 128.0
    enc[..., 1] = (T[..., 1] - T[:, :1, 1]) * ratio / 128.0
    enc[..., 2] = (T[..., 2] / T[:, :1, 2] - 1.0) * ratio
    enc[..., 3:7] = q
    enc[:, 0, :7] = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=F64)
    enc[..., 7] = fl[..., 0].clamp(0.1, 30.0)
    return enc.reshape(B * S, 8), w[:, 1:]


def pose_decode(enc, R_gt, T_gt, ratio, intr, B, S):
    """comet_pose_decode = pose_encoding_to_camera2 (utils.py:312-403) against frame 0 of each
    sequence's gt: enc [B*S, 7] -> (R [B*S, 4], T [B*S, 3], raw product w)."""
    fx, fy, cx, cy = intr
    ratio = float(ratio)
    e = enc.double().reshape(B, S, -1)
    q0 = R_gt.double().reshape(B, S, 4)[:, :1].expand(B, S, 4)
    t0 = T_gt.double().reshape(B, S, 3)[:, :1]
    u = t0[..., 0] + e[..., 0] / ratio * 128.0
    v = t0[..., 1] + e[..., 1] / ratio * 128.0
    dd = t0[..., 2] * (e[..., 2] / ratio + 1.0)
    T = torch.stack([(u - cx) * dd / fx, (v - cy) * dd / fy, dd], -1)
    q, w = quat_mul(e[..., 3:7], q0)
    return q.reshape(B * S, 4), T.reshape(B * S, 3), w


def pose_encode3(R, T, B, S):
    """comet_pose_encode3 = camera_to_pose_encoding3 (utils.py:591-627): (T_i - T_0, q_i * q_0^-1, 0),
    frame 0 = (0, 0, 0, 1, 0, 0, 0, 0); column 7 is padding. -> (enc [B*S, 8], raw product w)."""
    R, T = R.double().reshape(B, S, 4), T.double().reshape(B, S, 3)
    q, w = quat_mul(R, _conj(R[:, :1]).expand(B, S, 4))
    enc = torch.zeros(B, S, 8, dtype=F64)
    enc[..., :3] = T - T[:, :1]
    enc[..., 3:7] = q
    enc[:, 0, :7] = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=F64)
    return enc.reshape(B * S, 8), w[:, 1:]


def pose_decode3(enc, R_gt, T_gt, B, S):
    """comet_pose_decode3 = pose_encoding_to_camera3 (utils.py:270-310): R = dq * q_0, T = T_0 + dxyz."""
    e = enc.double().reshape(B, S, -1)
    q0 = R_gt.double().reshape(B, S, 4)[:, :1].expand(B, S, 4)
    T = T_gt.double().reshape(B, S, 3)[:, :1] + e[..., :3]
    q, w = quat_mul(e[..., 3:7], q0)
    return q.reshape(B * S, 4), T.reshape(B * S, 3), w


# ---- the inputs the GPU tests and the CPU pins share --------------------------------------------
def randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rand_dyadic(n, lo, hi, seed):
    """n x 2 float32 coordinates, multiples of 1/64 in [lo, hi]."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(int(lo * 64), int(hi * 64) + 1, (n, 2), generator=g).float() / 64.0


def sample_coords(H, W):
    """[2, 9, 2] pixel (x, y) for an H x W map: interior, exactly 0, exactly W-1 / H-1, negative,
    beyond the far edge and far out, every one a multiple of 1/64."""
    X, Y = float(W - 1), float(H - 1)
    c = [[(2.5, 1.75), (0.0, 0.0), (X, Y), (-0.75, 2.25), (3.25, -1.5), (X + 0.5, 1.0), (2.0, Y + 1.25),
          (500.0, -500.0), (-500.015625, 500.0)],
         [(0.0, Y), (X, 0.0), (X - 0.015625, Y - 0.015625), (0.015625, 0.015625), (-0.015625, Y + 0.015625),
          (X + 1.0, Y + 1.0), (-1.0, -1.0), (4.640625, 3.296875), (500.5, 2.0)]]
    return torch.tensor(c, dtype=torch.float32)


def patch_tracks(B, S, N, H, W, pradius, seed):
    """coarse [B, S, N, 2]: tracks whose patch origin is clamped on each of the four sides, one
    outside the frame on each axis and side, one in the W > H band, interior ones; the rest random.
    Multiples of 1/64, shuffled over (b, s, n) so that frame 0 holds fractional points too."""
    sp = [(1.5, 20.25), (H - 1.25, 10.5), (12.75, 2.0), (15.5, H - 0.5), (-3.25, 8.0), (W + 2.5, 9.0),
          (7.0, -2.75), (9.0, H + 3.5), (20.015625, 17.984375), (10.0, 10.0), (W - 2.0, 5.0), (0.0, 0.0)]
    n = B * S * N
    pts = torch.cat([torch.tensor(sp, dtype=torch.float32), rand_dyadic(n - len(sp), -4, H + 4, seed)])
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1))
    return pts[perm].reshape(B, S, N, 2).contiguous()


def score_inputs(B, S, N, P, C, seed):
    """(qfeat [B*N, C], pfeat [B*N, S, P, P, C], fine [B*N, S, 2]): unit-normal features (unit-std
    logits); window origins below the radius, above P - radius - 1, negative and beyond P on both
    axes, the rest random, all multiples of 1/64."""
    q = randn(B * N, C, seed=seed)
    pf = randn(B * N, S, P, P, C, seed=seed + 1)
    sp = [(0.5, 4.25), (4.0, 0.75), (P - 1.25, 3.5), (3.0, P - 1.5), (-1.25, 5.0), (5.5, -0.25), (P + 1.5, 2.0),
          (2.75, P + 0.5), (0.0, 0.0), (P - 1.0, P - 1.0), (-2.0, P + 2.0), (4.5, 4.5)]
    n = B * N * S
    fine = rand_dyadic(n, -2, P + 2, seed + 2)
    # flat (b s n) positions with s = 0 are never read: the special points go to positions that are
    m = torch.arange(n)
    read = m[(m // N) % S != 0]
    perm = torch.randperm(read.numel(), generator=torch.Generator().manual_seed(seed + 3))
    fine[read[perm[:len(sp)]]] = torch.tensor(sp, dtype=torch.float32)
    return q, pf, fine.reshape(B * N, S, 2).contiguous()


def unit_quats(n, seed):
    q = randn(n, 4, seed=seed)
    return q / q.norm(dim=-1, keepdim=True)


def codec_inputs(B, S, seed):
    """gt cameras for the pose codec: R [B*S, 4] unit quaternions of either sign of w, T_uvz with
    (u, v) within 100 px of (256, 256) and depth in [4, 6], T (xyz), focal lengths that include
    values below 0.1 and above 30, and a predicted encoding [B*S, 7]."""
    n = B * S
    g = torch.Generator().manual_seed(seed)
    R = unit_quats(n, seed + 1)
    uvz = torch.cat([256 + (torch.rand(n, 2, generator=g) * 200 - 100), 4 + 2 * torch.rand(n, 1, generator=g)], -1)
    xyz = randn(n, 3, seed=seed + 2)
    focal = 0.5 + 3 * torch.rand(n, 2, generator=g)
    focal[1, 0], focal[2, 0], focal[n - 1, 0], focal[n - 2, 0] = 0.05, 35.0, 0.0999, 30.5
    enc = torch.cat([randn(n, 3, seed=seed + 3, scale=0.3), unit_quats(n, seed + 4)], -1)
    return R, uvz, xyz, focal, enc


def gapr_inputs(B, S, seed):
    """(rot raw [B*S, 4] with row 3 all zero, uv, d, gt [B*S, 8] with identity frame-0 rows)."""
    n = B * S
    rot = randn(n, 4, seed=seed)
    rot[3] = 0.0
    uv, d = randn(n, 2, seed=seed + 1), randn(n, 1, seed=seed + 2)
    gt = torch.cat([randn(n, 3, seed=seed + 3, scale=0.5), unit_quats(n, seed + 4), torch.full((n, 1), 2.0)], -1)
    gt[::S, :7] = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float32)
    return rot, uv, d, gt.contiguous()
