"""The float64 restatements of tests/tracker_ref.py against oracle/comet_oracle.py (itself pinned to
the reference by tests/golden), at the shapes and inputs tests/test_tracker_ops_gpu.py uses: the GPU
tests' references are checked here, without a GPU. Discrete outputs compare exactly, floats to 1e-12
(the oracle is run with float64 as torch's default dtype, so its own constants are float64 too);
where the oracle itself rounds to float32 (`.float()` in camera_to_pose_encoding2, the float32
sin / cos of embed_2d) the bound is that rounding and says so. The conditions the GPU tests put on
their inputs (dyadic coordinates, score variances >= 1e-3, quaternion products with |w| >= 1e-3,
every clamp end reached) are asserted here on the references alone."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

import tracker_ref as TR
from oracle import comet_oracle as O

F64 = torch.float64


@contextlib.contextmanager
def f64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _eq12(a, b, what):
    err = (a.double() - b.double()).abs().max().item()
    assert err <= 1e-12 * max(1.0, b.double().abs().max().item()), f"{what}: {err:.3e}"


@pytest.mark.parametrize("H,W", [(5, 7), (1, 7)])
@pytest.mark.parametrize("C", [3, 64, 130])
def test_sample_bilinear_ref_is_the_oracles_sampler(H, W, C):
    fmap = TR.randn(2, H, W, C, seed=500)
    coords = TR.sample_coords(H, W)
    assert TR.dyadic(coords)
    nchw = fmap.double().permute(0, 3, 1, 2)
    with f64_default():
        want_b = O.sample_features4d(nchw, coords.double())
        want_z = O.bilinear_sampler(nchw, coords.double().unsqueeze(2), padding_mode="zeros")[..., 0].permute(0, 2, 1)
    _eq12(TR.sample_bilinear(fmap, coords, True), want_b, "border")
    _eq12(TR.sample_bilinear(fmap, coords, False), want_z, "zeros")
    # the expanded (stride 0) batch the position table is sampled with: the same map for every b
    ex = fmap[:1].expand(2, -1, -1, -1)
    got = TR.sample_bilinear(ex, coords, True)
    _eq12(got[1], TR.sample_bilinear(fmap[:1], coords[1:], True)[0], "expanded batch")
    # the edge cases are what they claim: exact corners return the corner pixel, far-out points the
    # border pixel (border) or zero (zeros)
    if H > 1:
        assert torch.equal(TR.sample_bilinear(fmap, coords, True)[0, 1], fmap[0, 0, 0].double())
        assert torch.equal(TR.sample_bilinear(fmap, coords, False)[0, 7], torch.zeros(C, dtype=F64))
        _eq12(TR.sample_bilinear(fmap, coords, True)[0, 7], fmap[0, 0, W - 1].double(), "far out, border")


@pytest.mark.parametrize("size", [(6, 10), (3, 5), (11, 7), (1, 1)])
def test_images_nhwc_ref_is_align_corners_interpolation(size):
    n, H, W = 2, 6, 10
    oh, ow = size
    x = TR.randn(n, 3, H, W, seed=510)
    ref = TR.images_nhwc(x, oh, ow, 8)
    assert (ref[..., 3:] == 0).all()
    want = torch.zeros(n, oh, ow, 3, dtype=F64)
    xd = x.double()
    for oy in range(oh):
        for ox in range(ow):
            fy = oy * (H - 1) / (oh - 1) if oh > 1 else 0.0
            fx = ox * (W - 1) / (ow - 1) if ow > 1 else 0.0
            y0, x0 = min(int(fy), H - 1), min(int(fx), W - 1)
            y1, x1 = min(y0 + 1, H - 1), min(x0 + 1, W - 1)
            ly, lx = fy - y0, fx - x0
            want[:, oy, ox] = ((1 - ly) * ((1 - lx) * xd[:, :, y0, x0] + lx * xd[:, :, y0, x1]) +
                               ly * ((1 - lx) * xd[:, :, y1, x0] + lx * xd[:, :, y1, x1]))
    _eq12(ref[..., :3], want, f"images_nhwc {size}")
    if size == (H, W):
        assert torch.equal(ref[..., :3], xd.permute(0, 2, 3, 1))
    with f64_default():  # the oracle's own resize call (comet_forward, image_features)
        _eq12(ref[..., :3], F.interpolate(xd, size, mode="bilinear", align_corners=True).permute(0, 2, 3, 1), "interpolate")


@pytest.mark.parametrize("ldc", [588, 640])
def test_dino_prep_ref_feeds_the_patch_embed_convolution(ldc):
    """cols @ flatten(weight)^T is the patch_embed convolution of the oracle (dinov2) on the image
    the oracle prepares (image_features: resize, ImageNet normalisation)."""
    BS, H, W, R, p = 2, 9, 13, 28, 14
    x = TR.randn(BS, 3, H, W, seed=520).abs()
    mean, std = O.RESNET_MEAN.reshape(3), O.RESNET_STD.reshape(3)
    cols = TR.dino_prep(x, R, p, ldc, mean, std)
    assert (cols[:, 3 * p * p:] == 0).all()
    w = TR.randn(5, 3, p, p, seed=521, scale=1.0 / math.sqrt(3 * p * p)).double()
    with f64_default():
        xi = F.interpolate(x.double(), (R, R), mode="bilinear", align_corners=True)
        xi = (xi - O.RESNET_MEAN.double()) / O.RESNET_STD.double()
        want = F.conv2d(xi, w, None, stride=p).flatten(2).transpose(1, 2).reshape(-1, 5)
    _eq12(cols[:, :3 * p * p] @ w.reshape(5, -1).t(), want, "patch embed")


@pytest.mark.parametrize("H,W", [(40, 40), (36, 44)])
def test_patch_gather_and_refine_combine_refs_are_refine_tracks(H, W, monkeypatch):
    """O.refine_track with its encoder, fine tracker and score stubbed out: the patches it cuts, the
    query points it hands the fine tracker and the way it puts the result back together."""
    B, S, N, pr = 2, 3, 5, 3
    P = 2 * pr + 1
    images = TR.randn(B, S, 3, H, W, seed=530)
    coarse = TR.patch_tracks(B, S, N, H, W, pr, seed=531)
    assert TR.dyadic(coarse)
    tl = coarse.floor().int() - pr
    lim = H - P
    for ax in range(2):  # every clamp end, on both axes; a point outside the frame on both sides
        assert (tl[..., ax] < 0).any() and (tl[..., ax] > lim).any()
        assert (coarse[..., ax] < 0).any() and (coarse[..., ax] > (W, H)[ax]).any()
    fine = TR.randn(B * N, S, 2, seed=532, scale=3.0).double() + pr
    seen = {}

    def enc(x, P_, name):
        seen["patch_in"] = x
        return x[:, :2]

    def trk(pq, feat, *a):
        seen["pq"] = pq
        return [fine.reshape(B * N, S, 1, 2)], None, None, torch.zeros(B, N, 2)

    monkeypatch.setattr(O, "shallow_encoder", enc)
    monkeypatch.setattr(O, "tracker_predictor", trk)
    monkeypatch.setattr(O, "compute_score", lambda *a: torch.zeros(B, S, N))
    with f64_default():
        refined, _ = O.refine_track(images.double(), None, coarse.double(), pradius=pr)
    patches, topleft, query = TR.patch_gather(images, coarse, pr, 4)
    assert torch.equal(topleft, tl)
    assert (patches[..., 3:] == 0).all()
    bsn = patches[..., :3].reshape(B, N, S, P, P, 3).permute(0, 2, 1, 5, 3, 4).reshape(B * S * N, 3, P, P)
    assert torch.equal(bsn, seen["patch_in"]), "patch values / (b n s) order"
    assert torch.equal(query, seen["pq"].reshape(B * N, 2)), "query points"
    assert torch.equal(TR.refine_combine(fine, topleft, coarse.double()), refined), "refine_combine"
    # frame 0 of the result is the coarse query point itself
    assert torch.equal(refined[:, 0], coarse[:, 0].double())


def test_coords_update_ref_is_the_predictors_update():
    """base_track_predictor.py:247-254 as oracle.tracker_predictor states it ([B, S, N, 2] there)."""
    B, N, S = 2, 5, 3
    coords = TR.randn(B, N, S, 2, seed=540, scale=10.0)
    delta = TR.randn(B * N * S, 2, seed=541)
    for scale in (8.0, 0.3):
        c = coords.double().permute(0, 2, 1, 3).clone()
        backup = c.clone()
        c = c + delta.double().reshape(B, N, S, 2).permute(0, 2, 1, 3)
        c[:, 0] = backup[:, 0]
        new, preds = TR.coords_update(coords, delta, scale)
        assert torch.equal(new.permute(0, 2, 1, 3), c)
        assert torch.equal(preds, c * scale)
        assert torch.equal(new[:, :, 0], coords[:, :, 0].double())


TOKEN_SHAPES = [(128, 405, 664), (32, 147, 216), (6, 9, 24), (6, 9, 23)]


def token_inputs(latent, corrdim, tdim, B=2, N=5, S=3):
    rows = B * N * S
    base = TR.randn(B * N, 1, 2, seed=550, scale=30.0)
    flow = (torch.rand(B * N, S, 2, generator=torch.Generator().manual_seed(551)) * 40 - 20)
    flow[:, 0] = 0
    coords = (base + flow).reshape(rows, 2).contiguous()
    feats = TR.randn(rows, latent, seed=552)
    corr = TR.randn(rows, corrdim + 4, seed=553)
    pos = TR.randn(B * N, tdim, seed=554)
    return coords, feats, corr, pos


@pytest.mark.parametrize("latent,corrdim,tdim", TOKEN_SHAPES)
def test_tracker_tokens_ref_is_the_predictors_token_assembly(latent, corrdim, tdim):
    B, N, S = 2, 5, 3
    coords, feats, corr, pos = token_inputs(latent, corrdim, tdim)
    ref = TR.tracker_tokens(coords, feats, latent, corr[:, :corrdim], corrdim, pos, tdim, S)
    E = latent // 2
    c3 = coords.reshape(B * N, S, 2)
    flows = c3 - c3[:, :1]  # float32, as the reference forms it
    assert flows.abs().max() > 15, "flows must reach the large-argument range"
    if E % 2 == 0:
        emb = O.embed_2d(flows, E)  # float32 arguments, float32 sin / cos
    else:  # get_2d_embedding needs an even width; the kernel's definition for an odd one, column by column
        k = torch.arange(E)
        div = (k - k % 2).float() * (torch.tensor(1000.0) / torch.tensor(float(E)))
        arg = flows[..., None] * div  # [BN, S, 2, E]
        emb = torch.where(k % 2 == 1, torch.cos(arg), torch.sin(arg)).reshape(B * N, S, 2 * E)
    x = torch.cat([emb, flows, corr[:, :corrdim].reshape(B * N, S, -1), feats.reshape(B * N, S, -1)], dim=2)
    x = torch.cat([x, torch.zeros(B * N, S, tdim - x.shape[2])], dim=2)
    want = (x + pos.reshape(B * N, 1, tdim)).reshape(B * N * S, tdim).double()
    # the oracle's sin / cos and its final add are float32: 1 ulp at magnitude 1 for the embedding
    # (a float64 ARGUMENT would differ by ~2e-3 here), one rounding of the sum everywhere
    err = (ref - want).abs()
    assert (err[:, :2 * E] <= 2.0 ** -23 + 2.0 ** -23 * want[:, :2 * E].abs()).all(), err[:, :2 * E].max()
    assert (err[:, 2 * E:] <= 2.0 ** -23 * want[:, 2 * E:].abs()).all(), err[:, 2 * E:].max()


SCORE_CASES = [(32, 2), (32, 1), (12, 2), (12, 1)]


@pytest.mark.parametrize("C,sradius", SCORE_CASES)
@pytest.mark.parametrize("bf16", [False, True])
def test_track_score_ref_is_compute_score_fn(C, sradius, bf16):
    B, S, N, P = 2, 4, 5, 9
    q, pf, fine = TR.score_inputs(B, S, N, P, C, seed=560 + C)
    if bf16:
        pf = pf.to(torch.bfloat16)
    assert TR.dyadic(fine)
    score, inv, var = TR.track_score(q, pf, fine, B, S, N, sradius)
    # conditioning of the comparison: every variance far above the 1e-10 clamp
    assert var.min().item() >= 1e-3, var.min().item()
    # both clamp ends on both axes, among the positions that are read
    m = torch.arange(B * S * N)
    rd = fine.reshape(-1, 2)[m[(m // N) % S != 0]]
    t = rd.floor() - sradius
    for ax in range(2):
        assert (t[:, ax] < 0).any() and (t[:, ax] > P - 2 * sradius - 1).any()
        assert (rd[:, ax] < 0).any() and (rd[:, ax] > P).any()
    with f64_default():
        want = O.compute_score(q.double().reshape(B, N, C), pf.double().permute(0, 1, 4, 2, 3),
                               fine.double().reshape(B * N, S, 1, 2), sradius, P, B, N, S, C)
        winv = 1.0 / (want + 1e-6)
        winv = winv / winv.max(dim=1, keepdim=True)[0]
    _eq12(score, want, "score")
    _eq12(inv, winv, "inv score")
    assert (score[:, 0] == 1).all()


@pytest.mark.parametrize("cols", [1, 63, 200])
def test_rowscale_refs_are_autograd(cols):
    x = TR.randn(7, cols, seed=570).double().requires_grad_(True)
    w = TR.randn(7, seed=571).double().requires_grad_(True)
    dy = TR.randn(7, cols, seed=572).double()
    y = x * w[:, None]
    y.backward(dy)
    _eq12(TR.rowscale(x.detach(), w.detach()), y.detach(), "rowscale")
    dx, dw = TR.rowscale_bwd(x.detach(), w.detach(), dy)
    _eq12(dx, x.grad, "dx")
    _eq12(dw, w.grad, "dw")


@pytest.mark.parametrize("B,S", [(2, 5), (20, 16)])
def test_gapr_ref_is_the_oracles_head_tail_and_pose_loss(B, S):
    rot, uv, d, gt = (t.double() for t in TR.gapr_inputs(B, S, seed=580))
    assert (rot[3] == 0).all() and 3 % S != 0
    assert torch.equal(gt[::S, :7], torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=F64).expand(B, 7))
    rot.requires_grad_(True)
    enc, losses = TR.gapr(rot, uv, d, gt, B, S)
    with f64_default():
        qn = F.normalize(rot.detach(), p=2, dim=-1, eps=1e-8)  # camera_head's last line
        uvd = torch.cat([uv, d], -1).reshape(B, S, 3)
        want = O.pose_loss(uvd, qn.reshape(B, S, 4), [gt[b * S:(b + 1) * S] for b in range(B)])
        e = torch.cat([uvd.clone(), qn.reshape(B, S, 4).clone()], -1)  # camera_predictor's frame-0 reset
        e[:, 0, :3] = 0
        e[:, 0, 3:] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    _eq12(losses.detach(), torch.stack(want), "losses")
    assert torch.equal(enc, e.reshape(-1, 7))
    # the all-zero quaternion takes F.normalize's 1e-8 clamp: qn = 0 and d qn / d rot = I / 1e-8
    up = torch.tensor([1.0, 0.5, -0.25], dtype=F64)
    (g,) = torch.autograd.grad((losses * up).sum(), rot)
    cr = (up[0] * 2.0 + up[2]) * 100 * 2 / (4 * (S - 1) * B)
    _eq12(g[3], cr * (0 - gt[3, 3:7]) / 1e-8, "zero-row gradient")
    assert (g[::S] == 0).all(), "frame 0 carries no loss"


def test_pose_codec_refs_are_the_oracles_encodings():
    B, S = 3, 4
    R, uvz, xyz, focal, enc = TR.codec_inputs(B, S, seed=590)
    ratio = 1.37
    assert focal[:, 0].min() < 0.1 and focal[:, 0].max() > 30
    e2, w2 = TR.pose_encode(R, uvz, focal, ratio, B, S)
    e3, w3 = TR.pose_encode3(R, xyz, B, S)
    intr = O.INTRINSICS["AMD_eval"]
    q2, T2, wd2 = TR.pose_decode(enc, R, uvz, ratio, intr, B, S)
    q3, T3, wd3 = TR.pose_decode3(enc, R, xyz, B, S)
    # the sign canonicalisation is never a coin toss
    for w in (w2, w3, wd2, wd3, R[:, 0]):
        assert w.abs().min().item() >= 1e-3, w.abs().min().item()
    with f64_default():
        Rd, ud, xd, fd, ed = R.double(), uvz.double(), xyz.double(), focal.double(), enc.double()
        for b in range(B):
            r = slice(b * S, (b + 1) * S)
            want = O.camera_to_pose_encoding2(Rd[r], ud[r], fd[r], ratio)
            # the oracle stores (du, dv, dd) through .float(): its own float32 rounding bounds them
            assert ((e2[r, :3] - want[:, :3]).abs() <= 2.0 ** -23 * want[:, :3].abs()).all()
            _eq12(e2[r, 3:], want[:, 3:], "encoding 2 quaternion / focal")
            want3 = O.camera_to_pose_encoding3(Rd[r], xd[r])
            _eq12(e3[r, :7], want3, "encoding 3")
            assert (e3[r, 7] == 0).all()
            q, T, _ = O.pose_encoding_to_camera2(torch.cat([ed[r], fd[r, :1]], -1), Rd[b * S], ud[b * S], ratio, "AMD_eval")
            _eq12(q2[r], q, "decode 2 R")
            _eq12(T2[r], T, "decode 2 T")
            q, T, _ = O.pose_encoding_to_camera3(ed[r], Rd[b * S], xd[b * S])
            _eq12(q3[r], q, "decode 3 R")
            _eq12(T3[r], T, "decode 3 T")
    # encode -> decode returns the cameras (R up to the w >= 0 canonical sign)
    fx, fy, cx, cy = intr
    qa, Ta, _ = TR.pose_decode(e2[:, :7], R, uvz, ratio, intr, B, S)
    canon = torch.where(R[:, :1] < 0, -R, R).double()
    # q * q0^-1 * q0 = q * |q0|^2, and a float32 unit quaternion has |q0|^2 = 1 +- 2^-22
    assert ((qa - canon).abs() <= 2.0 ** -22).all() and ((TR.pose_decode3(e3[:, :7], R, xyz, B, S)[0] - canon).abs() <= 2.0 ** -22).all()
    u, v, z = uvz.double().unbind(-1)
    _eq12(Ta, torch.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], -1), "round trip T")
    _eq12(TR.pose_decode3(e3[:, :7], R, xyz, B, S)[1], xyz.double(), "round trip T (3)")
