"""Kernel-level parity of the tracker and camera-head glue kernels (csrc/tracker.hip, csrc/head.hip)
with the float64 restatements of tests/tracker_ref.py, which tests/test_tracker_ref_cpu.py ties to
the oracle: clamping at every border, the (b s n) <-> (b n s) re-orderings, frame-0 pinning, strided
and expanded operands, padding, row counts that do not fill the last workgroup.

Every coordinate fed to a kernel that takes floor() of it is a multiple of 1/64 below 1024, so
float32 and float64 agree on floor and fraction and no case is left out of any comparison.

Tolerances: exact equality for integers, copies, layouts, pinned rows, padding and sentinels; bf16
outputs within 1 bf16 ulp of the float64 reference rounded to bf16; f32 interpolation within
1e-4 * max|ref| (src_index loses a few ulp of the map size, <~ 1e-5 px, times a gradient of at most
2 max|v|; the bound of test_corr_sample_vs_f64); scores 1e-4 / 1e-5, losses 1e-4, gt encodings 1e-6
as tests/test_model_gpu.py. Each test's docstring gives the error measured on an MI355X."""
import numpy as np
import pytest
import torch

import tracker_ref as TR
from oracle import comet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.0


def _ops():
    from comet_amd import ops
    return ops


def _rand(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _close(got, ref, rtol, atol, what=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = (err > tol)
    print(f"[measured] {what}: max err {err.max().item():.3e}, min slack x{(tol / err.clamp_min(1e-300)).min().item():.3g}")
    assert not bad.any(), f"{what}: max err {err.max().item():.3e} (ref max {ref.abs().max().item():.3e}), {bad.sum().item()} bad"


def _bf16_close(got, ref, atol32, what=""):
    """got (bf16) within 1 bf16 ulp of the float64 reference rounded to bf16. Where the float32
    value the kernel rounds may itself be off by atol32 (a sum near zero), a bf16 ulp finer than
    that cannot be asked for: the ulp is floored at atol32."""
    assert got.dtype == torch.bfloat16
    g = got.detach().double().cpu()
    r = TR.bf16_round(ref)
    ulp = torch.maximum(TR.bf16_ulp(torch.maximum(g.abs(), r.abs())), torch.full_like(r, atol32))
    err = (g - r).abs()
    print(f"[measured] {what}: max err {(err / ulp).max().item():.3g} bf16 ulp, {(err > 0).sum().item()} of {err.numel()} differ")
    assert (err <= ulp).all(), f"{what}: {(err / ulp).max().item():.3g} bf16 ulp"


INTERP_F32 = 2.0 ** -21  # eight float32 roundings on values up to max|ref|: the float32 slack under a bf16 ulp


def _interp_close(got, ref, what):
    _close(got, ref, 0.0, 1e-4 * ref.abs().max().item(), what)


# ---- sample_bilinear -----------------------------------------------------------------------------
@pytest.mark.parametrize("border", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [3, 64, 130])
def test_sample_bilinear_vs_grid_sample_f64(C, dtype, border):
    """comet_sample_bilinear on a [2, 5, 7, C] map, 9 rows per batch (18 waves: the last workgroup is
    partial): interior points, exactly 0 and W-1 / H-1, negative, beyond the far edge and +-500; `out`
    a column view of a wider sentinel buffer; an expanded (stride 0) batch; an H = 1 map.
    Measured: max err 3.8e-7 = 1.4e-7 * max|ref| (bound 1e-4 * max|ref|), the same for bf16 maps."""
    ops = _ops()
    for H, W in ((5, 7), (1, 7)):
        fmap = _rand(2, H, W, C, seed=500).to(dtype)
        coords = TR.sample_coords(H, W)
        assert TR.dyadic(coords)
        ref = TR.sample_bilinear(fmap, coords, border)
        buf = torch.full((2, 9, C + 5), SENT, device=DEV)
        out = buf[:, :, 2:2 + C]
        ops.sample_bilinear(fmap.to(DEV), coords.to(DEV), border=border, out=out)
        _interp_close(out, ref, f"sample C={C} {dtype} border={border} H={H}")
        assert (buf[:, :, :2] == SENT).all() and (buf[:, :, 2 + C:] == SENT).all(), "wrote outside its columns"
        assert not (out == SENT).any(), "left output columns unwritten"
    # one map for every batch entry (stride 0), as the position table is sampled
    fmap = _rand(1, 5, 7, C, seed=501).to(dtype)
    coords = TR.sample_coords(5, 7)
    ex = fmap.to(DEV).expand(2, -1, -1, -1)
    assert ex.stride(0) == 0
    got = ops.sample_bilinear(ex, coords.to(DEV), border=border)
    _interp_close(got, TR.sample_bilinear(fmap.expand(2, -1, -1, -1), coords, border), f"sample expanded C={C}")


# ---- images_nhwc ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cpad", [3, 4, 8])
@pytest.mark.parametrize("size", [(6, 10), (3, 5), (11, 7), (1, 1)])
def test_images_nhwc_vs_interpolate_f64(size, cpad, dtype):
    """comet_images_nhwc: [2, 3, 6, 10] to the identity size (a copy), (3, 5), (11, 7), (1, 1); pad
    channels exactly zero. Measured: f32 max err 6.7e-8 = 3.0e-8 * max|ref| (bound 1e-4 * max|ref|); bf16
    equal to the rounded reference everywhere (bound 1 ulp)."""
    ops = _ops()
    oh, ow = size
    x = _rand(2, 3, 6, 10, seed=510)
    ref = TR.images_nhwc(x, oh, ow, cpad)
    got = ops.images_nhwc(x.to(DEV), oh, ow, dtype, cpad=cpad)
    assert got.shape == (2, oh, ow, cpad) and got.dtype == dtype
    assert (got[..., 3:] == 0).all(), "pad channels"
    if dtype == torch.float32:
        if size == (6, 10):
            assert torch.equal(got[..., :3].cpu(), x.permute(0, 2, 3, 1)), "identity size is a copy"
        _interp_close(got[..., :3], ref[..., :3], f"images_nhwc {size} cpad={cpad}")
    else:
        _bf16_close(got, ref, INTERP_F32 * ref.abs().max().item(), f"images_nhwc bf16 {size} cpad={cpad}")


# ---- dino_prep -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ldc", [588, 640])
def test_dino_prep_vs_f64(ldc, dtype):
    """comet_dino_prep: [2, 3, 9, 13] -> 28 x 28 -> ImageNet normalisation -> 14 x 14 patch rows in
    (ci, ky, kx) column order, pad columns exactly zero. Measured: f32 max err 1.9e-6 = 1.8e-7 * max|ref| (bound
    1e-4 * max|ref|); bf16 equal to the rounded reference everywhere (bound 1 ulp)."""
    ops = _ops()
    BS, H, W, R, p = 2, 9, 13, 28, 14
    x = _rand(BS, 3, H, W, seed=520).abs()
    mean = torch.tensor([0.485, 0.456, 0.406])
    std = torch.tensor([0.229, 0.224, 0.225])
    ref = TR.dino_prep(x, R, p, ldc, mean, std)
    md, sd = mean.to(DEV), std.to(DEV)  # as models/dinov2.py passes them
    torch.cuda.synchronize()
    got = ops.dino_prep(x.to(DEV), R, p, ldc, md, sd, dtype)
    kk = 3 * p * p
    assert got.shape == (BS * 4, ldc) and got.dtype == dtype
    assert (got[:, kk:] == 0).all(), "pad columns"
    if dtype == torch.float32:
        _interp_close(got[:, :kk], ref[:, :kk], f"dino_prep ldc={ldc}")
    else:
        _bf16_close(got, ref, INTERP_F32 * ref.abs().max().item(), f"dino_prep bf16 ldc={ldc}")


# ---- patch_gather / refine_combine / coords_update ------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cpad", [3, 4, 8])
@pytest.mark.parametrize("H,W", [(40, 40), (36, 44)])
def test_patch_gather_exact(H, W, cpad, dtype):
    """comet_patch_gather, B = 2, S = 3, N = 5, 7 x 7 patches: origins clamped on all four sides,
    tracks outside the frame, the W > H band (x is clamped with H, the reference's contract). Patches
    equal the image values (or their bf16 rounding) in (b, n, s) order, topleft is the unclamped
    integer origin, query the frame-0 fraction + radius: all exact."""
    ops = _ops()
    B, S, N, pr = 2, 3, 5, 3
    images = _rand(B, S, 3, H, W, seed=530)
    coarse = TR.patch_tracks(B, S, N, H, W, pr, seed=531)
    assert TR.dyadic(coarse) and W >= H
    rp, rt, rq = TR.patch_gather(images, coarse, pr, cpad)
    patches, topleft, query = ops.patch_gather(images.to(DEV), coarse.to(DEV), pr, dtype, cpad=cpad)
    assert patches.shape == (B * N * S, 7, 7, cpad) and patches.dtype == dtype
    want = rp if dtype == torch.float32 else TR.bf16_round(rp)
    assert torch.equal(patches.double().cpu(), want), "patch values / order / pad channels"
    assert torch.equal(topleft.cpu(), rt), "topleft"
    assert torch.equal(query.double().cpu(), rq), "query"


def test_refine_combine_exact():
    """comet_refine_combine, B = 2, S = 3, N = 5, negative topleft entries: frame 0 is the coarse
    query bit for bit, the other frames the float32 sum fine[(b n), s] + topleft[b, s, n] bit for bit."""
    ops = _ops()
    B, S, N = 2, 3, 5
    fine = _rand(B * N, S, 2, seed=532, scale=3.0) + 3
    topleft = torch.randint(-20, 40, (B, S, N, 2), generator=torch.Generator().manual_seed(533), dtype=torch.int32)
    assert (topleft < 0).any()
    coarse = _rand(B, S, N, 2, seed=534, scale=20.0)
    got = ops.refine_combine(fine.to(DEV), topleft.to(DEV), coarse.to(DEV), B, S, N).cpu()
    assert torch.equal(got[:, 0], coarse[:, 0]), "frame 0"
    assert torch.equal(got, TR.refine_combine(fine, topleft, coarse)), "fine + topleft in (b, s, n) order"


@pytest.mark.parametrize("with_preds", [True, False])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_coords_update_vs_f64(dtype, with_preds):
    """comet_coords_update, B = 2, N = 5, S = 3, delta = the first two columns of a [rows, 34] matrix,
    scales 8 and float32(0.3): frame-0 rows unchanged bit for bit, preds in [B, S, N, 2] order.
    One float32 add and one multiply: rtol 2^-22 = 2.4e-7. Measured: coords 6.0e-8, preds 7.7e-8
    relative: one and two float32 roundings, which is all the bound allows for (hence within 4x of it)."""
    ops = _ops()
    B, N, S = 2, 5, 3
    rows = B * N * S
    coords0 = _rand(B, N, S, 2, seed=540, scale=10.0)
    delta = _rand(rows, 34, seed=541).to(dtype)
    for scale in (8.0, float(np.float32(0.3))):
        coords = coords0.clone().to(DEV)
        preds = torch.full((B, S, N, 2), SENT, device=DEV) if with_preds else None
        ops.coords_update(coords, delta.to(DEV), preds, scale, B, N, S)
        new, rp = TR.coords_update(coords0, delta[:, :2], scale)
        assert torch.equal(coords[:, :, 0].cpu(), coords0[:, :, 0]), "frame 0 moved"
        _close(coords, new, 2.0 ** -22, 0.0, f"coords {dtype} scale={scale}")
        if with_preds:
            _close(preds, rp, 2.0 ** -22, 0.0, f"preds {dtype} scale={scale}")


# ---- tracker_tokens ------------------------------------------------------------------------------
# (latent, corrdim, tdim): the coarse and fine trackers' shapes; odd E = 3 on the one-wave-per-row
# kernel with its sin / cos pairing off; tdim % 4 != 0 (the row-blocked kernel by default)
TOKEN_SHAPES = [(128, 405, 664), (32, 147, 216), (6, 9, 24), (6, 9, 23)]
TOK_ATOL = 2.0 ** -22  # 2 ulp of sinf / cosf / sincosf at magnitude 1
TOK_RTOL = 2.0 ** -23  # the float32 rounding of the final sum


def _token_inputs(latent, corrdim, tdim, B=2, N=5, S=3):
    rows = B * N * S
    base = _rand(B * N, 1, 2, seed=550, scale=30.0)
    flow = (torch.rand(B * N, S, 2, generator=torch.Generator().manual_seed(551)) * 40 - 20)
    flow[:, 0] = 0
    coords = (base + flow).reshape(rows, 2).contiguous()
    return coords, _rand(rows, latent, seed=552), _rand(rows, corrdim + 4, seed=553), _rand(B * N, tdim, seed=554)


@pytest.mark.parametrize("variant", ["default", "COMET_TOKENS_ROWS", "COMET_TOKENS_FLAT"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("latent,corrdim,tdim", TOKEN_SHAPES)
def test_tracker_tokens_vs_definition(latent, corrdim, tdim, dtype, variant, monkeypatch):
    """comet_tracker_tokens against the definition, 30 rows (not a multiple of 4), flows up to +-20 px
    (sin / cos arguments to ~2e4, formed in float32 as the kernel forms them and evaluated in float64),
    corr a strided column view, every kernel variant against the same reference; x pre-filled with a
    sentinel. Measured: f32 max err 9.5e-7 on sums of magnitude ~6, 2.5x
    inside 2^-22 + 2^-23 |ref| (the bound is two ulp of the function plus one rounding of the sum, so a
    correct kernel sits within a small factor of it); bf16 equal to the rounded reference everywhere."""
    ops = _ops()
    S = 3
    coords, feats, corr, pos = _token_inputs(latent, corrdim, tdim)
    rows = coords.shape[0]
    ref = TR.tracker_tokens(coords, feats, latent, corr[:, :corrdim], corrdim, pos, tdim, S)
    cd = corr.to(DEV)[:, :corrdim]
    assert cd.stride(0) == corrdim + 4
    if variant != "default":
        monkeypatch.setenv(variant, "1")
    x = torch.full((rows, tdim), SENT, device=DEV, dtype=dtype)
    ops.tracker_tokens(coords.to(DEV), feats.to(DEV), latent, cd, corrdim, pos.to(DEV), tdim, x, rows, S)
    if dtype == torch.float32:
        _close(x, ref, TOK_RTOL, TOK_ATOL, f"tokens {(latent, corrdim, tdim)} {variant}")
    else:
        _bf16_close(x, ref, TOK_ATOL, f"tokens bf16 {(latent, corrdim, tdim)} {variant}")
    if dtype == torch.float32:  # the zero-flow frame-0 rows: embedding (sin 0, cos 0, ..) = (0, 1, ..), flow 0
        E = latent // 2
        r0 = x[::S, :2 * E + 2].double().cpu() - pos[:, :2 * E + 2].double()
        want0 = torch.cat([((torch.arange(2 * E) % E) % 2).double(), torch.zeros(2)])
        assert (r0 - want0).abs().max() <= 2.0 ** -21  # the rounding of the sum with |pos| < 8


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tracker_tokens_padded_rows(dtype):
    """Rows padded to the consuming GEMM's k-tile (ldx = 256 > tdim = 216): the same tdim columns,
    exact zeros after them, nothing of the sentinel left."""
    ops = _ops()
    latent, corrdim, tdim, S, ldx = 32, 147, 216, 3, 256
    coords, feats, corr, pos = _token_inputs(latent, corrdim, tdim)
    rows = coords.shape[0]
    ref = TR.tracker_tokens(coords, feats, latent, corr[:, :corrdim], corrdim, pos, tdim, S)
    x = torch.full((rows, ldx), SENT, device=DEV, dtype=dtype)
    ops.tracker_tokens(coords.to(DEV), feats.to(DEV), latent, corr.to(DEV)[:, :corrdim], corrdim, pos.to(DEV), tdim, x,
                       rows, S)
    assert (x[:, tdim:] == 0).all(), "pad columns"
    if dtype == torch.float32:
        _close(x[:, :tdim], ref, TOK_RTOL, TOK_ATOL, "padded tokens")
    else:
        _bf16_close(x[:, :tdim], ref, TOK_ATOL, "padded tokens bf16")


# ---- track_score ---------------------------------------------------------------------------------
@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,sradius", [(32, 2), (32, 1), (12, 2), (12, 1)])
def test_track_score_vs_compute_score_fn(C, sradius, dtype, serial, monkeypatch):
    """comet_track_score against the restatement of compute_score_fn (feature map = patch (s=0, n=0)
    of the sequence, window origins read at the flat (b s n) position of the (b n, s) track, both clamp
    ends on both axes, 1 / (s + 1e-6) normalised by the per-track maximum). B = 2, S = 4, N = 5, P = 9;
    C = 12 takes the serial kernel, C = 32 the parallel one unless COMET_SCORE_SERIAL is set.
    Every reference variance is >= 1e-3 (asserted). Measured: score max err 2.2e-7, inv score 1.4e-7
    (bound 1e-4 |ref| + 1e-5, more than 600x above)."""
    ops = _ops()
    B, S, N, P = 2, 4, 5, 9
    q, pf, fine = TR.score_inputs(B, S, N, P, C, seed=560 + C)
    pf = pf.to(dtype)
    assert TR.dyadic(fine)
    rs, ri, var = TR.track_score(q, pf, fine, B, S, N, sradius)
    assert var.min().item() >= 1e-3
    if serial:
        monkeypatch.setenv("COMET_SCORE_SERIAL", "1")
    score, inv = ops.track_score(q.to(DEV), pf.to(DEV), fine.to(DEV), B, S, N, sradius)
    assert (score[:, 0] == 1).all()
    _close(score, rs, 1e-4, 1e-5, f"score C={C} r={sradius} {dtype} serial={serial}")
    _close(inv, ri, 1e-4, 1e-5, f"inv score C={C} r={sradius} {dtype} serial={serial}")


# ---- rowscale ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cols", [1, 63, 200])
def test_rowscale_fwd_bwd_vs_f64(cols, dtype):
    """comet_rowscale_fwd / _bwd, 7 rows (two workgroups of 4 waves, the second partial), every
    need_dx / need_dw combination. One product per element (rtol 2^-23) and a float32 sum of `cols`
    products for dw (atol cols * 2^-23 * max|dy x|). Measured: y / dx rel err 5.9e-8 (the half ulp of the one
    product, 2x inside its bound by construction), dw 3.3e-6 (6.9x inside); bf16 y equal to the rounded
    reference everywhere."""
    ops = _ops()
    rows = 7
    x = _rand(rows, cols, seed=570).to(dtype)
    w = _rand(rows, seed=571)
    dy = _rand(rows, cols, seed=572)
    y = ops.rowscale(x.to(DEV), w.to(DEV))
    if dtype == torch.float32:
        _close(y, TR.rowscale(x, w), 2.0 ** -23, 0.0, f"rowscale cols={cols}")
    else:
        _bf16_close(y, TR.rowscale(x, w), 0.0, f"rowscale bf16 cols={cols}")
    rdx, rdw = TR.rowscale_bwd(x, w, dy)
    for need_dx, need_dw in ((True, True), (True, False), (False, True), (False, False)):
        dx, dw = ops.rowscale_bwd(x.to(DEV), w.to(DEV), dy.to(DEV), need_dx, need_dw)
        assert (dx is None) == (not need_dx) and (dw is None) == (not need_dw)
        if need_dx:
            _close(dx, rdx, 2.0 ** -23, 0.0, f"rowscale dx cols={cols} {dtype}")
        if need_dw:
            _close(dw, rdw, 2.0 ** -23, cols * 2.0 ** -23 * (dy.double() * x.double()).abs().max().item(),
                   f"rowscale dw cols={cols} {dtype}")


# ---- GAPR ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(2, 5), (20, 16)])
def test_gapr_fwd_bwd_vs_f64_autograd(B, S):
    """functional.gapr against float64 autograd of the restatement: 10 rows and 320 rows (more than
    the single block's 256 threads: its strided loop and tree reduction), one all-zero raw quaternion
    (the 1e-8 clamp branch of both passes), upstream gradients on all three losses, frame-0 rows of
    enc forced to identity. Losses rtol / atol 1e-4 (tests/test_model_gpu.py); enc: copies exact,
    normalised quaternions 2^-22; gradients 2e-6 * max|ref| (about ten float32 operations each), the
    zero row's (scaled by 1e8) relative to its own size. Measured: losses 8.6e-6 (1500x inside), qn 9.3e-8
    (2.6x inside 2^-22: a square root and a division), drot 3.3e-7 * max|ref| (6.1x inside), duv and dd
    20x inside, the zero row 32x inside."""
    from comet_amd import functional as Fn
    rot, uv, d, gt = TR.gapr_inputs(B, S, seed=580)
    up = torch.tensor([1.0, 0.5, -0.25])
    r64, u64, d64 = (t.double().requires_grad_(True) for t in (rot, uv, d))
    renc, rl = TR.gapr(r64, u64, d64, gt.double(), B, S)
    rg = torch.autograd.grad((rl * up.double()).sum(), (r64, u64, d64))
    rd, ud, dd = (t.to(DEV).requires_grad_(True) for t in (rot, uv, d))
    enc, losses = Fn.gapr(rd, ud, dd, gt.to(DEV), B, S)
    (losses * up.to(DEV)).sum().backward()
    _close(losses, rl.detach(), 1e-4, 1e-4, f"gapr losses B={B} S={S}")
    e = enc.cpu()
    ident = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float32)
    assert torch.equal(e[::S], ident.expand(B, 7)), "frame 0 of enc"
    keep = torch.arange(B * S) % S != 0
    assert torch.equal(e[keep, :3], torch.cat([uv, d], -1)[keep]), "uvd copies"
    assert (e[3, 3:] == 0).all(), "zero quaternion"
    _close(e[:, 3:], renc[:, 3:], 0.0, 2.0 ** -22, f"gapr qn B={B} S={S}")
    nz = torch.ones(B * S, dtype=torch.bool)
    nz[3] = False
    for name, got, ref in (("drot", rd.grad, rg[0]), ("duv", ud.grad, rg[1]), ("dd", dd.grad, rg[2])):
        got = got.cpu()
        if name == "drot":
            _close(got[3], ref[3], 0.0, 2e-6 * ref[3].abs().max().item(), f"gapr drot zero row B={B}")
            assert ref[3].abs().max() > 1e4  # the clamp branch: gradients scaled by 1e8
        _close(got[nz], ref[nz], 0.0, 2e-6 * ref[nz].abs().max().item(), f"gapr {name} B={B} S={S}")
        assert (got[::S] == 0).all(), f"{name}: frame 0 carries no loss"


# ---- pose codec ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio_on_device", [False, True])
def test_pose_codec_vs_f64(ratio_on_device):
    """comet_pose_encode / _decode and the ...3 pair, B = 3, S = 4 (the frame-0 reference is per
    sequence), ratio a host float or a device float64 tensor, focal lengths below 0.1 and above 30,
    encode -> decode returning the cameras; every quaternion product has |w| >= 1e-3 (asserted), so
    the sign is never a coin toss. Encodings rtol / atol 1e-6 (gt_pose_enc in tests/test_model_gpu.py),
    decoded quaternions 1e-6, decoded T (float64 in the kernel) 1e-12 relative, T of encoding 3
    (float32) 2^-23. Measured: encoding 2 max err 8.0e-8 (its depth term (z / z0 - 1) is float32),
    encoding 3 1.2e-7, decoded quaternions 5.5e-8, T of encoding 2 equal to the reference, T of encoding
    3 8.9e-8 (4.5x inside 2^-23: its one float32 add), round trip R 8.9e-8 and T 2.6e-7 (bound 1e-6: the
    float32 encoding in between carries ~1e-7 of 128 / ratio pixels)."""
    ops = _ops()
    B, S = 3, 4
    R, uvz, xyz, focal, enc = TR.codec_inputs(B, S, seed=590)
    ratio = 1.37
    intr = O.INTRINSICS["AMD_eval"]
    e2, w2 = TR.pose_encode(R, uvz, focal, ratio, B, S)
    e3, w3 = TR.pose_encode3(R, xyz, B, S)
    q2, T2, wd2 = TR.pose_decode(enc, R, uvz, ratio, intr, B, S)
    q3, T3, wd3 = TR.pose_decode3(enc, R, xyz, B, S)
    for w in (w2, w3, wd2, wd3, R[:, 0]):
        assert w.abs().min().item() >= 1e-3
    Rd, ud, xd, fd, ed = (t.to(DEV) for t in (R, uvz, xyz, focal, enc))
    rt = torch.tensor([ratio], dtype=torch.float64, device=DEV) if ratio_on_device else ratio
    g2 = ops.pose_encode(Rd, ud, fd, rt, B, S)
    assert g2.shape == (B * S, 8)
    ident = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float32)
    assert torch.equal(g2[::S, :7].cpu(), ident.expand(B, 7)), "frame 0 of encoding 2"
    assert g2[:, 7].min().item() == pytest.approx(0.1) and g2[:, 7].max().item() == 30.0
    _close(g2, e2, 1e-6, 1e-6, "pose_encode")
    g3 = ops.pose_encode3(Rd, xd, B, S)
    assert torch.equal(g3[::S].cpu(), torch.cat([ident, torch.zeros(1)]).expand(B, 8)) and (g3[:, 7] == 0).all()
    _close(g3, e3, 1e-6, 1e-6, "pose_encode3")
    Rq, Tq = ops.pose_decode(ed, Rd, ud, rt, intr, B, S)
    assert Tq.dtype == torch.float64
    _close(Rq, q2, 1e-6, 1e-6, "pose_decode R")
    _close(Tq, T2, 1e-12, 1e-12, "pose_decode T")
    Rq3, Tq3 = ops.pose_decode3(ed, Rd, xd, B, S)
    _close(Rq3, q3, 1e-6, 1e-6, "pose_decode3 R")
    _close(Tq3, T3, 2.0 ** -23, 2.0 ** -23, "pose_decode3 T")
    # encode -> decode returns the cameras (R up to its w >= 0 sign)
    canon = torch.where(R[:, :1] < 0, -R, R)
    fx, fy, cx, cy = intr
    u, v, z = uvz.double().unbind(-1)
    Ra, Ta = ops.pose_decode(g2[:, :7].contiguous(), Rd, ud, rt, intr, B, S)
    _close(Ra, canon, 1e-6, 1e-6, "round trip R")
    _close(Ta, torch.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], -1), 1e-6, 1e-6, "round trip T")
    Rb, Tb = ops.pose_decode3(g3[:, :7].contiguous(), Rd, xd, B, S)
    _close(Rb, canon, 1e-6, 1e-6, "round trip R (3)")
    _close(Tb, xyz, 1e-6, 1e-6, "round trip T (3)")
