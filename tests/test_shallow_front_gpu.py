"""comet_shallow_front_nhwc (the fine ShallowEncoder's conv1 + InstanceNorm + ReLU and its two
stride-2 ResidualBlocks in one kernel) against the unfused op sequence it replaces -- seven
ops.conv2d_nhwc and seven ops.instnorm_nhwc calls -- bit for bit: torch.equal, no tolerance.

The reference is computed once, on all NREF patches: at 1030 patches every convolution of the chain
has >= 16384 output pixels (1030 x 16 for the 4 x 4 maps), so the reference runs the narrow
convolution kernel and the one-wave-per-image InstanceNorm the model runs at 65536 patches. Patches
are independent of each other, so the fused kernel on any subset must equal the reference's rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NREF = 1030   # more workgroups (258, four patches each) than one round of a 256-CU grid
PPW = 4       # patches per workgroup of the fused kernel
K = (72, 288, 288, 32, 288, 288, 32)  # conv1, l1.conv1, l1.conv2, l1.down, l2.conv1, l2.conv2, l2.down


def _ops():
    from comet_amd import ops
    return ops


def _unfused(ops, p, ws, bs):
    """ShallowEncoder.forward's front as separate launches (blocks.py / modules.py ResidualBlock.forward)."""
    x = ops.instnorm_nhwc(ops.conv2d_nhwc(p, ws[0], 3, 3, 2, 1, bias=bs[0]), relu=True)
    outs = [x]
    t = x
    for i in (1, 4):
        y = ops.instnorm_nhwc(ops.conv2d_nhwc(t, ws[i], 3, 3, 2, 1, bias=bs[i]), relu=True)
        y = ops.conv2d_nhwc(y, ws[i + 1], 3, 3, 1, 1, bias=bs[i + 1])
        d = ops.instnorm_nhwc(ops.conv2d_nhwc(t, ws[i + 2], 1, 1, 2, 0, bias=bs[i + 2]))
        t = ops.instnorm_nhwc(y, res=d, relu=True, relu_inner=True)
        outs.append(t)
    return outs


@pytest.fixture(scope="module")
def case():
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(31)
    p = torch.randn(NREF, 31, 31, 8, device=DEV, generator=g)
    p[..., 3:] = 0                      # RGB zero-padded to 8 channels, as patch_gather writes it
    p[1, :, :, 1] = 0.75                # one input channel constant over the image
    p[2] = 0.25                         # a constant patch: conv1's interior is constant
    p[3, ..., :3] += 50.0               # values far from zero: the shifted-moment statistics
    p = p.to(torch.bfloat16)
    ws = [(torch.randn(32, k, device=DEV, generator=g) * k ** -0.5).to(torch.bfloat16) for k in K]
    # a conv1 output channel that sees nothing but its bias: zero variance, the clamp path
    ws[0][5] = 0
    bs = [torch.randn(32, device=DEV, generator=g) for _ in K]   # non-zero biases
    ref = _unfused(ops, p, ws, bs)
    torch.cuda.synchronize()
    return p, ws, bs, ref


def _check(got, ref, n, what):
    for name, a, b in zip(("x", "tmp1", "tmp2"), got, ref):
        b = b[:n]
        assert a.shape == b.shape and a.dtype == b.dtype
        d = (a.float() - b.float()).abs().max().item()
        print(f"{what} {name}: max |diff| {d:.3e}")
        assert torch.equal(a, b), f"{what}: {name} differs from the unfused launches, max |diff| {d:.3e}"


@pytest.mark.parametrize("n", [1, 5, 4 * PPW + 3, NREF])
def test_fused_front_equals_unfused(case, n):
    """n = 1, 5, a ragged last workgroup (4 k + 3 patches at k = 4 per workgroup) and more workgroups
    than CUs (a second round for some waves)."""
    ops = _ops()
    p, ws, bs, ref = case
    sub = p[:n].contiguous()
    assert ops.shallow_front_ok(sub, ws, bs)
    _check(ops.shallow_front(sub, ws, bs), ref, n, f"n={n}")


def test_zero_variance_channel_takes_the_clamp(case):
    """Patch 1 has an input channel constant over the image and conv1's output channel 5 is its bias
    everywhere (zero weight row): zero variance, var clamps to 0, the output is (v - mean) * rsqrt(eps)
    = 0 exactly -- in both paths."""
    ops = _ops()
    p, ws, bs, ref = case
    x, t1, t2 = ops.shallow_front(p[:4].contiguous(), ws, bs)
    assert torch.isfinite(x.float()).all() and torch.isfinite(t1.float()).all() and torch.isfinite(t2.float()).all()
    assert (x[..., 5] == 0).all(), "a zero-variance channel normalises to 0"
    _check((x, t1, t2), ref, 4, "clamp")


def test_offset_patch_uses_shifted_moments(case):
    """Patch 3's RGB values sit at +50: the statistics are taken about pixel 0, as in the unfused
    kernel, and the result equals it bit for bit (also alone in the launch, at another wave slot)."""
    ops = _ops()
    p, ws, bs, ref = case
    got = ops.shallow_front(p[3:4].contiguous(), ws, bs)
    _check(got, [r[3:4] for r in ref], 1, "offset")
    assert got[0].float().abs().max().item() < 20.0  # normalised, not 50-sized


def _encoder():
    from comet_amd.models.track_modules.blocks import ShallowEncoder
    torch.manual_seed(7)
    enc = ShallowEncoder(input_dim=3, output_dim=32, stride=1).to(DEV)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.bias.normal_()
    return enc


def test_encoder_forward_switch_on_and_off(monkeypatch):
    """ShallowEncoder.forward(patches, with_pool=2) with the fused front and with
    COMET_SHALLOW_FRONT=0: the three outputs are equal, and the fused kernel did run."""
    from comet_amd import functional as CF
    ops = _ops()
    enc = _encoder()
    g = torch.Generator(device=DEV).manual_seed(64)
    p = torch.randn(64, 31, 31, 8, device=DEV, generator=g)
    p[..., 3:] = 0
    p = p.to(torch.bfloat16)
    calls = []
    real = ops.shallow_front
    monkeypatch.setattr(ops, "shallow_front", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with CF.precision(torch.bfloat16):
        monkeypatch.setenv("COMET_SHALLOW_FRONT", "1")
        on = enc(p, with_pool=2)
        assert len(calls) == 1, "the fused front did not run"
        monkeypatch.setenv("COMET_SHALLOW_FRONT", "0")
        off = enc(p, with_pool=2)
        assert len(calls) == 1, "COMET_SHALLOW_FRONT=0 must take the separate launches"
    assert len(on) == 3 and len(off) == 3
    for name, a, b in zip(("feat", "pool", "pool2"), on, off):
        assert torch.equal(a, b), f"{name}: max |diff| {(a.float() - b.float()).abs().max().item():.3e}"


@pytest.mark.parametrize("kind", ["fp32", "p29"])
def test_ineligible_input_takes_the_separate_launches(kind, monkeypatch):
    """fp32 patches, or 29 x 29 ones: not the fused kernel's case, the forward still returns."""
    from comet_amd import functional as CF
    ops = _ops()
    enc = _encoder()
    g = torch.Generator(device=DEV).manual_seed(29)
    P = 29 if kind == "p29" else 31
    p = torch.randn(16, P, P, 8, device=DEV, generator=g)
    p[..., 3:] = 0
    if kind == "p29":
        p = p.to(torch.bfloat16)
    monkeypatch.setattr(ops, "shallow_front", lambda *a, **k: pytest.fail("fused front on ineligible input"))
    monkeypatch.setenv("COMET_SHALLOW_FRONT", "1")
    with CF.precision(torch.bfloat16):
        feat, pool = enc(p, with_pool=True)
    torch.cuda.synchronize()
    assert tuple(feat.shape) == (16, P, P, 32) and torch.isfinite(feat.float()).all()
    assert tuple(pool.shape) == (16, P // 2, P // 2, 32)
