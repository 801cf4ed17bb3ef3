"""tests/conv_ref.py against F.conv2d in float64, and the error bound of the GPU tests against an
emulated correct kernel (f32 F.conv2d on the bf16 inputs, f32 epilogue, one rounding to the output
type) on every geometry of the GPU matrix: the bound is not tighter than a correct implementation.
No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

GEOS = [g for g, _ in R.all_geometries()]


def _nchw(wm, geo):
    n, h, w, c, cout, k, s, p = geo
    return wm.reshape(cout, k, k, c).permute(0, 3, 1, 2)


def test_matrix_names_every_skinny_instance():
    """Each (NT16, KC) pair the narrow-output launcher can select is the plan of some case."""
    want = {(nt, kc) for nt in (1, 2, 3, 4) for kc in (1, 2, 3, 4, 6, 8)} | {(1, 9), (1, 16), (2, 9), (2, 16), (4, 13)}
    have = {(p[1], p[2]) for _, p in R.all_geometries() if p[0] == 2}
    assert have == want, (want - have, have - want)
    for geo, p in R.all_geometries():
        if p[0] == 2:
            oh, ow = R.out_hw(geo)
            assert geo[0] * oh * ow >= 16384 and p[1] == geo[4] // 16, geo
    assert any(g[0] * R.out_hw(g)[0] * R.out_hw(g)[1] % 16 for g, p in R.all_geometries() if p[0] == 2)


@pytest.mark.parametrize("geo", [(2, 9, 7, 8, 5, 3, 2, 1), (1, 6, 8, 16, 3, 5, 1, 2), (3, 5, 5, 8, 4, 1, 2, 0),
                                 (1, 14, 14, 8, 6, 7, 2, 3), (2, 1, 9, 8, 4, 3, 1, 1), (1, 8, 8, 24, 4, 2, 2, 0)])
@pytest.mark.parametrize("epi", ["plain", "bias", "bias_relu_resid"])
def test_conv_ref_matches_torch_conv2d_f64(geo, epi):
    x, wbuf, bias, resid = R.make_inputs(geo, ldw_pad=8)
    wm = R.weight_view(wbuf, geo)
    s, p = geo[6], geo[7]
    b = None if epi == "plain" else bias
    want = F.conv2d(x.double().permute(0, 3, 1, 2), _nchw(wm, geo).double(), None if b is None else b.double(),
                    stride=s, padding=p).permute(0, 2, 3, 1)
    absw = F.conv2d(x.double().abs().permute(0, 3, 1, 2), _nchw(wm, geo).double().abs(), stride=s,
                    padding=p).permute(0, 2, 3, 1)
    kw = {}
    if b is not None:
        absw = absw + b.double().abs()
    if epi == "bias_relu_resid":
        want = F.relu(want) + R.BETA * resid.double()
        absw = absw + (R.BETA * resid.double()).abs()
        kw = dict(act=R.ACT_RELU, resid=resid, beta=R.BETA)
    ref, S = R.conv_ref(x, wm, geo, bias=b, **kw)
    assert ref.shape == want.shape
    # two float64 summation orders of K + 3 terms
    tol = (geo[5] * geo[5] * geo[3] + 4) * 2.0 ** -52 * absw
    assert ((ref - want).abs() <= tol).all()
    assert ((S - absw).abs() <= tol).all()


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "x".join(map(str, g)))
def test_correct_f32_kernel_stays_inside_the_bound(geo):
    """f32 accumulation (F.conv2d), f32 epilogue, one rounding to the output type: bias only and bias +
    ReLU + beta * resid, both output types. Prints the worst err / bound per geometry."""
    x, wm, bias, resid = R.make_inputs(geo)
    wm = R.weight_view(wm, geo)
    s, p = geo[6], geo[7]
    conv = F.conv2d(x.float().permute(0, 3, 1, 2), _nchw(wm, geo).float(), bias, stride=s,
                    padding=p).permute(0, 2, 3, 1)
    worst = {}
    for epi in ("bias", "bias_relu_resid"):
        if epi == "bias":
            emu = conv
            ref, S = R.conv_ref(x, wm, geo, bias=bias)
        else:
            emu = F.relu(conv) + R.BETA * resid.float()
            ref, S = R.conv_ref(x, wm, geo, bias=bias, act=R.ACT_RELU, resid=resid, beta=R.BETA)
        for dt in (torch.float32, torch.bfloat16):
            over, ratio = R.compare(emu.to(dt), ref, S, geo, dt)
            worst[(epi, dt)] = ratio
            assert over == 0, f"{geo} {epi} {dt}: {over} elements over the bound, worst err / bound {ratio:.3f}"
    print(f"conv bound {geo}: worst err / bound f32 {max(v for (e, d), v in worst.items() if d == torch.float32):.4f}"
          f" bf16 {max(v for (e, d), v in worst.items() if d == torch.bfloat16):.4f}")


def test_bound_rejects_a_one_ulp_bf16_error_and_an_unwritten_output():
    """The comparison bites: a result one bf16 ulp further from the reference than the rounded one, a
    dropped tap and a NaN are all over the bound."""
    geo = (2, 9, 7, 8, 16, 3, 1, 1)
    x, wm, bias, _ = R.make_inputs(geo)
    ref, S = R.conv_ref(x, wm, geo, bias=bias)
    good = ref.float().to(torch.bfloat16)
    assert R.compare(good, ref, S, geo, torch.bfloat16)[0] == 0
    # next bf16 value away from the reference
    up = good.double() >= ref
    bits = good.view(torch.int16).to(torch.int32)
    away = torch.where(up == (good.double() >= 0), bits + 1, bits - 1).to(torch.int16).view(torch.bfloat16)
    big = ref.abs() > 0.25  # where the bf16 ulp dominates the accumulation term
    over = ((away.double() - ref).abs() > R.bound(ref, S, geo, torch.bfloat16)) & big
    assert over.sum() > 0.9 * big.sum()
    wm2 = wm.clone()
    wm2[:, 4 * 8:5 * 8] = 0  # the centre tap
    dropped, _ = R.conv_ref(x, wm2, geo, bias=bias)
    assert R.compare(dropped.float(), ref, S, geo, torch.float32)[0] > 0
    nan = good.clone()
    nan[0, 0, 0, 0] = float("nan")
    assert R.compare(nan, ref, S, geo, torch.bfloat16)[0] == 1
