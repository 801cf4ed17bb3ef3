"""Float64 restatement of comet_conv2d_nhwc, its error bound, and the geometry matrix of the GPU tests
(no project imports; runs on the CPU or on a device).

The reference is written from the formula in include/comet_hip.h,
    y[(n*oh + oy)*ow + ox][co] = act(bias[co] + sum_{ky,kx,ci} x[n][oy*s-p+ky][ox*s-p+kx][ci]
                                     * weight[co][(ky*kw + kx)*c + ci]) + beta * resid[...],
as one float64 matmul per tap over strided slices of the zero-padded NHWC input. It shares no code
with the kernels (no im2col, no tiles). tests/test_conv_ref_cpu.py checks it against F.conv2d in
float64 and shows that a correct f32-accumulating kernel stays inside the bound on every geometry.

The bound. Let S = conv(|x|, |w|) + |bias| + |beta * resid| in float64 and K = kh * kw * c.
  f32 output :  |got - ref| <= (K + 4) * 2^-23 * S
  bf16 output:  |got - ref| <= 2^-8 * |ref| + (K + 4) * 2^-23 * S
bf16 x bf16 products are exact in f32; a sum of K + 1 terms (bias included) in any order, one rounding
of at most 2^-24 relative per addition, is off by at most (K + 1) * 2^-24 * S to first order, the
activation is exact, beta * resid and its addition round twice more: (K + 4) * 2^-23 * S keeps a factor
of two over that. The final rounding to bf16 moves the f32 value v by at most half an ulp, which is
between 2^-9 |v| and 2^-8 |v| across a binade: 2^-8 * |ref| covers it (v differs from ref by at most half
the accumulation term, which the spare factor absorbs). A correct kernel therefore reaches up to about
0.996 of the bf16 bound just above a power of two, and one bf16 ulp more is outside it.
No element may exceed the bound.
"""
import math

import torch

ACT_NONE, ACT_RELU = 0, 2
BETA = 0.5

# ---------------------------------------------------------------------------------------------
# The matrix. A geometry is (n, h, w, c, cout, k, stride, pad); a plan is what comet_conv_plan
# reports, (kind, NT16, KC, wide) with kind 0 = 128 x 128 implicit GEMM, 1 = 128 x 64, 2 = the
# narrow-output ("skinny") kernel, 3 = rows in LDS; wide is given for bf16 output (f32 output
# never stores wide). The plans are written out by hand: a test asserts them before it compares, so
# a dispatch change fails there instead of moving the case to another kernel.
#
# Skinny instances conv_skinny_kernel<TC, NT16, KC> the launcher can select, and the case that runs
# each (all with >= 16384 output pixels, the gate):
#   NT16 1..4 x KC 1, 2, 3, 4, 6, 8 : the six "all couts" geometries below, cout 16 / 32 / 48 / 64
#   (1, 9), (2, 9)                  : K = 288, cout 16 / 32 (and the fine encoder's own maps)
#   (1, 16), (2, 16)                : K = 360 and K = 504, cout 16 / 32
#   (4, 13)                         : the 7x7 stem (K = 392) and K = 288 < 13 * 32, cout 64
# No instance exists for NT16 = 3 with 9 or 10 chunks (cout 48, K in (256, 320]) although the
# fragment budget admits it: the dispatch sends it to the 128 x 64 implicit GEMM (CASE_COUT48).
# NT16 = 3 / 4 with KC 9 or 16 cannot be reached through the gate (more than 32 fragments).
# ---------------------------------------------------------------------------------------------
_ALL_COUTS = {
    1: (70, 16, 16, 8, None, 1, 1, 0),     # K = 8
    2: (70, 32, 32, 16, None, 2, 2, 0),    # K = 64
    3: (100, 31, 31, 8, None, 3, 2, 1),    # K = 72
    4: (70, 32, 32, 32, None, 2, 2, 0),    # K = 128
    6: (64, 20, 20, 16, None, 3, 1, 1),    # K = 144: 5 chunks, the fifth half masked
    8: (70, 16, 16, 8, None, 5, 1, 2),     # K = 200: 7 chunks
}


def _geo(g, cout):
    return g[:4] + (cout,) + g[5:]


SKINNY_INSTANCES = [(_geo(g, 16 * nt), (2, nt, kc, 1 if nt % 2 == 0 else 0))
                    for kc, g in _ALL_COUTS.items() for nt in (1, 2, 3, 4)]
SKINNY_INSTANCES += [
    ((70, 16, 16, 32, 16, 3, 1, 1), (2, 1, 9, 0)),    # K = 288
    ((70, 16, 16, 32, 32, 3, 1, 1), (2, 2, 9, 1)),
    ((70, 16, 16, 40, 16, 3, 1, 1), (2, 1, 16, 0)),   # K = 360: 12 chunks
    ((70, 16, 16, 40, 32, 3, 1, 1), (2, 2, 16, 1)),
    ((70, 16, 16, 56, 16, 3, 1, 1), (2, 1, 16, 0)),   # K = 504: 16 chunks, the last 3/4 masked
    ((70, 16, 16, 56, 32, 3, 1, 1), (2, 2, 16, 1)),
    ((1, 256, 256, 8, 64, 7, 2, 3), (2, 4, 13, 1)),   # BasicEncoder stem, K = 392
    ((70, 16, 16, 32, 64, 3, 1, 1), (2, 4, 13, 1)),   # K = 288 < 13 * 32: four all-zero chunks
]
# the fine ShallowEncoder's maps over 1030 patches (borders dominate), SuperPoint's 8 -> 64, and
# pixel counts that are no multiple of 16 (73 * 15 * 15 = 16425)
SKINNY_MODEL = [
    ((1030, 31, 31, 8, 32, 3, 2, 1), (2, 2, 3, 1)),
    ((1030, 16, 16, 32, 32, 3, 2, 1), (2, 2, 9, 1)),
    ((1030, 16, 16, 32, 32, 1, 2, 0), (2, 2, 1, 1)),
    ((1030, 8, 8, 32, 32, 3, 1, 1), (2, 2, 9, 1)),
    ((1030, 8, 8, 32, 32, 3, 2, 1), (2, 2, 9, 1)),
    ((1030, 8, 8, 32, 32, 1, 2, 0), (2, 2, 1, 1)),
    ((1030, 4, 4, 32, 32, 3, 1, 1), (2, 2, 9, 1)),
    ((1, 128, 130, 8, 64, 3, 1, 1), (2, 4, 3, 1)),
    ((73, 15, 15, 32, 32, 3, 1, 1), (2, 2, 9, 1)),
    ((73, 15, 15, 8, 48, 3, 1, 1), (2, 3, 3, 0)),
]
# more than 4096 * 32 * 16 output pixels: the grid is capped at 4096 workgroups and waves walk 9 steps
SKINNY_CAPPED = ((2, 1025, 1024, 8, 16, 1, 1, 0), (2, 1, 1, 0))
# wide (16-byte) against narrow (8-byte) bf16 stores
WIDE_CASES = [
    ((73, 15, 15, 32, 32, 3, 1, 1), (2, 2, 9, 1)),
    ((70, 16, 16, 8, 64, 5, 1, 2), (2, 4, 8, 1)),
    ((70, 16, 16, 32, 64, 3, 1, 1), (2, 4, 13, 1)),
]
# one or two geometries per kernel kind for the epilogue variants
EPILOGUE_CASES = [
    ((2, 33, 30, 64, 96, 3, 2, 1), (0, 0, 0, 0)),
    ((1, 12, 12, 416, 256, 3, 1, 1), (0, 0, 0, 0)),
    ((4, 40, 40, 64, 64, 3, 1, 1), (1, 0, 0, 0)),
    ((3, 21, 19, 64, 56, 3, 1, 1), (1, 0, 0, 0)),
    ((73, 15, 15, 32, 32, 3, 1, 1), (2, 2, 9, 1)),
    ((70, 30, 30, 8, 48, 3, 1, 1), (2, 3, 3, 0)),
    ((3, 100, 96, 64, 64, 3, 1, 1), (3, 0, 0, 0)),
]
# cout % 8 != 0: the implicit GEMMs' scalar epilogue
SCALAR_EPILOGUE_CASES = [
    ((3, 17, 13, 16, 20, 3, 1, 1), (1, 0, 0, 0)),
    ((2, 19, 23, 16, 100, 3, 2, 1), (0, 0, 0, 0)),
]
# weight rows K + 8 apart with garbage in the padding columns
LDW_CASES = [
    ((64, 20, 20, 16, 32, 3, 1, 1), (2, 2, 6, 1)),    # K = 144: the masked chunk ends in the padding
    ((70, 16, 16, 8, 64, 3, 1, 1), (2, 4, 3, 1)),
    ((3, 100, 96, 64, 64, 3, 1, 1), (3, 0, 0, 0)),
    ((3, 21, 19, 64, 56, 3, 1, 1), (1, 0, 0, 0)),
    ((2, 33, 30, 64, 96, 3, 2, 1), (0, 0, 0, 0)),
]
# cout 48 with 9 chunks: passes the skinny gate's fragment budget, has no skinny instance
CASE_COUT48 = ((70, 16, 16, 32, 48, 3, 1, 1), (1, 0, 0, 0))
# rows-in-LDS kernel (c = cout = 64, 3x3 / 1 / 1): (n, h, w). About 1300 rows, so that on 256 CUs a
# workgroup walks 6 rows and every slot of the 4-row ring is refilled while the walk continues
ROWS_CASES = [
    (1300, 1, 128),   # every row is a new image
    (650, 2, 96),     # h = 2
    (440, 3, 128),    # h = 3
    (200, 7, 96),     # image boundaries inside every range; ragged last workgroup
    (10, 130, 96),    # long walks inside one image; last range shorter
]


def rows_geo(nhw):
    n, h, w = nhw
    return (n, h, w, 64, 64, 3, 1, 1)


def all_geometries():
    """Every (geometry, plan) of the GPU matrix, once."""
    cases = (SKINNY_INSTANCES + SKINNY_MODEL + [SKINNY_CAPPED] + WIDE_CASES + EPILOGUE_CASES +
             SCALAR_EPILOGUE_CASES + LDW_CASES + [CASE_COUT48] + [(rows_geo(r), (3, 0, 0, 0)) for r in ROWS_CASES])
    return list(dict(cases).items())


# ---------------------------------------------------------------------------------------------
# inputs, reference, bound
# ---------------------------------------------------------------------------------------------
def out_hw(geo):
    n, h, w, c, cout, k, s, p = geo
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def make_inputs(geo, ldw_pad=0, seed=0):
    """Seeded inputs on the CPU: x [n, h, w, c] bf16, weight buffer [cout, K + ldw_pad] bf16 (columns
    (ky, kx, ci) scaled by K^-0.5, the padding columns filled with 1000; weight_view() is the [cout, K]
    matrix inside it), bias [cout] f32 (non-zero), resid [n, oh, ow, cout] bf16 (a bf16-representable
    residual serves both output types)."""
    n, h, w, c, cout, k, s, p = geo
    K = k * k * c
    oh, ow = out_hw(geo)
    g = torch.Generator().manual_seed(seed + sum(v * 31 ** i for i, v in enumerate(geo)) % 100003)
    x = torch.randn(n, h, w, c, generator=g).to(torch.bfloat16)
    wbuf = torch.full((cout, K + ldw_pad), 1000.0, dtype=torch.bfloat16)
    wbuf[:, :K] = (torch.randn(cout, K, generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(cout, generator=g)
    bias = torch.where(bias.abs() < 0.05, torch.full_like(bias, 0.05), bias)
    resid = torch.randn(n, oh, ow, cout, generator=g).to(torch.bfloat16)
    return x, wbuf, bias, resid


def weight_view(wbuf, geo):
    """The [cout, K] weight matrix of a make_inputs buffer (row pitch K + ldw_pad)."""
    return wbuf[:, :geo[5] * geo[5] * geo[3]]


def _conv_taps(x, wm, geo):
    """sum over taps of x_pad[:, ky::s, kx::s, :] @ w[:, tap]^T in float64: [n, oh, ow, cout]."""
    n, h, w, c, cout, k, s, p = geo
    oh, ow = out_hw(geo)
    xp = torch.zeros(n, h + 2 * p, w + 2 * p, c, dtype=torch.float64, device=x.device)
    xp[:, p:p + h, p:p + w] = x
    y = torch.zeros(n, oh, ow, cout, dtype=torch.float64, device=x.device)
    for ky in range(k):
        for kx in range(k):
            tap = ky * k + kx
            xs = xp[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s]
            y += xs @ wm[:, tap * c:(tap + 1) * c].t()
    return y


def conv_ref(x, wm, geo, bias=None, act=ACT_NONE, resid=None, beta=1.0):
    """(ref, S) in float64 on x's device. x bf16 NHWC, wm [cout, >= K] (only the first K columns of a row
    are read), bias f32 or None, resid any float type or None."""
    assert act in (ACT_NONE, ACT_RELU)
    xd, wd = x.double(), wm.double()
    ref = _conv_taps(xd, wd, geo)
    S = _conv_taps(xd.abs(), wd.abs(), geo)
    if bias is not None:
        ref = ref + bias.double()
        S = S + bias.double().abs()
    if act == ACT_RELU:
        ref = ref.clamp_min(0.0)
    if resid is not None:
        ref = ref + float(beta) * resid.double()
        S = S + (float(beta) * resid.double()).abs()
    return ref, S


def bound(ref, S, geo, out_dtype):
    n, h, w, c, cout, k, s, p = geo
    b = (k * k * c + 4) * 2.0 ** -23 * S
    if out_dtype == torch.bfloat16:
        b = b + 2.0 ** -8 * ref.abs()
    return b


def compare(got, ref, S, geo, out_dtype):
    """(number of elements over the bound, worst |got - ref| / bound). A non-finite element counts as over."""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    b = bound(ref, S, geo, out_dtype)
    return int((err > b).sum().item()), (err / b.clamp_min(1e-300)).max().item()
