"""The training backward kernels and the autograd Functions of comet_amd.functional against the f64
restatements of tests/backward_ref.py, at the shapes, strides and flags where they can go wrong.

bf16 attention bounds. For every case the test recomputes on the CPU
    e = max|attn_bwd_rounded - attn_bwd_ref| / max|attn_bwd_ref|
(the documented bf16 roundings with f64 accumulation, tests/test_backward_ref_cpu.py prints every value)
and allows the kernel 3 e: f32 instead of f64 accumulation, the bare v_exp_f32 and another summation
order. Largest e over D in {32, 48, 64, 96} and the 17 (lq, lk) shapes of backward_ref.ATTN_SHAPES:

    output   largest e    at (D, lq, lk)
    dq       4.966e-03    (48, 130, 3)
    dk       5.243e-03    (32, 64, 257)
    dv       5.835e-03    (64, 3, 130)
    (scale = 0.37 at (64, 65, 129):    3.840e-03  3.768e-03  2.773e-03)
    (|s scale| up to 80 at (64, 130, 77): 4.902e-03  4.646e-03  2.855e-03)

so the bounds are 0.5 - 1.8 % of max|ref|, against the blanket 2 % + 2 % of test_flash_attention_bwd.
Where the reference vanishes identically (lk = 1: dq = dk = 0) max|ref| is replaced by the f32 round-off
floor of backward_ref.attn_bwd_floor, which is also added to every bound (1e-3 of it elsewhere).

The Linear-family bf16 bounds of section f are measured the same way inside each test (a CPU run of the
same computation with operands, outputs and gradients rounded to bf16, times 3); for y = gelu(x W^T + b)
at K = 40, N = 24 the model's errors are 2.4e-3 ... 5.7e-3 of max|ref| (test_linear_rounding_model_error).
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as TF

import backward_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")


def _mods():
    from comet_amd import _lib, functional, ops
    return _lib, ops, functional


def _rand(*shape, seed=0, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _close(got, ref, rtol, atol, what=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())
    assert not bad.any(), (f"{what}: max err {err.max().item():.3e} (ref max {ref.abs().max().item():.3e}), "
                           f"{bad.sum().item()} bad of {bad.numel()}")


def _half_ulp_bf16(ref):
    """Half a bf16 ulp of |ref| (0 at 0)."""
    a = ref.abs().double()
    return torch.where(a > 0, 2.0 ** (torch.floor(torch.log2(a.clamp_min(1e-300))) - 8), torch.zeros_like(a))


def _count(monkeypatch, mod, name, counts):
    fn = getattr(mod, name)

    @functools.wraps(fn)
    def wrap(*a, **k):
        counts[name] = counts.get(name, 0) + 1
        return fn(*a, **k)
    monkeypatch.setattr(mod, name, wrap)


# =================================================================================================
# a. comet_attention_bwd vs f64
# =================================================================================================
@functools.lru_cache(maxsize=None)
def _attn_case(D, lq, lk, scale=None, gain=None):
    q, kv, do = R.attn_inputs(D, lq, lk, logit_gain=gain)
    C = q.shape[-1]
    sc = D ** -0.5 if scale is None else scale
    e, refs, floors = R.attn_model_error(q, kv[..., :C], kv[..., C:], do, R.ATTN_H, sc)
    return q, kv, do, sc, e, refs, floors


def _attn_bwd_run(q, kv, do, scale, pad_o=0, delta=None):
    """ops.attention forward + backward on packed buffers whose gradients sit in NaN-filled, padded
    allocations. Returns (dq, dk, dv, o, lse) after checking the canaries."""
    L, ops, _ = _mods()
    B, lq, C = q.shape
    lk = kv.shape[1]
    H = R.ATTN_H
    D = C // H
    qd, kvd = q.to(DEV), kv.to(DEV)
    k, v = kvd[..., :C], kvd[..., C:]
    if pad_o:  # o / do as row-strided views (row stride a multiple of 8, not C)
        obuf = torch.zeros(B, lq, C + pad_o, device=DEV, dtype=BF)
        gbuf = torch.zeros(B, lq, C + 2 * pad_o, device=DEV, dtype=BF)
        o, dod = obuf[..., :C], gbuf[..., pad_o:pad_o + C]
        dod.copy_(do)
        assert o.stride(1) % 8 == 0 and o.stride(1) != C and dod.stride(1) != C and not dod.is_contiguous()
        _, lse = ops.attention(qd, k, v, H, scale, out=o, lse=True)
    else:
        dod = do.to(DEV)
        o, lse = ops.attention(qd, k, v, H, scale, lse=True)
    dqb = torch.full((B, lq + 8, C + 8), NAN, device=DEV, dtype=BF)
    dkvb = torch.full((B, lk + 8, 2 * C + 8), NAN, device=DEV, dtype=BF)
    dq, dk, dv = dqb[:, :lq, :C], dkvb[:, :lk, :C], dkvb[:, :lk, C:2 * C]
    if delta is None:
        ops.attention_bwd(qd, k, v, o, lse, dod, H, scale, dq, dk, dv)
    else:
        a = L.AttnBwdArgs()
        a.dtype, a.head_dim = L.BF16, D
        a.batch, a.heads, a.lq, a.lk = B, H, lq, lk
        for name, t in (("q", qd), ("k", k), ("v", v), ("o", o), ("d", dod), ("dq", dq), ("dk", dk), ("dv", dv)):
            setattr(a, "dout" if name == "d" else name, t.data_ptr())
            setattr(a, f"s{name}_b", t.stride(0))
            setattr(a, f"s{name}_h", D)
            setattr(a, f"s{name}_l", t.stride(1))
        a.lse, a.delta, a.scale = lse.data_ptr(), delta.data_ptr(), float(scale)
        L.check(L.load().comet_attention_bwd(ctypes.byref(a), ops.stream()), "attention_bwd")
    torch.cuda.synchronize()
    for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.isfinite(t).all(), f"{name}: sentinel left or non-finite value inside the slice"
    assert torch.isnan(dqb[:, lq:]).all() and torch.isnan(dqb[:, :lq, C:]).all(), "dq write outside its slice"
    assert torch.isnan(dkvb[:, lk:]).all() and torch.isnan(dkvb[:, :lk, 2 * C:]).all(), "dk/dv write outside their slices"
    return dq, dk, dv, o, lse


def _attn_check(got3, e, refs, floors, what):
    for name, got, ev, ref, fl in zip(("dq", "dk", "dv"), got3, e, refs[2:], floors):
        g = got.double().cpu()
        m = max(ref.abs().max().item(), fl)
        err = (g - ref).abs()
        rel = err.max().item() / m
        print(f"{what} {name}: max err / max|ref| = {rel:.3e}, model e = {ev:.3e}, ratio {rel / max(ev, 1e-30):.2f}")
        assert err.max().item() <= 3 * ev * m + fl, f"{what} {name}: {rel:.3e} of max|ref| > 3 e = {3 * ev:.3e}"
        bad = err > 3 * ev * m + fl + 2.0 ** -7 * ref.abs()
        assert not bad.any(), f"{what} {name}: {bad.sum().item()} elements off"


_ATTN_TABLE = ([("small", s) for s in R.ATTN_SMALL] + [("forced", s) for s in R.ATTN_FORCED]
               + [("wide", s) for s in R.ATTN_WIDE])


@pytest.mark.parametrize("D", R.ATTN_DS)
@pytest.mark.parametrize("path,shape", _ATTN_TABLE, ids=[f"{p}-{s[0]}x{s[1]}" for p, s in _ATTN_TABLE])
def test_attention_bwd_vs_f64(D, path, shape, monkeypatch):
    """small: the 64-row kernels as dispatched (lq < 64 or lk < 64); forced: the same kernels by
    COMET_ATTN_BWD16=1 with multi-tile loops and ragged last tiles on both axes; wide: the 128-row
    kernels (lq, lk >= 64, 16-B aligned dk / dv, the switch unset) at their workgroup boundaries."""
    lq, lk = shape
    if path == "forced":
        monkeypatch.setenv("COMET_ATTN_BWD16", "1")
    else:
        monkeypatch.delenv("COMET_ATTN_BWD16", raising=False)
    assert (min(lq, lk) >= 64) == (path != "small")
    q, kv, do, scale, e, refs, floors = _attn_case(D, lq, lk)
    dq, dk, dv, o, lse = _attn_bwd_run(q, kv, do, scale)
    if path == "wide":
        assert dk.data_ptr() % 16 == 0 and dv.data_ptr() % 16 == 0
    _close(lse, refs[1], 1e-4, 1e-2, "lse")  # (test_attention_fwd's bf16 bound: the forward is not under test)
    _attn_check((dq, dk, dv), e, refs, floors, f"attn bwd {path} D={D} {lq}x{lk}")


@pytest.mark.parametrize("path,shape", [("small", (5, 11)), ("forced", (65, 129)), ("wide", (129, 129))])
def test_attention_bwd_delta(path, shape, monkeypatch):
    """The delta workspace equals rowsum(dO * O) of the o the backward was given."""
    if path == "forced":
        monkeypatch.setenv("COMET_ATTN_BWD16", "1")
    else:
        monkeypatch.delenv("COMET_ATTN_BWD16", raising=False)
    D = 48
    lq, lk = shape
    q, kv, do, scale, e, refs, floors = _attn_case(D, lq, lk)
    delta = torch.full((R.ATTN_B, R.ATTN_H, lq + 4), NAN, device=DEV)
    dflat = delta.view(-1)[:R.ATTN_B * R.ATTN_H * lq]
    dq, dk, dv, o, lse = _attn_bwd_run(q, kv, do, scale, delta=dflat)
    ref = R.attn_delta_ref(do, o.cpu(), R.ATTN_H)
    _close(dflat.view(R.ATTN_B, R.ATTN_H, lq), ref, 1e-5, 1e-5 * ref.abs().max().item(), "delta")
    assert torch.isnan(delta.view(-1)[R.ATTN_B * R.ATTN_H * lq:]).all()
    _attn_check((dq, dk, dv), e, refs, floors, f"attn bwd (own delta) {path}")


@pytest.mark.parametrize("path", ["forced", "wide"])
def test_attention_bwd_scale(path, monkeypatch):
    if path == "forced":
        monkeypatch.setenv("COMET_ATTN_BWD16", "1")
    else:
        monkeypatch.delenv("COMET_ATTN_BWD16", raising=False)
    q, kv, do, scale, e, refs, floors = _attn_case(64, 65, 129, scale=0.37)
    assert scale == 0.37
    got = _attn_bwd_run(q, kv, do, scale)
    _attn_check(got[:3], e, refs, floors, f"attn bwd scale=0.37 {path}")


@pytest.mark.parametrize("path", ["forced", "wide"])
def test_attention_bwd_large_logits(path, monkeypatch):
    """|s scale| up to 80: P = exp2(fma(s, scale log2e, -lse log2e)) subtracts numbers of that size."""
    if path == "forced":
        monkeypatch.setenv("COMET_ATTN_BWD16", "1")
    else:
        monkeypatch.delenv("COMET_ATTN_BWD16", raising=False)
    q, kv, do, scale, e, refs, floors = _attn_case(64, 130, 77, gain=80.0)
    got = _attn_bwd_run(q, kv, do, scale)
    _attn_check(got[:3], e, refs, floors, f"attn bwd large logits {path}")


@pytest.mark.parametrize("shape", [(5, 11), (129, 129)])
def test_attention_bwd_strided_o_and_do(shape):
    q, kv, do, scale, e, refs, floors = _attn_case(64, *shape)
    got = _attn_bwd_run(q, kv, do, scale, pad_o=16)
    _attn_check(got[:3], e, refs, floors, f"attn bwd strided o/do {shape}")


@pytest.mark.parametrize("shape", [(5, 11), (65, 129)])
def test_attention_bwd_zero_dout(shape):
    q, kv, do, scale, *_ = _attn_case(64, *shape)
    dq, dk, dv, _, _ = _attn_bwd_run(q, kv, torch.zeros_like(do), scale)
    assert not dq.float().any() and not dk.float().any() and not dv.float().any()


# =================================================================================================
# b. the materialised backward pieces and functional._Attention
# =================================================================================================
def _tol_piece(ref, dtype):
    f32_term = 1e-5 * ref.abs().max().item() + 1e-5 * ref.abs()
    return f32_term if dtype == F32 else f32_term + _half_ulp_bf16(ref) * (1 + 2.0 ** -7)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("cols", [1, 7, 64, 130])
def test_attn_probs_and_dsoftmax(dtype, rows, cols):
    """comet_attn_probs / comet_attn_dsoftmax as functional._attn_bwd calls them, on rows padded by 3
    (ld > cols) whose pad keeps its sentinel."""
    L, ops, _ = _mods()
    lib = L.load()
    ld, scale = cols + 3, 0.21
    s = _rand(rows, cols, seed=rows + cols, scale=4.0)
    lse = torch.logsumexp(s.double() * scale, -1).float()
    dp = _rand(rows, cols, seed=rows + cols + 1)
    delta = _rand(rows, seed=rows + cols + 2)
    sb = torch.full((rows, ld), NAN, device=DEV)
    sb[:, :cols] = s
    pb = torch.full((rows, ld), NAN, device=DEV, dtype=dtype)
    lse_d, delta_d = lse.to(DEV), delta.to(DEV)
    L.check(lib.comet_attn_probs(ops.dt(pb), sb.data_ptr(), lse_d.data_ptr(), pb.data_ptr(), rows, cols, ld, ld,
                                 scale, ops.stream()), "attn_probs")
    ref = R.attn_probs_ref(s, lse, scale)
    got = pb[:, :cols].double().cpu()
    assert ((got - ref).abs() <= _tol_piece(ref, dtype)).all(), f"probs: {(got - ref).abs().max().item():.3e}"
    assert torch.isnan(pb[:, cols:]).all()
    dpb = torch.full((rows, ld), NAN, device=DEV)
    dpb[:, :cols] = dp
    dsb = torch.full((rows, ld), NAN, device=DEV, dtype=dtype)
    L.check(lib.comet_attn_dsoftmax(ops.dt(pb), pb.data_ptr(), dpb.data_ptr(), delta_d.data_ptr(), dsb.data_ptr(),
                                    rows, cols, ld, scale, ops.stream()), "attn_dsoftmax")
    ref = R.attn_dsoftmax_ref(got, dp, delta, scale)  # of the P the kernel was given
    g2 = dsb[:, :cols].double().cpu()
    assert ((g2 - ref).abs() <= _tol_piece(ref, dtype)).all(), f"dsoftmax: {(g2 - ref).abs().max().item():.3e}"
    assert torch.isnan(dsb[:, cols:]).all() and torch.isnan(pb[:, cols:]).all()


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [32, 48, 96, 40])
def test_attn_delta(dtype, D):
    L, ops, _ = _mods()
    B, H, lq = 2, 3, 9
    C = H * D
    ob = _rand(B, lq, C + 8, seed=D, dtype=dtype).to(DEV)
    gb = _rand(B, lq, C + 24, seed=D + 1, dtype=dtype).to(DEV)
    o, do = ob[..., :C], gb[..., 16:16 + C]
    delta = torch.full((B * H * lq + 5,), NAN, device=DEV)
    L.check(L.load().comet_attn_delta(ops.dt(o), do.data_ptr(), o.data_ptr(), delta.data_ptr(), B, H, lq, D, o.stride(0),
                                      D, o.stride(1), do.stride(0), D, do.stride(1), ops.stream()), "attn_delta")
    ref = R.attn_delta_ref(do.cpu(), o.cpu(), H)
    _close(delta[:B * H * lq].view(B, H, lq), ref, 1e-5, 1e-5 * ref.abs().max().item(), f"delta D={D}")
    assert torch.isnan(delta[B * H * lq:]).all()


def _attention_ref(qsrc, kvsrc, H, C, cot):
    D = C // H
    qs = qsrc.double().detach().requires_grad_(True)
    ks = kvsrc.double().detach().requires_grad_(True) if kvsrc is not None else None
    if ks is None:
        q, k, v = qs[..., :C], qs[..., C:2 * C], qs[..., 2 * C:]
    else:
        q, k, v = qs, ks[..., :C], ks[..., C:]
    s = R._heads(q, H) @ R._heads(k, H).transpose(-1, -2) * D ** -0.5
    o = R._merge(torch.softmax(s, -1) @ R._heads(v, H))
    o.backward(cot.double())
    return o.detach(), qs.grad, (ks.grad if ks is not None else None)


@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("D", [32, 48])
@pytest.mark.parametrize("lq,lk", [(1, 16), (17, 130), (64, 64)])
def test_attention_function_f32(kind, D, lq, lk, monkeypatch):
    """functional._Attention in f32 (the materialised backward: comet_attn_probs / _delta / _dsoftmax and
    six batched GEMMs) vs f64 autograd, with test_gemm_layouts' f32 tolerance at K = max(D, lq, lk)."""
    _, ops, F = _mods()
    counts = {}
    _count(monkeypatch, ops, "attention_bwd", counts)
    _count(monkeypatch, F, "_attn_bwd", counts)
    B, H = 2, 3
    C = H * D
    if kind == "self":
        lq = lk
        qsrc, kvsrc = _rand(B, lk, 3 * C, seed=lq + D), None
    else:
        qsrc, kvsrc = _rand(B, lq, C, seed=lq + D), _rand(B, lk, 2 * C, seed=lk + D + 1)
    cot = _rand(B, lq, C, seed=7)
    qd = qsrc.to(DEV).requires_grad_(True)
    kd = kvsrc.to(DEV).requires_grad_(True) if kvsrc is not None else None
    with F.precision(F32):
        out = F.attention(qd, kd, H, C)
        out.backward(cot.to(DEV))
    assert counts == {"_attn_bwd": 1}
    o, gq, gkv = _attention_ref(qsrc, kvsrc, H, C, cot)
    tol = 2e-5
    K = max(D, lq, lk)
    _close(out, o, tol, tol * math.sqrt(K), "o")
    _close(qd.grad, gq, tol, tol * math.sqrt(K), "d qsrc")
    if kd is not None:
        _close(kd.grad, gkv, tol, tol * math.sqrt(K), "d kvsrc")


@pytest.mark.parametrize("branch", ["fused", "materialised"])
def test_attention_function_bf16_branches(branch, monkeypatch):
    """functional._Attention in bf16: the fused comet_attention_bwd, and the materialised backward with
    bf16 P / dS. comet_attention_fwd takes head sizes 32 / 48 / 64 / 96 only and the same stride and
    alignment rules as attention_bwd_ok, so no bf16 input that the forward accepts reaches the
    materialised branch on its own (D = 40 is rejected by the forward, asserted below): the branch is
    selected here by making attention_bwd_ok answer False."""
    L, ops, F = _mods()
    counts = {}
    _count(monkeypatch, ops, "attention_bwd", counts)
    _count(monkeypatch, F, "_attn_bwd", counts)
    if branch == "materialised":
        monkeypatch.setattr(ops, "attention_bwd_ok", lambda *a, **k: False)
    B, H, D, lq, lk = 2, 3, 32, 17, 130
    C = H * D
    qsrc, kvsrc = _rand(B, lq, C, seed=1, dtype=BF), _rand(B, lk, 2 * C, seed=2, dtype=BF)
    cot = _rand(B, lq, C, seed=3, dtype=BF)
    qd, kd = qsrc.to(DEV).requires_grad_(True), kvsrc.to(DEV).requires_grad_(True)
    with F.precision(BF):
        out = F.attention(qd, kd, H, C)
        out.backward(cot.to(DEV))
    assert counts == ({"attention_bwd": 1} if branch == "fused" else {"_attn_bwd": 1})
    e, refs, floors = R.attn_model_error(qsrc, kvsrc[..., :C], kvsrc[..., C:], cot, H, D ** -0.5)
    _attn_check((qd.grad, kd.grad[..., :C], kd.grad[..., C:]), e, refs, floors, f"_Attention bf16 {branch}")
    with pytest.raises(L.CometHipError, match="head_dim"):
        with F.precision(BF):
            F.attention(_rand(1, 4, 3 * 120, seed=1, dtype=BF).to(DEV).requires_grad_(True), None, 3, 120)  # D = 40


# =================================================================================================
# c. elementwise backward kernels
# =================================================================================================
_SPECIAL = [0.0, -0.0, 10.0, -10.0, 1e-3, -1e-3]


def _act_inputs(n, pdt, ddt, seed):
    pre = _rand(n, seed=seed, scale=2.0)
    pre[:min(n, len(_SPECIAL))] = torch.tensor(_SPECIAL[:n])
    if n >= 2 * len(_SPECIAL):  # n = 1, 7: a second draw covers the rest
        pre[-len(_SPECIAL):] = torch.tensor(_SPECIAL[::-1])
    dy = _rand(n, seed=seed + 1)
    return pre.to(pdt), dy.to(ddt)


def _act_bound(ref, dy, out_dt):
    """test_gemm_gelu_epilogue_precision allows the activation 3e-7 + one f32 rounding; its derivative
    times dy: 3e-7 |dy| + the roundings of g and of the product; bf16 output: half a bf16 ulp more."""
    b = 3e-7 * dy.abs().double() + 2.0 ** -23 * ref.abs()
    return b if out_dt == F32 else b + 2.0 ** -8 * (ref.abs() + b)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("dts", [(F32, F32, F32), (BF, BF, BF), (BF, F32, F32), (F32, BF, BF)],
                         ids=["f32", "bf16", "bf16pre", "bf16dy"])
@pytest.mark.parametrize("n", [1, 7, 255, 4099])
def test_act_bwd(act, dts, n):
    _, ops, _ = _mods()
    pdt, ddt, xdt = dts
    pre, dy = _act_inputs(n, pdt, ddt, seed=n + act)
    got = ops.act_bwd(act, pre.to(DEV), dy.to(DEV), out_dtype=xdt)
    assert got.dtype == xdt and got.shape == pre.shape
    ref = dy.double() * R.act_grad_ref(act, pre)
    err = (got.double().cpu() - ref).abs()
    assert (err <= _act_bound(ref, dy, xdt)).all(), f"act_bwd( act={act} n={n}: max err {err.max().item():.3e}"
    if act == R.ACT_RELU:  # p > 0: zero gradient at +0 and -0
        assert not got.double().cpu()[(pre.double() == 0)].any()


def test_act_bwd_erf_and_fast_gelu_grads_agree():
    """comet_act_bwd (libm erff) and comet_act_bwd_colsum (the branch-free erf) on one input."""
    _, ops, _ = _mods()
    rows, cols = 67, 40
    pre, dy = _act_inputs(rows * cols, F32, F32, seed=5)
    pre, dy = pre.view(rows, cols), dy.view(rows, cols)
    a = ops.act_bwd(R.ACT_GELU, pre.to(DEV), dy.to(DEV), out_dtype=F32).double().cpu()
    db = torch.zeros(cols, device=DEV)
    b = ops.act_bwd_colsum(R.ACT_GELU, pre.to(DEV), dy.to(DEV), out_dtype=F32, dbias=db).double().cpu()
    ref = dy.double() * R.act_grad_ref(R.ACT_GELU, pre)
    bound = _act_bound(ref, dy, F32)
    assert ((a - ref).abs() <= bound).all() and ((b - ref).abs() <= bound).all()
    assert ((a - b).abs() <= 2 * bound).all()
    _close(db, ref.sum(0), 1e-5, 1e-5 * math.sqrt(rows), "db")


@pytest.mark.parametrize("n", [1, 3, 1025])
@pytest.mark.parametrize("a,b", [(1.0, 0.0), (0.5, -2.0), (0.0, 1.0)])
def test_axpby(n, a, b):
    """comet_axpby: y = a x + b y. With these (a, b) both products are exact, so the result is the
    correctly rounded sum; 1 ulp is allowed for a fused multiply-add of other coefficients."""
    L, ops, _ = _mods()
    x, y = _rand(n, seed=n), _rand(n + 4, seed=n + 1)
    xd, yd = x.to(DEV), y.to(DEV)
    yd[n:] = NAN
    L.check(L.load().comet_axpby(xd.data_ptr(), yd.data_ptr(), a, b, n, ops.stream()), "axpby")
    ref = (a * x.double() + b * y[:n].double()).float()
    ulp = torch.maximum(ref.abs(), torch.tensor(2.0 ** -126)) * 2.0 ** -23
    assert ((yd[:n].cpu() - ref).abs() <= ulp).all()
    assert torch.isnan(yd[n:]).all()


def test_axpby_b_zero_propagates_nan():
    """The kernel evaluates a * x[i] + b * y[i] as written: with b = 0 a NaN (or inf) already in y stays
    NaN (0 * NaN), so y must be initialised even when b = 0 -- the header's formula is literal."""
    L, ops, _ = _mods()
    x = _rand(9, seed=1).to(DEV)
    y = torch.full((9,), NAN, device=DEV)
    y[4] = 1.5
    y[5] = float("inf")
    L.check(L.load().comet_axpby(x.data_ptr(), y.data_ptr(), 2.0, 0.0, 9, ops.stream()), "axpby")
    assert torch.isnan(y[[0, 1, 2, 3, 5, 6, 7, 8]]).all() and y[4].item() == 2.0 * x[4].item()


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 9, 4100])
@pytest.mark.parametrize("with_out", [False, True])
def test_binary_add_and_add_relu(dtype, n, with_out):
    """comet_binary through ops.add / ops.add_relu / ops.binary: the f32 result rounded once."""
    _, ops, _ = _mods()
    a, b = _rand(n, seed=n, dtype=dtype), _rand(n, seed=n + 1, dtype=dtype)
    a[0] = -b[0]  # an exact zero through the relu
    ad, bd = a.to(DEV), b.to(DEV)
    s = (a.double() + b.double()).float()
    for op, ref in ((0, s), (1, torch.relu(s)), (2, (a.double() * b.double()).float())):
        if with_out:
            buf = torch.full((n + 3,), NAN, device=DEV, dtype=dtype)
            got = ops.add(ad, bd, out=buf[:n]) if op == 0 else ops.binary(op, ad, bd, out=buf[:n])
            assert got.data_ptr() == buf.data_ptr() and torch.isnan(buf[n:]).all()
        else:
            got = ops.add(ad, bd) if op == 0 else ops.add_relu(ad, bd) if op == 1 else ops.binary(2, ad, bd)
        assert got.dtype == dtype
        assert torch.equal(got.cpu(), ref.to(dtype)), f"binary op {op}"


def _cast_values(n, dtype):
    x = _rand(n, seed=n, scale=3.0)
    # exact ties between two bf16 values (to even: down, up, down), +-inf, NaN, +-0, the largest bf16
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, float("inf"), float("-inf"), NAN,
                         0.0, -0.0, 3.3895314e38])
    if n == 1:
        x[0] = ties[1]
    elif n == 7:
        x[:] = ties[:7]
    else:
        x[:ties.numel()] = ties
    return x.to(dtype)


@pytest.mark.parametrize("src,dst", [(F32, BF), (BF, F32), (F32, F32), (BF, BF)])
@pytest.mark.parametrize("n", [1, 7, 4099])
def test_cast_bit_exact(src, dst, n):
    """comet_cast vs torch.Tensor.to (round to nearest even), bit for bit, NaN to NaN."""
    _, ops, _ = _mods()
    x = _cast_values(n, src)
    buf = torch.zeros(n + 3, device=DEV, dtype=dst)
    got = ops.cast(x.to(DEV), dst, out=buf[:n]).cpu()
    ref = x.to(dst)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    it = torch.int32 if dst == F32 else torch.int16
    assert torch.equal(got[~nan].view(it), ref[~nan].view(it))
    assert not buf[n:].float().any()


# =================================================================================================
# d. LayerNorm backward
# =================================================================================================
def _ln_case(rows, cols, xdt=F32, dydt=F32, affine=False, seed=0, eps=1e-6):
    x = (_rand(rows, cols, seed=seed + 1, scale=2.0) + 0.7).to(xdt)
    dy = _rand(rows, cols, seed=seed + 2).to(dydt)
    w = _rand(cols, seed=seed + 3) if affine else None
    mean, rstd = R.ln_stats_ref(x, eps)
    return x, dy, w, mean.float().to(DEV), rstd.float().to(DEV), eps


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("rows", [1, 9, 67])
@pytest.mark.parametrize("cols", [8, 264, 384, 520, 1024])
@pytest.mark.parametrize("dydt", [F32, BF], ids=["dy32", "dy16"])
@pytest.mark.parametrize("affine", [False, True])
def test_layernorm_bwd_res(rows, cols, dydt, affine):
    """comet_layernorm_bwd_res (dres in ln_bwd_vec_kernel, CH = 4, nk = cols / 256 rounded up = 1..4, the
    last chunk partly filled at 8, 264 and 520) = dres + LN backward, and = layernorm_bwd(...) + dres."""
    _, ops, _ = _mods()
    x, dy, w, mean, rstd, eps = _ln_case(rows, cols, dydt=dydt, affine=affine, seed=rows + cols)
    dres = _rand(rows, cols, seed=9)
    dx_ref, dw_ref, db_ref = R.ln_bwd_ref(x, dy, None, w, eps)
    dw = torch.zeros(cols, device=DEV) if affine else None
    db = torch.zeros(cols, device=DEV) if affine else None
    dx = ops.layernorm_bwd_res(_dev(x), _dev(dy), _dev(dres), mean, rstd, _dev(w), dw, db)
    assert dx.dtype == F32
    _close(dx, dres.double() + dx_ref, 1e-4, 1e-4, "bwd_res dx")
    if affine:
        _close(dw, dw_ref, 1e-4, 1e-3, "bwd_res dw")
        _close(db, db_ref, 1e-4, 1e-3, "bwd_res db")
    plain = ops.layernorm_bwd(_dev(x), _dev(dy), mean, rstd, _dev(w)) + _dev(dres)
    _close(dx, plain, 1e-4, 1e-4, "bwd_res vs bwd + dres")


def test_layernorm_bwd_res_rejects_unsupported_shapes():
    L, ops, _ = _mods()
    lib = L.load()
    t = torch.zeros(4 * 264, device=DEV)
    p = t.data_ptr()
    rc = lib.comet_layernorm_bwd_res(L.F32, L.F32, p, p, p, p, p, None, p, None, None, 4, 130, ops.stream())
    assert rc == -1 and b"cols % 8 == 0" in lib.comet_last_error()
    rc = lib.comet_layernorm_bwd_res(L.BF16, L.F32, p, p, p, p, p, None, p, None, None, 4, 264, ops.stream())
    assert rc == -1 and b"x must be f32" in lib.comet_last_error()


@pytest.mark.parametrize("rows", [1, 9, 67])
@pytest.mark.parametrize("cols,dxdt", [(384, F32), (520, F32), (130, F32), (384, BF), (264, BF)])
def test_layernorm_bwd_accumulates(rows, cols, dxdt):
    """dx_accumulate = 1 adds into dx (ln_bwd_vec_kernel reads the previous dx in its own dtype, so a
    bf16 dx accumulates too, rounded once more; cols = 130: the scalar kernel, f32 dx only, with a
    weight) and dweight / dbias are += (pre-filled with 2.5)."""
    _, ops, _ = _mods()
    x, dy, w, mean, rstd, eps = _ln_case(rows, cols, affine=True, seed=rows + cols)
    prev = _rand(rows, cols, seed=4).to(dxdt)
    dx_ref, dw_ref, db_ref = R.ln_bwd_ref(x, dy, None, w, eps)
    dx = prev.to(DEV).clone()
    dw = torch.full((cols,), 2.5, device=DEV)
    db = torch.full((cols,), 2.5, device=DEV)
    out = ops.layernorm_bwd(_dev(x), _dev(dy), mean, rstd, _dev(w), dw, db, dx=dx, accumulate=True)
    assert out.data_ptr() == dx.data_ptr()
    want = prev.double() + dx_ref
    if dxdt == F32:
        _close(dx, want, 1e-4, 1e-4, "accumulated dx")
    else:
        err = (dx.double().cpu() - want).abs()
        tol = 1e-4 + 1e-4 * want.abs()
        assert (err <= tol + 2.0 ** -8 * (want.abs() + tol)).all(), f"accumulated bf16 dx: {err.max().item():.3e}"
    _close(dw, 2.5 + dw_ref, 1e-4, 1e-3, "dw +=")
    _close(db, 2.5 + db_ref, 1e-4, 1e-3, "db +=")


@pytest.mark.parametrize("rows", [1, 9, 67])
@pytest.mark.parametrize("cols", [264, 520, 1024])
def test_layernorm_bwd_all_bf16(rows, cols):
    """x, dy and dx all bf16: the only instantiation with 8-wide chunks (CH = 8 when no operand is
    4 bytes wide); nk = cols / 512 rounded up: 1 at 264, 2 at 520 (second chunk holds 8 of 512 columns)
    and 1024."""
    _, ops, _ = _mods()
    x, dy, w, mean, rstd, eps = _ln_case(rows, cols, xdt=BF, dydt=BF, affine=True, seed=rows + cols)
    assert all(t.element_size() == 2 for t in (x, dy)) and (cols + 511) // 512 == (1 if cols == 264 else 2)
    dx_ref, dw_ref, db_ref = R.ln_bwd_ref(x, dy, None, w, eps)
    dw, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
    dx = ops.layernorm_bwd(_dev(x), _dev(dy), mean, rstd, _dev(w), dw, db, dx_dtype=BF)
    assert dx.dtype == BF
    err = (dx.double().cpu() - dx_ref).abs()
    tol = 1e-4 + 1e-4 * dx_ref.abs()
    assert (err <= tol + 2.0 ** -8 * (dx_ref.abs() + tol)).all(), f"all-bf16 dx: {err.max().item():.3e}"
    _close(dw, dw_ref, 1e-4, 1e-3, "dw")
    _close(db, db_ref, 1e-4, 1e-3, "db")


@pytest.mark.parametrize("rows", [1, 9, 67])
@pytest.mark.parametrize("cols", [264, 130])
def test_layernorm_bwd_bf16_dy_f32_x(rows, cols):
    _, ops, _ = _mods()
    x, dy, w, mean, rstd, eps = _ln_case(rows, cols, dydt=BF, seed=rows + cols)
    dx = ops.layernorm_bwd(_dev(x), _dev(dy), mean, rstd)
    assert dx.dtype == F32
    _close(dx, R.ln_bwd_ref(x, dy, None, None, eps)[0], 1e-4, 1e-4, "bf16 dy -> f32 dx")


@pytest.mark.parametrize("rows", [9, 67])
@pytest.mark.parametrize("res", [False, True])
def test_layernorm_bwd_rows_per_wave_switch(rows, res, monkeypatch):
    """COMET_LNB_RPW = 1 / 64 regroup rows over waves only: dx bit for bit that of the default; dweight
    is summed by atomics in another order (the bound, not bits)."""
    _, ops, _ = _mods()
    cols = 384
    x, dy, w, mean, rstd, eps = _ln_case(rows, cols, affine=True, seed=rows)
    dres = _rand(rows, cols, seed=9).to(DEV)
    _, dw_ref, _ = R.ln_bwd_ref(x, dy, None, w, eps)

    def run():
        dw = torch.zeros(cols, device=DEV)
        if res:
            return ops.layernorm_bwd_res(_dev(x), _dev(dy), dres, mean, rstd, _dev(w), dw, None), dw
        return ops.layernorm_bwd(_dev(x), _dev(dy), mean, rstd, _dev(w), dw, None), dw
    monkeypatch.delenv("COMET_LNB_RPW", raising=False)
    base, _ = run()
    for rpw in ("1", "64"):
        monkeypatch.setenv("COMET_LNB_RPW", rpw)
        dx, dw = run()
        assert torch.equal(dx, base), f"rpw={rpw}"
        _close(dw, dw_ref, 1e-4, 1e-3, f"dw rpw={rpw}")


# =================================================================================================
# e. comet_adamw_multi
# =================================================================================================
_ADAMW_SIZES = [1, 2, 3, 5, 7, 8, 1023, 4097, 9, 15, 16, 17, 31, 33, 63, 65, 100, 127, 129, 255, 257, 511, 513, 6, 10, 11,
                13, 14, 2049, 4]


def _f32(v):
    return float(torch.tensor(v, dtype=F32).item())


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("clip", ["none", "above", "below"])
def test_adamw_multi_vs_ref(wd, clip):
    """30 tensors (MT_MAX = 24: two launches, the second with 6; tensors 24.. are checked like the rest),
    three steps with carried moments; every step is compared with adamw_ref of the state the kernel
    started that step from, with the f32 values of the hyper-parameters the ABI receives."""
    L, ops, _ = _mods()
    lib = L.load()
    n = len(_ADAMW_SIZES)
    assert n == 30 and n > 24
    lr, b1, b2, eps = _f32(1e-2), _f32(0.9), _f32(0.999), _f32(1e-8)
    wdf = _f32(wd)
    SENT = 12345.0
    bufs = {k: [torch.full((s + 5,), SENT, device=DEV) for s in _ADAMW_SIZES] for k in "pgmv"}
    for i, s in enumerate(_ADAMW_SIZES):
        bufs["p"][i][:s] = _rand(s, seed=i).to(DEV)
        bufs["m"][i][:s] = 0
        bufs["v"][i][:s] = 0
    arr = {k: (ctypes.c_void_p * n)(*[t.data_ptr() for t in bufs[k]]) for k in "pgmv"}
    sz = (ctypes.c_int64 * n)(*_ADAMW_SIZES)
    for step in (1, 2, 3):
        gs = [_rand(s, seed=1000 * step + i, scale=0.5) for i, s in enumerate(_ADAMW_SIZES)]
        for i, s in enumerate(_ADAMW_SIZES):
            bufs["g"][i][:s] = gs[i].to(DEV)
        sq = torch.tensor([sum((g.double() ** 2).sum().item() for g in gs)], dtype=F32)
        norm = math.sqrt(sq.item())
        max_norm = {"none": 0.0, "above": _f32(norm / 7.3), "below": _f32(norm * 1.5)}[clip]
        before = {k: [t[:s].double().cpu() for t, s in zip(bufs[k], _ADAMW_SIZES)] for k in "pmv"}
        sqd = sq.to(DEV)
        L.check(lib.comet_adamw_multi(arr["p"], arr["g"], arr["m"], arr["v"], sz, n, lr, b1, b2, eps, wdf, step,
                                      None if clip == "none" else sqd.data_ptr(), max_norm, ops.stream()), "adamw")
        torch.cuda.synchronize()
        worst = {"p": 0.0, "m": 0.0, "v": 0.0}
        for i, s in enumerate(_ADAMW_SIZES):
            pr, mr, vr, upd = R.adamw_ref(before["p"][i], gs[i], before["m"][i], before["v"][i], lr, b1, b2, eps, wdf,
                                          step, None if clip == "none" else sq.item(), max_norm)
            p, m, v = (bufs[k][i][:s].double().cpu() for k in "pmv")
            ulp = lambda t: torch.maximum(t.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64)) * 2.0 ** -23
            bp = 4 * lr * 2.0 ** -23 * (1 + upd.abs()) + 2 * ulp(pr)
            # m = m + (1 - b1) (g clip - m): each of the three roundings is half an ulp of its own result, so
            # where the sum cancels the 2 ulp are those of the largest term, not of the new m
            clipc = 1.0 if clip == "none" else min(1.0, max_norm / (math.sqrt(sq.item()) + 1e-6))
            mterm = torch.maximum(torch.maximum(before["m"][i].abs(), mr.abs()),
                                  ((1 - b1) * (gs[i].double() * clipc - before["m"][i])).abs())
            for k, got, ref, bound in (("p", p, pr, bp), ("m", m, mr, 2 * ulp(mterm)), ("v", v, vr, 2 * ulp(vr))):
                ratio = ((got - ref).abs() / bound).max().item()
                worst[k] = max(worst[k], ratio)
            for k in "pgmv":
                assert (bufs[k][i][s:] == SENT).all(), f"tensor {i} ({k}): write past its {s} elements"
        print(f"adamw wd={wd} clip={clip} step={step}: worst err / bound p {worst['p']:.2f} m {worst['m']:.2f} v {worst['v']:.2f}")
        assert worst["p"] <= 1 and worst["m"] <= 1 and worst["v"] <= 1, worst
        if step == 1 and clip == "above":  # the clip did scale the gradient: m = (1 - b1) g clip
            g0, m0 = gs[7].double(), bufs["m"][7][:4097].double().cpu()
            assert torch.allclose(m0, (1 - b1) * g0 / 7.3, rtol=1e-5, atol=0)
        if step == 1 and clip == "below":  # coef >= 1: exactly no clip
            none = R.adamw_ref(before["p"][7], gs[7], before["m"][7], before["v"][7], lr, b1, b2, eps, wdf, 1)[1]
            assert torch.equal(bufs["m"][7][:4097].cpu(), none.float())
    rc = lib.comet_adamw_multi(arr["p"], arr["g"], arr["m"], arr["v"], sz, n, lr, b1, b2, eps, wdf, 0, None, 0.0,
                               ops.stream())
    assert rc != 0 and b"step must be >= 1" in lib.comet_last_error()


# =================================================================================================
# f. autograd Functions vs autograd of the plain formulation
# =================================================================================================
def _leaf(t, dtype=F32):
    return None if t is None else t.to(DEV, dtype).requires_grad_(True)


def _leaf64(t):
    return None if t is None else t.double().detach().requires_grad_(True)


def _backward(outs, cots):
    pairs = [(o, c) for o, c in zip(outs, cots) if c is not None]
    torch.autograd.backward([o for o, _ in pairs], [c.to(o.device, o.dtype) for o, c in pairs])


def _cmp_grads(dev, ref, rtol, atol, what):
    for i, (d, r) in enumerate(zip(dev, ref)):
        if r is None:
            continue
        assert d.grad is not None, f"{what}: no gradient for input {i}"
        _close(d.grad, r.grad if r.grad is not None else torch.zeros_like(r), rtol, atol, f"{what} grad[{i}]")


def _act_torch(act, t):
    return {0: lambda v: v, 1: TF.gelu, 2: torch.relu, 3: torch.sigmoid}[act](t)


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("N", [24, 40])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("extras", ["plain", "bias", "bias_resid_beta"])
def test_linear_function_f32(rows, N, act, extras, monkeypatch):
    """functional._Linear in f32: the fallback branch of _linear_bwd (comet_act_bwd + comet_colsum, never
    comet_act_bwd_colsum), for every activation with and without bias / residual / beta."""
    _, ops, F = _mods()
    counts = {}
    for name in ("act_bwd", "act_bwd_colsum", "colsum"):
        _count(monkeypatch, ops, name, counts)
    K = 40
    x, w = _rand(3, rows, K, seed=1), _rand(N, K, seed=2, scale=K ** -0.5)
    b = _rand(N, seed=3) if extras != "plain" else None
    r = _rand(3, rows, N, seed=4) if extras == "bias_resid_beta" else None
    beta = 0.5 if r is not None else 1.0
    cot = _rand(3, rows, N, seed=5)
    dev = [_leaf(t) for t in (x, w, b, r)]
    with F.precision(F32):
        y = F.linear(dev[0], dev[1], dev[2], act=act, resid=dev[3], beta=beta, out_dtype=F32)
        y.backward(cot.to(DEV))
    assert "act_bwd_colsum" not in counts and counts.get("act_bwd", 0) == (1 if act else 0)
    assert counts.get("colsum", 0) == (1 if b is not None else 0)
    ref = [_leaf64(t) for t in (x, w, b, r)]
    yr = _act_torch(act, ref[0] @ ref[1].t() + (ref[2] if b is not None else 0))
    if r is not None:
        yr = yr + beta * ref[3]
    yr.backward(cot.double())
    tol = 2e-5
    _close(y, yr, tol, tol * math.sqrt(K), "linear y")
    _cmp_grads(dev, ref, tol, tol * math.sqrt(max(K, 3 * rows)), f"linear act={act} {extras}")


def _bf16_model_check(dev_grads, plain_grads, model_grads, what):
    """bound = 3 e, e = the CPU rounding model's error relative to max|plain f64 gradient|."""
    names, devs = dev_grads
    for name, d, p, m in zip(names, devs, plain_grads, model_grads):
        scale = p.abs().max().item()
        e = ((m - p).abs().max() / scale).item()
        err = ((d.double().cpu() - p).abs().max() / scale).item()
        print(f"{what} {name}: err {err:.3e} of max|ref|, model e {e:.3e}")
        assert e < 2e-2
        # (+ 2e-5: f32 accumulation where the model rounds nothing, e.g. the bias gradient of bf16 cotangents)
        assert err <= 3 * e + 2e-5, f"{what} {name}: {err:.3e} > 3 e = {3 * e:.3e}"


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("N,branch", [(24, "act_bwd_colsum"), (20, "act_bwd")])
def test_linear_function_bf16(rows, N, branch, monkeypatch):
    """functional._Linear in bf16 with GELU and bias: N % 8 == 0 takes comet_act_bwd_colsum (one pass),
    N = 20 the comet_act_bwd + comet_colsum + cast fallback."""
    _, ops, F = _mods()
    counts = {}
    for name in ("act_bwd", "act_bwd_colsum", "colsum"):
        _count(monkeypatch, ops, name, counts)
    K = 40
    x, w, b = _rand(rows, K, seed=1), _rand(N, K, seed=2, scale=K ** -0.5), _rand(N, seed=3)
    cot = _rand(rows, N, seed=5)
    dev = [_leaf(t) for t in (x, w, b)]
    with F.precision(BF):
        y = F.linear(dev[0], dev[1], dev[2], act=R.ACT_GELU)
        y.backward(cot.to(DEV, BF))
    assert y.dtype == BF
    assert (counts.get("act_bwd_colsum", 0) > 0) == (branch == "act_bwd_colsum")
    assert (counts.get("act_bwd", 0) > 0) == (branch == "act_bwd") and (counts.get("colsum", 0) > 0) == (branch == "act_bwd")
    plain = [_leaf64(t) for t in (x, w, b)]
    TF.gelu(plain[0] @ plain[1].t() + plain[2]).backward(R.bf16(cot.double()))
    model = [_leaf64(t) for t in (x, w, b)]
    R.linear_rounded(model[0], model[1], model[2], R.ACT_GELU).backward(R.bf16(cot.double()))
    _bf16_model_check((("dx", "dw", "db"), [t.grad for t in dev]), [t.grad for t in plain], [t.grad for t in model],
                      f"linear bf16 rows={rows} N={N}")


def _mlp_models(x, w1, b1, w2, b2, r, cot):
    plain = [_leaf64(t) for t in (x, w1, b1, w2, b2, r)]
    (TF.gelu(plain[0] @ plain[1].t() + plain[2]) @ plain[3].t() + plain[4] + plain[5]).backward(cot.double())
    model = [_leaf64(t) for t in (x, w1, b1, w2, b2, r)]
    h = R.linear_rounded(model[0], model[1], model[2], R.ACT_GELU)
    R.linear_rounded(h, model[3], model[4], resid=model[5], out_bf16=False).backward(cot.double())
    return [t.grad for t in plain], [t.grad for t in model]


@pytest.mark.parametrize("rows,C,Hd,N,branch", [(67, 40, 24, 40, "two_gemm"), (1, 24, 40, 24, "two_gemm"),
                                                (4133, 64, 1024, 256, "dact")])
def test_mlp_function_bf16(rows, C, Hd, N, branch, monkeypatch):
    """functional._Mlp (bf16 only; f32 takes two _Linear nodes): fc2's input gradient fused with the GELU
    backward (comet_gemm_dact, 4133 x 256 x 1024) or the GEMM + comet_act_bwd_colsum fallback."""
    _, ops, F = _mods()
    counts = {}
    for name in ("linear_dact", "act_bwd_colsum"):
        _count(monkeypatch, ops, name, counts)
    monkeypatch.setattr(F, "_MLP_UNFUSED", False)
    x, r, cot = _rand(rows, C, seed=1), _rand(rows, N, seed=6), _rand(rows, N, seed=7)
    w1, b1 = _rand(Hd, C, seed=2, scale=C ** -0.5), _rand(Hd, seed=3)
    w2, b2 = _rand(N, Hd, seed=4, scale=Hd ** -0.5), _rand(N, seed=5)
    dev = [_leaf(t) for t in (x, w1, b1, w2, b2, r)]
    with F.precision(BF):
        y = F.mlp(*dev[:5], resid=dev[5])
        y.backward(cot.to(DEV))
    assert y.dtype == F32
    assert (counts.get("linear_dact", 0) == 1) == (branch == "dact"), counts
    plain, model = _mlp_models(x, w1, b1, w2, b2, r, cot)
    _bf16_model_check((("dx", "dw1", "db1", "dw2", "db2", "dres"), [t.grad for t in dev]), plain[:5], model[:5],
                      f"mlp bf16 {branch}")
    _close(dev[5].grad, cot, 0, 0, "mlp dres")


def test_mlp_f32_is_two_linear_nodes(monkeypatch):
    _, ops, F = _mods()
    counts = {}
    for name in ("linear_dact", "act_bwd_colsum", "act_bwd"):
        _count(monkeypatch, ops, name, counts)
    rows, C, Hd, N = 67, 40, 24, 40
    x, r, cot = _rand(rows, C, seed=1), _rand(rows, N, seed=6), _rand(rows, N, seed=7)
    w1, b1 = _rand(Hd, C, seed=2, scale=C ** -0.5), _rand(Hd, seed=3)
    w2, b2 = _rand(N, Hd, seed=4, scale=Hd ** -0.5), _rand(N, seed=5)
    dev = [_leaf(t) for t in (x, w1, b1, w2, b2, r)]
    with F.precision(F32):
        F.mlp(*dev[:5], resid=dev[5]).backward(cot.to(DEV))
    assert counts == {"act_bwd": 1}
    plain, _ = _mlp_models(x, w1, b1, w2, b2, r, cot)
    for i, (d, p) in enumerate(zip(dev, plain)):
        _close(d.grad, p, 2e-5, 2e-5 * math.sqrt(rows), f"mlp f32 grad[{i}]")


@pytest.mark.parametrize("prec", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,C", [(1, 24), (67, 40)])
@pytest.mark.parametrize("used", ["both", "q", "kv"])
def test_linear_pair_function(prec, rows, C, used):
    """functional._LinearPair: both halves of the [3C, C] weight gradient from one node; an unused
    output leaves its half zero."""
    _, ops, F = _mods()
    xq, xkv = _rand(2, rows, C, seed=1), _rand(2, rows + 2, C, seed=2)
    w, b = _rand(3 * C, C, seed=3, scale=C ** -0.5), _rand(3 * C, seed=4)
    cq, ckv = _rand(2, rows, C, seed=5), _rand(2, rows + 2, 2 * C, seed=6)
    if prec == BF:
        cq, ckv = cq.to(BF).float(), ckv.to(BF).float()
    cots = (cq if used != "kv" else None, ckv if used != "q" else None)
    dev = [_leaf(t) for t in (xq, xkv, w, b)]
    with F.precision(prec):
        _backward(F.linear_pair(*dev, C), cots)

    def run(rounded):
        t = [_leaf64(v) for v in (xq, xkv, w, b)]
        if rounded:
            outs = (R.linear_rounded(t[0], t[2][:C], t[3][:C]), R.linear_rounded(t[1], t[2][C:], t[3][C:]))
        else:
            outs = (t[0] @ t[2][:C].t() + t[3][:C], t[1] @ t[2][C:].t() + t[3][C:])
        _backward(outs, cots)
        return [v.grad if v.grad is not None else torch.zeros_like(v) for v in t]
    plain = run(False)
    idx = [i for i in range(4) if not (i == 0 and used == "kv") and not (i == 1 and used == "q")]
    if prec == F32:
        for i in idx:
            _close(dev[i].grad, plain[i], 2e-5, 2e-5 * math.sqrt(max(C, 2 * rows + 4)), f"linear_pair grad[{i}]")
    else:
        model = run(True)
        names = ("dxq", "dxkv", "dw", "db")
        _bf16_model_check(([names[i] for i in idx], [dev[i].grad for i in idx]), [plain[i] for i in idx],
                          [model[i] for i in idx], f"linear_pair bf16 {used}")
    if used == "q":
        assert dev[1].grad is None and not dev[2].grad[C:].any() and not dev[3].grad[C:].any()
    if used == "kv":
        assert dev[0].grad is None and not dev[2].grad[:C].any() and not dev[3].grad[:C].any()


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("case", ["res_only", "normed_only", "both_vec", "both_cols20", "both_bf16"])
def test_res_layer_norm_function(rows, case, monkeypatch):
    """functional._ResLayerNorm's four backward branches: only the residual used (no kernel), only the
    normed output (comet_layernorm_bwd), both with f32 x and cols % 8 == 0 (comet_layernorm_bwd_res), both
    with cols = 20 (comet_layernorm_bwd + add); both_bf16: the bwd_res branch fed a bf16 dy."""
    _, ops, F = _mods()
    counts = {}
    for name in ("layernorm_bwd", "layernorm_bwd_res"):
        _count(monkeypatch, ops, name, counts)
    cols = 20 if case == "both_cols20" else 384
    prec = BF if case == "both_bf16" else F32
    x = _rand(2, rows, cols, seed=1, scale=2.0) + 0.5
    c_res = None if case == "normed_only" else _rand(2, rows, cols, seed=2)
    c_y = None if case == "res_only" else _rand(2, rows, cols, seed=3)
    if prec == BF:
        c_y = c_y.to(BF).float()
    xd = _leaf(x)
    with F.precision(prec):
        res, y = F.res_layer_norm(xd, eps=1e-6)
        assert y.dtype == prec and res.dtype == F32
        _backward((res, y), (c_res, c_y))
    want = {"res_only": {}, "normed_only": {"layernorm_bwd": 1}, "both_vec": {"layernorm_bwd_res": 1},
            "both_cols20": {"layernorm_bwd": 1}, "both_bf16": {"layernorm_bwd_res": 1}}[case]
    assert counts == want
    xr = _leaf64(x)
    _backward((xr * 1.0, TF.layer_norm(xr, (cols,), eps=1e-6)), (c_res, c_y))
    _close(y, TF.layer_norm(x.double(), (cols,), eps=1e-6), *((1e-5, 1e-5) if prec == F32 else (2.0 ** -8, 1e-5)), "normed")
    assert torch.equal(res.detach().cpu(), x)
    _close(xd.grad, xr.grad, 1e-4, 1e-4, f"res_layer_norm {case}")


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("used", ["both", "f32_only", "bf16_only"])
def test_layer_norm_dual_function_bf16(rows, used, monkeypatch):
    """functional._LayerNormDual (bf16 compute): dx from the f32 and the bf16 cotangent in one kernel."""
    _, ops, F = _mods()
    counts = {}
    _count(monkeypatch, ops, "layernorm_bwd", counts)
    cols = 384
    x = _rand(2, rows, cols, seed=1, scale=2.0) + 0.5
    c32 = None if used == "bf16_only" else _rand(2, rows, cols, seed=2)
    c16 = None if used == "f32_only" else _rand(2, rows, cols, seed=3).to(BF).float()
    xd = _leaf(x)
    with F.precision(BF):
        y, y16 = F.layer_norm_dual(xd, eps=1e-6)
        assert y.dtype == F32 and y16.dtype == BF
        _backward((y, y16), (c32, c16))
    assert counts == {"layernorm_bwd": 1}
    xr = _leaf64(x)
    yr = TF.layer_norm(xr, (cols,), eps=1e-6)
    _backward((yr, yr * 1.0), (c32, c16))
    _close(y, yr, 1e-5, 1e-5, "dual y")
    _close(y16, yr, 2.0 ** -8, 1e-5, "dual y16")
    _close(xd.grad, xr.grad, 1e-4, 1e-4, f"layer_norm_dual {used}")


def test_layer_norm_dual_function_f32_is_one_layer_norm():
    _, ops, F = _mods()
    x = _rand(67, 40, seed=1, scale=2.0)
    xd = _leaf(x)
    with F.precision(F32):
        y, y2 = F.layer_norm_dual(xd, eps=1e-6)
    assert y is y2
    (y * 2).sum().backward()
    xr = _leaf64(x)
    (TF.layer_norm(xr, (40,), eps=1e-6) * 2).sum().backward()
    _close(xd.grad, xr.grad, 1e-4, 1e-4, "dual f32")


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("cols", [24, 130, 384])
@pytest.mark.parametrize("relu", [False, True])
def test_layer_norm_affine_and_relu_functions(rows, cols, relu, monkeypatch):
    """functional._LayerNorm (affine) and _LayerNormReLU (comet_act_bwd on the saved output, then the LN
    backward); cols = 130 takes the scalar LN kernels."""
    _, ops, F = _mods()
    counts = {}
    for name in ("layernorm_bwd", "act_bwd"):
        _count(monkeypatch, ops, name, counts)
    x, w, b = _rand(2, rows, cols, seed=1, scale=2.0) + 0.3, _rand(cols, seed=2), _rand(cols, seed=3)
    cot = _rand(2, rows, cols, seed=4)
    dev = [_leaf(t) for t in (x, w, b)]
    with F.precision(F32):
        y = F.layer_norm_relu(*dev, eps=1e-5) if relu else F.layer_norm(*dev, eps=1e-5)
        y.backward(cot.to(DEV))
    assert counts == ({"layernorm_bwd": 1, "act_bwd": 1} if relu else {"layernorm_bwd": 1})
    ref = [_leaf64(t) for t in (x, w, b)]
    yr = TF.layer_norm(ref[0], (cols,), ref[1], ref[2], 1e-5)
    if relu:  # (a pre-activation within f32 round-off of 0 could land on the other side of the ReLU)
        assert (yr.detach().abs() > 1e-5).all(), "a pre-activation within 1e-5 of zero: pick another seed"
        yr = torch.relu(yr)
    yr.backward(cot.double())
    _close(y, yr, 1e-5, 1e-5, "ln y")
    _close(dev[0].grad, ref[0].grad, 1e-4, 1e-4, "ln dx")
    _close(dev[1].grad, ref[1].grad, 1e-4, 1e-3, "ln dw")
    _close(dev[2].grad, ref[2].grad, 1e-4, 1e-3, "ln db")


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("C", [24, 40])
def test_elementwise_functions(rows, C):
    """functional.add / add_rows / cast / rowscale vs the plain formulation (one f32 rounding)."""
    _, ops, F = _mods()
    a, b, cot = _rand(2, rows, C, seed=1), _rand(2, rows, C, seed=2), _rand(2, rows, C, seed=3)
    table = _rand(rows, C, seed=4)
    wrow = _rand(2, rows, 1, seed=5)
    tol = dict(rtol=2.0 ** -23, atol=1e-7)
    # add
    dev = [_leaf(a), _leaf(b)]
    y = F.add(*dev)
    y.backward(cot.to(DEV))
    _close(y, a.double() + b.double(), **tol, what="add")
    assert torch.equal(dev[0].grad.cpu(), cot) and torch.equal(dev[1].grad.cpu(), cot)
    # add_rows: x + table[row % period]
    xd = _leaf(a)
    y = F.add_rows(xd, table.to(DEV), rows)
    y.backward(cot.to(DEV))
    _close(y, a.double() + table.double()[None], **tol, what="add_rows")
    assert torch.equal(xd.grad.cpu(), cot)
    # cast: f32 -> bf16 -> gradient back in f32
    xd = _leaf(a)
    y = F.cast(xd, BF)
    y.backward(cot.to(DEV, BF))
    assert torch.equal(y.detach().cpu(), a.to(BF)) and torch.equal(xd.grad.cpu(), cot.to(BF).float()) and xd.grad.dtype == F32
    # rowscale
    dev = [_leaf(a), _leaf(wrow)]
    y = F.rowscale(*dev)
    y.backward(cot.to(DEV))
    ref = [_leaf64(a), _leaf64(wrow)]
    (ref[0] * ref[1]).backward(cot.double())
    _close(y, ref[0] * ref[1], **tol, what="rowscale")
    _close(dev[0].grad, ref[0].grad, **tol, what="rowscale dx")
    _close(dev[1].grad, ref[1].grad, 1e-5, 1e-5 * math.sqrt(C), "rowscale dw")


@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("cov", ["none", "grad", "nograd"])
def test_harmonic_function(rows, append, cov):
    """functional._Harmonic vs harmonic_ref. The kernel rounds e = x f to f32 as the reference model does,
    so sin / cos move by up to 2^-24 |x| f, times f in dx: the bound sums that over both halves."""
    _, ops, F = _mods()
    dim, n = 3, 4
    x = _rand(rows, dim, seed=1)
    c = (_rand(rows, dim, seed=2).abs() * 0.05) if cov != "none" else None
    f = 2.0 ** torch.arange(n, dtype=F32)
    cot = _rand(rows, dim * (2 * n + int(append)), seed=3)
    xd = _leaf(x)
    cd = None if c is None else (_leaf(c) if cov == "grad" else c.to(DEV))
    y = F.harmonic(xd, f.to(DEV), append, cd)
    y.backward(cot.to(DEV))
    xr, cr = _leaf64(x), _leaf64(c)
    yr = R.harmonic_ref(xr, f.double(), append, cr)
    yr.backward(cot.double())
    xmax, gmax, f2 = x.abs().max().item(), cot.abs().max().item(), (f.double() ** 2).sum().item()
    _close(y, yr, 1e-6, 2.0 ** -23 * (1 + xmax * f.max().item()), "harmonic y")
    _close(xd.grad, xr.grad, 1e-5, 2.0 ** -22 * (1 + xmax) * f2 * gmax, "harmonic dx")
    if cov == "grad":
        _close(cd.grad, cr.grad, 1e-5, 2.0 ** -22 * (1 + xmax) * f2 * f.max().item() * gmax, "harmonic dcov")
    elif cov == "nograd":
        assert cd.grad is None


@pytest.mark.parametrize("unused", [None, 0, 1, 2, (0, 1), (1, 2)])
def test_frame_split_function(unused):
    """functional._FrameSplit: tok -> (tok[:, 0:1], tok[:, 0], tok[:, 1:]); every None branch of its
    backward (each output unused in turn, and pairs of them)."""
    _, ops, F = _mods()
    B, S, P, C = 2, 3, 5, 24
    tok = _rand(B, S, P, C, seed=1)
    skip = () if unused is None else (unused,) if isinstance(unused, int) else unused
    cots = [_rand(B, 1, P, C, seed=2), _rand(B, P, C, seed=3), _rand(B, S - 1, P, C, seed=4)]
    cots = [None if i in skip else c for i, c in enumerate(cots)]
    td = _leaf(tok)
    outs = F.frame_split(td)
    assert [tuple(o.shape) for o in outs] == [(B, 1, P, C), (B, P, C), (B, S - 1, P, C)]
    _backward(outs, cots)
    tr = _leaf64(tok)
    _backward((tr[:, 0:1], tr[:, 0], tr[:, 1:]), cots)
    assert torch.equal(td.grad.cpu(), tr.grad.float())


def test_frame_join_function():
    _, ops, F = _mods()
    t0, fo, cot = _rand(2, 1, 5, 24, seed=1), _rand(2, 3, 5, 24, seed=2), _rand(2, 4, 5, 24, seed=3)
    dev = [_leaf(t0), _leaf(fo)]
    y = F.frame_join(*dev)
    y.backward(cot.to(DEV))
    assert torch.equal(y.detach().cpu(), torch.cat([t0, fo], 1))
    assert torch.equal(dev[0].grad.cpu(), cot[:, 0:1]) and torch.equal(dev[1].grad.cpu(), cot[:, 1:])
    assert dev[1].grad.is_contiguous()


def test_gather_rows_function():
    """functional._GatherRows: repeated rows accumulate, rows never selected get zero."""
    _, ops, F = _mods()
    x = _rand(9, 24, seed=1)
    idx = torch.tensor([3, 3, 0, 8, 3, 5, 0])
    cot = _rand(idx.numel(), 24, seed=2)
    xd = _leaf(x)
    y = F.gather_rows(xd, idx.to(DEV))
    y.backward(cot.to(DEV))
    xr = _leaf64(x)
    xr[idx].backward(cot.double())
    assert torch.equal(y.detach().cpu(), x[idx])
    _close(xd.grad, xr.grad, 0, 3 * 2.0 ** -23 * cot.abs().max().item(), "gather_rows dx")  # index_add_ of <= 3 rows, any order
    assert not xd.grad[[1, 2, 4, 6, 7]].any()
