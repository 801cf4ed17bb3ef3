"""Float64 restatements of the training-side operators (no GPU, no project imports).

Every function is written from the header comments of include/comet_hip.h and the formulas in the
kernel sources' comments, in plain torch float64, so the GPU tests compare the kernels with an
independent statement of the same operation. tests/test_backward_ref_cpu.py checks these functions
against autograd / gradcheck / torch.optim, so the GPU tests do not rest on an unchecked helper.
"""
import math

import torch
import torch.nn.functional as F

ACT_NONE, ACT_GELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3

# ---------------------------------------------------------------------------------------------
# attention backward cases shared by the CPU tolerance measurement and the GPU tests
# ---------------------------------------------------------------------------------------------
ATTN_DS = (32, 48, 64, 96)
ATTN_B, ATTN_H = 2, 3
# 64-row kernels, dispatched naturally (lq < 64 or lk < 64)
ATTN_SMALL = ((1, 16), (1, 200), (9, 1), (5, 11), (63, 63), (63, 200), (200, 63), (130, 3), (3, 130))
# 64-row kernels forced by COMET_ATTN_BWD16=1: multi-tile loops, ragged last tiles on both axes
ATTN_FORCED = ((64, 64), (65, 129), (129, 65))
# wide (128-row) kernels at their workgroup boundaries
ATTN_WIDE = ((64, 64), (127, 128), (128, 127), (129, 129), (64, 257), (257, 64))
ATTN_SHAPES = tuple(dict.fromkeys(ATTN_SMALL + ATTN_FORCED + ATTN_WIDE))


def bf16(x):
    """x (f64) rounded to bf16, as f64 (through f32: the second rounding moves a value only when it
    lies within 2^-29 relative of a bf16 tie, far below anything measured here)."""
    return x.float().bfloat16().double()


def attn_inputs(D, lq, lk, seed=50, heads=ATTN_H, batch=ATTN_B, logit_gain=None):
    """Seeded bf16 q [B, lq, C], kv [B, lk, 2C] (k | v), do [B, lq, C]. logit_gain: scale q and k so
    that max |s * D^-0.5| is about that value (softmax rows from one-hot to flat)."""
    C = heads * D
    g = torch.Generator().manual_seed(seed + 1000 * D + 10 * lq + lk)
    q = torch.randn(batch, lq, C, generator=g)
    kv = torch.randn(batch, lk, 2 * C, generator=g)
    do = torch.randn(batch, lq, C, generator=g)
    if logit_gain is not None:
        # rows differ in gain, so some stay flat and some become one-hot
        row = torch.linspace(0.02, 1.0, lq).view(1, lq, 1)
        s = _heads(q.double() * row, heads) @ _heads(kv[..., :C].double(), heads).transpose(-1, -2) * D ** -0.5
        a = math.sqrt(logit_gain / s.abs().max().item())
        q = q * row * a
        kv[..., :C] *= a
    return q.to(torch.bfloat16), kv.to(torch.bfloat16), do.to(torch.bfloat16)


def _heads(x, heads):
    B, L, C = x.shape
    return x.reshape(B, L, heads, C // heads).transpose(1, 2)


def _merge(x):
    B, H, L, D = x.shape
    return x.transpose(1, 2).reshape(B, L, H * D)


def attn_bwd_ref(q, k, v, do, heads, scale):
    """(o, lse, dq, dk, dv) of o = softmax(q k^T * scale) v per head by f64 autograd; all [B, L, C]
    but lse [B, heads, lq]."""
    qh = _heads(q.double(), heads).detach().requires_grad_(True)
    kh = _heads(k.double(), heads).detach().requires_grad_(True)
    vh = _heads(v.double(), heads).detach().requires_grad_(True)
    s = qh @ kh.transpose(-1, -2) * scale
    o = torch.softmax(s, -1) @ vh
    o.backward(_heads(do.double(), heads))
    return (_merge(o.detach()), torch.logsumexp(s.detach(), -1), _merge(qh.grad), _merge(kh.grad), _merge(vh.grad))


def attn_bwd_rounded(q, k, v, do, heads, scale):
    """The same formulas with the roundings comet_attention_bwd documents, nothing else changed:
    bf16 inputs; o rounded to bf16 before delta = rowsum(dO * O); P and dS (unscaled, as the kernel
    packs them) rounded to bf16 before the second GEMMs; f64 accumulation; bf16 outputs. The
    tolerance model of the bf16 tests, not an expected value. Returns (dq, dk, dv)."""
    qh, kh, vh, gh = (_heads(bf16(t.double()), heads) for t in (q, k, v, do))
    s = qh @ kh.transpose(-1, -2) * scale
    P = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    o = bf16(P @ vh)
    delta = (gh * o).sum(-1, keepdim=True)
    dP = gh @ vh.transpose(-1, -2)
    P16 = bf16(P)
    dS16 = bf16(P * (dP - delta))
    dv = bf16(P16.transpose(-1, -2) @ gh)
    dq = bf16(dS16 @ kh * scale)
    dk = bf16(dS16.transpose(-1, -2) @ qh * scale)
    return _merge(dq), _merge(dk), _merge(dv)


def attn_bwd_floor(q, k, v, do, heads, scale):
    """Absolute f32 round-off floor per output (dq, dk, dv): D * 2^-23 times the largest value of the
    same sums taken over absolute values. dS = P (dP - delta) subtracts two D-term f32 dot products;
    where that difference cancels to zero in exact arithmetic (lk = 1: P = 1, dP = delta, so dq = dk = 0)
    the reference is 0 and only this floor is a meaningful scale. It is three orders of magnitude below
    the bf16 rounding error wherever the reference does not vanish."""
    qh, kh, vh, gh = (_heads(t.double(), heads).abs() for t in (q, k, v, do))
    D = qh.shape[-1]
    s = _heads(q.double(), heads) @ _heads(k.double(), heads).transpose(-1, -2) * scale
    P = torch.softmax(s, -1)
    dPa = gh @ vh.transpose(-1, -2)
    dSa = P * (dPa + (P * dPa).sum(-1, keepdim=True))
    u = D * 2.0 ** -23
    return (u * (dSa @ kh * scale).max().item(), u * (dSa.transpose(-1, -2) @ qh * scale).max().item(),
            u * (P.transpose(-1, -2) @ gh).max().item())


def attn_model_error(q, k, v, do, heads, scale):
    """e = max|rounded - ref| / max(max|ref|, floor) per output -> ((e_dq, e_dk, e_dv), refs, floors);
    refs = (o, lse, dq, dk, dv) of attn_bwd_ref."""
    refs = attn_bwd_ref(q, k, v, do, heads, scale)
    rnd = attn_bwd_rounded(q, k, v, do, heads, scale)
    fl = attn_bwd_floor(q, k, v, do, heads, scale)
    e = tuple(((r - t).abs().max() / max(t.abs().max().item(), f)).item() for r, t, f in zip(rnd, refs[2:], fl))
    return e, refs, fl


def attn_probs_ref(s, lse, scale):
    """probs[r, j] = exp(s[r, j] * scale - lse[r]); s [rows, cols], lse [rows]."""
    return torch.exp(s.double() * scale - lse.double()[:, None])


def attn_delta_ref(do, o, heads):
    """delta[b, h, q] = sum_d dO[b, q, h*D + d] * O[b, q, h*D + d] -> [B, heads, lq]."""
    return (_heads(do.double(), heads) * _heads(o.double(), heads)).sum(-1)


def attn_dsoftmax_ref(p, dp, delta, scale):
    """dS[r, j] = P[r, j] * (dP[r, j] - delta[r]) * scale."""
    return p.double() * (dp.double() - delta.double()[:, None]) * scale


# ---------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------
def act_ref(act, x):
    x = x.double()
    if act == ACT_GELU:
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))
    if act == ACT_RELU:
        return torch.clamp_min(x, 0)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    return x


def act_grad_ref(act, pre):
    """d act(pre) / d pre: NONE 1, exact-erf GELU cdf + pre * pdf, RELU pre > 0, SIGMOID s (1 - s)."""
    p = pre.double()
    if act == ACT_GELU:
        return 0.5 * (1 + torch.erf(p / math.sqrt(2))) + p * torch.exp(-0.5 * p * p) / math.sqrt(2 * math.pi)
    if act == ACT_RELU:
        return (p > 0).double()
    if act == ACT_SIGMOID:
        s = torch.sigmoid(p)
        return s * (1 - s)
    return torch.ones_like(p)


# ---------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------
def ln_bwd_ref(x, dy, dy2=None, weight=None, eps_stats=1e-5):
    """(dx, dweight, dbias) of F.layer_norm(x, weight, bias) for the cotangent dy (+ dy2) in f64;
    dweight / dbias are None without a weight."""
    xr = x.double().detach().requires_grad_(True)
    C = x.shape[-1]
    w = weight.double().detach().requires_grad_(True) if weight is not None else None
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True) if weight is not None else None
    y = F.layer_norm(xr, (C,), w, b, eps_stats)
    g = dy.double() if dy2 is None else dy.double() + dy2.double()
    y.backward(g)
    return xr.grad, (w.grad if w is not None else None), (b.grad if b is not None else None)


def ln_stats_ref(x, eps):
    """(mean, rstd) per row in f64 (biased variance, as nn.LayerNorm)."""
    xd = x.double()
    return xd.mean(-1), 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + eps)


# ---------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------
def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, sqnorm=None, max_norm=0.0):
    """One torch.optim.AdamW step in f64 as the comment above adamw_kernel states it (new tensors):
    g *= min(1, max_norm / (sqrt(sqnorm) + 1e-6)) when sqnorm is given; p *= 1 - lr wd;
    m.lerp_(g, 1 - b1); v = b2 v + (1 - b2) g^2; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).
    Returns (p, m, v, m / denom)."""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if sqnorm is not None:
        g = g * min(1.0, max_norm / (math.sqrt(float(sqnorm)) + 1e-6))
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    upd = m / (torch.sqrt(v) / math.sqrt(bc2) + eps)
    return p - lr / bc1 * upd, m, v, upd


# ---------------------------------------------------------------------------------------------
# harmonic embedding
# ---------------------------------------------------------------------------------------------
def harmonic_ref(x, freqs, append_input, diag_cov=None):
    """HarmonicEmbedding.forward: cat(sin(e), cos(e) [, x]) with e[..., i * n + k] = x[..., i] * f[k];
    with diag_cov both halves are scaled by exp(-0.5 * diag_cov[..., i] * f[k]^2)."""
    f = freqs.to(x.dtype)
    e = (x[..., None] * f).reshape(*x.shape[:-1], -1)
    e = torch.cat([e, e + 0.5 * math.pi], -1)
    y = torch.sin(e)
    if diag_cov is not None:
        var = (diag_cov[..., None] * f * f).reshape(*x.shape[:-1], -1)
        y = y * torch.exp(-0.5 * torch.cat([var, var], -1))
    return torch.cat([y, x], -1) if append_input else y


# ---------------------------------------------------------------------------------------------
# bf16 tolerance models of the Linear-family autograd Functions (test_backward_gpu.py section f)
# ---------------------------------------------------------------------------------------------
class _Round(torch.autograd.Function):
    """bf16 rounding of the value in the forward and of the gradient in the backward (a bf16 tensor's
    gradient is bf16)."""

    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


class _RoundFwd(torch.autograd.Function):
    """bf16 rounding of the value only (an f32 tensor cast for a GEMM whose gradient stays f32)."""

    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    """bf16 rounding of the gradient only (the pre-activation gradient, written in bf16 as the operand
    of both backward GEMMs and summed, rounded, into the bias gradient)."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


def rnd(x):
    return _Round.apply(x)


def rnd_fwd(x):
    return _RoundFwd.apply(x)


def linear_rounded(x, w, b, act=ACT_NONE, resid=None, out_bf16=True):
    """act(rnd(x) rnd(w)^T + b) (+ resid), output rounded when the compute dtype is the output's;
    operands and incoming gradients rounded to bf16, accumulation in f64."""
    y = rnd(x) @ rnd_fwd(w).t()
    if b is not None:
        y = y + b
    y = _RoundBwd.apply(y)
    if act != ACT_NONE:
        y = {ACT_GELU: lambda t: F.gelu(t), ACT_RELU: torch.relu, ACT_SIGMOID: torch.sigmoid}[act](y)
    if resid is not None:
        y = y + resid
    return rnd(y) if out_bf16 else y
