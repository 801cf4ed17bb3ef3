"""Differentiable operators of the hot path, forward AND backward on libcomet_hip.so.

Each op is a torch.autograd.Function whose forward/backward only call comet kernels (torch is
used for allocation and views). Under no_grad (tracker, DINOv2) the same functions run the
forward kernels without building a graph.

Precision policy (mirrors accelerate mixed_precision="bf16" autocast, abl_ours.yaml:102):
  * compute dtype COMPUTE (bf16 by default, f32 for parity runs): GEMM / attention operands;
  * residual stream, LayerNorm statistics and outputs, softmax statistics, losses and all
    gradients w.r.t. parameters: f32.
"""
import contextlib

import os

import torch

from . import _lib as L
from . import ops


class _State:
    # process-wide (NOT thread-local): autograd runs backward on its own device thread
    dtype = torch.bfloat16


_state = _State()


def compute_dtype():
    return _state.dtype


@contextlib.contextmanager
def precision(dtype):
    old = _state.dtype
    _state.dtype = dtype
    try:
        yield
    finally:
        _state.dtype = old


# ------------------------------------------------------------------------------------------
# weight copies in the compute dtype (cast once, invalidated after every optimizer step)
# ------------------------------------------------------------------------------------------
_wcache = {}


def wcast(p, dt=None):
    """p (an f32 parameter or a view of one) in the compute dtype; cached by storage address
    and shape, so the frozen tracker / DINOv2 weights are cast once."""
    dt = dt or compute_dtype()
    if p.dtype == dt:
        return p
    key = (p.data_ptr(), tuple(p.shape), tuple(p.stride()), dt)
    hit = _wcache.get(key)
    # an in-place write through torch (load_state_dict, copy_) bumps the version counter the
    # detached source shares; the optimizer's raw-pointer update re-casts via refresh_weight_cache
    if hit is not None and _wver.get(key) == p._version:
        return hit
    c = ops.cast(p.detach(), dt)
    _wcache[key] = c
    _wsrc[key] = p.detach()  # pins the source storage: its address cannot be reused while cached
    _wver[key] = p._version
    return c


_wsrc = {}
_wver = {}


def refresh_weight_cache(params):
    """Re-cast, in place and in one multi-tensor launch, the cached bf16 copies of `params` (and
    of contiguous views of them) after an optimizer step updated them; other cached entries of
    those params are dropped (re-cast at next use)."""
    spans = [(p.data_ptr(), p.data_ptr() + p.numel() * p.element_size()) for p in params]

    def ptr(k):
        return k[1] if k[0] == "conv" else k[0]
    hits = [k for k in _wcache if any(lo <= ptr(k) < hi for lo, hi in spans)]
    src, dst = [], []
    for k in hits:
        s = _wsrc.get(k)
        d = _wcache[k]
        if (s is not None and s.dtype == torch.float32 and d.dtype == torch.bfloat16 and s.is_contiguous()
                and d.is_contiguous() and s.numel() == d.numel()):
            src.append(s)
            dst.append(d)
            _wver[k] = s._version  # the copy is current again, whatever bumped the version
        else:
            del _wcache[k]
            _wsrc.pop(k, None)
            _wver.pop(k, None)
    if src:
        ops.cast_multi_f32_bf16(src, dst)


def invalidate_weight_cache(params=None):
    """Drop cached copies of `params` (all when None); called after every optimizer step."""
    if params is None:
        _wcache.clear()
        _wsrc.clear()
        _wver.clear()
        return
    spans = [(p.data_ptr(), p.data_ptr() + p.numel() * p.element_size()) for p in params]

    def ptr(k):
        return k[1] if k[0] == "conv" else k[0]
    for k in [k for k in _wcache if any(lo <= ptr(k) < hi for lo, hi in spans)]:
        del _wcache[k]
        _wsrc.pop(k, None)
        _wver.pop(k, None)


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


# ------------------------------------------------------------------------------------------
# cast
# ------------------------------------------------------------------------------------------
class _Cast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return ops.cast(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return ops.cast(g, ctx.src), None


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    if _needs_grad(x):
        return _Cast.apply(x, dtype)
    return ops.cast(x, dtype)


def to_compute(x):
    return cast(x, compute_dtype())


# ------------------------------------------------------------------------------------------
# linear: y = act(x W^T + b) + beta * resid
# ------------------------------------------------------------------------------------------
def _vec8(t):
    return t.is_contiguous() and t.shape[-1] % 8 == 0 and t.data_ptr() % 32 == 0


def _linear_bwd(x2, wc, dy2, act, aux, need_dx, need_dw, need_db, dx_dtype):
    """dy2 [M, N] (dL/d output) -> dx [M, K] (dx_dtype), dW [N, K] f32, db [N] f32.
    bf16 compute: act', the bf16 GEMM operand and the bias gradient in one pass
    (comet_act_bwd_colsum); x2 was saved in bf16 by the forward."""
    M, N = dy2.shape
    K = x2.shape[1]
    dx = dw = db = None
    cdt = wc.dtype
    if cdt == torch.bfloat16 and _vec8(dy2) and (aux is None or _vec8(aux)):
        if need_db:
            db = torch.empty(N, device=dy2.device, dtype=torch.float32)
        if act != L.ACT_NONE or dy2.dtype != torch.bfloat16:
            # one pass: act' (if any), bf16 GEMM operand, bias gradient
            dpre = ops.act_bwd_colsum(act, aux, dy2, out_dtype=torch.bfloat16, dbias=db)
        else:
            dpre = dy2
            if need_db:
                ops.act_bwd_colsum(L.ACT_NONE, None, dy2, dbias=db, want_out=False)
    else:
        dpre = ops.act_bwd(act, aux, dy2, out_dtype=torch.float32) if act != L.ACT_NONE else dy2
        if need_db:
            db = ops.colsum(dpre)
        if dpre.dtype != cdt:
            dpre = ops.cast(dpre, cdt)
    if need_dx:
        dx = torch.empty(M, K, device=dy2.device, dtype=dx_dtype)
        ops.gemm_raw(dpre, wc, dx, m=M, n=K, k=N, layout_a=0, lda=dpre.stride(0), layout_b=1,
                     ldb=wc.stride(0), ldc=K, compute=cdt)
    if need_dw:
        xc = x2 if (x2.dtype == cdt or cdt == torch.bfloat16) else ops.cast(x2, cdt)
        dw = torch.empty(N, K, device=dy2.device, dtype=torch.float32)
        ops.gemm_raw(dpre, xc, dw, m=N, n=K, k=M, layout_a=1, lda=dpre.stride(0), layout_b=1,
                     ldb=xc.stride(0), ldc=K, compute=cdt)
    return dx, dw, db


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, resid, act, beta, out_dtype):
        ctx.cdt = compute_dtype()
        wc = wcast(w, ctx.cdt)
        xc = x if x.dtype == wc.dtype else ops.cast(x, wc.dtype)
        shp = x.shape
        x2 = xc.reshape(-1, shp[-1])
        N = w.shape[0]
        aux = None
        if act != L.ACT_NONE:
            aux = torch.empty(x2.shape[0], N, device=x.device, dtype=out_dtype)
        y = ops.linear(x2, wc, bias=b, act=act, resid=(resid.reshape(-1, N) if resid is not None else None),
                       beta=beta, out_dtype=out_dtype, aux=aux)
        ctx.save_for_backward(x2, w, aux)
        ctx.act, ctx.beta, ctx.xdtype, ctx.shape = act, beta, x.dtype, shp
        ctx.has_b, ctx.has_r = b is not None, resid is not None
        return y.reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, w, aux = ctx.saved_tensors
        N = w.shape[0]
        dy2 = dy.reshape(-1, N)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        wc = wcast(w, ctx.cdt)
        # dx straight in the input's dtype (the reference's autocast grad of a bf16 tensor is bf16)
        dx_dtype = ctx.xdtype if ctx.cdt == torch.bfloat16 else torch.float32
        dx, dw, db = _linear_bwd(x2, wc, dy2, ctx.act, aux, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                 ctx.has_b and ctx.needs_input_grad[2], dx_dtype)
        if dx is not None:
            dx = dx.reshape(ctx.shape)
            if dx.dtype != ctx.xdtype:
                dx = ops.cast(dx, ctx.xdtype)
        dres = None
        if ctx.has_r and ctx.needs_input_grad[3]:
            dres = dy if ctx.beta == 1.0 else dy * ctx.beta
        return dx, dw, db, dres, None, None, None


def linear(x, w, b=None, act=L.ACT_NONE, resid=None, beta=1.0, out_dtype=None):
    """nn.Linear (+ fused activation / residual). Operands in the compute dtype, f32 accumulate."""
    out_dtype = out_dtype or compute_dtype()
    if _needs_grad(x, w, b, resid):
        return _Linear.apply(x, w, b, resid, act, beta, out_dtype)
    wc = wcast(w)
    xc = x if x.dtype == wc.dtype else ops.cast(x, wc.dtype)
    return ops.linear(xc, wc, bias=b, act=act, resid=resid, beta=beta, out_dtype=out_dtype)


class _Mlp(torch.autograd.Function):
    """fc1 -> GELU -> fc2 (+ residual) as one node (timm Mlp of the camera head's blocks,
    modules.py:18-40), so that its backward can hand fc1's GELU backward and bias gradient to the
    epilogue of fc2's input-gradient GEMM (comet_gemm_dact): the [M, hidden] gradient is written
    once in bf16 instead of written (dH), read with the pre-activation and written again
    (comet_act_bwd_colsum). The forward and the four other GEMMs of the backward are _Linear's."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, resid, out_dtype):
        wc1, wc2 = wcast(w1, torch.bfloat16), wcast(w2, torch.bfloat16)
        xc = x if x.dtype == torch.bfloat16 else ops.cast(x, torch.bfloat16)
        shp = x.shape
        x2 = xc.reshape(-1, shp[-1])
        Hd, N = w1.shape[0], w2.shape[0]
        aux = torch.empty(x2.shape[0], Hd, device=x.device, dtype=torch.bfloat16)
        h = ops.linear(x2, wc1, bias=b1, act=L.ACT_GELU, out_dtype=torch.bfloat16, aux=aux)
        y = ops.linear(h, wc2, bias=b2, resid=(resid.reshape(-1, N) if resid is not None else None),
                       out_dtype=out_dtype)
        ctx.save_for_backward(x2, h, aux, w1, w2)
        ctx.xdtype, ctx.shape = x.dtype, shp
        ctx.has_b1, ctx.has_b2, ctx.has_r = b1 is not None, b2 is not None, resid is not None
        return y.reshape(*shp[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, h, aux, w1, w2 = ctx.saved_tensors
        N = w2.shape[0]
        dy2 = dy.reshape(-1, N)
        if not _vec8(dy2):  # the colsum kernels need 8-column rows at 32-B alignment (N % 8: mlp())
            dy2 = dy2.clone(memory_format=torch.contiguous_format)
        wc1, wc2 = wcast(w1, torch.bfloat16), wcast(w2, torch.bfloat16)
        ni = ctx.needs_input_grad
        # fc2: the bf16 operand of its two GEMMs and its bias gradient in one pass, then dW2 (its dX
        # is the fused GEMM below)
        db2 = torch.empty(N, device=dy.device, dtype=torch.float32) if ctx.has_b2 and ni[4] else None
        if dy2.dtype == torch.bfloat16:
            dpre2 = dy2
            if db2 is not None:
                ops.act_bwd_colsum(L.ACT_NONE, None, dy2, dbias=db2, want_out=False)
        else:
            dpre2 = ops.act_bwd_colsum(L.ACT_NONE, None, dy2, out_dtype=torch.bfloat16, dbias=db2)
        _, dw2, _ = _linear_bwd(h, wc2, dpre2, L.ACT_NONE, None, False, ni[3], False, torch.bfloat16)
        db1 = torch.empty(w1.shape[0], device=dy.device, dtype=torch.float32) if ctx.has_b1 and ni[2] else None
        if ops.linear_dact_ok(dpre2, wc2, aux, L.ACT_GELU):
            dpre1 = ops.linear_dact(dpre2, wc2, aux, L.ACT_GELU, dbias=db1)
        else:
            dh = torch.empty(h.shape, device=dy.device, dtype=torch.bfloat16)
            ops.gemm_raw(dpre2, wc2, dh, m=dh.shape[0], n=dh.shape[1], k=N, layout_a=0, lda=dpre2.stride(0),
                         layout_b=1, ldb=wc2.stride(0), ldc=dh.shape[1], compute=torch.bfloat16)
            dpre1 = ops.act_bwd_colsum(L.ACT_GELU, aux, dh, out_dtype=torch.bfloat16, dbias=db1)
        # fc1: dpre1 is already the activation's input gradient and db1 its column sum
        dx, dw1, _ = _linear_bwd(x2, wc1, dpre1, L.ACT_NONE, None, ni[0], ni[1], False, ctx.xdtype)
        if dx is not None:
            dx = dx.reshape(ctx.shape)
            if dx.dtype != ctx.xdtype:
                dx = ops.cast(dx, ctx.xdtype)
        dres = dy if ctx.has_r and ni[5] else None
        return dx, dw1, db1, dw2, db2, dres, None


def mlp(x, w1, b1, w2, b2, resid=None, out_dtype=torch.float32):
    """fc2(GELU(fc1(x))) (+ resid). In bf16 compute with gradients, one autograd node (_Mlp) whose
    backward fuses fc1's GELU backward into fc2's input-gradient GEMM (COMET_MLP_UNFUSE=1: two Linear
    nodes, the path the fp32 compute and no-grad forwards always take)."""
    # (the fused node's column-sum kernels need widths that are multiples of 8: the GAPR quaternion
    # head's Mlp 768 -> 1536 -> 4 stays on the two-Linear path)
    if (compute_dtype() == torch.bfloat16 and _needs_grad(x, w1, b1, w2, b2, resid) and not _MLP_UNFUSED
            and w1.shape[0] % 8 == 0 and w2.shape[0] % 8 == 0):
        return _Mlp.apply(x, w1, b1, w2, b2, resid, out_dtype)
    h = linear(x, w1, b1, act=L.ACT_GELU)
    return linear(h, w2, b2, resid=resid, out_dtype=out_dtype)


# default since round 5 (one node per Mlp: -1.1 ms/step, same box, profiles/r05_attn); COMET_MLP_UNFUSE=1
# keeps two Linear nodes
_MLP_UNFUSED = os.environ.get("COMET_MLP_UNFUSE") is not None


# ------------------------------------------------------------------------------------------
# layernorm (f32 in / f32 out)
# ------------------------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps, out_dtype):
        y, mean, rstd = ops.layernorm(x, w, b, eps=eps, out_dtype=out_dtype, stats=True)
        ctx.save_for_backward(x, w, mean, rstd)
        ctx.has_w, ctx.has_b = w is not None, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        C = x.shape[-1]
        dw = torch.zeros(C, device=x.device) if ctx.has_w and ctx.needs_input_grad[1] else None
        db = torch.zeros(C, device=x.device) if ctx.has_b and ctx.needs_input_grad[2] else None
        dx = ops.layernorm_bwd(x, dy, mean, rstd, w, dw, db, dx_dtype=x.dtype)
        return dx, dw, db, None, None


class _LayerNormDual(torch.autograd.Function):
    """LN whose output feeds both an f32 residual and a bf16 GEMM (AttnBlock / CrossAttnBlock
    norm1: the reference adds the attention output to the NORMED x, modules.py:290-293): one
    kernel writes both copies, backward sums both incoming gradients in the LN kernel."""

    @staticmethod
    def forward(ctx, x, eps):
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        y, y16, mean, rstd = ops.layernorm(x, None, None, eps=eps, out_dtype=torch.float32, stats=True, dual=True)
        ctx.save_for_backward(x, mean, rstd)
        return y, y16

    @staticmethod
    def backward(ctx, dy, dy16):
        x, mean, rstd = ctx.saved_tensors
        if dy is None:
            dy, dy16 = dy16, None
        if dy is None:
            return None, None
        dx = ops.layernorm_bwd(x, dy, mean, rstd, dy2=dy16, dx_dtype=x.dtype)
        return dx, None


class _ResLayerNorm(torch.autograd.Function):
    """(x, LN(x) non-affine in the compute dtype) for `x + Mlp(LN(x))` (modules.py:293-294,
    342-343): the backward folds the residual branch's gradient into the LN backward kernel
    (comet_layernorm_bwd_res) instead of autograd adding the two gradients of x in a separate pass."""

    @staticmethod
    def forward(ctx, x, eps):
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        y, mean, rstd = ops.layernorm(x, eps=eps, out_dtype=compute_dtype(), stats=True)
        ctx.save_for_backward(x, mean, rstd)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, dres, dy):
        x, mean, rstd = ctx.saved_tensors
        if dy is None:
            return dres, None
        if dres is None:
            return ops.layernorm_bwd(x, dy, mean, rstd, dx_dtype=x.dtype), None
        if x.dtype == torch.float32 and x.shape[-1] % 8 == 0:
            return ops.layernorm_bwd_res(x, dy, dres, mean, rstd), None
        return ops.layernorm_bwd(x, dy, mean, rstd, dx_dtype=x.dtype) + dres, None


def res_layer_norm(x, eps=1e-6):
    """(x, LN(x) in the compute dtype): the residual and the normed Mlp input of x + Mlp(LN(x))."""
    if _needs_grad(x):
        return _ResLayerNorm.apply(x, eps)
    return x, ops.layernorm(x, eps=eps, out_dtype=compute_dtype())


class _LinearPair(torch.autograd.Function):
    """q = xq W[:C]^T + b[:C], kv = xkv W[C:]^T + b[C:] (the cross-attention in_proj of
    nn.MultiheadAttention, modules.py:339): the backward writes both weight / bias gradient halves
    straight into one [3C, C] / [3C] tensor -- autograd's slice backward would zero-fill a full
    gradient per slice and add them."""

    @staticmethod
    def forward(ctx, xq, xkv, w, b, C):
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        ctx.cdt = compute_dtype()
        wc = wcast(w, ctx.cdt)
        xq2 = xq.reshape(-1, xq.shape[-1])
        xkv2 = xkv.reshape(-1, xkv.shape[-1])
        xq2 = xq2 if xq2.dtype == wc.dtype else ops.cast(xq2, wc.dtype)
        xkv2 = xkv2 if xkv2.dtype == wc.dtype else ops.cast(xkv2, wc.dtype)
        q = ops.linear(xq2, wc[:C], bias=b[:C], out_dtype=ctx.cdt)
        kv = ops.linear(xkv2, wc[C:], bias=b[C:], out_dtype=ctx.cdt)
        ctx.save_for_backward(xq2, xkv2, w)
        ctx.C, ctx.shapes, ctx.dtypes = C, (xq.shape, xkv.shape), (xq.dtype, xkv.dtype)
        return q.reshape(*xq.shape[:-1], C), kv.reshape(*xkv.shape[:-1], 2 * C)

    @staticmethod
    def backward(ctx, dq, dkv):
        xq2, xkv2, w = ctx.saved_tensors
        C = ctx.C
        wc = wcast(w, ctx.cdt)
        dw = torch.zeros(w.shape, device=w.device, dtype=torch.float32) if (dq is None or dkv is None) \
            else torch.empty(w.shape, device=w.device, dtype=torch.float32)
        db = torch.zeros(w.shape[0], device=w.device, dtype=torch.float32) if (dq is None or dkv is None) \
            else torch.empty(w.shape[0], device=w.device, dtype=torch.float32)
        grads = []
        for d, x2, sl, shp, xdt in ((dq, xq2, slice(0, C), ctx.shapes[0], ctx.dtypes[0]),
                                    (dkv, xkv2, slice(C, 3 * C), ctx.shapes[1], ctx.dtypes[1])):
            if d is None:
                grads.append(None)
                continue
            d2 = d.reshape(-1, d.shape[-1])
            if not d2.is_contiguous():
                d2 = d2.contiguous()
            dx_dtype = xdt if ctx.cdt == torch.bfloat16 else torch.float32
            dx = _linear_bwd_into(x2, wc[sl], d2, dw[sl], db[sl], dx_dtype, ctx.cdt)
            dx = dx.reshape(shp)
            grads.append(dx if dx.dtype == xdt else ops.cast(dx, xdt))
        return grads[0], grads[1], dw, db, None


def _linear_bwd_into(x2, wc, dy2, dw, db, dx_dtype, cdt):
    """dx of y = x W^T + b, with dW / db written into the given (row-contiguous) views."""
    M, N = dy2.shape
    K = x2.shape[1]
    if cdt == torch.bfloat16 and _vec8(dy2):
        dpre = dy2 if dy2.dtype == torch.bfloat16 else ops.act_bwd_colsum(L.ACT_NONE, None, dy2,
                                                                          out_dtype=torch.bfloat16, dbias=db)
        if dy2.dtype == torch.bfloat16:
            ops.act_bwd_colsum(L.ACT_NONE, None, dy2, dbias=db, want_out=False)
    else:
        dpre = dy2
        db.copy_(ops.colsum(dpre))
        if dpre.dtype != cdt:
            dpre = ops.cast(dpre, cdt)
    dx = torch.empty(M, K, device=dy2.device, dtype=dx_dtype)
    ops.gemm_raw(dpre, wc, dx, m=M, n=K, k=N, layout_a=0, lda=dpre.stride(0), layout_b=1,
                 ldb=wc.stride(0), ldc=K, compute=cdt)
    xc = x2 if (x2.dtype == cdt or cdt == torch.bfloat16) else ops.cast(x2, cdt)
    ops.gemm_raw(dpre, xc, dw, m=N, n=K, k=M, layout_a=1, lda=dpre.stride(0), layout_b=1,
                 ldb=xc.stride(0), ldc=dw.stride(0), compute=cdt)
    return dx


def linear_pair(xq, xkv, w, b, C):
    """(xq W[:C]^T + b[:C], xkv W[C:]^T + b[C:]) in the compute dtype (see _LinearPair)."""
    if _needs_grad(xq, xkv, w, b):
        return _LinearPair.apply(xq, xkv, w, b, C)
    return linear(xq, w[:C], b[:C]), linear(xkv, w[C:], b[C:])


class _FrameSplit(torch.autograd.Function):
    """tok [B, S, P, C] -> (tok[:, 0:1], tok[:, 0], tok[:, 1:]) as views: the per-layer split of
    get_2D_image_features (camera_predictor10.py:663-683: frame 0 is both kept and the cross-attention
    context, frames 1.. are the queries). One backward node assembles d tok with a single copy of the
    frames-1.. gradient -- autograd's select / slice backwards would zero-fill three full-size
    gradients and add them."""

    @staticmethod
    def forward(ctx, tok):
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        ctx.shape, ctx.dtype = tok.shape, tok.dtype
        # frames 1.. as one contiguous copy: the consumers (LayerNorm forward and backward of the
        # cross-attention block) would each make it contiguous otherwise
        fo = tok[:, 1:]
        return tok[:, 0:1], tok[:, 0], (fo if _FRAME_VIEWS else fo.contiguous())

    @staticmethod
    def backward(ctx, d_t0, d_f0, d_fo):
        dtok = torch.empty(ctx.shape, device=(d_fo if d_fo is not None else d_f0 if d_f0 is not None else d_t0).device,
                           dtype=ctx.dtype)
        if d_fo is not None:
            dtok[:, 1:].copy_(d_fo)
        else:
            dtok[:, 1:].zero_()
        if d_t0 is not None and d_f0 is not None:
            torch.add(d_t0[:, 0], d_f0, out=dtok[:, 0])
        elif d_t0 is not None:
            dtok[:, 0].copy_(d_t0[:, 0])
        elif d_f0 is not None:
            dtok[:, 0].copy_(d_f0)
        else:
            dtok[:, 0].zero_()
        return dtok


class _FrameJoin(torch.autograd.Function):
    """cat([t0, fo], dim=1) whose backward hands out the frames-1.. gradient as one contiguous
    copy (autograd's CatBackward gives a strided view, which the cross-attention block's Linear and
    residual-LayerNorm backwards would each copy)."""

    @staticmethod
    def forward(ctx, t0, fo):
        return torch.cat([t0, fo], dim=1)

    @staticmethod
    def backward(ctx, d):
        return d[:, 0:1], d[:, 1:].contiguous()


class _GatherRows(torch.autograd.Function):
    """x2 [R, C] -> x2[idx] with one backward node: a zero gradient and one index_add_ of the
    gathered rows' gradients (repeated rows accumulate), instead of per-view select / slice
    backwards that each zero-fill a full-size gradient and are then added."""

    @staticmethod
    def forward(ctx, x2, idx):
        ctx.save_for_backward(idx)
        ctx.rows = x2.shape[0]
        return x2.index_select(0, idx)

    @staticmethod
    def backward(ctx, d):
        (idx,) = ctx.saved_tensors
        dx = torch.zeros(ctx.rows, d.shape[1], device=d.device, dtype=d.dtype)
        dx.index_add_(0, idx, d)
        return dx, None


def gather_rows(x2, idx):
    """x2[idx] over the rows of a 2-D tensor (see _GatherRows)."""
    if _needs_grad(x2):
        return _GatherRows.apply(x2, idx)
    return x2.index_select(0, idx)


_FRAME_VIEWS = bool(os.environ.get("COMET_FRAME_VIEWS"))  # A/B switch: strided frames-1.. views, plain cat


def frame_join(t0, fo):
    """torch.cat([t0, fo], dim=1) (see _FrameJoin)."""
    if _needs_grad(t0, fo) and not os.environ.get("COMET_NO_FRAME_SPLIT") and not _FRAME_VIEWS:
        return _FrameJoin.apply(t0, fo)
    return torch.cat([t0, fo], dim=1)


def frame_split(tok):
    """(tok[:, 0:1], tok[:, 0], tok[:, 1:]) with one backward node (see _FrameSplit)."""
    if _needs_grad(tok) and not os.environ.get("COMET_NO_FRAME_SPLIT"):
        return _FrameSplit.apply(tok)
    return tok[:, 0:1], tok[:, 0], tok[:, 1:]


def layer_norm(x, w=None, b=None, eps=1e-5, out_dtype=torch.float32):
    """nn.LayerNorm; out_dtype = compute dtype when the output only feeds a GEMM (the reference's
    autocast rounds it to bf16 at the Linear anyway)."""
    if _needs_grad(x, w, b):
        return _LayerNorm.apply(x, w, b, eps, out_dtype)
    return ops.layernorm(x, w, b, eps=eps, out_dtype=out_dtype)


def layer_norm_dual(x, eps=1e-5):
    """(y f32, y in the compute dtype) of a non-affine LN: residual copy + GEMM operand."""
    if compute_dtype() != torch.bfloat16:
        y = layer_norm(x, eps=eps)
        return y, y
    if _needs_grad(x):
        return _LayerNormDual.apply(x, eps)
    y, y16 = ops.layernorm(x, eps=eps, out_dtype=torch.float32, dual=True)
    return y, y16


# ------------------------------------------------------------------------------------------
# multi-head attention core: o = softmax(q k^T * scale) v, per head
# q [B, Lq, C], k/v [B, Lk, C] views with unit-stride last dim (may be slices of packed
# projections). Backward is the materialised form on batched GEMMs.
# ------------------------------------------------------------------------------------------
def _attn_bwd(q, k, v, o, lse, do, heads, scale, dq, dk, dv):
    """Materialised attention backward on batched GEMMs; dq/dk/dv are (possibly strided) views
    [B, L, C] into the packed gradient buffers."""
    B, Lq, C = q.shape
    Lk = k.shape[1]
    D = C // heads
    dt = q.dtype
    dev = q.device
    BH = (B, heads)
    sz = heads * Lq * Lk
    S = torch.empty(B, heads, Lq, Lk, device=dev, dtype=torch.float32)
    ops.gemm_raw(q, k, S, m=Lq, n=Lk, k=D, layout_a=0, lda=q.stride(1), layout_b=0, ldb=k.stride(1),
                 ldc=Lk, batch=BH, stride_a=(q.stride(0), D), stride_b=(k.stride(0), D),
                 stride_c=(sz, Lq * Lk))
    P = torch.empty(B, heads, Lq, Lk, device=dev, dtype=dt)
    rows = B * heads * Lq
    L.check(L.load().comet_attn_probs(ops.dt(P), S.data_ptr(), lse.data_ptr(), P.data_ptr(), rows, Lk, Lk, Lk,
                                      float(scale), ops.stream()), "attn_probs")
    dP = S  # dP overwrites S
    ops.gemm_raw(do, v, dP, m=Lq, n=Lk, k=D, layout_a=0, lda=do.stride(1), layout_b=0, ldb=v.stride(1),
                 ldc=Lk, batch=BH, stride_a=(do.stride(0), D), stride_b=(v.stride(0), D),
                 stride_c=(sz, Lq * Lk))
    delta = torch.empty(B, heads, Lq, device=dev, dtype=torch.float32)
    L.check(L.load().comet_attn_delta(ops.dt(o), do.data_ptr(), o.data_ptr(), delta.data_ptr(), B, heads, Lq, D,
                                      o.stride(0), D, o.stride(1), do.stride(0), D, do.stride(1), ops.stream()),
            "attn_delta")
    dS = torch.empty(B, heads, Lq, Lk, device=dev, dtype=dt)
    L.check(L.load().comet_attn_dsoftmax(ops.dt(P), P.data_ptr(), dP.data_ptr(), delta.data_ptr(), dS.data_ptr(),
                                         rows, Lk, Lk, float(scale), ops.stream()), "attn_dsoftmax")
    del S, dP
    # dV = P^T dO
    ops.gemm_raw(P, do, dv, m=Lk, n=D, k=Lq, layout_a=1, lda=Lk, layout_b=1, ldb=do.stride(1), ldc=dv.stride(1),
                 batch=BH, stride_a=(sz, Lq * Lk), stride_b=(do.stride(0), D), stride_c=(dv.stride(0), D))
    # dQ = dS K
    ops.gemm_raw(dS, k, dq, m=Lq, n=D, k=Lk, layout_a=0, lda=Lk, layout_b=1, ldb=k.stride(1), ldc=dq.stride(1),
                 batch=BH, stride_a=(sz, Lq * Lk), stride_b=(k.stride(0), D), stride_c=(dq.stride(0), D))
    # dK = dS^T Q
    ops.gemm_raw(dS, q, dk, m=Lk, n=D, k=Lq, layout_a=1, lda=Lk, layout_b=1, ldb=q.stride(1), ldc=dk.stride(1),
                 batch=BH, stride_a=(sz, Lq * Lk), stride_b=(q.stride(0), D), stride_c=(dk.stride(0), D))


def _split(qsrc, kvsrc, C):
    if kvsrc is None:  # packed self-attention projections [B, L, 3C]
        return qsrc[..., :C], qsrc[..., C:2 * C], qsrc[..., 2 * C:]
    return qsrc, kvsrc[..., :C], kvsrc[..., C:]


class _Attention(torch.autograd.Function):
    """qsrc: packed [B, L, 3C] (self) or [B, Lq, C] (cross, with kvsrc [B, Lk, 2C])."""

    @staticmethod
    def forward(ctx, qsrc, kvsrc, heads, scale, C):
        q, k, v = _split(qsrc, kvsrc, C)
        o, lse = ops.attention(q, k, v, heads, scale, lse=True)
        ctx.save_for_backward(qsrc, kvsrc, o, lse)
        ctx.heads, ctx.scale, ctx.C = heads, scale, C
        return o

    @staticmethod
    def backward(ctx, do):
        qsrc, kvsrc, o, lse = ctx.saved_tensors
        C = ctx.C
        q, k, v = _split(qsrc, kvsrc, C)
        do = do if do.dtype == q.dtype else ops.cast(do, q.dtype)
        if not do.is_contiguous():
            do = do.contiguous()
        dqsrc = torch.empty_like(qsrc)
        dkvsrc = None if kvsrc is None else torch.empty_like(kvsrc)
        dq, dk, dv = _split(dqsrc, dkvsrc, C)
        if ops.attention_bwd_ok(q, k, v, o, do, ctx.heads) and all(t.data_ptr() % 16 == 0 and t.stride(1) % 8 == 0
                                                                    for t in (dq, dk, dv)):
            ops.attention_bwd(q, k, v, o, lse, do, ctx.heads, ctx.scale, dq, dk, dv)
        else:  # f32 (parity precision) or unsupported head size: materialised backward
            _attn_bwd(q, k, v, o, lse, do, ctx.heads, ctx.scale, dq, dk, dv)
        return dqsrc, dkvsrc, None, None, None


def attention(qsrc, kvsrc, heads, C, scale=None):
    """softmax(q k^T * scale) v per head on packed projections (see _Attention)."""
    scale = (C // heads) ** -0.5 if scale is None else scale
    if _needs_grad(qsrc, kvsrc):
        return _Attention.apply(qsrc, kvsrc, heads, scale, C)
    q, k, v = _split(qsrc, kvsrc, C)
    return ops.attention(q, k, v, heads, scale)


# ------------------------------------------------------------------------------------------
# small differentiable helpers of the camera head
# ------------------------------------------------------------------------------------------
class _LayerNormReLU(torch.autograd.Function):
    """relu(LN_affine(x)) (TrajectoryEncoder, camera_predictor10.py:79-81)."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        y, mean, rstd = ops.layernorm(x, w, b, eps=eps, out_dtype=torch.float32, stats=True, relu=True)
        ctx.save_for_backward(x, w, mean, rstd, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd, y = ctx.saved_tensors
        dpre = ops.act_bwd(L.ACT_RELU, y, dy.contiguous(), out_dtype=torch.float32)
        C = x.shape[-1]
        dw = torch.zeros(C, device=x.device) if ctx.needs_input_grad[1] else None
        db = torch.zeros(C, device=x.device) if ctx.needs_input_grad[2] else None
        dx = ops.layernorm_bwd(x, dpre, mean, rstd, w, dw, db) if (ctx.needs_input_grad[0] or dw is not None or db is not None) else None
        return dx, dw, db, None


def layer_norm_relu(x, w, b, eps=1e-5):
    if _needs_grad(x, w, b):
        return _LayerNormReLU.apply(x, w, b, eps)
    return ops.layernorm(x, w, b, eps=eps, out_dtype=torch.float32, relu=True)


class _RowScale(torch.autograd.Function):
    """y[r, :] = x[r, :] * w[r] (confidence gating, camera_predictor10.py:332-333)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return ops.rowscale(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx, dw = ops.rowscale_bwd(x, w, dy, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, dw


def rowscale(x, w):
    """x [..., C], w [...] or [..., 1] (f32)."""
    w = w.reshape(x.shape[:-1])
    if _needs_grad(x, w):
        return _RowScale.apply(x, w)
    return ops.rowscale(x, w)


class _Add(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return ops.add(a, b)

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    if _needs_grad(a, b):
        return _Add.apply(a, b)
    return ops.add(a, b)


class _AddRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, period):
        return ops.add_rows(x, table, period, out_dtype=torch.float32)

    @staticmethod
    def backward(ctx, g):
        return g, None, None


def add_rows(x, table, period):
    """x [..., C] + table[row % period] (constant positional / time embedding table)."""
    if _needs_grad(x):
        return _AddRows.apply(x, table, period)
    return ops.add_rows(x, table, period, out_dtype=torch.float32)


class _GAPR(torch.autograd.Function):
    """Fused GAPR tail (camera_predictor10.py:385-460): quaternion F.normalize, pose loss vs the
    GT encoding, frame-0 reset. Returns (pred_pose_enc [B*S, 7], losses [3])."""

    @staticmethod
    def forward(ctx, rot, uv, d, gt_enc, B, S, w_trans, w_rot):
        rot2, uv2, d2 = rot.reshape(B * S, 4).contiguous(), uv.reshape(B * S, 2).contiguous(), d.reshape(B * S, 1).contiguous()
        qn = torch.empty(B * S, 4, device=rot.device, dtype=torch.float32)
        enc = torch.empty(B * S, 7, device=rot.device, dtype=torch.float32)
        losses = torch.zeros(3, device=rot.device, dtype=torch.float32)
        L.check(L.load().comet_gapr_fwd(rot2.data_ptr(), 4, uv2.data_ptr(), 2, d2.data_ptr(), 1,
                                        None if gt_enc is None else gt_enc.data_ptr(), qn.data_ptr(), enc.data_ptr(),
                                        losses.data_ptr(), B, S, float(w_trans), float(w_rot), ops.stream()), "gapr_fwd")
        ctx.save_for_backward(rot2, uv2, d2, gt_enc, qn)
        ctx.meta = (B, S, w_trans, w_rot, rot.shape, uv.shape, d.shape)
        ctx.mark_non_differentiable(enc)
        return enc, losses

    @staticmethod
    def backward(ctx, denc, dlosses):
        rot2, uv2, d2, gt_enc, qn = ctx.saved_tensors
        B, S, wt, wr, rs, us, ds = ctx.meta
        if dlosses is None or gt_enc is None:
            return None, None, None, None, None, None, None, None
        dl = dlosses.contiguous().float()
        drot = torch.empty(B * S, 4, device=rot2.device)
        duv = torch.empty(B * S, 2, device=rot2.device)
        dd = torch.empty(B * S, 1, device=rot2.device)
        L.check(L.load().comet_gapr_bwd(rot2.data_ptr(), 4, uv2.data_ptr(), 2, d2.data_ptr(), 1, gt_enc.data_ptr(),
                                        qn.data_ptr(), dl.data_ptr(), drot.data_ptr(), duv.data_ptr(), dd.data_ptr(),
                                        B, S, float(wt), float(wr), ops.stream()), "gapr_bwd")
        return drot.reshape(rs), duv.reshape(us), dd.reshape(ds), None, None, None, None, None


def gapr(rot, uv, d, gt_enc, B, S, w_trans=1.0, w_rot=2.0):
    """(pred_pose_enc [B*S, 7], losses [3] = (loss, loss_trans, loss_rot))."""
    return _GAPR.apply(rot, uv, d, gt_enc, B, S, w_trans, w_rot)


class _Harmonic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, diag_cov, freqs, append):
        ctx.save_for_backward(x, diag_cov, freqs)
        ctx.append = append
        return ops.harmonic_fwd(x, freqs, append, diag_cov)

    @staticmethod
    def backward(ctx, dy):
        x, cov, freqs = ctx.saved_tensors
        dx, dcov = ops.harmonic_bwd(x, freqs, ctx.append, dy, cov)
        return dx, (dcov if ctx.needs_input_grad[1] else None), None, None


def harmonic(x, freqs, append_input, diag_cov=None):
    if _needs_grad(x, diag_cov):
        return _Harmonic.apply(x, diag_cov, freqs, append_input)
    return ops.harmonic_fwd(x, freqs, append_input, diag_cov)


def wcast_kpad(w, kpad):
    """Linear weight [N, K] in the compute dtype with its K columns zero-padded to kpad (cached like
    wcast_conv): the operand for inputs whose rows carry zero padding up to a 64-deep k-tile multiple,
    so the GEMM takes the persistent kernel (K % 64 == 0) with the same products and sums."""
    dt = compute_dtype()
    n, k = w.shape
    key = ("conv", w.data_ptr(), tuple(w.shape), dt, "kpad", kpad)
    hit = _wcache.get(key)
    if hit is not None and _wver.get(key) == w._version:
        return hit
    wm = torch.zeros(n, kpad, device=w.device, dtype=dt)
    wm[:, :k].copy_(ops.cast(w.detach().contiguous(), dt))
    _wcache[key] = wm
    _wver[key] = w._version
    _wsrc[key] = w.detach()  # pins the source storage: its address cannot be reused while cached
    return wm


def wcast_conv(w, k_align=8, cin_pad=None):
    """Conv weight [Cout, Cin, kh, kw] -> GEMM operand [Cout, Kpad] in the compute dtype, column
    order (ky, kx, ci) matching comet_im2col_nhwc / comet_conv2d_nhwc, input channels padded with
    zeros to cin_pad (channel-padded RGB inputs) and K to k_align (cached)."""
    dt = compute_dtype()
    cout, cin, kh, kw = w.shape
    cp = cin_pad or cin
    key = ("conv", w.data_ptr(), tuple(w.shape), dt, cp)
    hit = _wcache.get(key)
    if hit is not None and _wver.get(key) == w._version:
        return hit
    K = cp * kh * kw
    Kp = (K + k_align - 1) // k_align * k_align
    wm = torch.zeros(cout, Kp, device=w.device, dtype=dt)
    wp = torch.zeros(cout, kh, kw, cp, device=w.device, dtype=dt)
    wp[..., :cin] = w.detach().permute(0, 2, 3, 1).to(dt)
    wm[:, :K] = wp.reshape(cout, K)
    _wcache[key] = wm
    _wver[key] = w._version
    _wsrc[key] = w.detach()  # pins the source storage: its address cannot be reused while cached
    return wm
