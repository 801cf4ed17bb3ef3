"""The float64 restatements of tests/backward_ref.py against independent truths (autograd gradcheck,
central differences, torch.optim.AdamW), and the measurement of the bf16 rounding model's error that
the GPU bounds of tests/test_backward_gpu.py are built from. No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import backward_ref as R


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("clip", ["none", "above", "below"])
def test_adamw_ref_matches_torch_adamw(wd, clip):
    sizes = [1, 5, 8, 33]
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    ps = [torch.nn.Parameter(_rand(n, seed=n)) for n in sizes]
    opt = torch.optim.AdamW(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    mine = [(p.detach().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
            for p, n in zip(ps, sizes)]
    max_norm = {"none": 0.0, "above": 0.5, "below": 1e3}[clip]
    for step in (1, 2, 3):
        gs = [_rand(n, seed=100 * step + n, scale=2.0) for n in sizes]
        sq = sum((g * g).sum().item() for g in gs)
        if clip == "above":
            assert math.sqrt(sq) > max_norm
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        if clip != "none":
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        mine = [R.adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, None if clip == "none" else sq, max_norm)[:3]
                for (p, m, v), g in zip(mine, gs)]
        for p, (pm, _, _) in zip(ps, mine):
            assert torch.allclose(p.detach(), pm, rtol=1e-12, atol=1e-14)
    for p, (_, m, v) in zip(ps, mine):
        assert torch.allclose(opt.state[p]["exp_avg"], m, rtol=1e-12, atol=1e-16)
        assert torch.allclose(opt.state[p]["exp_avg_sq"], v, rtol=1e-12, atol=1e-16)


def test_attn_bwd_ref_gradcheck():
    B, H, lq, lk, D = 1, 1, 3, 5, 4
    q, k, v, do = _rand(B, lq, D, seed=1), _rand(B, lk, D, seed=2), _rand(B, lk, D, seed=3), _rand(B, lq, D, seed=4)
    scale = 0.6

    def fwd(q_, k_, v_):
        return torch.softmax(q_ @ k_.transpose(-1, -2) * scale, -1) @ v_

    assert torch.autograd.gradcheck(fwd, [t.clone().requires_grad_(True) for t in (q, k, v)])
    o, lse, dq, dk, dv = R.attn_bwd_ref(q, k, v, do, H, scale)
    # central differences of <o, do> in a few coordinates of each input
    h = 1e-6
    for name, t, grad in (("q", q, dq), ("k", k, dk), ("v", v, dv)):
        for idx in [(0, 0, 0), (0, t.shape[1] - 1, D - 1), (0, 1, 2)]:
            tp, tm = t.clone(), t.clone()
            tp[idx] += h
            tm[idx] -= h
            args_p = [tp if n == name else x for n, x in (("q", q), ("k", k), ("v", v))]
            args_m = [tm if n == name else x for n, x in (("q", q), ("k", k), ("v", v))]
            fd = ((fwd(*args_p) - fwd(*args_m)) * do).sum().item() / (2 * h)
            assert abs(fd - grad[idx].item()) < 1e-7, (name, idx)
    assert torch.allclose(o, fwd(q, k, v))
    assert torch.allclose(lse[0, 0], torch.logsumexp(q[0] @ k[0].t() * scale, -1))
    # the materialised pieces reproduce the same gradients
    s = q[0] @ k[0].t()
    P = R.attn_probs_ref(s, lse[0, 0], scale)
    assert torch.allclose(P.sum(-1), torch.ones(lq, dtype=torch.float64))
    delta = R.attn_delta_ref(do, o, H)[0, 0]
    dS = R.attn_dsoftmax_ref(P, do[0] @ v[0].t(), delta, scale)
    assert torch.allclose(dS @ k[0], dq[0]) and torch.allclose(dS.t() @ q[0], dk[0])
    assert torch.allclose(P.t() @ do[0], dv[0])


def test_attn_bwd_ref_multi_head_layout():
    """heads are column slices of C: a 2-head call equals two 1-head calls on the slices."""
    B, H, lq, lk, D = 2, 2, 4, 6, 8
    q, k, v, do = (_rand(B, n, H * D, seed=s) for n, s in ((lq, 1), (lk, 2), (lk, 3), (lq, 4)))
    full = R.attn_bwd_ref(q, k, v, do, H, 0.3)
    for h in range(H):
        sl = slice(h * D, (h + 1) * D)
        one = R.attn_bwd_ref(q[..., sl], k[..., sl], v[..., sl], do[..., sl], 1, 0.3)
        for a, b in zip((full[0], full[2], full[3], full[4]), (one[0], one[2], one[3], one[4])):
            assert torch.allclose(a[..., sl], b)
        assert torch.allclose(full[1][:, h], one[1][:, 0])


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_act_grad_ref_central_differences(act):
    x = torch.tensor([-10.0, -3.0, -1.0, -1e-3, 1e-3, 0.5, 2.0, 10.0], dtype=torch.float64)
    h = 1e-6
    fd = (R.act_ref(act, x + h) - R.act_ref(act, x - h)) / (2 * h)
    assert torch.allclose(R.act_grad_ref(act, x), fd, rtol=1e-7, atol=1e-9)
    assert R.act_grad_ref(R.ACT_RELU, torch.tensor([0.0, -0.0])).tolist() == [0.0, 0.0]
    xr = x.clone().requires_grad_(True)
    ref = {0: lambda t: t, 1: F.gelu, 2: torch.relu, 3: torch.sigmoid}[act](xr)
    ref.sum().backward()
    assert torch.allclose(R.act_grad_ref(act, x), xr.grad, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("affine", [False, True])
def test_ln_bwd_ref_gradcheck(affine):
    rows, cols, eps = 3, 6, 1e-5
    x, dy, dy2 = _rand(rows, cols, seed=1, scale=2.0), _rand(rows, cols, seed=2), _rand(rows, cols, seed=3)
    w = _rand(cols, seed=4) if affine else None
    ins = [x.clone().requires_grad_(True)] + ([w.clone().requires_grad_(True), torch.zeros(cols, dtype=torch.float64, requires_grad=True)] if affine else [])
    assert torch.autograd.gradcheck(lambda *a: F.layer_norm(a[0], (cols,), *(a[1:] if affine else (None, None)), eps), ins)
    dx, dw, db = R.ln_bwd_ref(x, dy, dy2, w, eps)
    # the closed form the kernel header states: dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy w
    mean, rstd = R.ln_stats_ref(x, eps)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = (dy + dy2) * (w if affine else 1.0)
    want = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    assert torch.allclose(dx, want, rtol=1e-10, atol=1e-12)
    if affine:
        assert torch.allclose(dw, ((dy + dy2) * xh).sum(0)) and torch.allclose(db, (dy + dy2).sum(0))
    else:
        assert dw is None and db is None


@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("cov", [False, True])
def test_harmonic_ref_layout_and_gradcheck(append, cov):
    rows, dim, n = 3, 2, 4
    x = _rand(rows, dim, seed=1)
    c = _rand(rows, dim, seed=2).abs() * 0.1 if cov else None
    f = 2.0 ** torch.arange(n, dtype=torch.float64)
    y = R.harmonic_ref(x, f, append, c)
    assert y.shape == (rows, dim * (2 * n + int(append)))
    for r in range(rows):
        for i in range(dim):
            for k in range(n):
                att = math.exp(-0.5 * c[r, i].item() * f[k].item() ** 2) if cov else 1.0
                assert abs(y[r, i * n + k].item() - math.sin(x[r, i].item() * f[k].item()) * att) < 1e-12
                assert abs(y[r, dim * n + i * n + k].item() - math.cos(x[r, i].item() * f[k].item()) * att) < 1e-12
    if append:
        assert torch.equal(y[:, 2 * dim * n:], x)
    ins = [x.clone().requires_grad_(True)] + ([c.clone().requires_grad_(True)] if cov else [])
    assert torch.autograd.gradcheck(lambda *a: R.harmonic_ref(a[0], f, append, a[1] if cov else None), ins)


def test_bf16_rounding_helpers():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 3.14159, 1e-3], dtype=torch.float64)
    # ties go to even: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert R.bf16(x)[:3].tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0]
    assert ((R.bf16(x) - x).abs() <= 2.0 ** -8 * x.abs()).all()  # half of the 2^-7 spacing
    t = x.clone().requires_grad_(True)
    (R.rnd(t) * x).sum().backward()
    assert torch.equal(t.grad, R.bf16(x))
    t = x.clone().requires_grad_(True)
    (R.rnd_fwd(t) * x).sum().backward()
    assert torch.equal(t.grad, x)


# -------------------------------------------------------------------------------------------------
# the tolerance measurement
# -------------------------------------------------------------------------------------------------
_WORST = {"dq": (0.0, None), "dk": (0.0, None), "dv": (0.0, None)}


@pytest.mark.parametrize("D", R.ATTN_DS)
@pytest.mark.parametrize("lq,lk", R.ATTN_SHAPES)
def test_attention_rounding_model_error(D, lq, lk):
    """e = max|attn_bwd_rounded - attn_bwd_ref| / max|attn_bwd_ref| per output for every case of the GPU
    attention table: finite and below the old blanket 2e-2. test_backward_gpu.py recomputes the same e
    for its bound (3 e); the largest values are recorded in the table at its top."""
    q, kv, do = R.attn_inputs(D, lq, lk)
    C = q.shape[-1]
    e, _, _ = R.attn_model_error(q, kv[..., :C], kv[..., C:], do, R.ATTN_H, D ** -0.5)
    print(f"attn rounding model D={D} lq={lq} lk={lk}: e_dq={e[0]:.3e} e_dk={e[1]:.3e} e_dv={e[2]:.3e}")
    for name, v in zip(("dq", "dk", "dv"), e):
        assert math.isfinite(v) and v < 2e-2, (name, v)
        if v > _WORST[name][0]:
            _WORST[name] = (v, (D, lq, lk))
        if lk > 1 or name == "dv":
            assert v > 0  # (lk = 1: dq = dk = 0 exactly, with or without the roundings)


@pytest.mark.parametrize("kind", ["scale", "large_logits"])
def test_attention_rounding_model_error_special_cases(kind):
    D = 64
    if kind == "scale":
        q, kv, do = R.attn_inputs(D, 65, 129)
        scale = 0.37
    else:
        q, kv, do = R.attn_inputs(D, 130, 77, logit_gain=80.0)
        scale = D ** -0.5
    C = q.shape[-1]
    e, refs, _ = R.attn_model_error(q, kv[..., :C], kv[..., C:], do, R.ATTN_H, scale)
    print(f"attn rounding model {kind}: e_dq={e[0]:.3e} e_dk={e[1]:.3e} e_dv={e[2]:.3e}")
    assert all(math.isfinite(v) and 0 < v < 2e-2 for v in e)
    if kind == "large_logits":
        s = R._heads(q.double(), R.ATTN_H) @ R._heads(kv[..., :C].double(), R.ATTN_H).transpose(-1, -2) * scale
        assert 60 < s.abs().max().item() < 100
        pmax = torch.softmax(s, -1).max(-1).values
        assert pmax.max().item() > 0.999 and pmax.min().item() < 0.2  # from one-hot to flat rows


def test_attention_rounding_model_worst_cases_printed():
    """Prints the table copied to the top of test_backward_gpu.py (runs after the measurement)."""
    for name, (v, case) in _WORST.items():
        print(f"largest e_{name} = {v:.3e} at (D, lq, lk) = {case}")


# the Linear-family bf16 tolerance model: one measurement per case of test_backward_gpu.py section f
@pytest.mark.parametrize("rows", [1, 67])
def test_linear_rounding_model_error(rows):
    """bf16 rounding of operands, outputs and gradients of y = gelu(x W^T + b) against plain f64: the
    per-gradient error relative to max|ref| stays below 2e-2 (bf16 rounds by at most 2^-8 relative)."""
    K, N = 40, 24
    x, w, b, g = _rand(rows, K, seed=1), _rand(N, K, seed=2, scale=K ** -0.5), _rand(N, seed=3), _rand(rows, N, seed=4)
    outs = []
    for rounded in (False, True):
        xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = R.linear_rounded(xs, ws, bs, R.ACT_GELU) if rounded else F.gelu(xs @ ws.t() + bs)
        y.backward(g)
        outs.append((y.detach(), xs.grad, ws.grad, bs.grad))
    for name, a, r in zip(("y", "dx", "dw", "db"), outs[1], outs[0]):
        e = ((a - r).abs().max() / r.abs().max()).item()
        print(f"linear rounding model rows={rows} {name}: e={e:.3e}")
        assert 0 < e < 2e-2
