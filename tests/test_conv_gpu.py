"""comet_conv2d_nhwc against the float64 reference of tests/conv_ref.py on the paths the model runs:
every narrow-output ("skinny") kernel instance, the wide bf16 stores, the epilogues of each kernel
kind, off-model ABI shapes, and the rows-in-LDS kernel's ring at image edges. Every case asserts the
plan comet_conv_plan reports before it compares, and compares under the derived bound of conv_ref.py
(zero elements over it). The matrix and the list of skinny instances are in conv_ref.py."""
import functools

import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTS = {"bf16": torch.bfloat16, "f32": torch.float32}
EPIS = {
    "nobias": dict(bias=False, act=R.ACT_NONE, resid=False),
    "bias": dict(bias=True, act=R.ACT_NONE, resid=False),
    "bias_relu_resid": dict(bias=True, act=R.ACT_RELU, resid=True),
}


def _ops():
    from comet_amd import ops
    return ops


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=2)
def _problem(geo, epi, ldw_pad=0):
    """Device inputs and the float64 reference / S of one case, shared by the output types (and the
    tests) that use it; never modified."""
    e = EPIS[epi]
    x, wbuf, bias, resid = (t.to(DEV) for t in R.make_inputs(geo, ldw_pad))
    wm = R.weight_view(wbuf, geo)  # row pitch K + ldw_pad
    bias = bias if e["bias"] else None
    resid = resid if e["resid"] else None
    ref, S = R.conv_ref(x, wm, geo, bias=bias, act=e["act"], resid=resid, beta=R.BETA)
    return x, wm, bias, resid, ref, S


def _kwargs(prob, epi, dt):
    x, wm, bias, resid, ref, S = prob
    kw = dict(bias=bias, act=EPIS[epi]["act"], out_dtype=dt)
    if resid is not None:
        kw.update(resid=resid.to(dt), beta=R.BETA)  # the residual has the output type
    return kw


def _expect(plan, dt):
    return plan if dt == torch.bfloat16 else plan[:3] + (0,)


def _run(geo, plan, epi, dt, ldw_pad=0, prefill=None):
    """Assert the plan, run the convolution, compare with float64. Returns (y, worst err / bound)."""
    ops = _ops()
    prob = _problem(geo, epi, ldw_pad)
    x, wm, bias, resid, ref, S = prob
    k, s, p = geo[5], geo[6], geo[7]
    kw = _kwargs(prob, epi, dt)
    if prefill is not None:
        oh, ow = R.out_hw(geo)
        kw["out"] = torch.full((geo[0], oh, ow, geo[4]), prefill, device=DEV, dtype=dt)
    got_plan = ops.conv_plan(x, wm, k, k, s, p, **kw)
    assert got_plan == _expect(plan, dt), f"{geo} {dt}: plan {got_plan}, written for {_expect(plan, dt)}"
    y = ops.conv2d_nhwc(x, wm, k, k, s, p, **kw)
    over, ratio = R.compare(y, ref, S, geo, dt)
    print(f"conv {geo} {epi} {dt} plan {got_plan}: worst err / bound {ratio:.4f}")
    assert over == 0, f"{geo} {epi} {dt} plan {got_plan}: {over} elements over the bound, worst err / bound {ratio:.3f}"
    return y, ratio


# ---- a. every skinny instance, the model's own maps, a capped grid --------------------------------
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("geo,plan", R.SKINNY_INSTANCES + R.SKINNY_MODEL, ids=_id)
def test_skinny_instances_vs_f64(geo, plan, dt):
    _run(geo, plan, "bias", DTS[dt])


@pytest.mark.parametrize("dt", list(DTS))
def test_skinny_capped_grid_vs_f64(dt):
    """More output pixels than 4096 workgroups x 4 waves x 8 steps x 16: the grid is capped and waves
    walk a ninth step (the regime of the fine encoder's 65536 patches)."""
    geo, plan = R.SKINNY_CAPPED
    oh, ow = R.out_hw(geo)
    assert geo[0] * oh * ow > 4096 * 32 * 16
    _run(geo, plan, "bias", DTS[dt])


# ---- b. wide against narrow bf16 stores -------------------------------------------------------------
@pytest.mark.parametrize("epi", ["bias", "bias_relu_resid"])
@pytest.mark.parametrize("geo,plan", R.WIDE_CASES, ids=_id)
def test_skinny_wide_store_equals_narrow_store(geo, plan, epi, monkeypatch):
    """cout 32 / 64 with bf16 output stores 16 bytes per lane after a permlane16 swap; with
    COMET_CONV_NO_WIDE=1 the same instance stores 8 bytes. Both round the same f32 values."""
    assert plan[3] == 1
    y, _ = _run(geo, plan, epi, torch.bfloat16)
    monkeypatch.setenv("COMET_CONV_NO_WIDE", "1")
    y2, _ = _run(geo, plan[:3] + (0,), epi, torch.bfloat16)
    assert torch.equal(y, y2)


# ---- c. epilogues on each kernel kind -----------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("epi", ["nobias", "bias_relu_resid"])
@pytest.mark.parametrize("geo,plan", R.EPILOGUE_CASES, ids=_id)
def test_epilogues_on_each_kind_vs_f64(geo, plan, epi, dt):
    _run(geo, plan, epi, DTS[dt])


# ---- d. off-model ABI shapes --------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("epi", ["bias", "bias_relu_resid"])
@pytest.mark.parametrize("geo,plan", R.SCALAR_EPILOGUE_CASES, ids=_id)
def test_cout_not_multiple_of_8_vs_f64(geo, plan, epi, dt):
    assert geo[4] % 8 != 0
    _run(geo, plan, epi, DTS[dt])


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("geo,plan", R.LDW_CASES, ids=_id)
def test_padded_weight_rows_vs_f64(geo, plan, dt):
    """ldw = K + 8 with 1000.0 in the eight padding columns of every weight row."""
    prob = _problem(geo, "bias", 8)
    K = geo[5] * geo[5] * geo[3]
    assert prob[1].stride(0) == K + 8 and prob[1].shape[1] == K
    assert (prob[1].as_strided((geo[4], 8), (K + 8, 1), K) == 1000.0).all()
    _run(geo, plan, "bias", DTS[dt], ldw_pad=8)


# ---- e. cout 48 with 9 k chunks -----------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("epi", ["bias", "bias_relu_resid"])
def test_cout48_nine_chunks_is_computed(epi, dt):
    """cout 48, K = 288: (cout / 16) * ceil(K / 32) = 27 <= 32 passes the skinny gate, but NT16 = 3 has
    instances up to 8 chunks only. The launcher used to return COMET_OK without launching; the shared
    plan now sends the case to the 128 x 64 implicit GEMM. The output starts as NaN."""
    geo, plan = R.CASE_COUT48
    y, _ = _run(geo, plan, epi, DTS[dt], prefill=float("nan"))
    assert torch.isfinite(y).all()


# ---- f. rows-in-LDS kernel: ring wrap and image edges ---------------------------------------------------
@pytest.mark.parametrize("epi", ["bias", "bias_relu_resid"])
@pytest.mark.parametrize("nhw", R.ROWS_CASES, ids=_id)
def test_rows_ring_and_image_edges_vs_f64(nhw, epi, monkeypatch):
    """A workgroup of the rows kernel walks rows_per = ceil(n * h / CUs) consecutive output rows over a
    ring of four input rows: with rows_per >= 5 every slot is refilled during the walk, and h = 1, 2, 3
    and image boundaries inside a range rebuild the window. bf16 output against float64, and against the
    implicit GEMM (COMET_CONV_NO_ROWS=1) within one bf16 ulp."""
    ops = _ops()
    geo = R.rows_geo(nhw)
    n, h, w = nhw
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows_per = -(-n * h // cus)
    assert rows_per >= 5, f"{cus} CUs: {rows_per} rows per workgroup do not wrap the ring"
    y, _ = _run(geo, (3, 0, 0, 0), epi, torch.bfloat16)
    monkeypatch.setenv("COMET_CONV_NO_ROWS", "1")
    prob = _problem(geo, epi)
    kw = _kwargs(prob, epi, torch.bfloat16)
    assert ops.conv_plan(prob[0], prob[1], 3, 3, 1, 1, **kw)[0] == 1
    y2 = ops.conv2d_nhwc(prob[0], prob[1], 3, 3, 1, 1, **kw)
    d = (y.float() - y2.float()).abs()
    assert (d <= 2 ** -7 * y2.float().abs() + 1e-6).all(), f"rows vs generic: max diff {d.max().item():.3e}"
