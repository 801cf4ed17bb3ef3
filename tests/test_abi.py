"""CPU-side checks of the drop-in boundary: libcomet_hip.so loads (no GPU needed) and exports
every entry point declared in include/comet_hip.h; the ctypes signatures cover them all."""
import os
import re

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "comet_hip.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(comet_\w+)\(", src, re.M)))


def test_header_declares_core_entry_points():
    names = _declared()
    for n in ["comet_version", "comet_last_error", "comet_gemm", "comet_attention_fwd",
              "comet_layernorm_fwd", "comet_layernorm_bwd", "comet_adamw_multi"]:
        assert n in names


def test_library_exports_every_declared_symbol():
    from comet_amd import _lib
    lib = _lib.load()
    for n in _declared():
        assert hasattr(lib, n), f"missing export {n}"
    assert set(_declared()) == set(_lib.SIGNATURES), "ctypes SIGNATURES out of sync with header"
    assert lib.comet_version() >= 1


def test_error_path_reports_message():
    import ctypes
    from comet_amd import _lib
    lib = _lib.load()
    g = _lib.GemmArgs()
    g.layout_a = 7
    rc = lib.comet_gemm(ctypes.byref(g), None)
    assert rc == -1
    assert b"layout" in lib.comet_last_error() or b"batch" in lib.comet_last_error()


def test_conv_plan_is_host_only_and_matches_the_gpu_matrix():
    """comet_conv_plan decides from the arguments alone (it never reads a pointer and launches nothing,
    so it runs without a GPU): every hand-written plan of the GPU convolution matrix
    (tests/conv_ref.py), both output types; cout 48 with 9 k chunks, which has no narrow-output
    instance, plans the 128 x 64 implicit GEMM; bad arguments are rejected as comet_conv2d_nhwc's."""
    import ctypes
    import conv_ref as R
    from comet_amd import _lib
    lib = _lib.load()

    def plan(geo, dtype_y, y=1 << 20, ldw_pad=0):
        n, h, w, c, cout, k, s, p = geo
        a = _lib.ConvArgs()
        a.dtype, a.dtype_y = _lib.BF16, dtype_y
        a.x, a.n, a.h, a.w, a.c = 1 << 12, n, h, w, c  # aligned addresses that are never read
        a.weight, a.cout, a.ldw = 1 << 13, cout, k * k * c + ldw_pad
        a.kh, a.kw, a.stride, a.pad = k, k, s, p
        a.y, a.ldy = y, cout
        out = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
        rc = lib.comet_conv_plan(ctypes.byref(a), out)
        return rc, tuple(out)

    for geo, want in R.all_geometries():
        assert plan(geo, _lib.BF16) == (0, want), geo
        assert plan(geo, _lib.F32) == (0, want[:3] + (0,)), geo
        assert plan(geo, _lib.BF16, ldw_pad=8) == (0, want), geo
    assert plan(R.CASE_COUT48[0], _lib.BF16) == (0, (1, 0, 0, 0))
    # an output that is only 8-byte aligned keeps the instance and drops the wide stores
    assert plan((70, 16, 16, 32, 32, 3, 1, 1), _lib.BF16, y=(1 << 20) + 8) == (0, (2, 2, 9, 0))
    rc, _ = plan((70, 16, 16, 12, 32, 3, 1, 1), _lib.BF16)
    assert rc != 0 and b"multiple of 8" in lib.comet_last_error()


def test_library_has_no_packed_fp32_high_src1_reads():
    """The built library holds no packed-FP32 VOP3P instruction whose low result reads the high dword
    of its second / third source (op_sel:[x,1,..]): on gfx950 those return wrong values beside a
    co-resident MFMA wave (round 6, tools/isa_hazard.py; the Makefile builds with
    -fno-slp-vectorize). The probe kernel that reproduces the hazard on purpose is exempt."""
    import os
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_hazard
    bad = isa_hazard.check()
    assert not bad, {k[:80]: len(v) for k, v in bad.items()}


def test_round6_entry_points_reject_bad_arguments_before_launching():
    """The round-6 entry points check their arguments on the host and report them through
    comet_last_error without touching the GPU: the fused fine-encoder tail rejects channel counts
    its MFMA tile does not cover and an LDS footprint above 64 KiB, the fused resize + pool rejects
    channel counts whose column pairs would straddle a wave, and the token kernel a row pitch below
    the token width."""
    import ctypes
    from comet_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256  # 256-B aligned host address (never read)
    # c = 48: not 32 / 64
    rc = lib.comet_conv1x1_resize_pool_nhwc(p, None, 0, 0, None, 0, 0, p, None, p, p, None, 4, 48, 16, 16, 31, 31,
                                            None)
    assert rc != 0 and b"c in {32, 64}" in lib.comet_last_error()
    # 64 x 64 x 32 input: 256 KiB of LDS
    rc = lib.comet_conv1x1_resize_pool_nhwc(p, None, 0, 0, None, 0, 0, p, None, p, p, None, 4, 32, 64, 64, 31, 31,
                                            None)
    assert rc != 0 and b"64 KiB" in lib.comet_last_error()
    # c = 24: 2 x 3 lanes per column pair does not divide a wave
    rc = lib.comet_resize_bilinear_pool_nhwc(1, 1, p, p, p, 4, 24, 8, 8, 15, 15, None)
    assert rc != 0 and b"c in {8, 16, 32, 64, 128, 256}" in lib.comet_last_error()
    # row pitch below the token width
    rc = lib.comet_tracker_tokens(1, p, p, 32, p, 147, 147, p, 216, p, 200, 16, 4, None)
    assert rc != 0 and b"bad args" in lib.comet_last_error()
