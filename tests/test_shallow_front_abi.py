"""CPU-side checks of comet_shallow_front_nhwc's boundary: the entry point validates its arguments on
the host and reports them through comet_last_error without touching the GPU."""
import ctypes

COMET_EINVAL = -1
BF16, F32 = 1, 0


def _lib():
    from comet_amd import _lib
    assert (_lib.BF16, _lib.F32) == (BF16, F32)
    return _lib.load()


def _args():
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256  # aligned host address (never read)
    W = (ctypes.c_void_p * 7)(*([p] * 7))
    B = (ctypes.c_void_p * 7)(*([p] * 7))
    return buf, p, W, B


def test_rejects_bad_dtype():
    lib = _lib()
    buf, p, W, B = _args()
    rc = lib.comet_shallow_front_nhwc(F32, p, W, B, p, p, p, 4, 31, 8, 1e-5, None)
    assert rc == COMET_EINVAL and b"bf16" in lib.comet_last_error()


def test_rejects_null_pointers():
    lib = _lib()
    buf, p, W, B = _args()
    for a in ((None, W, B, p, p, p), (p, None, B, p, p, p), (p, W, None, p, p, p), (p, W, B, None, p, p),
              (p, W, B, p, None, p), (p, W, B, p, p, None)):
        rc = lib.comet_shallow_front_nhwc(BF16, *a, 4, 31, 8, 1e-5, None)
        assert rc == COMET_EINVAL and b"null pointer" in lib.comet_last_error()
    W2 = (ctypes.c_void_p * 7)(*([p] * 6 + [None]))
    rc = lib.comet_shallow_front_nhwc(BF16, p, W2, B, p, p, p, 4, 31, 8, 1e-5, None)
    assert rc == COMET_EINVAL and b"null weight or bias" in lib.comet_last_error()


def test_rejects_other_geometry_alignment_and_size():
    lib = _lib()
    buf, p, W, B = _args()
    for ph, c in ((29, 8), (31, 16)):
        rc = lib.comet_shallow_front_nhwc(BF16, p, W, B, p, p, p, 4, ph, c, 1e-5, None)
        assert rc == COMET_EINVAL and b"geometry" in lib.comet_last_error()
    rc = lib.comet_shallow_front_nhwc(BF16, p + 8, W, B, p, p, p, 4, 31, 8, 1e-5, None)
    assert rc == COMET_EINVAL and b"16-byte aligned" in lib.comet_last_error()
    W2 = (ctypes.c_void_p * 7)(*([p] * 3 + [p + 2] + [p] * 3))
    rc = lib.comet_shallow_front_nhwc(BF16, p, W2, B, p, p, p, 4, 31, 8, 1e-5, None)
    assert rc == COMET_EINVAL and b"16-byte aligned" in lib.comet_last_error()
    for n in (0, (1 << 31) // 256):
        rc = lib.comet_shallow_front_nhwc(BF16, p, W, B, p, p, p, n, 31, 8, 1e-5, None)
        assert rc == COMET_EINVAL and b"2^31 / 256" in lib.comet_last_error()


def test_python_eligibility_rejects_what_the_entry_point_rejects():
    """ops.shallow_front_ok on CPU tensors of the right and wrong shapes (never eligible off the GPU)."""
    import torch
    from comet_amd import ops
    K = (72, 288, 288, 32, 288, 288, 32)
    ws = [torch.zeros(32, k, dtype=torch.bfloat16) for k in K]
    bs = [torch.zeros(32) for _ in K]
    p = torch.zeros(4, 31, 31, 8, dtype=torch.bfloat16)
    assert not ops.shallow_front_ok(p, ws, bs)                      # not on the device
    assert not ops.shallow_front_ok(p.float(), ws, bs)
    assert not ops.shallow_front_ok(p[:, :29, :29], ws, bs)
    assert not ops.shallow_front_ok(p, ws[:6], bs[:6])
    assert not ops.shallow_front_ok(p, ws, bs[:6] + [None])
