"""Debug mode: the `make DEBUG=1` library's device-side index checks and the NaN / Inf
check hooks (comet_amd/debug.py).

* In a fresh process with COMET_DEBUG=1 (libcomet_hip_debug.so): a patch gather inside the frame
  passes and records nothing; a W < H frame never reaches the kernel (the entry point rejects it:
  the reference clamps both patch origins with H, refine_track.py); a ring gather whose device slot
  list names a slot outside the ring -- unlike the host copy the library checks before it launches
  -- fails its COMET_DASSERT and the op raises CometHipError naming it. The kernel skips such a
  slot, so nothing is read or written outside the ring.
* FiniteCheck names the first submodule whose output holds a NaN; check_grads the first
  parameter whose gradient does."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

SCRIPT = r"""
import sys
sys.path.insert(0, {pkg!r})
import torch
from comet_amd import _lib as L, debug, ops
assert L.LIB_PATH.endswith("libcomet_hip_debug.so"), L.LIB_PATH
assert debug.debug_library() and debug.debug_flags() == 0
imgs = torch.rand(1, 2, 3, 32, 40, device="cuda")   # H = 32 <= W = 40
coarse = torch.full((1, 2, 4, 2), 30.0, device="cuda")
ops.patch_gather(imgs, coarse, 15, torch.float32)  # x0 = min(15, H - 31 = 1) = 1: inside
torch.cuda.synchronize()
assert debug.debug_flags() == 0
try:
    ops.patch_gather(imgs.transpose(3, 4).contiguous(), coarse, 15, torch.float32)  # H = 40 > W = 32
except L.CometHipError as e:
    assert "W >= H" in str(e), str(e)
    assert debug.debug_flags() == 0                  # rejected on the host: nothing ran
else:
    raise SystemExit("the W < H frame was not rejected")
import ctypes
ring = torch.arange(8 * 64, dtype=torch.float32, device="cuda").reshape(8, 64)
win = torch.zeros(4, 64, device="cuda")
host = (ctypes.c_int32 * 4)(5, 6, 7, 0)
slots = torch.tensor([5, 6, 7, 0], dtype=torch.int32, device="cuda")
ops.ring_gather([(ring, win)], slots, host)
torch.cuda.synchronize()
assert torch.equal(win, ring[[5, 6, 7, 0]]) and debug.debug_flags() == 0
slots[2] = 11                                        # outside the ring of 8; the host copy still says 7
try:
    ops.ring_gather([(ring, win)], slots, host)
except L.CometHipError as e:
    assert "index check failed" in str(e), str(e)
    assert debug.debug_flags() != 0
    print("DEBUG-OK", e)
else:
    raise SystemExit("the slot outside the ring was not reported")
"""


def test_debug_library_reports_failed_index_check():
    lib = os.path.join(PKG, "libcomet_hip_debug.so")
    if not os.path.isfile(lib):
        pytest.fail("libcomet_hip_debug.so missing: build it with `make -C comet-pose-estimation_amd DEBUG=1`")
    env = dict(os.environ, COMET_DEBUG="1")
    env.pop("COMET_HIP_LIB", None)
    r = subprocess.run([sys.executable, "-c", SCRIPT.format(pkg=PKG)], capture_output=True, text=True, env=env,
                       timeout=240, cwd=ROOT)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "DEBUG-OK" in r.stdout


def test_finite_check_names_the_module_and_the_gradient():
    from comet_amd import debug
    from comet_amd import functional as F
    from comet_amd._lib import CometHipError
    from comet_amd.models.modules import AttnBlock
    torch.manual_seed(0)
    blk = AttnBlock(128, 4).cuda()
    x = torch.randn(2, 20, 128, device="cuda")
    with F.precision(torch.float32), debug.FiniteCheck(blk):
        blk(x).sum().backward()  # finite: no error
    debug.check_grads(blk)
    assert not debug.debug_library() or debug.debug_flags() == 0
    x[1, 3, 5] = float("nan")
    with pytest.raises(CometHipError, match="non-finite values .* output of"):
        with F.precision(torch.float32), debug.FiniteCheck(blk):
            blk(x)
    blk.zero_grad()
    with F.precision(torch.float32):
        blk(x).sum().backward()
    with pytest.raises(CometHipError, match="gradient of"):
        debug.check_grads(blk)
    y = torch.tensor([1.0, float("inf"), float("nan"), 2.0], device="cuda")
    assert debug.count_nonfinite(y) == 2 and debug.count_nonfinite(y.to(torch.bfloat16)) == 2
