"""Host checks of the image metrics (cips_3dplusplus_amd/metrics.py, csrc/metrics.hip): PSNR from the squared error, every
argument error on CPU tensors (none of them may reach the library), the new keyword of `project_wplus`, and the C ABI's
declarations and argument checks.  Nothing here launches a kernel."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from cips_3dplusplus_amd import _lib, metrics as M, projector as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cips3d_image_metrics", "cips3d_image_metrics_workspace_bytes", "cips3d_image_metrics_tile")


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the HIP library fails the test."""
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "_lib", None)


def test_psnr_from_sse():
    n = 3 * 8 * 8
    assert M.psnr_from_sse(0, n) == math.inf
    assert M.psnr_from_sse(65025 * n, n) == 0.0                                   # every pixel off by the full range
    assert abs(M.psnr_from_sse(n, n) - 48.1308036086791) < 1e-12                  # every pixel off by one grey level
    t = M.psnr_from_sse(torch.tensor([0, n, 100 * n, 65025 * n]), n)
    assert t.dtype == torch.float64 and t.shape == (4,)
    assert t[0] == math.inf and float(t[1]) == M.psnr_from_sse(n, n) and float(t[3]) == 0.0
    assert abs(float(t[2]) - (10.0 * math.log10(65025.0) - 20.0)) < 1e-12
    big = 65025 * 3 * 2 ** 20                                                      # a 1024^2 RGB image, all 0 against all 255
    assert M.psnr_from_sse(big, 3 * 2 ** 20) == 0.0


def test_argument_errors_are_raised_before_the_library_is_touched(no_library):
    f = torch.zeros(2, 3, 9, 9)
    u = torch.zeros(2, 3, 9, 9, dtype=torch.uint8)
    for fn in (M.image_metrics, M.psnr, M.ssim, M.image_sse_ssim):
        with pytest.raises(ValueError, match="shape"):
            fn(f, torch.zeros(2, 3, 9, 10))
        with pytest.raises(ValueError, match="shape"):
            fn(f, u[:1])
        with pytest.raises(ValueError, match="float32"):
            fn(f, f.double())
        with pytest.raises(ValueError, match="float32"):
            fn(f.half(), f)
        with pytest.raises(ValueError, match="float32"):
            fn(u.to(torch.int32), u)
        with pytest.raises(ValueError, match="win_size"):
            fn(torch.zeros(1, 3, 6, 9), torch.zeros(1, 3, 6, 9))
        with pytest.raises(ValueError, match="win_size"):
            fn(torch.zeros(1, 3, 9, 6, dtype=torch.uint8), torch.zeros(1, 3, 9, 6, dtype=torch.uint8))
        with pytest.raises(ValueError, match="channels"):
            fn(torch.zeros(1, 2, 9, 9), torch.zeros(1, 2, 9, 9))
        with pytest.raises(ValueError, match="channels"):
            fn(torch.zeros(1, 4, 9, 9), torch.zeros(1, 4, 9, 9))
        with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
            fn(torch.zeros(9, 9), torch.zeros(9, 9))
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(0, 3, 9, 9), torch.zeros(0, 3, 9, 9))
        with pytest.raises(RuntimeError, match="HIP tensors"):                    # valid arguments on the CPU: no fallback
            fn(f, u)


def test_metrics_log_argument_errors(no_library):
    target = torch.zeros(1, 3, 9, 9)
    with pytest.raises(ValueError, match="one image"):
        M.MetricsLog(torch.zeros(2, 3, 9, 9), 4)
    with pytest.raises(ValueError, match="win_size"):
        M.MetricsLog(torch.zeros(3, 6, 6), 4)
    with pytest.raises(ValueError, match="channels"):
        M.MetricsLog(torch.zeros(2, 9, 9), 4)
    with pytest.raises(ValueError, match="float32"):
        M.MetricsLog(target.double(), 4)
    with pytest.raises(ValueError, match="capacity"):
        M.MetricsLog(target, 0)
    log = M.MetricsLog(target[0], 2)                                               # [C, H, W] is one image
    assert log.capacity == 2 and log.target.shape == (1, 3, 9, 9)
    with pytest.raises(ValueError, match="shape"):
        log.update(0, torch.zeros(1, 3, 9, 10))
    with pytest.raises(ValueError, match="shape"):
        log.update(0, torch.zeros(2, 3, 9, 9))
    with pytest.raises(ValueError, match="float32"):
        log.update(0, target.double())
    with pytest.raises(ValueError, match="outside the record"):
        log.update(0, target, row=2)
    with pytest.raises(ValueError, match="outside the record"):
        log.update(0, target, row=-1)
    with pytest.raises(RuntimeError, match="HIP tensors"):
        log.update(0, torch.zeros(1, 3, 9, 9, dtype=torch.uint8))
    assert log.result()["steps"] == [] and log.result()["ssim"].shape == (0,)
    assert log.result()["psnr"].shape == (0,) and log.result()["psnr"].dtype == torch.float64
    log.steps.update({0: 10, 1: 11})                                               # both rows taken
    with pytest.raises(ValueError, match="full"):
        log.update(12, target)


def test_project_wplus_metrics_every_needs_target_images():
    sig = inspect.signature(P.FlipProjector.project_wplus).parameters
    assert sig["metrics_every"].default == 0
    proj = P.FlipProjector(G=None, device="cpu")                                   # (raises before the generator is touched)
    with pytest.raises(ValueError, match="metrics_every > 0 needs target_images"):
        proj.project_wplus({"img_size": 8}, {}, lambda rgb, thumb: rgb.sum(), N_steps_pose=1, metrics_every=5)
    with pytest.raises(ValueError, match="non-negative integer"):
        proj.project_wplus({"img_size": 8}, {}, lambda rgb, thumb: rgb.sum(), N_steps_pose=1, metrics_every=-1)


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.EXPORTED and s in _lib._SIGS and hasattr(raw, s), s
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 38
    assert "metrics.hip" in __import__("cips_3dplusplus_amd.build", fromlist=["SOURCES"]).SOURCES


def test_c_abi_argument_errors_and_sizes_do_not_launch():
    lib = _lib.load()
    th, tw, threads = M.tile()
    assert th >= 1 and tw >= 1 and threads % 64 == 0 and (th * tw) % threads == 0
    ws = lib.cips3d_image_metrics_workspace_bytes
    assert ws(1, 3, 6, 9) == -1 and ws(1, 3, 9, 6) == -1 and ws(0, 3, 9, 9) == -1 and ws(1, 0, 9, 9) == -1
    one = ws(1, 1, 7, 7)
    assert one > 0 and one % 16 == 0
    # one tile covers th x tw window origins = (th + 6) x (tw + 6) pixels; one more row or column of pixels starts another
    assert ws(1, 1, th + 6, tw + 6) == one
    assert ws(1, 1, th + 7, tw + 6) == 2 * one and ws(1, 1, th + 6, tw + 7) == 2 * one and ws(1, 1, th + 7, tw + 7) == 4 * one
    assert ws(3, 3, 2 * th + 7, tw + 7) == 3 * 3 * 3 * 2 * one
    f = lib.cips3d_image_metrics
    assert f(None, 0, None, 0, 1, 3, 9, 9, None, None, 0, None) == -1
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    assert f(p, 1, p, 1, 1, 3, 6, 9, p, p, 0, None) == -1                         # a side under 7
    assert f(p, 1, p, 1, 1, 3, 9, 9, p, p, -1, None) == -1                        # a negative row
    assert f(p, 1, p, 1, 0, 3, 9, 9, p, p, 0, None) == -1
    assert f(p, 1, p, 1, 1, 3, 9, 9, p + 8, p, 0, None) == -2                     # a misaligned workspace
    assert f(p + 1, 0, p, 1, 1, 3, 9, 9, p, p, 0, None) == -2                     # a misaligned fp32 image
