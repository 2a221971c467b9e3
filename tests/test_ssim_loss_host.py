"""Host checks of the Gaussian-window SSIM loss (csrc/ssim_loss.hip; metrics.ssim_gaussian, projector.ssim_loss): the C ABI's
declarations, the torch expression against an independent numpy / scipy evaluation of the definition, every argument error on
CPU tensors (none may reach the library), and the CPU route of `projector.ssim_loss`.  Nothing here launches a kernel."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy.ndimage import correlate1d

from cips_3dplusplus_amd import _lib, hip, metrics as M, projector as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cips3d_ssim_loss_tile", "cips3d_ssim_loss_workspace_bytes", "cips3d_ssim_loss", "cips3d_ssim_loss_bwd")


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the HIP library fails the test."""
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "_lib", None)


def test_abi_exports_and_version():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    for s in ENTRY_POINTS:
        assert s in _lib.EXPORTED and s in _lib._SIGS and hasattr(raw, s), s
        assert re.search(r"\b%s\(" % s, header), s
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 40


def test_host_side_argument_checks_of_the_library():
    lib = _lib.load()
    th, tw, threads = hip.ssim_loss_tile()
    assert th >= 1 and tw >= 1 and threads % 64 == 0 and (th * tw) % threads == 0
    ws = lib.cips3d_ssim_loss_workspace_bytes
    assert ws(2, 3, 10, 64, 0) < 0 and ws(2, 3, 64, 10, 1) < 0 and ws(0, 3, 64, 64, 0) < 0 and ws(1, 0, 64, 64, 0) < 0
    tiles = -(-(64 - 10) // th) * -(-(64 - 10) // tw)
    small, big = ws(2, 3, 64, 64, 0), ws(2, 3, 64, 64, 1)
    assert small >= 4 * 2 * 3 * tiles and small % 16 == 0
    assert big - small == 3 * 4 * 2 * 3 * 54 * 54                     # three fp32 maps of [B,C,H-10,W-10]
    assert ws(1, 3, 1024, 1024, 1) - ws(1, 3, 1024, 1024, 0) == 3 * 4 * 3 * 1014 * 1014      # 37 MB per 1024^2 RGB image
    # null pointers and bad shapes are refused before anything is launched
    assert lib.cips3d_ssim_loss(None, None, 1, 3, 32, 32, 1.0, 2.0, None, 0, None, None, None, None) != 0
    assert lib.cips3d_ssim_loss_bwd(None, None, 1, 3, 32, 32, 1.0, None, None, None, None) != 0


def numpy_ssim(a, b, data_range):
    """The definition with numpy and scipy.ndimage.correlate1d, float64: -> (ssim [B], S [B,C,H-10,W-10])."""
    i = np.arange(11, dtype=np.float64)
    g = np.exp(-(i - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    g /= g.sum()

    def E(x):
        y = correlate1d(correlate1d(x, g, axis=-1, mode="constant"), g, axis=-2, mode="constant")
        return y[..., 5:-5, 5:-5]                                     # the windows wholly inside the image
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = E(a), E(b)
    vx, vy, vxy = E(a * a) - mx * mx, E(b * b) - my * my, E(a * b) - mx * my
    S = (2 * mx * my + c1) * (2 * vxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return S.mean(axis=(1, 2, 3)), S


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(11, 11), (12, 75), (43, 41)])
@pytest.mark.parametrize("data_range", [2.0, 1.0])
def test_torch_expression_matches_numpy(H, W, C, data_range):
    g = torch.Generator().manual_seed(H * 100 + W + C)
    a = torch.rand(2, C, H, W, generator=g, dtype=torch.float64) * 2 - 1
    b = a + 0.1 * torch.randn(2, C, H, W, generator=g, dtype=torch.float64)
    ssim, S = M._ssim_gaussian_torch(a, b, data_range)
    want, want_S = numpy_ssim(a.numpy(), b.numpy(), data_range)
    assert ssim.dtype == torch.float64 and S.shape == (2, C, H - 10, W - 10)
    assert np.abs(S.numpy() - want_S).max() <= 1e-12 and np.abs(ssim.numpy() - want).max() <= 1e-12
    same, same_S = M._ssim_gaussian_torch(a, a.clone(), data_range)
    assert bool((same == 1.0).all()) and bool((same_S == 1.0).all())  # exactly
    # the public entry point on CPU tensors is this expression: float64 [B] on the CPU, the map on request
    out, smap = M.ssim_gaussian(a, b, data_range, return_map=True)
    assert out.dtype == torch.float64 and torch.equal(out, ssim) and torch.equal(smap, S)
    assert torch.equal(M.ssim_gaussian(a[0], b[0], data_range), ssim[:1])          # [C, H, W] is one image


def test_argument_errors_never_touch_the_library(no_library):
    a = torch.zeros(2, 3, 16, 16)
    for bad in (torch.zeros(2, 3, 10, 16), torch.zeros(2, 3, 16, 10)):
        with pytest.raises(ValueError, match="win_size 11"):
            M.ssim_gaussian(bad, bad)
        with pytest.raises(ValueError, match="win_size 11"):
            P.ssim_loss(bad, bad, 1.0)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        M.ssim_gaussian(torch.zeros(1, 2, 16, 16), torch.zeros(1, 2, 16, 16))
    with pytest.raises(ValueError, match="differ in shape"):
        M.ssim_gaussian(a, torch.zeros(2, 3, 16, 17))
    with pytest.raises(ValueError, match="differ in shape"):
        P.ssim_loss(a, torch.zeros(1, 3, 16, 16), 1.0)
    with pytest.raises(ValueError, match="must be a tensor"):
        M.ssim_gaussian(a.numpy(), a)
    with pytest.raises(ValueError, match="must be a tensor"):
        M.ssim_gaussian(a, None)
    with pytest.raises(ValueError, match="floating-point"):
        M.ssim_gaussian(a.to(torch.uint8), a.to(torch.uint8))
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        M.ssim_gaussian(torch.zeros(16, 16), torch.zeros(16, 16))
    with pytest.raises(ValueError, match="data_range"):
        M.ssim_gaussian(a, a, data_range=0.0)
    assert not hip.ssim_loss_supported(a, a) and not hip.ssim_loss_supported(None, a)      # CPU tensors: the torch expression
    # project_wplus: the new knob needs the target images; checked before anything is built
    assert inspect.signature(P.FlipProjector.project_wplus).parameters["ssim_weight"].default == 0.0
    with pytest.raises(ValueError, match="ssim_weight > 0 needs target_images"):
        P.FlipProjector(None, "cpu").project_wplus({}, {}, None, ssim_weight=1.0)


def test_projector_ssim_loss_on_cpu_tensors(no_library):
    g = torch.Generator().manual_seed(5)
    rgb = (torch.rand(2, 3, 20, 23, generator=g) * 2 - 1).requires_grad_(True)
    target = (rgb.detach() + 0.1 * torch.randn(2, 3, 20, 23, generator=g)).requires_grad_(True)
    loss = P.ssim_loss(rgb, target.detach(), 2.5)
    want = 2.5 * (1 - M._ssim_gaussian_torch(rgb.detach(), target.detach(), 2.0)[0]).mean()
    assert loss.dtype == torch.float32 and float(loss.detach()) == float(want) and 0 < float(want) < 2.5
    loss.backward()
    assert rgb.grad is not None and float(rgb.grad.abs().max()) > 0 and target.grad is None
    # the gradient is that of the definition: against fp64 autograd
    r64 = rgb.detach().double().requires_grad_(True)
    (2.5 * (1 - M._ssim_gaussian_torch(r64, target.detach().double(), 2.0)[0]).mean()).backward()
    assert float((rgb.grad.double() - r64.grad).abs().max()) <= 1e-4 * float(r64.grad.abs().max())
    assert float(P.ssim_loss(rgb.detach(), rgb.detach().clone(), 4.0)) == 0.0
