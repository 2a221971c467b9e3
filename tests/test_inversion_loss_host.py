"""Host checks of the inversion loss terms added beside the perceptual loss (reference:
/root/reference/exp/cips3d/models/projector_v10.py:1164-1200): `projector.mask_blend` and `projector.noise_regulariser` on CPU
tensors against the reference's torch expressions in fp64, the new keywords of `project_wplus`, and the C ABI's argument checks
(nothing here launches a kernel)."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

from cips_3dplusplus_amd import _lib, projector as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_regulariser(bufs):
    """projector_v10.py:1185-1194, verbatim but for the names."""
    reg = 0
    for v in bufs:
        noise = v
        while True:
            reg = reg + (noise * torch.roll(noise, shifts=1, dims=3)).mean() ** 2
            reg = reg + (noise * torch.roll(noise, shifts=1, dims=2)).mean() ** 2
            if noise.shape[2] <= 8:
                break
            noise = F.avg_pool2d(noise, kernel_size=2)
    return reg


def reference_mask(mask, channels, size):
    """`_G_forward`, :269-273: 1 - mask, expanded to the image's channels, bicubic to the image's size."""
    mt = 1 - mask.detach().expand(-1, channels, -1, -1)
    return F.interpolate(mt, scale_factor=size / mt.shape[-1], recompute_scale_factor=False, mode="bicubic")


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("cips3d_noise_reg_supported", "cips3d_noise_reg_launches", "cips3d_noise_reg_workspace", "cips3d_noise_reg",
              "cips3d_noise_reg_bwd", "cips3d_mask_blend", "cips3d_mask_blend_bwd"):
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.EXPORTED and hasattr(raw, s), s
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 37
    assert "inversion_loss.hip" in __import__("cips_3dplusplus_amd.build", fromlist=["SOURCES"]).SOURCES


def test_argument_errors_and_shape_support_do_not_launch():
    lib = _lib.load()
    sup = lib.cips3d_noise_reg_supported
    assert [sup(1, s) for s in (1, 4, 7, 8, 16, 32, 48, 96, 1024, 32768)] == [1] * 10
    assert [sup(1, s) for s in (9, 18, 36, 100, 65536)] == [0] * 5            # a pooled level with an odd side; too many levels
    assert sup(0, 16) == 0 and sup(2, 16) == 1
    tab = (_lib.NoiseBuf * 2)()
    tab[0].B, tab[0].S, tab[1].B, tab[1].S = 1, 16, 2, 1024
    pyramid = 64 + 2 * (512 ** 2 + 256 ** 2 + 128 ** 2 + 64 ** 2 + 32 ** 2 + 16 ** 2 + 8 ** 2)
    blocks = 1 + 1 + sum(-(-2 * s * s // 4096) for s in (1024, 512, 256, 128, 64, 32, 16, 8))
    assert lib.cips3d_noise_reg_workspace(tab, 2) == 4 * (pyramid + 2 * blocks + 2 * (2 + 8))
    tab[0].S = 18
    assert lib.cips3d_noise_reg_workspace(tab, 2) == -1
    assert lib.cips3d_noise_reg(tab, 2, 1.0, None, None, None) == -1
    assert lib.cips3d_noise_reg(None, 2, 1.0, None, None, None) == -1
    assert lib.cips3d_noise_reg_bwd(tab, 2, 1.0, None, None, None) == -1
    assert lib.cips3d_mask_blend(None, None, None, 1, 3, 8, 8, 1, None) == -1
    assert lib.cips3d_mask_blend_bwd(None, None, None, 1, 3, 8, 8, 1, None) == -1
    # the launch count does not grow with the number of buffers or levels (32 buffers share a launch)
    n = lib.cips3d_noise_reg_launches
    assert n(1, 8, 0) == 2 and n(1, 16, 0) == 3 and n(17, 512, 0) == 3 and n(32, 1024, 0) == 4 and n(9, 32768, 0) == 4
    assert n(1, 8, 1) == n(32, 1024, 1) == 1 and n(33, 1024, 1) == 2


@pytest.mark.parametrize("sizes", [[(1, 4)], [(1, 8), (1, 16), (1, 16), (2, 32)], [(1, 7)], [(2, 18)]])
def test_noise_regulariser_cpu_is_weight_times_the_reference(sizes):
    g = torch.Generator().manual_seed(3)
    bufs = [torch.randn(b, 1, s, s, generator=g, dtype=torch.float64).requires_grad_(True) for b, s in sizes]
    ref = reference_regulariser(bufs)
    assert torch.equal(P.noise_regulariser(bufs), ref)                       # weight 1: the old expression, bit for bit
    w = 1e5
    out = P.noise_regulariser(bufs, weight=w)
    assert abs(float(out.detach()) - w * float(ref.detach())) <= 1e-15 * w * float(ref.detach())
    grads = torch.autograd.grad(out, bufs)
    grads_ref = torch.autograd.grad(ref, bufs)
    for a, b in zip(grads, grads_ref):
        assert float((a - w * b).abs().max()) <= 1e-14 * w * float(b.abs().max())


@pytest.mark.parametrize("mask_hw,img_hw", [((8, 8), (8, 8)), ((8, 8), (32, 32)), ((5, 7), (10, 14)), ((4, 4), (12, 12))])
def test_mask_blend_cpu_matches_the_reference_expression(mask_hw, img_hw):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, *img_hw, generator=g, dtype=torch.float64).requires_grad_(True)
    mask = torch.rand(2, 1, *mask_hw, generator=g, dtype=torch.float64)
    mask[0, 0, 0, :3] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    m = reference_mask(mask, 3, img_hw[-1])
    assert m.shape == x.shape
    out = P.mask_blend(x, mask)
    ref = x * m + x.detach() * (1 - m)
    assert torch.equal(out, ref)
    assert float((out - x).abs().max()) <= 4 * 2.0 ** -53 * float((x.abs() * (m.abs() + (1 - m).abs())).max())
    gout = torch.randn(x.shape, generator=g, dtype=torch.float64)
    (gx,) = torch.autograd.grad(out, x, gout)
    assert torch.equal(gx, gout * m)                                          # the gradient is g * bicubic(1 - mask)
    assert not mask.requires_grad


def test_project_wplus_has_the_reference_keywords():
    sig = inspect.signature(P.FlipProjector.project_wplus).parameters
    assert sig["mask_background"].default is False
    assert sig["mse_weight"].default == 0.0 and isinstance(sig["mse_weight"].default, float)
    assert sig["target_images"].default is None
    assert sig["optim_noise_bufs"].default is False and sig["regularize_noise_weight"].default == 1e5
    assert inspect.signature(P.noise_regulariser).parameters["weight"].default == 1.0


def test_mse_weight_without_target_images_raises():
    proj = P.FlipProjector(G=None, device="cpu")                             # (raises before the generator is touched)
    with pytest.raises(ValueError, match="target_images"):
        proj.project_wplus({"img_size": 8}, {}, lambda rgb, thumb: rgb.sum(), N_steps_pose=1, mse_weight=1.0)
