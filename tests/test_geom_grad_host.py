"""Host checks of the gradient through the render's mask / depth / xyz maps and of the silhouette term (the geometry
arguments of csrc/nerf_bwd.hip's compositing and camera entry points, projector.silhouette_loss, project_wplus's `silhouette_weight` / `target_masks`): the C ABI's declarations
and argument checks, the knobs' defaults and errors, and the CPU route of the loss.  Nothing here launches a kernel."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

from cips_3dplusplus_amd import _lib, projector as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cips3d_nerf_bwd_composite", "cips3d_nerf_bwd_camera")


def test_abi_exports_and_version():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    for s in ENTRY_POINTS:
        assert s in _lib.EXPORTED and s in _lib._SIGS and hasattr(raw, s), s
        assert re.search(r"\b%s\(" % s, header), s
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 41
    # the fused backward's params struct grew at its end by the three optional pointers; the binding's layout is the library's
    assert lib.cips3d_sizeof_struct(7) == ctypes.sizeof(_lib.NerfBwdFusedParams)
    names = [n for n, _ in _lib.NerfBwdFusedParams._fields_]
    assert names[-3:] == ["d_mask", "d_xyz", "xyz"] and names[-5:-3] == ["fwd_sdf", "fwd_crgb"]
    for n in ("d_mask", "d_xyz", "xyz"):
        assert re.search(r"const float\* %s;" % n, header), n


def test_library_refuses_incomplete_geometry_arguments():
    """Refused on the host, before anything is launched: null required pointers; d_mask without the forward's xyz; an upstream
    without the two per-ray sum buffers."""
    lib = _lib.load()
    geom = _lib.NerfBwdGeom()
    one = ctypes.cast(ctypes.pointer(ctypes.c_float(0.0)), ctypes.c_void_p).value       # a non-null host address: never read
    geom.cam_poses = geom.focals = geom.near_ = geom.far_ = one
    geom.B, geom.img_size, geom.n_samples, geom.static_viewdirs = 1, 2, 4, 0
    gp = ctypes.byref(geom)
    req = [one] * 10                                                                    # sdf .. ddnorm
    comp = lib.cips3d_nerf_bwd_composite
    assert comp(None, *req, None, None, None, None, None, None, None) != 0
    assert comp(gp, *req, None, one, None, None, one, one, None) != 0                   # d_mask without xyz
    assert comp(gp, *req, None, None, one, None, None, None, None) != 0                 # d_xyz without wsum / wzsum
    assert comp(gp, *req, None, one, one, one, one, None, None) != 0                    # ... without wzsum
    cam = lib.cips3d_nerf_bwd_camera                                                    # (dfocal = None throughout)
    assert cam(gp, one, one, one, one, None, None, one, one, 0, one, None, None) != 0   # d_mask without xyz
    assert cam(gp, one, one, one, None, one, None, None, None, 1, one, None, None) != 0 # d_xyz without the sums
    assert cam(gp, one, one, one, None, None, None, None, None, 0, None, None, None) != 0  # no dcam
    geom.B = 0                                                                          # an empty batch is a no-op
    assert comp(gp, *req, None, one, one, one, one, one, None) == 0
    assert cam(gp, one, one, one, one, one, one, one, one, 1, one, None, None) == 0


def test_project_wplus_has_the_silhouette_keywords():
    sig = inspect.signature(P.FlipProjector.project_wplus).parameters
    assert sig["silhouette_weight"].default == 0.0 and isinstance(sig["silhouette_weight"].default, float)
    assert sig["target_masks"].default is None
    assert list(inspect.signature(P.silhouette_loss).parameters) == ["mask", "target_masks", "weight"]


@pytest.mark.parametrize("masks", [None, torch.zeros(2, 1, 16, 16), torch.zeros(2, 8, 8), torch.zeros(1, 1, 8, 8),
                                   torch.zeros(2, 3, 8, 8)])
def test_silhouette_weight_needs_masks_of_the_render_resolution(masks):
    proj = P.FlipProjector(G=None, device="cpu")                             # (raises before the generator is touched)
    with pytest.raises(ValueError, match="target_masks"):
        proj.project_wplus({"img_size": 8, "fov_ang": 6, "dist_radius": 0.12}, {"N_samples": 4}, lambda rgb, thumb: rgb.sum(),
                           N_steps_pose=1, silhouette_weight=1.0, target_masks=masks)


@pytest.mark.parametrize("weight", [1.0, 0.37, 25.0])
def test_silhouette_loss_cpu_is_the_weighted_mse_against_the_background(weight):
    g = torch.Generator().manual_seed(7)
    mask = torch.rand(2, 1, 8, 8, generator=g, dtype=torch.float64).requires_grad_(True)
    target = torch.rand(2, 1, 8, 8, generator=g, dtype=torch.float64).round().requires_grad_(True)     # a hard segmentation
    out = P.silhouette_loss(mask, target, weight)
    ref = weight * F.mse_loss(mask, 1 - target.detach())
    assert torch.equal(out, ref)
    gm, gt = torch.autograd.grad(out, [mask, target], allow_unused=True)
    assert gt is None                                                        # the segmentation is a constant
    assert torch.equal(gm, torch.autograd.grad(ref, mask)[0])
    assert torch.allclose(gm, weight * 2 * (mask.detach() - (1 - target.detach())) / mask.numel(), rtol=1e-14, atol=0)
