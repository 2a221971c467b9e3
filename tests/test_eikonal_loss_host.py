"""The eikonal / minimal-surface losses without a GPU: the recipe's oracle against oracle.path.renderer_forward, the restatement of
the kernel's arithmetic and the torch expression behind VolumeFeatureRenderer.eikonal_loss against the oracle's double backward in
fp64, the new entry points' host-only answers, and the argument checks of project_wplus."""
import ctypes
import os
import re

import pytest
import torch

from cips_3dplusplus_amd import _lib, hip
from cips_3dplusplus_amd.projector import FlipProjector
from cips_3dplusplus_amd.renderer import VolumeFeatureRenderer
from oracle import path as O

import _eikonal_loss_cases as EC
import _sdf_grad_cases as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_renderer(D, hidden=SG.H, with_sdf=True, dt=torch.float64):
    ren = VolumeFeatureRenderer(N_layers_renderer=D, input_dim=3, hidden_dim=hidden, style_dim=hidden, view_dim=3, with_sdf=with_sdf,
                                output_features=True).eval().requires_grad_(False)
    sd = SG.synth_renderer_sd(D, hidden)
    ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()}, strict=True)
    return ren.to(dt), sd


def rel_max(x, ref):
    return float((x.double() - ref.double()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("D", [2, 6])
def test_recipe_trunk_is_the_oracle_renderer(D):
    """The recipe restates the trunk with gamma / beta as leaves: its sdf is oracle.path.renderer_forward's, in fp64."""
    sd = SG.synth_renderer_sd(D)
    inp = EC.case_inputs(D, 2, 37, 5)
    sdd, c = EC._cast(sd, inp, torch.float64)
    want = O.renderer_forward(sdd, "renderer", c["pts"], c["rays_d"], c["viewdirs"], c["z"], c["near"], c["far"], c["styles"], D)[2]
    got = EC.trunk_sdf(sdd, EC.film_of(sdd, c["styles"], D), c["pts"].reshape(2, -1, 3), c["near"], c["far"], D)
    assert float((got.reshape(want.shape) - want).abs().max()) <= 1e-13


@pytest.mark.parametrize("D,B,R,N", [(2, 2, 37, 5), (6, 1, 1, 1), (8, 3, 16, 24)])
def test_restatement_of_the_kernel_arithmetic_is_the_double_backward(D, B, R, N):
    """Forward-mode pass, seeds and reverse sweep as csrc/nerf_eikonal.hip performs them, in fp64 torch ops, against autograd's
    double backward: d L / d film to 1e-10 of its largest entry, both values to 1e-12 relative; the view row is exactly zero."""
    sd = SG.synth_renderer_sd(D)
    inp = EC.case_inputs(D, B, R, N)
    o = EC.oracle(sd, inp, D, torch.float64, lam_e=0.3, lam_m=0.7)
    r = EC.restatement(sd, inp, D, torch.float64, lam_e=0.3, lam_m=0.7)
    assert rel_max(r["dfilm"], o["dfilm"]) <= 1e-10
    assert EC.rel(r["eik"], o["eik"]) <= 1e-12 and EC.rel(r["ms"], o["ms"]) <= 1e-12
    assert not bool(r["dfilm"][:, D].any()) and not bool(o["dfilm"][:, D].any())


@pytest.mark.parametrize("D,perturb", [(2, False), (6, True)])
def test_torch_expression_of_eikonal_loss_is_the_oracle_in_fp64(D, perturb):
    """VolumeFeatureRenderer.eikonal_loss on CPU tensors (the A/B partner of the kernel): camera points, FiLM table and the double
    backward in torch ops.  d (0.3 eik + 0.7 ms) / d styles against the oracle to 1e-10 relative, in fp64."""
    c = EC.CAMERA_CASE
    cam, u, _, _ = EC.camera_case_inputs()
    styles = EC.weights.det_normal("eikhost.styles", (c["B"], D + 1, SG.H), 0.5, D).double()
    inp = SG.camera_inputs(cam, c["S"], c["N"], u if perturb else None, False, torch.float64, D, styles)
    ren, sd = cpu_renderer(D)
    o = EC.oracle(sd, inp, D, torch.float64, lam_e=0.3, lam_m=0.7)
    leaf = styles.clone().requires_grad_(True)
    eik, ms = ren.eikonal_loss(cam[0].double(), cam[1].double(), cam[2].double(), cam[3].double(), leaf, c["S"], c["N"],
                               perturb_u=u.double() if perturb else None)
    assert eik.dim() == 0 and ms.dim() == 0
    (0.3 * eik + 0.7 * ms).backward()
    assert EC.rel(float(eik.detach()), o["eik"]) <= 1e-10 and EC.rel(float(ms.detach()), o["ms"]) <= 1e-10
    assert rel_max(leaf.grad, o["dstyles"]) <= 1e-10
    # a [1, D+1, style_dim] latent is broadcast over the views: its gradient is the sum over them
    one = styles[:1].clone().requires_grad_(True)
    tot, e1, m1 = ren.eikonal_loss(cam[0].double(), cam[1].double(), cam[2].double(), cam[3].double(), one, c["S"], c["N"],
                                   perturb_u=u.double() if perturb else None, weights=(0.3, 0.7))
    tot.backward()
    o1 = EC.oracle(sd, dict(inp, styles=styles[:1].expand(c["B"], -1, -1)), D, torch.float64, lam_e=0.3, lam_m=0.7)
    assert rel_max(one.grad, o1["dstyles"].sum(0, keepdim=True)) <= 1e-10
    assert EC.rel(float(tot.detach()), 0.3 * o1["eik"] + 0.7 * o1["ms"]) <= 1e-10 and not e1.requires_grad and not m1.requires_grad


def test_exports_abi_and_signature():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 49
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cips3d_nerf_eikonal_loss", "cips3d_nerf_eikonal_supported", "cips3d_nerf_eikonal_workspace_bytes"):
        assert name in _lib.EXPORTED and hasattr(raw, name) and re.search(r"\b%s\(" % name, header), name
    # the call takes cips3d_nerf_params, whose layout the table checks, and scalars: eleven arguments, as the header declares
    assert len(_lib._SIGS["cips3d_nerf_eikonal_loss"][1]) == 11
    decl = re.search(r"int cips3d_nerf_eikonal_loss\((.*?)\);", header, flags=re.S).group(1)
    assert len(decl.split(",")) == 11
    assert lib.cips3d_sizeof_struct(2) == ctypes.sizeof(_lib.NerfParams)
    # host-only answers
    assert hip.nerf_eikonal_supported(256, 1) and hip.nerf_eikonal_supported(256, 64)
    assert not hip.nerf_eikonal_supported(128, 2) and not hip.nerf_eikonal_supported(256, 65) and not hip.nerf_eikonal_supported(256, 0)
    per_wg = 32 * 16 * 256 * 6 + 8 * 16 * 4 * 16 * 2 * 6 * 4 + 16       # scratch: 32 points x 16 H D bytes; slots; loss partials
    assert hip.nerf_eikonal_workspace_bytes(256, 6, 1) == per_wg
    assert hip.nerf_eikonal_workspace_bytes(256, 6, 256) == 256 * per_wg
    assert hip.nerf_eikonal_workspace_bytes(256, 6, 256, values_only=True) == 256 * 16
    assert hip.nerf_eikonal_workspace_bytes(128, 6, 256) == 0 and hip.nerf_eikonal_workspace_bytes(256, 6, 0) == 0
    # argument errors do not launch
    assert lib.cips3d_nerf_eikonal_loss(None, None, 1.0, 1.0, 100.0, 0, None, 0, None, None, None) == -1
    p = _lib.NerfParams()
    assert lib.cips3d_nerf_eikonal_loss(ctypes.byref(p), None, 1.0, 1.0, 100.0, 0, None, 0, None, None, None) == -1


def test_project_wplus_argument_checks():
    proj = FlipProjector(None, "cpu")           # every check below is made before the generator is touched
    cam_cfg, ncfg = {"img_size": 8}, {"N_samples": 6}
    with pytest.raises(ValueError, match="optim_render_params"):
        proj.project_wplus(cam_cfg, ncfg, None, optim_render_params=True, eikonal_weight=0.1)
    with pytest.raises(ValueError, match="optim_render_params"):
        proj.project_wplus(cam_cfg, ncfg, None, optim_render_params=True, minimal_surface_weight=0.1)
    for bad in (-1, 0, 1.5):
        with pytest.raises(ValueError, match="eikonal_every"):
            proj.project_wplus(cam_cfg, ncfg, None, eikonal_weight=0.1, eikonal_every=bad)
    with pytest.raises(ValueError, match="non-negative"):
        proj.project_wplus(cam_cfg, ncfg, None, eikonal_weight=-0.1)
    with pytest.raises(ValueError, match="eikonal_img_size"):
        proj.project_wplus(cam_cfg, ncfg, None, eikonal_weight=0.1, eikonal_img_size=0)


def test_refusals_name_the_limit():
    cam, u, _, _ = EC.camera_case_inputs()
    ren128, _ = cpu_renderer(2, hidden=128, dt=torch.float32)
    with pytest.raises(NotImplementedError, match="hidden_dim = 256"):
        ren128.eikonal_loss(cam[0], cam[1], cam[2], cam[3], torch.zeros(2, 3, 128), 8, 5)
    rend, _ = cpu_renderer(2, with_sdf=False, dt=torch.float32)
    with pytest.raises(NotImplementedError, match="with_sdf=False"):
        rend.eikonal_loss(cam[0], cam[1], cam[2], cam[3], torch.zeros(2, 3, 256), 8, 5)
    with pytest.raises(NotImplementedError, match="hidden_dim = 256"):
        hip.nerf_eikonal_loss(near_=cam[2], far_=cam[3], w_first=None, packed32=None, packed32_t=None, film=None, layer_bias=None,
                              w_sigma=None, b_sigma=None, B=2, n_samples=5, hidden=128, depth=2)
