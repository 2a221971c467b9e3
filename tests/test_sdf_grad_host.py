"""The SDF gradient (eikonal term) without a GPU: the recorded reference values against the oracle's autograd, the oracle's
gradient against finite differences, the diagnostics of losses.py, and the host-only answers of the new entry points."""
import os
import re

import pytest
import torch

from cips_3dplusplus_amd import _lib, losses
from oracle import path as O

import _sdf_grad_cases as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_case(golden, D):
    fx = golden("sdf_grad")
    inp = {k: fx[f"d{D}.{k}"] for k in ("pts", "rays_d", "viewdirs", "z", "near", "far", "styles")}
    return fx, inp


@pytest.mark.parametrize("D", [2, 6])
def test_fixture_inputs_follow_the_recipe(golden, D):
    """The fixture stores no weights and its inputs are formula-generated: the recipe reproduces them bit for bit."""
    fx, inp = fixture_case(golden, D)
    again = SG.explicit_inputs(2, 37, 5, D, tag="sgfix")
    for k, v in inp.items():
        assert torch.equal(v, again[k]), k
    assert not torch.equal(inp["styles"][0], inp["styles"][1]) and float(inp["near"][0]) != float(inp["near"][1])


@pytest.mark.parametrize("D", [2, 6])
def test_reference_eikonal_term_is_the_oracle_gradient(golden, D):
    """The reference's eikonal_term (fp32 autograd through its own modules) equals the fp64 gradient of
    oracle.path.renderer_forward to within fp32 noise, measured as |oracle fp32 - oracle fp64|, times 2."""
    fx, inp = fixture_case(golden, D)
    sd = SG.synth_renderer_sd(D)
    s64, g64 = SG.oracle_sdf_grad(sd, inp, D, torch.float64)
    s32, g32 = SG.oracle_sdf_grad(sd, inp, D, torch.float32)
    noise_max, noise_rms = SG.err_stats(g32, g64)
    e_max, e_rms = SG.err_stats(fx[f"d{D}.eikonal_term"], g64)
    print(f"D={D}: |fixture - fp64| max {e_max:.2e} rms {e_rms:.2e}; |oracle fp32 - fp64| max {noise_max:.2e} rms {noise_rms:.2e}; "
          f"largest component {float(g64.abs().max()):.1f}")
    assert noise_max > 0
    assert e_max <= 2 * noise_max and e_rms <= 2 * noise_rms
    assert SG.err_stats(fx[f"d{D}.sdf"], s64)[0] <= 2 * SG.err_stats(s32, s64)[0] + 1e-7


@pytest.mark.parametrize("D", [2, 6])
def test_oracle_gradient_agrees_with_central_differences(D):
    """fp64: (sdf(p + h e_k) - sdf(p - h e_k)) / 2h, h = 1e-6.  The truncation term is h^2 / 6 times the third derivative
    (~ (30 * 2 / span)^3 |g| per layer at worst: ~1e-5 relative), the rounding term 1e-16 / h ~ 1e-10."""
    sd = SG.synth_renderer_sd(D)
    inp = SG.explicit_inputs(2, 9, 3, D, tag="sgfd")
    _, g64 = SG.oracle_sdf_grad(sd, inp, D, torch.float64)
    sdd = {k: v.double() for k, v in sd.items()}
    c = {k: v.double() for k, v in inp.items()}
    h = 1e-6
    fd = torch.zeros_like(g64)
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[k] = h
        f = lambda p: O.renderer_forward(sdd, "renderer", p, c["rays_d"], c["viewdirs"], c["z"], c["near"], c["far"], c["styles"], D)[2]  # noqa: E731
        fd[..., k] = ((f(c["pts"] + e) - f(c["pts"] - e)) / (2 * h))[..., 0]
    err = float((fd - g64).abs().max())
    print(f"D={D}: |central differences - autograd| {err:.2e}, largest component {float(g64.abs().max()):.1f}")
    assert err <= 1e-4 * float(g64.abs().max())


@pytest.mark.parametrize("D", [2, 6])
def test_eikonal_loss_reproduces_the_reference(golden, D):
    fx, _ = fixture_case(golden, D)
    eik, sdf = fx[f"d{D}.eikonal_term"], fx[f"d{D}.sdf"]
    le, lm = losses.eikonal_loss(eik, sdf=sdf, beta=100)
    assert torch.equal(le, fx[f"d{D}.eikonal_loss"]) and torch.equal(lm, fx[f"d{D}.minimal_surface_loss"])
    le0, lm0 = losses.eikonal_loss(eik)
    assert torch.equal(le0, fx[f"d{D}.eikonal_loss_nosdf"]) and float(lm0) == 0.0 and lm0.device == eik.device


def test_eikonal_loss_of_a_distance_field_is_zero():
    g = torch.nn.functional.normalize(torch.randn(4, 7, 3, 3, dtype=torch.float64), dim=-1)
    le, lm = losses.eikonal_loss(g, sdf=torch.zeros(4, 7, 3, 1, dtype=torch.float64), beta=100)
    assert float(le) < 1e-30 and float(lm) == 1.0
    assert losses.eikonal_loss(None, sdf=torch.ones(3))[0] == 0


def test_sdf_grad_supported_is_a_host_answer():
    lib = _lib.load()
    for hidden, depth, want in ((256, 1, 1), (256, 8, 1), (256, 64, 1), (128, 2, 0), (256, 65, 0), (256, 0, 0)):
        assert lib.cips3d_nerf_sdf_grad_supported(hidden, depth) == want, (hidden, depth)


def test_abi_version_names_the_new_entry_points():
    lib = _lib.load()
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "cips3d_hip.h")).read())
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION
    assert _lib.ABI_VERSION >= 32
    assert "cips3d_nerf_sdf_grad" in _lib.EXPORTED and "cips3d_nerf_sdf_grad_supported" in _lib.EXPORTED


def test_plain_tensor_entry_points_still_refuse_and_say_where_to_go():
    from cips_3dplusplus_amd.nerf_utils import Render
    with pytest.raises(NotImplementedError, match="sdf_gradient"):
        Render.get_eikonal_term(torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3, 1))
    with pytest.raises(NotImplementedError, match="return_eikonal"):
        Render.volume_integration(None, None, None, None, None, None, return_eikonal=True)
