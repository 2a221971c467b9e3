"""The SDF gradient kernel (csrc/nerf_sdf_grad.hip) and the `eikonal_reg` / `return_eikonal` call surface built on it.

Yardstick: the fp64 autograd gradient of oracle.path.renderer_forward on the same inputs.  THE RULE, per case: with the fp32
oracle's own error against fp64 measured in the test (maximum and RMS),
    kernel RMS error <= 2 x the fp32 RMS error        (the project's rule for fp32 noise: test_gpu_split_fp16.py)
    kernel max error <= 4 x the fp32 max error        (a single-sample statistic, and the kernel sums in another order)
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, hip, weights
from cips_3dplusplus_amd.renderer import VolumeFeatureRenderer
from oracle import path as O

import _sdf_grad_cases as SG

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.5


def cu(t):
    return t.to(DEV).contiguous()


_REN = {}


def renderer(D, hidden=SG.H, with_sdf=True):
    key = (D, hidden, with_sdf)
    if key not in _REN:
        ren = VolumeFeatureRenderer(N_layers_renderer=D, input_dim=3, hidden_dim=hidden, style_dim=hidden, view_dim=3,
                                    with_sdf=with_sdf, output_features=True).eval().requires_grad_(False)
        sd = SG.synth_renderer_sd(D, hidden)
        ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()}, strict=True)
        _REN[key] = (ren.to(DEV), sd)
    return _REN[key]


def check_rule(name, got, g64, g32):
    n_max, n_rms = SG.err_stats(g32, g64)
    k_max, k_rms = SG.err_stats(got.cpu(), g64)
    print(f"{name}: kernel max {k_max:.3e} rms {k_rms:.3e} | fp32 oracle max {n_max:.3e} rms {n_rms:.3e} | ratios max "
          f"{k_max / max(n_max, 1e-30):.2f} rms {k_rms / max(n_rms, 1e-30):.2f} | largest component {float(g64.abs().max()):.1f}")
    assert torch.isfinite(got).all()
    assert k_rms <= 2 * n_rms, f"{name}: RMS error {k_rms:.3e} > 2 x {n_rms:.3e}"
    assert k_max <= 4 * n_max, f"{name}: max error {k_max:.3e} > 4 x {n_max:.3e}"


def kernel_explicit(ren, inp, pad=64):
    """(sdf [B,R,N], grad [B,R,N,3]) of the kernel on explicit points, written into sentinel-padded buffers that are checked."""
    B, R, N = inp["z"].shape
    styles_buf, film, tab = ren._film_table(B, torch.device(DEV))
    styles_buf.copy_(cu(inp["styles"]))
    tab.run(B)
    gbuf = torch.full((pad + B * R * N * 3 + pad,), SENTINEL, device=DEV)
    sbuf = torch.full((pad + B * R * N + pad,), SENTINEL, device=DEV)
    grad = gbuf[pad:pad + B * R * N * 3].view(B, R, N, 3)
    sdf = sbuf[pad:pad + B * R * N].view(B, R, N)
    ren._sdf_grad(film, cu(inp["near"]), cu(inp["far"]), B, N, x_pts=cu(inp["pts"]), n_rays=R, grad_out=grad, sdf_out=sdf)
    torch.cuda.synchronize()
    for buf, n in ((gbuf, B * R * N * 3), (sbuf, B * R * N)):
        assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all()), "store outside the output"
        assert not bool((buf[pad:pad + n] == SENTINEL).any()), "an output element was not written"
    return sdf.clone(), grad.clone()


@pytest.mark.parametrize("R,N", [(37, 5), (1, 1), (16, 24), (4099, 3)])
@pytest.mark.parametrize("D", [2, 6, 8])
def test_explicit_form_against_fp64_oracle(D, R, N):
    ren, sd = renderer(D)
    inp = SG.explicit_inputs(2, R, N, D, tag=f"sgx{R}")
    s64, g64 = SG.oracle_sdf_grad(sd, inp, D, torch.float64)
    s32, g32 = SG.oracle_sdf_grad(sd, inp, D, torch.float32)
    sdf, grad = kernel_explicit(ren, inp)
    check_rule(f"explicit D={D} R={R} N={N}", grad, g64, g32)
    e_sdf = SG.err_stats(sdf.cpu(), s64[..., 0])[0]
    print(f"   sdf: |kernel - fp64| {e_sdf:.2e}")
    assert e_sdf <= 1e-5


@pytest.mark.parametrize("D", [1, 16])
def test_explicit_form_at_the_depth_limits(D):
    """D = 1: no matrix layer at all (layer 0 feeds the head); D = 16: the FiLM table no longer fits beside the weight ring and
    is read from memory.  Same rule."""
    ren, sd = renderer(D)
    inp = SG.explicit_inputs(2, 37, 5, D, tag="sgdeep")
    _, g64 = SG.oracle_sdf_grad(sd, inp, D, torch.float64)
    _, g32 = SG.oracle_sdf_grad(sd, inp, D, torch.float32)
    _, grad = kernel_explicit(ren, inp)
    check_rule(f"explicit D={D}", grad, g64, g32)


@pytest.mark.parametrize("D", [2, 6])
def test_fixture_against_kernel(golden, D):
    """The reference's recorded eikonal_term is the fp32 side of the rule here."""
    fx = golden("sdf_grad")
    inp = {k: fx[f"d{D}.{k}"] for k in ("pts", "rays_d", "viewdirs", "z", "near", "far", "styles")}
    ren, sd = renderer(D)
    _, g64 = SG.oracle_sdf_grad(sd, inp, D, torch.float64)
    out = ren(cu(inp["pts"]), cu(inp["rays_d"]), cu(inp["viewdirs"]), cu(inp["z"]), cu(inp["near"]), cu(inp["far"]),
              styles=cu(inp["styles"]), return_eikonal=True)
    eik = out[5]
    assert eik.shape == inp["pts"].shape and eik.dtype == torch.float32 and eik.is_contiguous()
    check_rule(f"fixture D={D}", eik, g64, fx[f"d{D}.eikonal_term"])
    assert float((out[2].cpu() - fx[f"d{D}.sdf"]).abs().max()) <= 1e-5
    # the default call still returns None there, and so does a density renderer
    assert ren(cu(inp["pts"]), cu(inp["rays_d"]), cu(inp["viewdirs"]), cu(inp["z"]), cu(inp["near"]), cu(inp["far"]),
               styles=cu(inp["styles"]))[5] is None


def sample_points(total, at_least=4096, seed=7):
    """A fixed strided sample of the flat point index: prime stride, seeded start."""
    stride = max(1, total // at_least)
    while stride > 1 and any(stride % q == 0 for q in range(2, int(stride ** 0.5) + 1)):
        stride -= 1
    start = int(torch.randint(0, stride, (1,), generator=torch.Generator().manual_seed(seed)))
    idx = torch.arange(start, total, stride)
    assert idx.numel() >= at_least
    return idx


@pytest.mark.parametrize("D,S,N,perturb", [(2, 64, 24, True), (8, 64, 24, True), (2, 128, 128, False)])
def test_camera_form_against_fp64_oracle(D, S, N, perturb):
    ren, sd = renderer(D)
    B = 2 if S == 64 else 1
    locs = torch.tensor([[0.3, 0.1], [-0.2, 0.05]])[:B]
    cam = O.camera_params(locs, S, 6, 0.12)
    u = weights.det_unit_uniform("sgcam.u", (B, S * S), S) if perturb else None
    styles = weights.det_normal("sgcam.styles", (B, D + 1, SG.H), 0.5, D)
    idx = sample_points(S * S * N)

    def oracle(dt, static):
        full = SG.camera_inputs(cam, S, N, u, static, dt, D, styles)
        ray = idx // N
        sub = dict(pts=full["pts"].reshape(B, S * S * N, 1, 3)[:, idx], rays_d=full["rays_d"][:, ray], viewdirs=full["viewdirs"][:, ray],
                   z=full["z"].reshape(B, S * S * N, 1)[:, idx], near=full["near"], far=full["far"], styles=full["styles"])
        return SG.oracle_sdf_grad(sd, sub, D, dt)
    s64, g64 = oracle(torch.float64, False)
    s32, g32 = oracle(torch.float32, False)
    args = (cu(cam[0]), cu(cam[1]), cu(cam[2]), cu(cam[3]), cu(styles), S, N)
    pu = None if u is None else cu(u)
    sdf, grad = ren.sdf_gradient(*args, perturb_u=pu, static_viewdirs=False)
    assert sdf.shape == (B, S, S, N, 1) and grad.shape == (B, S, S, N, 3) and grad.is_contiguous()
    sdf_s, grad_s = ren.sdf_gradient(*args, perturb_u=pu, static_viewdirs=True)
    assert torch.equal(grad, grad_s) and torch.equal(sdf, sdf_s)          # the view layer is not part of it
    check_rule(f"camera D={D} {S}^2 x {N}", grad.reshape(B, -1, 3)[:, idx.to(DEV)].unsqueeze(2), g64, g32)
    # both kernels sampled the oracle's points: their sdf against fp64, the project's bar for NeRF maps
    r_sdf = ren.render(*args, perturb_u=pu, static_viewdirs=False, return_sdf=True)[2]
    for name, t in (("gradient kernel", sdf), ("render kernel", r_sdf)):
        e = SG.err_stats(t.reshape(B, -1)[:, idx.to(DEV)].cpu(), s64.reshape(B, -1))[0]
        print(f"   sdf of the {name}: |. - fp64| {e:.2e}")
        assert e <= 1e-5, name


def generator_case(name):
    if name == "ffhq1024_d2":
        return pkg.build_generator(configs.ffhq_G_cfg(1024, 2), DEV, seed=4), 64, 24, None
    if name == "ffhq256_d6":
        return pkg.build_generator(configs.ffhq_G_cfg(256, 6), DEV, seed=4), 64, 24, None
    return pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=4), 32, 12, 3        # style mixing: the per-op path


def generator_inputs(G, S, B=1):
    g = torch.Generator().manual_seed(11)
    zs = [cu(torch.randn(B, G.z_dim, generator=g)), cu(torch.randn(B, G.z_dim, generator=g))]
    cam = O.camera_params(torch.tensor([[0.25, -0.05]]).expand(B, 2).contiguous(), S, 6, 0.12)
    return zs, cam


@pytest.mark.parametrize("name", ["ffhq1024_d2", "ffhq256_d6", "per_op_inject"])
def test_generator_eikonal_term(name):
    G, S, N, inject = generator_case(name)
    zs, cam = generator_inputs(G, S)
    kw = dict(zs=zs, cam_poses=cu(cam[0]), focals=cu(cam[1]), img_size=S, near=cu(cam[2]), far=cu(cam[3]), inject_index=inject,
              return_sdf=True, return_xyz=True)
    planned = inject is None and G._forward_plan(1, S, N, False) is not None
    assert planned == (inject is None), "the planned configs must plan, the per-op one must not"

    # ---- perturb = False: values, layout, and every other entry unchanged
    ncfg = dict(N_samples=N, perturb=False, static_viewdirs=False)
    torch.manual_seed(3)
    ref = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in G(**kw, nerf_cfg=ncfg, eikonal_reg=False).items()}
    assert ref["eikonal_term"] is None
    torch.manual_seed(3)
    ret = G(**kw, nerf_cfg=ncfg, eikonal_reg=True)
    eik = ret["eikonal_term"]
    assert eik.shape == (1, S * S, N, 3) and eik.dtype == torch.float32 and eik.is_contiguous()
    for k, v in ref.items():
        if k != "eikonal_term":
            assert (v is None and ret[k] is None) or torch.equal(v, ret[k]), k
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items() if k.startswith("renderer.")}
    D = G.renderer.N_layers_renderer
    style_r, _ = G.mapping_networks(zs=zs, truncation=1, inject_index=inject)
    idx = sample_points(S * S * N)

    def oracle(dt, u):
        full = SG.camera_inputs(cam, S, N, u, False, dt, D, style_r.cpu())
        ray = idx // N
        sub = dict(pts=full["pts"].reshape(1, S * S * N, 1, 3)[:, idx], rays_d=full["rays_d"][:, ray], viewdirs=full["viewdirs"][:, ray],
                   z=full["z"].reshape(1, S * S * N, 1)[:, idx], near=full["near"], far=full["far"], styles=full["styles"])
        return SG.oracle_sdf_grad(sd, sub, D, dt)
    _, g64 = oracle(torch.float64, None)
    _, g32 = oracle(torch.float32, None)
    check_rule(f"Generator {name}", eik.reshape(1, -1, 3)[:, idx.to(DEV)].unsqueeze(2), g64, g32)

    # ---- perturb = True under a seed: same draw, same generator offset, gradient at the forward's jittered points
    ncfg = dict(N_samples=N, perturb=True, static_viewdirs=False)
    torch.manual_seed(5)
    ref = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in G(**kw, nerf_cfg=ncfg, eikonal_reg=False).items()}
    state_ref = torch.cuda.get_rng_state()
    torch.manual_seed(5)
    ret = G(**kw, nerf_cfg=ncfg, eikonal_reg=True)
    assert torch.equal(torch.cuda.get_rng_state(), state_ref)
    for k, v in ref.items():
        if k != "eikonal_term":
            assert (v is None and ret[k] is None) or torch.equal(v, ret[k]), k
    if planned:
        plan = G._forward_plan(1, S, N, False)
        u = plan.last_perturb_u
        assert u is not None and u.shape == (1, S * S)
        sdf2, grad2 = G.renderer.sdf_gradient(kw["cam_poses"], kw["focals"], kw["near"], kw["far"], None, S, N, perturb_u=u,
                                              film=plan.film)
        assert torch.equal(grad2.reshape(1, S * S, N, 3), ret["eikonal_term"])
        assert float((sdf2 - ret["sdf"]).abs().max()) <= 2e-5
        # ... and it is a different field from the un-jittered one
        assert not torch.equal(ret["eikonal_term"], eik)
    # ---- two runs give the same bits
    torch.manual_seed(5)
    again = G(**kw, nerf_cfg=ncfg, eikonal_reg=True)["eikonal_term"]
    assert torch.equal(again, ret["eikonal_term"])


def test_non_default_stream_and_reruns():
    D, S, N = 6, 32, 12
    ren, sd = renderer(D)
    cam = O.camera_params(torch.tensor([[0.1, 0.0]]), S, 6, 0.12)
    styles = weights.det_normal("sgst.styles", (1, D + 1, SG.H), 0.5, D)
    args = (cu(cam[0]), cu(cam[1]), cu(cam[2]), cu(cam[3]), cu(styles), S, N)
    sdf0, g0 = ren.sdf_gradient(*args)
    sdf1, g1 = ren.sdf_gradient(*args)
    assert torch.equal(g0, g1) and torch.equal(sdf0, sdf1)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sdf2, g2 = ren.sdf_gradient(*args)
    st.synchronize()
    assert torch.equal(g0, g2) and torch.equal(sdf0, sdf2)


def test_refusals():
    G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=4)
    S, N = 16, 6
    zs, cam = generator_inputs(G, S)
    kw = dict(cam_poses=cu(cam[0]), focals=cu(cam[1]), img_size=S, near=cu(cam[2]), far=cu(cam[3]),
              nerf_cfg=dict(N_samples=N, perturb=False, static_viewdirs=False))
    # the differentiable path: a graph through the gradient would be double backward
    s_r, s_d = G.mapping_networks(zs=zs, truncation=1, inject_index=None)
    s_r = s_r.detach().clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="double backward"):
        G(zs=zs, style_render=s_r, style_decoder=s_d.detach(), eikonal_reg=True, **kw)
    with pytest.raises(NotImplementedError, match="path_reg"):
        G(zs=zs, path_reg=True, **kw)
    # hidden 128: the limit is named
    G128 = pkg.build_generator(configs.tiny_G_cfg(128, 2, 1), DEV, seed=1)
    z128 = [cu(torch.randn(1, G128.z_dim)), cu(torch.randn(1, G128.z_dim))]
    with pytest.raises(NotImplementedError, match="hidden_dim = 256"):
        G128(zs=z128, eikonal_reg=True, **kw)
    ren128, _ = renderer(2, hidden=128)
    with pytest.raises(NotImplementedError, match="hidden_dim = 256"):
        ren128.sdf_gradient(kw["cam_poses"], kw["focals"], kw["near"], kw["far"], cu(torch.zeros(1, 3, 128)), S, N)
    # a density renderer has no SDF: None, as in the reference
    cfg = configs.ffhq_G_cfg(256, 2)
    cfg["renderer_cfg"]["with_sdf"] = False
    Gd = pkg.build_generator(cfg, DEV, seed=4)
    ret = Gd(zs=zs, eikonal_reg=True, **kw)
    assert ret["eikonal_term"] is None and ret["rgb"].shape[0] == 1
    inp = SG.explicit_inputs(1, 5, 3, 2, tag="sgraw")
    rend, _ = renderer(2, with_sdf=False)
    assert rend(cu(inp["pts"]), cu(inp["rays_d"]), cu(inp["viewdirs"]), cu(inp["z"]), cu(inp["near"]), cu(inp["far"]),
                styles=cu(inp["styles"]), return_eikonal=True)[5] is None
    # rays_forward hands the tensor through
    out = G.rays_forward(None, cu(inp["pts"]), cu(inp["rays_d"]), cu(inp["viewdirs"]), cu(inp["z"]), cu(inp["near"]), cu(inp["far"]),
                         cu(inp["styles"]), eikonal_reg=True)
    assert out[5].shape == inp["pts"].shape
    assert G.rays_forward(None, cu(inp["pts"]), cu(inp["rays_d"]), cu(inp["viewdirs"]), cu(inp["z"]), cu(inp["near"]),
                          cu(inp["far"]), cu(inp["styles"]))[5] is None


def test_tool_prints_json():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sdf_grad.py"), "--depth", "2", "--img-size", "32", "--samples", "8",
                        "--time", "--reps", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["points"] == 32 * 32 * 8 and d["grad_norm"]["max"] >= d["grad_norm"]["mean"] >= d["grad_norm"]["min"] >= 0
    assert d["eikonal_loss"] >= 0 and 0 <= d["minimal_surface_loss"] <= 1 and d["sdf_grad_ms"] > 0 and d["render_exact_ms"] > 0
