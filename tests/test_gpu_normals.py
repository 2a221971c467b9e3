"""Composited surface normals and the shaded geometry frame (csrc/nerf_normals.hip), the call surface built on them
(`VolumeFeatureRenderer.normal_map`, `Generator.forward(return_normal=True)`, `sample_multi_view(gather=(..., "normal", "shaded"))`,
tools/normals.py), and the marching-cubes vertex normals (cips3d_marching_cubes_normals in csrc/mesh.hip).

Yardsticks.  Compositing: `oracle.path.volume_integration` in fp64 with the gradients in the place of the points -- its `xyz`
output is then exactly normal_raw.  Per ray, with w the fp64 weights,
    |kernel - fp64| <= (2 N + 16) 2^-23 sum_i w_i |grad_i|
(a few ulp per weight, an N-term product and an N-term sum).  End to end: the rule of test_gpu_sdf_grad.py, the fp32 oracle
pipeline as the noise yardstick (RMS <= 2 x, max <= 4 x).  Shading: the formula in fp64 on the same inputs,
|d| <= (kd + s ks) 16 2^-23.  Vertex normals: an fp64 numpy restatement of the header's contract, per component
|d| <= 8 2^-23 max|A| / |g64| + 4 2^-23."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import _lib, configs, gen_images, hip, mesh, weights
from cips_3dplusplus_amd.renderer import VolumeFeatureRenderer
from oracle import path as O

import _sdf_grad_cases as SG

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.5
SENTINEL_U8 = 201
PAD = 64
ULP = 2.0 ** -23


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


def padded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), SENTINEL_U8 if dtype == torch.uint8 else SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(*shape)


def check_padded(buf, what):
    """Nothing outside the output was written; (fp32) nothing inside was left."""
    sent = SENTINEL_U8 if buf.dtype == torch.uint8 else SENTINEL
    n = buf.numel() - 2 * PAD
    assert bool((buf[:PAD] == sent).all()) and bool((buf[PAD + n:] == sent).all()), f"{what}: store outside the output"
    if buf.dtype != torch.uint8:
        assert not bool((buf[PAD:PAD + n] == sent).any()), f"{what}: an output element was not written"


def run_explicit(sdf, grad, beta, z, rays_d, shade=None, **phong):
    """hip.nerf_normals in its explicit form, every output in a sentinel-padded buffer -> dict of CPU tensors."""
    B, R, N = sdf.shape
    bufs = {"normal_raw": padded((B, 3, R)), "normal": padded((B, 3, R))}
    kw = {}
    if shade is not None:
        bufs["shade"], bufs["shade_u8"] = padded((B, R)), padded((B, 3, R), torch.uint8)
        kw = dict(xyz=cu(shade["xyz"]), eye=cu(shade["eye"]), light=cu(shade["light"]), **phong)
    out = hip.nerf_normals(sdf=cu(sdf), grad=cu(grad), sigmoid_beta=cu(beta.reshape(1).float()), B=B, n_samples=N, x_z_vals=cu(z),
                           x_rays_d=cu(rays_d), n_rays=R, want=(), **{k + "_out": v[1] for k, v in bufs.items()}, **kw)
    torch.cuda.synchronize()
    assert set(out) == set(bufs)
    for k, (buf, _) in bufs.items():
        check_padded(buf, k)
    return {k: v.cpu().clone() for k, v in out.items()}


def composite64(sdf, grad, z, rays_d, beta):
    """(normal_raw (B,R,3), sum_i w_i |grad_i| (B,R)) by the oracle's volume integration in fp64, gradients as points."""
    s, g = sdf.double().reshape(*grad.shape[:-1], 1), grad.double()
    zero3, zero1 = torch.zeros_like(g), torch.zeros_like(s)
    args = (zero3, s, zero1, z.double(), rays_d.double())
    raw = O.volume_integration(*args, g, beta.double())[2]
    wsum = O.volume_integration(*args, g.norm(dim=-1, keepdim=True).expand_as(g), beta.double())[2][..., 0]
    return raw, wsum


def check_compositing_bound(name, raw_kernel, raw64, wsum, N):
    """raw_kernel (B,3,R) against raw64 (B,R,3), per ray."""
    err = (raw_kernel.double().transpose(1, 2) - raw64).abs().amax(-1)
    bound = (2 * N + 16) * ULP * wsum
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, largest err / bound {ratio:.3f}, smallest |normal_raw| {float(raw64.norm(dim=-1).min()):.3f}")
    assert torch.isfinite(raw_kernel).all()
    assert bool((err <= bound).all()), f"{name}: err / bound = {ratio:.2f}"


def check_normalised(name, out):
    want = F.normalize(out["normal_raw"], dim=1, eps=1e-12)
    d = float((out["normal"] - want).abs().max())
    print(f"{name}: |normal - F.normalize(normal_raw)| {d:.2e}")
    assert d <= 4 * ULP


# ------------------------------------------------------------------------------------------------ 1. compositing in isolation
# (1,1): only the infinite last interval; (37,5), (16,24): segments that do not fill a wave; (130,64): a full wave per ray and a
# ray count that leaves a partial block; (3,129): two carries plus one sample; (4099,3): a ray count that is no multiple of anything
@pytest.mark.parametrize("R,N", [(1, 1), (37, 5), (16, 24), (130, 64), (3, 129), (4099, 3)])
@pytest.mark.parametrize("D", [2, 8])
def test_compositing_explicit_form_against_fp64(D, R, N):
    sd = SG.synth_renderer_sd(D)
    inp = SG.explicit_inputs(2, R, N, D, tag=f"nrm{R}")
    s32, g32 = SG.oracle_sdf_grad(sd, inp, D, torch.float32)
    beta = sd["renderer.sigmoid_beta"]
    raw64, wsum = composite64(s32, g32, inp["z"], inp["rays_d"], beta)
    out = run_explicit(s32[..., 0], g32, beta, inp["z"], inp["rays_d"])
    name = f"explicit D={D} R={R} N={N}"
    check_compositing_bound(name, out["normal_raw"], raw64, wsum, N)
    check_normalised(name, out)


# ------------------------------------------------------------------------------------------------ 2. degenerate weights
def test_degenerate_weights():
    """beta = 1e-3.  sdf = +1e4: sigmoid(-1e7) = 0, every weight is 0.  sdf = -1e4: sigma = 1000, and the first interval of view 1
    is at least (1.25 - 0.80) / 5 x |d| = 0.09 long, so the first sample leaves a transmittance of exp(-90) < 1e-39: every later
    weight is below the 1e-10 the reference adds, 1e-5 of the bound."""
    R, N = 37, 5
    inp = SG.explicit_inputs(2, R, N, 2, tag="nrmdeg")
    beta = torch.tensor([1e-3])
    grad = weights.det_normal("nrmdeg.g", (2, R, N, 3), 1.0, R)
    sdf = torch.empty(2, R, N)
    sdf[0], sdf[1] = 1e4, -1e4
    shade = dict(xyz=torch.zeros(2, 3, R), eye=torch.tensor([[0.0, 0.0, 1.0]] * 2), light=torch.tensor([[0.0, 0.0, 5.0]] * 2))
    out = run_explicit(sdf, grad, beta, inp["z"], inp["rays_d"], shade=shade)
    for k in ("normal_raw", "normal", "shade"):
        assert torch.isfinite(out[k]).all(), k
    assert bool((out["normal_raw"][0] == 0).all()) and bool((out["normal"][0] == 0).all())
    assert bool((out["shade"][0] == torch.tensor(hip.PHONG_DEFAULTS["ka"], dtype=torch.float32)).all())
    assert bool((out["shade_u8"][0] == 26).all())                       # floor(25.5 + 0.5)
    raw64, wsum = composite64(sdf, grad, inp["z"], inp["rays_d"], beta)
    check_compositing_bound("sdf = -1e4 against fp64", out["normal_raw"][1:], raw64[1:], wsum[1:], N)
    first = grad[1:, :, 0].double()
    check_compositing_bound("sdf = -1e4 against grad[:, :, 0]", out["normal_raw"][1:], first, first.norm(dim=-1), N)


# ------------------------------------------------------------------------------------------------ 3. end to end, camera form
def check_rule(name, got, ref64, ref32):
    n_max, n_rms = SG.err_stats(ref32, ref64)
    k_max, k_rms = SG.err_stats(got, ref64)
    print(f"{name}: kernel max {k_max:.3e} rms {k_rms:.3e} | fp32 oracle max {n_max:.3e} rms {n_rms:.3e} | ratios max "
          f"{k_max / max(n_max, 1e-30):.2f} rms {k_rms / max(n_rms, 1e-30):.2f}")
    assert torch.isfinite(got).all()
    assert k_rms <= 2 * n_rms, f"{name}: RMS error {k_rms:.3e} > 2 x {n_rms:.3e}"
    assert k_max <= 4 * n_max, f"{name}: max error {k_max:.3e} > 4 x {n_max:.3e}"


@pytest.mark.parametrize("D,S,N,perturb", [(2, 32, 24, True), (8, 32, 12, False)])
def test_normal_map_camera_form_against_fp64_oracle(D, S, N, perturb):
    ren, sd = renderer(D)
    B, R = 2, S * S
    cam = O.camera_params(torch.tensor([[0.3, 0.1], [-0.2, 0.05]]), S, 6, 0.12)
    u = weights.det_unit_uniform("nrmcam.u", (B, R), S) if perturb else None
    styles = weights.det_normal("nrmcam.styles", (B, D + 1, SG.H), 0.5, D)

    def oracle(dt):
        inp = SG.camera_inputs(cam, S, N, u, False, dt, D, styles)
        s, g = SG.oracle_sdf_grad(sd, inp, D, dt)
        zero3, zero1 = torch.zeros_like(g), torch.zeros_like(s)
        return O.volume_integration(zero3, s, zero1, inp["z"], inp["rays_d"], g, sd["renderer.sigmoid_beta"].to(dt))[2]
    n64, n32 = oracle(torch.float64), oracle(torch.float32)
    args = (cu(cam[0]), cu(cam[1]), cu(cam[2]), cu(cam[3]), cu(styles), S, N)
    pu = None if u is None else cu(u)
    out = ren.normal_map(*args, perturb_u=pu)
    assert set(out) == {"normal", "normal_raw"}
    assert out["normal"].shape == out["normal_raw"].shape == (B, 3, S, S) and out["normal"].is_contiguous()
    raw = out["normal_raw"].reshape(B, 3, R).transpose(1, 2).cpu()
    check_rule(f"camera D={D} {S}^2 x {N}", raw, n64, n32)
    check_normalised("camera", {k: v.cpu() for k, v in out.items()})
    # handing the gradient in gives the same bits; so do a second run and a run on another stream
    sdf, grad = ren.sdf_gradient(*args, perturb_u=pu)
    again = ren.normal_map(*args, perturb_u=pu, grad=grad, sdf=sdf)
    twice = ren.normal_map(*args, perturb_u=pu)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        other = ren.normal_map(*args, perturb_u=pu)
    st.synchronize()
    for k in out:
        assert torch.equal(out[k], again[k]) and torch.equal(out[k], twice[k]) and torch.equal(out[k], other[k]), k


_GEOM_CAM = []


@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("N", [1, 5, 24])
def test_camera_form_equals_explicit_form_on_the_stand_alone_geometry(N, perturb):
    """The camera form builds its rays and depths in the kernel; the explicit form reads what hip.rays_in_world and hip.z_vals
    wrote.  Both evaluate the expressions of csrc/nerf_geom.h in fp32 with contraction off (division and square root correctly
    rounded), so the two forms must give the same bits, not merely close ones."""
    from cips_3dplusplus_amd.camera import Camera
    B, S = 2, 8
    R = S * S
    if not _GEOM_CAM:
        _GEOM_CAM.append(Camera.generate_camera_params(S, DEV, locations=torch.tensor([[0.3, 0.1], [-0.2, 0.05]], device=DEV))[:4])
    extr, focal, near, far = _GEOM_CAM[0]
    beta = cu(SG.synth_renderer_sd(2)["renderer.sigmoid_beta"].reshape(1).float())
    sdf = cu(weights.det_normal("nrmgeom.sdf", (B, R, N), 1.0, N)) * beta
    grad = cu(weights.det_normal("nrmgeom.grad", (B, R, N, 3), 1.0, N))
    u = cu(weights.det_unit_uniform("nrmgeom.u", (B, R), N)) if perturb else None
    common = dict(sdf=sdf, grad=grad, sigmoid_beta=beta, B=B, n_samples=N)
    cam = hip.nerf_normals(img_size=S, cam_poses=extr.float().contiguous(), focals=focal.float().reshape(B).contiguous(),
                           near_=near.float().reshape(B).contiguous(), far_=far.float().reshape(B).contiguous(), perturb_u=u,
                           **common)
    rays_d = hip.rays_in_world(extr, focal, S)[1].reshape(B, R, 3).contiguous()
    z = hip.z_vals(near, far, B, R, N, u)
    exp = hip.nerf_normals(x_rays_d=rays_d, x_z_vals=z, n_rays=R, **common)
    torch.cuda.synchronize()
    for k in ("normal_raw", "normal"):
        d = float((cam[k] - exp[k]).abs().max())
        print(f"N={N} perturb={perturb} {k}: max |camera - explicit| {d:.3e}, max |{k}| {float(cam[k].abs().max()):.3e}")
        assert torch.isfinite(cam[k]).all() and float(cam[k].abs().max()) > 0
        assert torch.equal(cam[k], exp[k]), f"{k}: camera and explicit forms differ by {d:.3e}"


# ------------------------------------------------------------------------------------------------ 4. shading in isolation
def phong64(n_raw, xyz, eye, light, ka, kd, ks, s):
    """n_raw (B,R,3), xyz (B,R,3), eye / light (B,3), all fp64 -> shade (B,R)."""
    unit = lambda v: v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)      # noqa: E731
    n = unit(n_raw)
    l, v = unit(light[:, None] - xyz), unit(eye[:, None] - xyz)
    c = (n * l).sum(-1)
    spec = ((v * (2 * c[..., None] * n - l)).sum(-1)).clamp_min(0) ** s
    return ka + kd * c.clamp_min(0) + ks * (c > 0) * spec, c


@pytest.mark.parametrize("phong", [{}, dict(ka=0.2, kd=0.5, ks=0.4, shininess=10.0)])
def test_shading_in_isolation(phong):
    """N = 1: alpha = 1 - exp(-sigma 1e10 |d|) = 1 and T = 1, so normal_raw is the gradient handed in, exactly."""
    B, R = 2, 1000
    g = torch.Generator().manual_seed(21)
    rnd = lambda *s: torch.randn(*s, generator=g)        # noqa: E731
    n_raw = F.normalize(rnd(B, R, 3), dim=-1) * (0.5 + 2.5 * torch.rand(B, R, 1, generator=g))
    xyz = F.normalize(rnd(B, R, 3), dim=-1) * 0.15 * torch.rand(B, R, 1, generator=g)
    eye = F.normalize(rnd(B, 3), dim=-1)
    light = 5 * F.normalize(rnd(B, 3), dim=-1)
    # rays with n . l exactly 0: view 0 lit from (0, 0, 5), the point at the origin (l = (0, 0, 1) exactly), the normal in the x-y plane
    light[0] = torch.tensor([0.0, 0.0, 5.0])
    xyz[0, :8] = 0
    n_raw[0, :8, 2] = 0
    inp = SG.explicit_inputs(B, R, 1, 2, tag="nrmshade")
    xyz_planar = xyz.transpose(1, 2).contiguous()
    out = run_explicit(torch.zeros(B, R, 1), n_raw.view(B, R, 1, 3), torch.tensor([0.1]), inp["z"], inp["rays_d"],
                       shade=dict(xyz=xyz_planar, eye=eye, light=light), **phong)
    assert torch.equal(out["normal_raw"].transpose(1, 2), n_raw)
    ph = dict(hip.PHONG_DEFAULTS, **phong)
    want, c = phong64(n_raw.double(), xyz.double(), eye.double(), light.double(), ph["ka"], ph["kd"], ph["ks"], ph["shininess"])
    assert bool((c[0, :8] == 0).all()) and int((c < 0).sum()) > R // 4 and int((c > 0).sum()) > R // 4
    err = float((out["shade"].double() - want).abs().max())
    bound = (ph["kd"] + ph["shininess"] * ph["ks"]) * 16 * ULP
    print(f"shade {ph}: |kernel - fp64| {err:.3e}, bound {bound:.3e}; range {float(want.min()):.3f} .. {float(want.max()):.3f}")
    assert err <= bound
    assert bool((out["shade"][0, :8] == torch.tensor(ph["ka"], dtype=torch.float32)).all())
    u8 = torch.floor(255 * out["shade"].clamp(0, 1) + 0.5).to(torch.uint8)
    for ch in range(3):
        assert torch.equal(out["shade_u8"][:, ch], u8), ch
    assert int(u8.max()) > int(u8.min())


# ------------------------------------------------------------------------------------------------ 5. Generator
def generator_inputs(G, S, B=1):
    g = torch.Generator().manual_seed(11)
    zs = [cu(torch.randn(B, G.z_dim, generator=g)), cu(torch.randn(B, G.z_dim, generator=g))]
    cam = O.camera_params(torch.tensor([[0.25, -0.05]]).expand(B, 2).contiguous(), S, 6, 0.12)
    return zs, cam


def snapshot(ret):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ret.items()}


@pytest.mark.parametrize("inject", [None, 3])
def test_generator_return_normal(inject):
    G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=4)
    S, N = 32, 12
    zs, cam = generator_inputs(G, S)
    kw = dict(zs=zs, cam_poses=cu(cam[0]), focals=cu(cam[1]), img_size=S, near=cu(cam[2]), far=cu(cam[3]), inject_index=inject,
              return_sdf=True, return_xyz=True, nerf_cfg=dict(N_samples=N, perturb=True, static_viewdirs=False))
    planned = inject is None and G._forward_plan(1, S, N, False) is not None
    assert planned == (inject is None), "the plain call must plan, style mixing must not"
    if not planned:
        kw["perturb_u"] = cu(weights.det_unit_uniform("nrmgen.u", (1, S, S, 1), S))
    torch.manual_seed(5)
    ref = snapshot(G(**kw))
    state_ref = torch.cuda.get_rng_state()
    assert "normal" not in ref and "shade" not in ref
    torch.manual_seed(5)
    ret = snapshot(G(**kw, return_normal=True))
    assert torch.equal(torch.cuda.get_rng_state(), state_ref)
    nrm = ret["normal"]
    assert nrm.shape == (1, 3, S, S) and nrm.dtype == torch.float32 and nrm.is_contiguous() and torch.isfinite(nrm).all()
    assert float((nrm.norm(dim=1) - 1).abs().max()) <= 4 * ULP
    assert set(ret) == set(ref) | {"normal"}
    for k, v in ref.items():
        assert (v is None and ret[k] is None) or torch.equal(v, ret[k]), k
    # one gradient pass serves both
    torch.manual_seed(5)
    both = G(**kw, return_normal=True, eikonal_reg=True)
    assert torch.equal(torch.cuda.get_rng_state(), state_ref)
    assert torch.equal(both["normal"], nrm) and both["eikonal_term"].shape == (1, S * S, N, 3)
    torch.manual_seed(5)
    assert torch.equal(G(**kw, eikonal_reg=True)["eikonal_term"], both["eikonal_term"])
    geom = (kw["cam_poses"], kw["focals"], kw["near"], kw["far"])
    if planned:
        plan = G._forward_plan(1, S, N, False)
        assert plan.last_perturb_u is not None
        direct = G.renderer.normal_map(*geom, None, S, N, perturb_u=plan.last_perturb_u, film=plan.film)
    else:
        style_r, _ = G.mapping_networks(zs=zs, truncation=1, inject_index=inject)
        direct = G.renderer.normal_map(*geom, style_r, S, N, perturb_u=kw["perturb_u"])
    assert torch.equal(direct["normal"], nrm)


def test_generator_refusals():
    G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=4)
    S, N = 16, 6
    zs, cam = generator_inputs(G, S)
    kw = dict(cam_poses=cu(cam[0]), focals=cu(cam[1]), img_size=S, near=cu(cam[2]), far=cu(cam[3]),
              nerf_cfg=dict(N_samples=N, perturb=False, static_viewdirs=False))
    s_r, s_d = G.mapping_networks(zs=zs, truncation=1, inject_index=None)
    s_r = s_r.detach().clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="double backward"):
        G(zs=zs, style_render=s_r, style_decoder=s_d.detach(), return_normal=True, **kw)
    G128 = pkg.build_generator(configs.tiny_G_cfg(128, 2, 1), DEV, seed=1)
    z128 = [cu(torch.randn(1, G128.z_dim)), cu(torch.randn(1, G128.z_dim))]
    with pytest.raises(NotImplementedError, match="hidden_dim = 256"):
        G128(zs=z128, return_normal=True, **kw)
    ren128, _ = renderer(2, hidden=128)
    with pytest.raises(NotImplementedError, match="hidden_dim = 256"):
        ren128.normal_map(kw["cam_poses"], kw["focals"], kw["near"], kw["far"], cu(torch.zeros(1, 3, 128)), S, N)
    rend, _ = renderer(2, with_sdf=False)
    with pytest.raises(NotImplementedError, match="with_sdf"):
        rend.normal_map(kw["cam_poses"], kw["focals"], kw["near"], kw["far"], cu(torch.zeros(1, 3, SG.H)), S, N)
    cfg = configs.ffhq_G_cfg(256, 2)
    cfg["renderer_cfg"]["with_sdf"] = False
    Gd = pkg.build_generator(cfg, DEV, seed=4)
    ret = Gd(zs=zs, return_normal=True, **kw)
    assert ret["normal"] is None and ret["rgb"].shape[0] == 1
    with pytest.raises(ValueError, match="return_normal"):
        G(zs=zs, shade=dict(light=cu(torch.zeros(1, 3))), **kw)


# ------------------------------------------------------------------------------------------------ 6. sequence
def test_sample_multi_view_gathers_normal_and_shaded():
    """FFHQ 256^2 weights (hidden 256, the width the gradient kernel is built for) at 32^2 rays x 12 samples, 3 frames."""
    from cips_3dplusplus_amd.camera import cameras_from_trajectory
    from cips_3dplusplus_amd.multiview import sample_multi_view
    G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=3)
    S, N, n = 32, 12, 3
    g = torch.Generator(device=DEV).manual_seed(11)
    zs = [torch.randn(1, 256, device=DEV, generator=g), torch.randn(1, 256, device=DEV, generator=g)]
    nb = [torch.randn(b.shape, device=DEV, generator=g) for b in G.create_noise_bufs(S, DEV)]
    G.style_render_mean = 0.1 * torch.randn(1, 256, device=DEV, generator=g)
    G.style_decoder_mean = 0.1 * torch.randn(1, 512, device=DEV, generator=g)
    cam_cfg = {"img_size": S, "fov_ang": 12, "dist_radius": 0.12}
    kw = dict(view_mode="yaw", N_frames=n, truncation_ratio=0.7, N_samples=N, noise_bufs=nb)
    base = sample_multi_view(G, cam_cfg, {"static_viewdirs": False}, zs, **kw)
    assert set(base) == {"rgb", "thumb_rgb", "xyz", "trajectory"}
    out = sample_multi_view(G, cam_cfg, {"static_viewdirs": False}, zs, gather=("rgb", "xyz", "normal", "shaded"), **kw)
    torch.cuda.synchronize()
    assert set(out) == {"rgb", "xyz", "normal", "shaded", "trajectory"}
    R_img = base["rgb"].shape[-1]
    assert out["rgb"].shape == (n, 3, R_img, R_img) and out["rgb"].dtype == torch.uint8
    assert out["xyz"].shape == out["normal"].shape == (n, 3, S, S) and out["normal"].dtype == torch.float32
    assert out["shaded"].shape == (n, 3, S, S) and out["shaded"].dtype == torch.uint8 and out["shaded"].is_contiguous()
    assert torch.equal(out["rgb"], base["rgb"]) and torch.equal(out["xyz"], base["xyz"])
    assert torch.equal(out["trajectory"], base["trajectory"])
    # frame j against normal_map for that frame's camera and light, through the FiLM table of a forward of the same latent
    traj = out["trajectory"]
    ext, foc, near, far = cameras_from_trajectory(traj, S, torch.device(DEV), 0.12)
    ncfg = dict(N_samples=N, perturb=False, static_viewdirs=False)
    G(zs=zs, cam_poses=ext[:1].contiguous(), focals=foc[:1].contiguous(), img_size=S, near=near[:1].contiguous(),
      far=far[:1].contiguous(), noise_bufs=nb, truncation=0.7, nerf_cfg=ncfg)
    plan = G._forward_plan(1, S, N, False)
    assert plan is not None
    azim = traj[:, 0].float()
    lights = torch.stack([5 * torch.sin(azim), torch.zeros_like(azim), 5 * torch.cos(azim)], 1)       # (5 sin azim, 0, 5 cos azim)
    for j in range(n):
        cams = [t[j:j + 1].contiguous() for t in (ext, foc, near, far)]
        ref = G.renderer.normal_map(*cams, None, S, N, film=plan.film, shade=dict(light=cu(lights[j:j + 1]), xyz=out["xyz"][j:j + 1]))
        assert torch.equal(ref["normal"], out["normal"][j:j + 1]), j
        assert torch.equal(ref["shade_u8"], out["shaded"][j:j + 1]), j
        assert bool((out["shaded"][j, 0] == out["shaded"][j, 1]).all()) and bool((out["shaded"][j, 0] == out["shaded"][j, 2]).all())
    assert not torch.equal(out["shaded"][0], out["shaded"][1])


# ------------------------------------------------------------------------------------------------ 7. vertex normals
def normals64(A, verts_index, level, affine):
    """The header's contract in fp64 numpy.  The vertex -> edge mapping comes from the index-space vertex positions: the one
    non-integer coordinate names the axis, the floor the edge's lower end.  -> (normals [V,3], |g| [V])"""
    A = A.astype(np.float64)
    Gi, Gj, Gk = np.gradient(A)                          # d / d row (y), d / d column (x), d / d depth (z); edge_order = 1
    frac = np.abs(verts_index - np.round(verts_index))
    axis = frac.argmax(1)
    assert ((frac > 1e-4).sum(1) == 1).all(), "a vertex within 1e-4 of a lattice point: the test cannot name its edge"
    lo = np.floor(verts_index + 1e-6 * (np.arange(3)[None] != axis[:, None])).astype(np.int64)        # (x, y, z) of the lower end
    hi = lo.copy()
    hi[np.arange(len(hi)), axis] += 1
    at = lambda T, p: T[p[:, 1], p[:, 0], p[:, 2]]       # noqa: E731  A[i = y, j = x, k = z]
    va, vb = at(A, lo), at(A, hi)
    assert ((va < level) != (vb < level)).all()
    t = ((level - va) / (vb - va))[:, None]
    grad_at = lambda p: np.stack([at(Gj, p), at(Gi, p), at(Gk, p)], 1)       # noqa: E731
    g = (1 - t) * grad_at(lo) + t * grad_at(hi)
    scale = np.ones(3) if affine is None else np.array([a[0] for a in affine], np.float64)
    nrm = g / scale
    return nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-12), np.linalg.norm(g, axis=1)


def normals_padded(vol, level, affine, n_verts):
    """cips3d_marching_cubes_normals straight after the count call (no emit in between), into a sentinel-padded buffer."""
    import ctypes as C
    ws, totals = hip.marching_cubes_count(vol, level)
    assert int(totals[0]) == n_verts
    buf, view = padded((n_verts, 3))
    aff = None if affine is None else (C.c_float * 6)(*[float(v) for pair in affine for v in pair])
    h, w, d = vol.shape
    _lib.check(_lib.load().cips3d_marching_cubes_normals(vol.data_ptr(), h, w, d, float(level), aff, ws.data_ptr(), view.data_ptr(),
                                                         n_verts, _lib.stream_ptr()), "cips3d_marching_cubes_normals")
    torch.cuda.synchronize()
    check_padded(buf, "vertex normals")
    return view.clone()


def check_vertex_normals(name, A, affine):
    vol = cu(torch.from_numpy(A))
    v_idx, f_idx = hip.marching_cubes(vol, 0.0)
    verts, faces, nrm = hip.marching_cubes(vol, 0.0, affine=affine, normals=True)
    plain = hip.marching_cubes(vol, 0.0, affine=affine)
    assert len(plain) == 2 and torch.equal(plain[0], verts) and torch.equal(plain[1], faces) and torch.equal(faces, f_idx)
    assert nrm.shape == verts.shape and nrm.dtype == torch.float32
    again = hip.marching_cubes(vol, 0.0, affine=affine, normals=True)[2]
    assert torch.equal(again, nrm) and torch.equal(normals_padded(vol, 0.0, affine, verts.shape[0]), nrm)
    want, gnorm = normals64(A, v_idx.cpu().numpy().astype(np.float64), 0.0, affine)
    keep = gnorm >= 1e-3
    assert keep.mean() >= 0.99
    err = np.abs(nrm.cpu().numpy().astype(np.float64) - want)[keep]
    bound = (8 * ULP * np.abs(A).max() / gnorm[keep] + 4 * ULP)[:, None]
    print(f"{name}: V {verts.shape[0]} F {faces.shape[0]}, max |err| {err.max():.3e}, largest err / bound {(err / bound).max():.3f}, "
          f"smallest |g| {gnorm.min():.3f}, skipped {int((~keep).sum())}")
    assert (err <= bound).all()
    return verts, faces, nrm


def seeded_volume():
    return torch.randn(5, 7, 6, generator=torch.Generator().manual_seed(3)).numpy()


def test_vertex_normals_one_inside_corner():
    A = np.ones((2, 2, 2), np.float32)
    A[0, 0, 0] = -1
    verts, faces, nrm = check_vertex_normals("2x2x2", A, None)
    assert verts.shape[0] == 3 and faces.shape[0] == 1
    # every lattice gradient of this volume is one-sided; at the three vertices (t = 1/2) the normal leaves the inside corner
    assert bool((nrm > 0).all())


@pytest.mark.parametrize("with_affine", [False, True])
def test_vertex_normals_seeded_volume(with_affine):
    A = seeded_volume()
    check_vertex_normals("5x7x6" + (" affine" if with_affine else ""), A, mesh.reference_affine(*A.shape) if with_affine else None)


def test_vertex_normals_sphere_and_no_crossing():
    n, radius = 24, 7.3
    centre = np.array([11.2, 12.6, 10.9])                                        # (x, y, z) = (column, row, depth)
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    A = (np.sqrt((j - centre[0]) ** 2 + (i - centre[1]) ** 2 + (k - centre[2]) ** 2) - radius).astype(np.float32)
    vol = cu(torch.from_numpy(A))[None]
    plain = mesh.extract_mesh_with_marching_cubes(vol, 0.0)
    verts, faces, nrm = mesh.extract_mesh_with_marching_cubes(vol, 0.0, normals=True)
    assert len(plain) == 2 and torch.equal(plain[0], verts) and torch.equal(plain[1], faces) and verts.shape[0] > 500
    assert torch.equal(mesh.extract_mesh_with_marching_cubes(vol, 0.0, normals=True)[2], nrm)
    v, f, nr = verts.cpu().numpy().astype(np.float64), faces.cpu().numpy(), nrm.cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(nr, axis=1) - 1).max() <= 4 * ULP
    assert ((gen_images.vertex_normals(v, f) * nr).sum(1) > 0).all()              # the side the winding faces
    aff = np.array(mesh.reference_affine(n, n, n))
    radial = v - (centre * aff[:, 0] + aff[:, 1])                                 # outward, in the output frame
    cosine = (radial * nr).sum(1) / np.linalg.norm(radial, axis=1)
    print(f"sphere: V {len(v)} F {len(f)}, smallest cosine between normal and radius {cosine.min():.4f}")
    assert (cosine > 0).all()
    # no crossing: None, as without normals
    assert mesh.extract_mesh_with_marching_cubes(cu(torch.ones(1, 4, 5, 6)), 0.0, normals=True) is None
    assert mesh.extract_mesh_with_marching_cubes(cu(torch.ones(1, 4, 5, 6)), 0.0) is None


# ------------------------------------------------------------------------------------------------ 8. tools
def last_json(stdout):
    return json.loads([ln for ln in stdout.splitlines() if ln.startswith("{")][-1])


def test_normals_tool_prints_json_and_writes_pngs(tmp_path):
    from PIL import Image
    prefix = str(tmp_path / "t_")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "normals.py"), "--depth", "2", "--img-size", "32", "--samples", "8",
                        "--out-prefix", prefix, "--time", "--reps", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1].startswith("{")
    d = last_json(r.stdout)
    assert d["points"] == 8192 and d["sdf_grad_ms"] > 0 and d["normals_ms"] > 0 and d["copy_ms"] > 0
    for name in ("normal.png", "shaded.png"):
        assert np.array(Image.open(prefix + name)).shape == (32, 32, 3), name


def test_extract_mesh_tool_writes_normals(tmp_path):
    path = str(tmp_path / "m.obj")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--resolution", "32", "--normals", "--out", path],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(path).read().splitlines()
    n_v, n_vn = sum(ln.startswith("v ") for ln in lines), sum(ln.startswith("vn ") for ln in lines)
    assert n_v == n_vn > 0 and all("//" in ln for ln in lines if ln.startswith("f "))
