"""The eikonal / minimal-surface loss kernel (csrc/nerf_eikonal.hip), its autograd node, the renderer's `eikonal_loss` and the
inversion loop's regulariser.

Yardstick: the double backward of the recipe's trunk (_eikonal_loss_cases.oracle) in fp64.  THE RULE for gradients, the project's
own (test_gpu_sdf_grad.py), per case, with the fp32 oracle's error against fp64 measured in the test:
    kernel RMS error <= 2 x the fp32 RMS error,     kernel max error <= 4 x the fp32 max error.
The two loss VALUES are scalars: each within 4 x max(the fp32 oracle's relative error, _eikonal_loss_cases.VALUE_FLOOR).
"""
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import autograd as AG, configs, hip, weights
from cips_3dplusplus_amd.optim import HipAdam
from cips_3dplusplus_amd.projector import FlipProjector, surrogate_loss
from cips_3dplusplus_amd.renderer import VolumeFeatureRenderer

import _eikonal_loss_cases as EC
import _sdf_grad_cases as SG

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.5


def cu(t):
    return t.to(DEV).contiguous()


_REN, _ORACLE = {}, {}


def renderer(D, zero_sigma=False):
    key = (D, zero_sigma)
    if key not in _REN:
        ren = VolumeFeatureRenderer(N_layers_renderer=D, input_dim=3, hidden_dim=SG.H, style_dim=SG.H, view_dim=3, with_sdf=True,
                                    output_features=True).eval().requires_grad_(False)
        sd = SG.synth_renderer_sd(D)
        if zero_sigma:
            sd = dict(sd)
            sd["renderer.network.sigma_linear.weight"] = torch.zeros_like(sd["renderer.network.sigma_linear.weight"])
        ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()}, strict=True)
        _REN[key] = (ren.to(DEV), sd)
    return _REN[key]


def oracles(key, sd, inp, D, inp32=None, **lam):
    """(fp64, fp32) oracle of a case, computed once and shared by the tests that need it.  inp32: the fp32 side's own inputs (camera
    form: the oracle's rays and points generated in fp32, as in test_gpu_sdf_grad.py -- the kernel generates them in fp32 too)."""
    if key not in _ORACLE:
        _ORACLE[key] = (EC.oracle(sd, inp, D, torch.float64, **lam), EC.oracle(sd, inp if inp32 is None else inp32, D, torch.float32, **lam))
    return _ORACLE[key]


def check_rule(name, got, g64, g32):
    n_max, n_rms = SG.err_stats(g32, g64)
    k_max, k_rms = SG.err_stats(got.cpu(), g64)
    print(f"{name}: kernel max {k_max:.3e} rms {k_rms:.3e} | fp32 oracle max {n_max:.3e} rms {n_rms:.3e} | ratios max "
          f"{k_max / max(n_max, 1e-30):.2f} rms {k_rms / max(n_rms, 1e-30):.2f} | largest component {float(g64.abs().max()):.3g}")
    assert torch.isfinite(got).all()
    assert k_rms <= 2 * n_rms, f"{name}: RMS error {k_rms:.3e} > 2 x {n_rms:.3e}"
    assert k_max <= 4 * n_max, f"{name}: max error {k_max:.3e} > 4 x {n_max:.3e}"


def check_values(name, loss, o64, o32):
    for i, k in enumerate(("eik", "ms")):
        got, e32 = float(loss[i]), EC.rel(o32[k], o64[k])
        e = EC.rel(got, o64[k])
        print(f"{name}: {k} kernel {got:.9g} fp64 {o64[k]:.9g} | rel err {e:.2e} | fp32 oracle {e32:.2e} | floor {EC.VALUE_FLOOR:.1e}")
        assert e <= 4 * max(e32, EC.VALUE_FLOOR), f"{name}: {k} relative error {e:.3e}"


def film_of(ren, styles, B):
    styles_buf, film, tab = ren._film_table(B, torch.device(DEV))
    styles_buf.copy_(cu(styles))
    tab.run(B)
    return film


def kernel_explicit(ren, inp, lam_e=1.0, lam_m=1.0, values_only=False, pad=64):
    """(loss [2] fp64 on the host, dfilm [B, D+1, 2, H] | None) of the kernel on explicit points; dfilm is written into a
    sentinel-padded buffer that is checked."""
    B, R, N = inp["z"].shape
    D, H = ren.N_layers_renderer, ren.hidden_dim
    film = film_of(ren, inp["styles"], B)
    n = B * (D + 1) * 2 * H
    buf = torch.full((pad + n + pad,), SENTINEL, device=DEV)
    dfilm = buf[pad:pad + n].view(B, D + 1, 2, H)
    call = ren._eikonal_args(cu(inp["near"]), cu(inp["far"]), B, N, x_pts=cu(inp["pts"].reshape(B, R, N, 3)), n_rays=R, beta=EC.BETA)
    loss, d = hip.nerf_eikonal_loss(**call(film), lambda_eikonal=lam_e, lambda_minimal_surface=lam_m, values_only=values_only,
                                    dfilm_out=None if values_only else dfilm)
    torch.cuda.synchronize()
    assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all()), "store outside dfilm"
    if values_only:
        assert d is None and bool((buf == SENTINEL).all()), "the values-only call wrote dfilm"
        return loss.cpu(), None
    assert not bool((dfilm == SENTINEL).any()), "a dfilm element was not written"
    return loss.cpu(), dfilm.clone()


@pytest.mark.parametrize("D,B,R,N", EC.KERNEL_CASES)
def test_explicit_form_against_fp64_oracle(D, B, R, N):
    """Values and dfilm under the rules of the module docstring; the view layer's row exactly zero; two runs bit-identical; the
    values-only call returns the same two values bit for bit and writes no dfilm.  (2, 37, 5): ragged in the 4-point tile and the
    32-point step; (1, 1, 1): one point; (3, 16, 24): three views with distinct styles and near / far; (1, 4099, 3): more steps
    than workgroups; D = 16: FiLM rows read from memory."""
    ren, sd = renderer(D)
    inp = EC.case_inputs(D, B, R, N)
    o64, o32 = oracles(("x", D, B, R, N), sd, inp, D)
    loss, dfilm = kernel_explicit(ren, inp)
    name = f"explicit D={D} B={B} R={R} N={N}"
    check_values(name, loss, o64, o32)
    check_rule(name, dfilm, o64["dfilm"], o32["dfilm"])
    assert not bool(dfilm[:, D].any()), "the view layer's row of dfilm must be exactly zero"
    loss2, dfilm2 = kernel_explicit(ren, inp)
    assert torch.equal(loss, loss2) and torch.equal(dfilm, dfilm2), "two runs differ"
    loss3, _ = kernel_explicit(ren, inp, values_only=True)
    assert torch.equal(loss, loss3), "the values-only call returns other values"


def test_camera_form_against_fp64_oracle():
    c = EC.CAMERA_CASE
    D, B, S, N = c["D"], c["B"], c["S"], c["N"]
    ren, sd = renderer(D)
    cam, u, styles, inp = EC.camera_case_inputs()
    o64, o32 = oracles(("cam",), sd, inp, D, inp32=EC.camera_case_inputs(torch.float32)[3])
    film = film_of(ren, styles, B)
    call = ren._eikonal_args(cu(cam[2]), cu(cam[3]), B, N, img_size=S, cam_poses=cu(cam[0]), focals=cu(cam[1]).reshape(B),
                             perturb_u=cu(u), beta=EC.BETA)
    loss, dfilm = hip.nerf_eikonal_loss(**call(film))
    check_values("camera", loss.cpu(), o64, o32)
    check_rule("camera", dfilm, o64["dfilm"], o32["dfilm"])
    assert not bool(dfilm[:, D].any())
    loss2, dfilm2 = hip.nerf_eikonal_loss(**call(film))
    assert torch.equal(loss, loss2) and torch.equal(dfilm, dfilm2)


@pytest.mark.parametrize("D", [2, 6])
def test_zero_sigma_head(D):
    """sigma_linear.weight = 0: g = 0 everywhere, so the eikonal value is exactly 1 and its seed the |g| = 0 convention (no
    gradient); sdf = b_sigma, so the minimal-surface value is exp(-beta |b_sigma|).  Its bound: the fp32 product beta |b_sigma| errs
    by 2^-24 relative, i.e. beta |b_sigma| 2^-24 in the exponent, which is the result's relative error; expf adds 2 ulp and the
    mean of equal terms in fp64 nothing: (beta |b_sigma| + 4) 2^-24."""
    ren, sd = renderer(D, zero_sigma=True)
    inp = EC.case_inputs(D, 2, 37, 5)
    loss, dfilm = kernel_explicit(ren, inp)
    assert float(loss[0]) == 1.0
    arg = EC.BETA * abs(float(sd["renderer.network.sigma_linear.bias"][0]))
    want = float(torch.exp(torch.tensor(-arg, dtype=torch.float64)))
    print(f"zero head D={D}: ms {float(loss[1]):.9g} want {want:.9g} (exponent {arg:.3f})")
    assert abs(float(loss[1]) - want) <= (arg + 4) * 2.0 ** -24 * want
    assert bool(torch.isfinite(dfilm).all())
    loss0, dfilm0 = kernel_explicit(ren, inp, lam_e=1.0, lam_m=0.0)
    assert torch.equal(loss0, loss) and not bool(dfilm0.any()), "lambda_m = 0 with a zero head: dfilm must be exactly zero"


def node_inputs():
    c = EC.CAMERA_CASE
    cam, u, styles, _ = EC.camera_case_inputs()
    one = styles[:1].contiguous()
    inp, inp32 = (SG.camera_inputs(cam, c["S"], c["N"], u, False, dt, c["D"], one.expand(c["B"], -1, -1))
                  for dt in (torch.float64, torch.float32))
    return c, cam, u, one, inp, inp32


def test_renderer_eikonal_loss_node(monkeypatch):
    """renderer.eikonal_loss with a [1, D+1, 256] leaf broadcast to B = 2: .backward() of 0.3 eik + 0.7 ms against the oracle's
    d / d styles (summed over the views) under the rule, and against its torch partner (CIPS3D_FUSED_EIKONAL=0) under the rule."""
    c, cam, u, one, inp, inp32 = node_inputs()
    D, S, N = c["D"], c["S"], c["N"]
    ren, sd = renderer(D)
    o64, o32 = oracles(("node",), sd, inp, D, inp32=inp32, lam_e=0.3, lam_m=0.7)
    g64, g32 = o64["dstyles"].sum(0, keepdim=True), o32["dstyles"].sum(0, keepdim=True)
    args = (cu(cam[0]), cu(cam[1]), cu(cam[2]), cu(cam[3]))

    def run():
        leaf = cu(one).requires_grad_(True)
        eik, ms = ren.eikonal_loss(*args, leaf, S, N, perturb_u=cu(u))
        assert eik.dim() == 0 and ms.dim() == 0 and eik.dtype == torch.float32 and ms.dtype == torch.float32
        (0.3 * eik + 0.7 * ms).backward()
        return eik.detach(), ms.detach(), leaf.grad

    eik, ms, g = run()
    check_values("node", torch.stack([eik, ms]).cpu().double(), o64, o32)
    check_rule("node d/dstyles", g, g64, g32)
    # the weighted form: one call, the same gradient up to the order of the two terms' sum
    leaf = cu(one).requires_grad_(True)
    tot, e1, m1 = ren.eikonal_loss(*args, leaf, S, N, perturb_u=cu(u), weights=(0.3, 0.7))
    tot.backward()
    assert torch.equal(e1, eik) and torch.equal(m1, ms) and not e1.requires_grad
    check_rule("node (weighted) d/dstyles", leaf.grad, g64, g32)
    monkeypatch.setenv("CIPS3D_FUSED_EIKONAL", "0")
    eik_t, ms_t, g_t = run()
    check_rule("torch partner d/dstyles", g_t, g64, g32)
    n_max, n_rms = SG.err_stats(g32, g64)
    d_max, d_rms = SG.err_stats(g.cpu(), g_t.cpu().double())
    print(f"fused - partner: max {d_max:.3e} rms {d_rms:.3e} | fp32 oracle max {n_max:.3e} rms {n_rms:.3e}")
    assert d_rms <= 2 * n_rms and d_max <= 4 * n_max
    assert abs(float(eik) - float(eik_t)) <= 4 * EC.VALUE_FLOOR * abs(float(eik_t))


@pytest.mark.parametrize("D", [2, 6])
def test_regulariser_lowers_the_eikonal_term(D):
    """30 HipAdam steps at lr 0.01 on the styles, eikonal term alone, on explicit_inputs(1, 64, 6, D)'s geometry: the final value
    is below 0.6 x the initial one (the fp32 oracle with torch's Adam on these inputs reaches 0.42 x at D = 2, 0.17 x at D = 6)."""
    ren, _ = renderer(D)
    inp = SG.explicit_inputs(1, 64, 6, D)
    styles = cu(inp["styles"]).requires_grad_(True)
    opt = HipAdam([styles], lr=0.01)
    call = ren._eikonal_args(cu(inp["near"]), cu(inp["far"]), 1, 6, x_pts=cu(inp["pts"]), n_rays=64, beta=EC.BETA)
    hist = []
    for _ in range(31):
        opt.zero_grad(set_to_none=True)
        tot, eik, _ = AG.EikonalLossFn.apply(AG.film_table(ren, styles), call, (1.0, 0.0))
        hist.append(eik)
        tot.backward()
        opt.step()
    hist = torch.stack(hist).cpu()
    print(f"D={D}: eikonal {float(hist[0]):.5g} -> {float(hist[-1]):.5g} (x {float(hist[-1] / hist[0]):.3f})")
    assert bool(torch.isfinite(hist).all()) and float(hist[-1]) < 0.6 * float(hist[0])


def test_project_wplus_with_the_regulariser(monkeypatch):
    """The loop on the tiny generator of the inversion tests at hidden 256, 3 + 2 steps.

    Both weights 0: the node is never launched, the dict has the same keys, and the call is compared with one that does not pass
    the new arguments.  Bit-identity is asserted for what two identical calls of the loop reproduce: the loss history (what
    test_gpu_ssim_loss.py compares for its weight-0 case), the renderer's state dict and the noise buffers (not optimised here).
    The tensors Adam moves (azim, elev, w_render_opt, w_decoder_opt, the decoder's state dict) are NOT reproducible run to run in
    this project, with or without this feature: two plain calls of the parent's loop differ in them at hidden 32 and 256, on the
    tiny and the FFHQ configuration alike (measured: d w_render, d w_decoder and 7-52 decoder gradients of ONE forward + backward
    differ between two runs; the backward's kernels sum with floating-point atomics).  Adam turns a gradient into a step of size
    lr whatever its magnitude, so a noise-level gradient whose sign flips moves an element by 2 lr per step: no bound on those
    tensors would be a check, so none is asserted; the largest differences of (zero, plain) and of (plain, plain) are printed
    (measured on an MI355X: 4.8e-07 and 5.4e-07).
    What is asserted for the weight-0 call is that the node is never launched.

    eikonal_weight = 0.1 on 8^2 rays, every 2nd step: w_render differs, everything returned is finite, and the node launches on
    steps 0, 2 and 4 only."""
    G = pkg.build_generator(configs.tiny_G_cfg(256, 2, 1), DEV, seed=2)
    g = torch.Generator(device=DEV).manual_seed(0)
    t_rgb = torch.randn(2, 3, 32, 32, device=DEV, generator=g).clamp(-1, 1)
    t_thumb = torch.randn(2, 3, 8, 8, device=DEV, generator=g).clamp(-1, 1)
    proj = FlipProjector(G, DEV)
    cam_cfg = {"img_size": 8, "fov_ang": 6, "dist_radius": 0.12}
    ncfg = {"N_samples": 6, "perturb": False, "static_viewdirs": True}

    def run(**kw):
        torch.manual_seed(3)                # (the loop draws its mean latents from torch's generator)
        return proj.project_wplus(cam_cfg, ncfg, surrogate_loss(t_rgb, t_thumb), N_steps_pose=3, N_steps_app=2, w_avg_samples=64, **kw)

    def tensors(out):
        flat = {k: v for k, v in out.items() if torch.is_tensor(v)}
        flat.update({f"noise.{i}": b for i, b in enumerate(out["noise_bufs"])})
        for name in ("render_state_dict", "decoder_state_dict"):
            flat.update({f"{name}.{k}": v for k, v in out[name].items()})
        return flat

    calls, step = [], [0]
    real = hip.nerf_eikonal_loss
    monkeypatch.setattr(hip, "nerf_eikonal_loss", lambda **kw: (calls.append(step[0]), real(**kw))[1])
    base, base2 = run(), run()
    zero = run(eikonal_weight=0.0, minimal_surface_weight=0.0, eikonal_img_size=8, eikonal_every=2)
    assert calls == [] and set(base) == set(zero)
    tb, tb2, tz = tensors(base), tensors(base2), tensors(zero)
    assert set(tb) == set(tz) and len(tb) > 10
    moved = lambda k: k in ("azim", "elev", "w_render_opt", "w_decoder_opt") or k.startswith("decoder_state_dict.")
    worst_z = worst_p = 0.0
    for k in tb:
        if not moved(k):
            assert torch.equal(tb[k], tz[k]), k
            continue
        dz, dp = float((tz[k].double() - tb[k].double()).abs().max()), float((tb2[k].double() - tb[k].double()).abs().max())
        worst_z, worst_p = max(worst_z, dz), max(worst_p, dp)
    print(f"weights 0 against plain: largest difference {worst_z:.3e}; plain against plain: {worst_p:.3e}")

    def on_step(s, loss, azim, elev):
        assert bool(torch.isfinite(loss))
        step[0] = s + 1
    reg = run(eikonal_weight=0.1, eikonal_img_size=8, eikonal_every=2, on_step=on_step)
    assert calls == [0, 2, 4]
    for k, v in tensors(reg).items():
        assert bool(torch.isfinite(v).all()), k
    assert float((reg["w_render_opt"] - base["w_render_opt"]).abs().max()) > 10 * worst_p + 1e-6
