"""GPU parity: HIP kernels (through the C ABI) vs the CPU oracle and the committed golden vectors.

Tolerances: the path is IEEE fp32.  north_star asks <= 1e-3 max-abs on generator outputs; kernel-
level checks use the tighter bounds written next to each assert (a few fp32 ulps of the value range).
"""
import math

import numpy as np
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import _lib, configs, hip, op, weights
from cips_3dplusplus_amd.camera import Camera
from conftest import maxdiff
from oracle import path as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cu(t):
    return t.to(DEV).contiguous()


def _dec_mod():
    import cips_3dplusplus_amd.decoder as dec      # lazily exported sub-module: import it explicitly
    return dec


# ------------------------------------------------------------------------------------------ ops
def test_upfirdn2d_golden(golden):
    fx = golden("ops")
    for name in fx["ufd_names"]:
        up, down, p0, p1 = [int(v) for v in fx[f"ufd_{name}_cfg"]]
        y = op.upfirdn2d(cu(fx[f"ufd_{name}_x"]), cu(fx[f"ufd_{name}_k"]), up=up, down=down, pad=(p0, p1))
        assert y.shape == fx[f"ufd_{name}_y"].shape, name
        assert maxdiff(y.cpu(), fx[f"ufd_{name}_y"]) < 2e-6, name


@pytest.mark.parametrize("shape,k,up,down,pad", [
    ((2, 3, 64, 64), 4, 2, 1, (2, 1)), ((1, 8, 127, 127), 4, 1, 1, (2, 2)), ((1, 2, 100, 37), 4, 1, 2, (1, 1)),
    ((1, 1, 9, 200), 3, 1, 1, (1, 1)), ((1, 2, 40, 40), 12, 1, 1, (6, 5)), ((3, 1, 5, 5), 4, 2, 2, (3, 3)),
    ((1, 4, 16, 16), 4, 1, 1, (-1, -1)),
])
def test_upfirdn2d_vs_oracle(shape, k, up, down, pad):
    g = torch.Generator().manual_seed(sum(shape) + k)
    x = torch.randn(*shape, generator=g)
    kern = torch.rand(k, k, generator=g)
    y = op.upfirdn2d(cu(x), cu(kern), up=up, down=down, pad=pad)
    ref = O.upfirdn2d(x, kern, up, down, pad)
    assert y.shape == ref.shape
    assert maxdiff(y.cpu(), ref) < 1e-5 * max(1.0, k * k / 16)


@pytest.mark.parametrize("shape,up,down,pads", [
    ((2, 3, 64, 64), 2, 1, (2, 1, 2, 1)),        # Upsample of the RGB skip
    ((1, 5, 33, 70), 2, 1, (1, 2, 2, 1)),        # x and y phases differ
    ((1, 2, 31, 29), 2, 1, (3, 0, 0, 3)),
    ((1, 2, 40, 200), 2, 1, (-1, 4, 5, -2)),     # crops
    ((1, 8, 127, 127), 1, 1, (2, 2, 2, 2)),
    ((1, 3, 129, 261), 1, 1, (1, 1, 1, 1)),      # Blur after a transposed conv; output width not a multiple of 4
    ((2, 2, 50, 300), 1, 1, (0, 3, 3, 0)),
    ((1, 2, 100, 37), 1, 2, (1, 1, 1, 1)),
    ((1, 3, 64, 530), 1, 2, (2, 1, 0, 2)),
    ((1, 1, 4, 4), 2, 1, (2, 1, 2, 1)),
    ((2, 1, 1, 1), 2, 1, (2, 1, 2, 1)),          # one pixel in, 2 x 2 out
    ((1, 2, 3, 5), 1, 1, (2, 1, 1, 2)),          # output narrower than one 4-pixel block row
    ((1, 1, 7, 1), 1, 2, (2, 2, 2, 2)),          # a single input column
    ((3, 1, 130, 6), 2, 1, (2, 1, 2, 1)),        # more than one tile high, narrower than one tile
])
def test_upfirdn2d_fast_kernel_vs_oracle_and_bit_identical_to_the_tiled_kernel(shape, up, down, pads):
    """The compile-time polyphase kernel (csrc/upfirdn2d.hip: upfirdn2d_fast, the 4 x 4 FIR of the generator's Blur / Upsample)
    accumulates every output's taps in the tiled kernel's order: same bits.  The tiled kernel is reached through a child
    process with CIPS3D_UPFIRDN_FAST=0 (the knob is read once per process)."""
    import os
    import subprocess
    import sys
    import tempfile
    g = torch.Generator().manual_seed(sum(shape) + up * 7 + down)
    x = torch.randn(*shape, generator=g)
    kern = torch.rand(4, 4, generator=g)
    n, c, h, w = shape
    px0, px1, py0, py1 = pads
    y = op.upfirdn2d_raw(cu(x).reshape(n * c, h, w, 1), cu(kern), up, up, down, down, px0, px1, py0, py1)
    # oracle: symmetric API only -> pad x and y separately through two 1-sided calls is not available; use the package-own
    # torch evaluation of the definition (op._upfirdn2d_cpu, pinned by the reference fixtures in tests/test_host.py)
    ref = op._upfirdn2d_cpu(x, kern, (up, up), (down, down), (px0, px1, py0, py1))
    assert tuple(y.shape) == (n * c, ref.shape[2], ref.shape[3], 1)
    assert maxdiff(y.cpu().reshape(ref.shape), ref) < 1e-5
    with tempfile.TemporaryDirectory() as d:
        torch.save({"x": x, "k": kern}, os.path.join(d, "in.pt"))
        code = ("import torch, sys; from cips_3dplusplus_amd import op; t = torch.load(sys.argv[1] + '/in.pt');"
                f"y = op.upfirdn2d_raw(t['x'].cuda().reshape({n * c}, {h}, {w}, 1), t['k'].cuda(), {up}, {up}, {down}, {down}, {px0}, {px1}, {py0}, {py1});"
                "torch.save(y.cpu(), sys.argv[1] + '/out.pt')")
        env = dict(os.environ, CIPS3D_UPFIRDN_FAST="0")
        subprocess.run([sys.executable, "-c", code, d], check=True, env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        y_tiled = torch.load(os.path.join(d, "out.pt"))
    assert torch.equal(y.cpu(), y_tiled)


def test_upfirdn2d_generic_minor_dim():
    # the native binding layout [major, H, W, minor] with minor > 1 takes the generic kernel
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 9, 10, 2, generator=g)
    kern = torch.rand(4, 4, generator=g)
    y = op.upfirdn2d_raw(cu(x), cu(kern), 2, 2, 1, 1, 2, 1, 2, 1)
    ref = O.upfirdn2d(x.permute(0, 3, 1, 2).contiguous(), kern, 2, 1, (2, 1)).permute(0, 2, 3, 1)
    assert maxdiff(y.cpu(), ref) < 1e-5


def test_fused_leaky_relu_golden(golden):
    fx = golden("ops")
    for name in ("2d_g1", "2d_gs", "4d", "4d_nob", "3d"):
        b = cu(fx[f"flr_{name}_b"]) if f"flr_{name}_b" in fx else None
        y = op.fused_leaky_relu(cu(fx[f"flr_{name}_x"]), b, scale=float(fx[f"flr_{name}_scale"]))
        assert maxdiff(y.cpu(), fx[f"flr_{name}_y"]) < 1e-6, name


def test_fused_leaky_relu_large_and_empty():
    x = torch.randn(2, 32, 128, 128)
    b = torch.randn(32)
    y = op.fused_leaky_relu(cu(x), cu(b))
    assert maxdiff(y.cpu(), O.fused_leaky_relu(x, b)) < 1e-6
    e = op.fused_leaky_relu(torch.empty(0, 4, device=DEV), cu(torch.randn(4)))
    assert e.numel() == 0
    x = torch.randn(3, 5, 7)   # odd sizes -> scalar path
    assert maxdiff(op.fused_leaky_relu(cu(x), cu(b[:5]), scale=1.0).cpu(), O.fused_leaky_relu(x, b[:5], scale=1.0)) < 1e-6


def test_op_backward_matches_autograd_of_oracle():
    x = torch.randn(2, 6, 9, 9, requires_grad=True)
    b = torch.randn(6, requires_grad=True)
    gy = torch.randn(2, 6, 9, 9)
    O.fused_leaky_relu(x, b).backward(gy)
    xg, bg = cu(x.detach()).requires_grad_(True), cu(b.detach()).requires_grad_(True)
    op.fused_leaky_relu(xg, bg).backward(cu(gy))
    assert maxdiff(xg.grad.cpu(), x.grad) < 1e-6 and maxdiff(bg.grad.cpu(), b.grad) < 1e-4
    x2 = torch.randn(1, 3, 8, 8, requires_grad=True)
    kern = O.make_blur_kernel(gain=4.0)
    gy2 = torch.randn(1, 3, 16, 16)
    O.upfirdn2d(x2, kern, up=2, pad=(2, 1)).backward(gy2)
    x2g = cu(x2.detach()).requires_grad_(True)
    op.upfirdn2d(x2g, cu(kern), up=2, pad=(2, 1)).backward(cu(gy2))
    assert maxdiff(x2g.grad.cpu(), x2.grad) < 1e-5


# ------------------------------------------------------------------------------------------ camera / mapping
def test_camera_golden(golden):
    fx = golden("camera")
    for tag, cam in (("ffhq", configs.FFHQ_CAM_CFG), ("cars", configs.COMPCARS_CAM_CFG)):
        e, f, n, fa, vp = Camera.generate_camera_params(64, DEV, locations=cu(fx["locs"]), fov_ang=cam["fov_ang"],
                                                        dist_radius=cam["dist_radius"])
        assert maxdiff(e.cpu(), fx[f"{tag}_extr"]) < 2e-6
        assert maxdiff(f.cpu(), fx[f"{tag}_focal"]) < 1e-3 and f.shape == (4, 1, 1)
        assert maxdiff(n.cpu(), fx[f"{tag}_near"]) < 1e-7 and maxdiff(fa.cpu(), fx[f"{tag}_far"]) < 1e-7
    e, f, *_ = Camera.generate_camera_params(64, DEV, locations=cu(fx["locs"]), fov_ang=cu(fx["fovt"]))
    assert maxdiff(e.cpu(), fx["fovt_extr"]) < 2e-6 and maxdiff(f.cpu(), fx["fovt_focal"]) < 1e-3
    e, *_ = Camera.generate_camera_params_v1(64, DEV, locations=torch.zeros(8, 2, device=DEV), up=cu(fx["roll_ups"]))
    assert maxdiff(e.cpu(), fx["roll_extr"]) < 2e-6
    e, *_ = Camera.generate_camera_params(64, DEV, locations=cu(fx["deg_locs"]))
    assert maxdiff(e.cpu(), fx["deg_extr"]) < 2e-6


def test_linear_and_table():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 96, generator=g)
    W = torch.randn(40, 96, generator=g)
    b = torch.randn(40, generator=g)
    mean = torch.randn(40, generator=g)
    y = hip.linear(cu(x), cu(W), cu(b), w_scale=0.3, b_scale=0.5, pixelnorm=True, lrelu=True, act_gain=2 ** 0.5,
                   trunc_mean=cu(mean), trunc_psi=0.7)
    ref = O.fused_leaky_relu(torch.nn.functional.linear(O.pixel_norm(x), W * 0.3), b * 0.5)
    ref = mean + 0.7 * (ref - mean)
    assert maxdiff(y.cpu(), ref) < 2e-5
    # odd in_dim -> scalar path; no bias
    x2, W2 = torch.randn(2, 7, generator=g), torch.randn(3, 7, generator=g)
    assert maxdiff(hip.linear(cu(x2), cu(W2)).cpu(), x2 @ W2.t()) < 1e-5
    # table: two heads reading different style rows, writing into one buffer with an affine output map
    styles = cu(torch.randn(3, 2, 32, generator=g))
    Wa, Wb = cu(torch.randn(8, 32, generator=g)), cu(torch.randn(16, 32, generator=g))
    ba = cu(torch.randn(8, generator=g))
    out = torch.zeros(3, 24, device=DEV)
    tab = hip.LinearTable(DEV)
    tab.add(Wa, ba, styles, 64, out, 24, out_scale=15.0, out_shift=30.0, x_offset=0, out_offset=0)
    tab.add(Wb, None, styles, 64, out, 24, w_scale=0.5, x_offset=32, out_offset=8)
    tab.run(3)
    ref = torch.cat([15 * (styles[:, 0].cpu() @ Wa.cpu().t() + ba.cpu()) + 30, (styles[:, 1].cpu() @ Wb.cpu().t()) * 0.5], 1)
    assert maxdiff(out.cpu(), ref) < 1e-4


# ------------------------------------------------------------------------------------------ NeRF renderer
def _render_vs_oracle(cfg, seed, B, img, N, perturb, static, chunks=None, tol=5e-5):
    G = pkg.build_generator(cfg, DEV, seed=seed)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(seed + 100)
    D = cfg["renderer_cfg"]["N_layers_renderer"]
    S = cfg["mapping_renderer_cfg"]["style_dim"]
    styles = torch.randn(B, D + 1, S, generator=g)
    locs = (torch.rand(B, 2, generator=g) - 0.5) * torch.tensor([1.2, 0.3])
    cam = O.camera_params(locs, img, 6, 0.12)
    u = torch.rand(B, img, img, 1, generator=g) if perturb else None
    thumb, feat, sdf, mask, xyz = G.renderer.render(cu(cam[0]), cu(cam[1]), cu(cam[2]), cu(cam[3]), cu(styles), img, N,
                                                    perturb_u=None if u is None else cu(u), static_viewdirs=static,
                                                    return_sdf=True, n_chunks=chunks)
    rays_o, rays_d, vd = O.rays_in_world(cam[1], img, cam[0], static)
    z = O.z_vals(cam[2], cam[3], B, img, img, N, u)
    pts = O.ray_points(rays_o, rays_d, z)
    R = img * img
    r_thumb, r_feat, r_sdf, r_mask, r_xyz = O.renderer_forward(
        sd, "renderer", pts.reshape(B, R, N, 3), rays_d.reshape(B, R, 3), vd.reshape(B, R, 3), z.reshape(B, R, N),
        cam[2], cam[3], styles, D)
    img_of = lambda t: t.transpose(1, 2).reshape(B, t.shape[-1], img, img)
    assert maxdiff(sdf.cpu(), r_sdf.reshape(B, img, img, N, 1)) < tol
    assert maxdiff(feat.cpu(), img_of(r_feat)) < tol
    assert maxdiff(thumb.cpu(), img_of(r_thumb)) < tol
    assert maxdiff(xyz.cpu(), img_of(r_xyz)) < tol
    assert maxdiff(mask.cpu(), img_of(r_mask)) < tol


@pytest.mark.parametrize("D,N,perturb,static,chunks", [
    (2, 6, False, False, None), (3, 5, True, True, 2), (2, 7, False, False, 7), (1, 4, True, False, 1)])
def test_nerf_render_tiny_hidden32(D, N, perturb, static, chunks):
    _render_vs_oracle(configs.tiny_G_cfg(32, D), seed=3 + D, B=2, img=8, N=N, perturb=perturb, static=static, chunks=chunks)


@pytest.mark.parametrize("D,N,img,B,chunks", [(2, 24, 16, 1, None), (8, 6, 8, 2, 3), (6, 24, 12, 1, 8)])
def test_nerf_render_hidden256(D, N, img, B, chunks):
    # ragged: img=12 -> 144 rays = 9 groups of 16; chunks that do not divide N
    _render_vs_oracle(configs.ffhq_G_cfg(256, D), seed=11 + D, B=B, img=img, N=N, perturb=True, static=False,
                      chunks=chunks, tol=2e-4)


@pytest.mark.parametrize("hidden,D,img,N,B,NC", [(256, 2, 10, 24, 1, 8), (256, 8, 8, 9, 2, 8), (64, 2, 9, 16, 2, 8),
                                                 (256, 2, 10, 24, 2, 4), (256, 2, 9, 24, 4, 2), (64, 3, 11, 10, 3, 1),
                                                 (64, 2, 6, 7, 2, 4)])
def test_nerf_in_kernel_chunk_combination_is_bit_identical(hidden, D, img, N, B, NC, monkeypatch):
    """When the chunk count divides the eight waves of a workgroup (8 at batch 1, 4 / 2 / 1 at batches 2 / 4 / 8+) the render
    kernel combines the partials itself (cips3d_nerf_fuses_finish); the result must equal the `part` + cips3d_nerf_finish route
    bit for bit -- ragged ray groups (img^2 % 16 != 0), N not a multiple of the chunk count, padded tasks."""
    cfg = configs.ffhq_G_cfg(256, D) if hidden == 256 else configs.tiny_G_cfg(hidden, D)
    G = pkg.build_generator(cfg, DEV, seed=5)
    g = torch.Generator().manual_seed(1)
    styles = cu(torch.randn(B, D + 1, cfg["mapping_renderer_cfg"]["style_dim"], generator=g))
    cam = [cu(t) for t in O.camera_params((torch.rand(B, 2, generator=g) - 0.5) * 0.8, img, 6, 0.12)[:4]]
    u = cu(torch.rand(B, img, img, 1, generator=g))
    seen = {}
    real = hip.nerf_render_maps

    def spy(**kw):
        seen.update(kw)
        return real(**kw)

    monkeypatch.setattr(hip, "nerf_render_maps", spy)
    thumb, feat, _, mask, xyz = G.renderer.render(*cam, styles, img, N, perturb_u=u, n_chunks=NC)
    p = hip._nerf_params(seen)
    out = [torch.empty_like(t) for t in (feat, thumb, xyz, mask)]
    p.o_features, p.o_thumb, p.o_xyz, p.o_mask = (t.data_ptr() for t in out)
    from cips_3dplusplus_amd import _lib
    import ctypes
    assert _lib.load().cips3d_nerf_fuses_finish(ctypes.byref(p)) == 1
    part = torch.empty(NC, B, hidden + 8, img * img, device=DEV)
    hip.nerf_render(**{**seen, "part": part})
    f2, t2, x2, m2 = hip.nerf_finish(part, NC, B, img, hidden)
    assert torch.equal(feat, f2) and torch.equal(thumb, t2) and torch.equal(xyz, x2) and torch.equal(mask, m2)


def test_nerf_chunk_count_does_not_change_result():
    cfg = configs.ffhq_G_cfg(256, 2)
    G = pkg.build_generator(cfg, DEV, seed=2)
    g = torch.Generator().manual_seed(0)
    styles = cu(torch.randn(1, 3, 256, generator=g))
    cam = [cu(t) for t in O.camera_params(torch.tensor([[0.2, 0.05]]), 16, 6, 0.12)[:4]]
    outs = [G.renderer.render(*cam, styles, 16, 24, n_chunks=c) for c in (1, 3, 8, 24)]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            if a is not None:
                assert maxdiff(a, b) < 3e-6


# ------------------------------------------------------------------------------------------ decoder blocks
def test_modulated_conv_golden_generality_path(golden):
    fx = golden("modconv")
    for tag in fx["mc_names"]:
        tag = str(tag)
        k = 3 if tag.startswith("k3") else 1
        m = _dec_mod().ModulatedConv2d(8, 12, k, 16, demodulate="_d1" in tag, upsample="_up1" in tag)
        m.load_state_dict(fx.sub(f"mc_{tag}.sd."))
        m = m.to(DEV)
        y = m(cu(fx[f"mc_{tag}.x"]), cu(fx[f"mc_{tag}.style"]))
        assert maxdiff(y.cpu(), fx[f"mc_{tag}.y"]) < 3e-5, tag


@pytest.mark.parametrize("shape", [(2, 32, 1, 7), (1, 64, 5, 1), (3, 8, 1, 1)])
def test_modulated_conv_on_one_pixel_wide_inputs(shape):
    """model_v3.py:302-306: for height == 1 or width == 1 the reference replaces the grouped conv by a bmm over the pixels --
    the same per-sample GEMM this package always runs for k = 1.  Checked against the oracle on such inputs."""
    dec = _dec_mod()
    B, cin, H, W = shape
    g = torch.Generator().manual_seed(H * 10 + W)
    m = dec.ModulatedConv2d(cin, 24, 1, 16)
    sd = {"m." + k: v.clone() for k, v in m.state_dict().items()}
    x, st = torch.randn(B, cin, H, W, generator=g), torch.randn(B, 16, generator=g)
    y = m.to(DEV)(cu(x), cu(st))
    ref = O.modulated_conv2d(sd, "m", x, st)
    assert y.shape == ref.shape and maxdiff(y.cpu(), ref) < 3e-5


def test_styled_conv_and_torgb_golden(golden):
    fx = golden("modconv")
    import cips_3dplusplus_amd.decoder as dec
    for tag in ("up0", "up1"):
        up = tag == "up1"
        sc = dec.StyledConv(8, 12, 1, 16, upsample=up)
        sc.load_state_dict(fx.sub(f"sc_{tag}.sd."))
        sc = sc.to(DEV)
        y = sc(cu(fx[f"sc_{tag}.x"]), cu(fx[f"sc_{tag}.style"]), noise=cu(fx[f"sc_{tag}.noise"]))
        assert maxdiff(y.cpu(), fx[f"sc_{tag}.y"]) < 3e-5
        tr = dec.ToRGB(12, 16, upsample=up)
        tr.load_state_dict(fx.sub(f"rgb_{tag}.sd."))
        tr = tr.to(DEV)
        y = tr(cu(fx[f"rgb_{tag}.x"]), cu(fx[f"rgb_{tag}.style"]), skip=cu(fx[f"rgb_{tag}.skip"]))
        assert maxdiff(y.cpu(), fx[f"rgb_{tag}.y"]) < 3e-5
        y = tr(cu(fx[f"rgb_{tag}.x"]), cu(fx[f"rgb_{tag}.style"]))
        assert maxdiff(y.cpu(), fx[f"rgb_{tag}.y_noskip"]) < 3e-5


@pytest.mark.parametrize("cin,cout,hw,up,B", [
    (32, 32, 16, False, 2), (64, 32, 16, True, 1), (64, 64, 24, False, 1), (128, 128, 16, False, 2),
    (256, 128, 8, True, 1), (512, 512, 8, False, 1), (256, 512, 12, False, 1), (96, 160, 6, False, 2)])
def test_styled_conv_mfma_path_vs_oracle(cin, cout, hw, up, B):
    import cips_3dplusplus_amd.decoder as dec
    torch.manual_seed(cin + cout + hw)
    sc = dec.StyledConv(cin, cout, 1, 64, upsample=up)
    sc.noise.weight.data.fill_(0.3)
    sc.activate.bias.data = torch.randn(cout) * 0.2
    sd = {"m." + k: v.clone() for k, v in sc.state_dict().items()}
    x = torch.randn(B, cin, hw, hw)
    st = torch.randn(B, 64)
    ho = 2 * hw if up else hw
    nz = torch.randn(1, 1, ho, ho)
    assert sc.conv.fast(hw * hw)
    y = sc.to(DEV)(cu(x), cu(st), noise=cu(nz))
    ref = O.styled_conv(sd, "m", x, st, nz, upsample=up)
    assert maxdiff(y.cpu(), ref) < 3e-5 * max(1.0, float(ref.abs().max()))
    # per-sample noise
    nzb = torch.randn(B, 1, ho, ho)
    y = sc(cu(x), cu(st), noise=cu(nzb))
    assert maxdiff(y.cpu(), O.styled_conv(sd, "m", x, st, nzb, upsample=up)) < 3e-5 * max(1.0, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------ generator
def _tiny_cfg(tag):
    return configs.tiny_G_cfg(32, 3 if "d3" in tag else 2, 3 if "k3" in tag else 1)


@pytest.mark.parametrize("tag", ["h32_d2", "h32_d3", "h32_d2_k3"])
def test_tiny_generator_golden(golden, tag):
    fx = golden("tiny_generator")
    cfg = _tiny_cfg(tag)
    G = pkg.build_generator(cfg, DEV, state_dict=fx.sub(f"{tag}.sd."))
    zs = [cu(fx[f"{tag}.z0"]), cu(fx[f"{tag}.z1"])]
    e, f, n, fa, _ = Camera.generate_camera_params(8, DEV, locations=cu(fx[f"{tag}.locs"]))
    nb = [cu(fx[f"{tag}.noise{i}"]) for i in range(G.decoder.num_layers)]
    G.style_render_mean, G.style_decoder_mean = cu(fx[f"{tag}.mean_r"]), cu(fx[f"{tag}.mean_d"])
    runs = (("a", dict(N_samples=6, perturb=False, static_viewdirs=False), 1.0, None),
            ("b", dict(N_samples=5, perturb=False, static_viewdirs=True), 0.5, None),
            ("c", dict(N_samples=6, perturb=True, static_viewdirs=False), 1.0, cu(fx[f"{tag}.c.u"])))
    for vtag, ncfg, trunc, u in runs:
        r = G(zs=zs, cam_poses=e, focals=f, img_size=8, near=n, far=fa, noise_bufs=nb, truncation=trunc,
              nerf_cfg=ncfg, return_sdf=True, return_xyz=True, perturb_u=u)
        for k in ("rgb", "thumb_rgb", "sdf", "xyz", "mask", "depth"):
            ref = fx[f"{tag}.{vtag}.{k}"]
            assert r[k].shape == ref.shape and r[k].is_contiguous()
            assert maxdiff(r[k].cpu(), ref) < 1e-3, (tag, vtag, k)          # north_star bound
            assert maxdiff(r[k].cpu(), ref) < 1e-4, (tag, vtag, k)          # what fp32 actually gives here
        assert r["style_decoder"] is None and r["eikonal_term"] is None


def test_mean_latent_golden(golden):
    fx = golden("tiny_generator")
    tag = "h32_d2"
    G = pkg.build_generator(_tiny_cfg(tag), DEV, state_dict=fx.sub(f"{tag}.sd."))
    mr = G._run_style(cu(fx[f"{tag}.ml_zr"])).mean(0, keepdim=True)
    md = G._run_style_decoder(cu(fx[f"{tag}.ml_zd"])).mean(0, keepdim=True)
    assert maxdiff(mr.cpu(), fx[f"{tag}.ml_r"]) < 1e-5 and maxdiff(md.cpu(), fx[f"{tag}.ml_d"]) < 1e-5


FULL = [("r256_d2_n24", 256, 2, 24, False, 1.0), ("r256_d8_n24", 256, 8, 24, False, 1.0),
        ("r1024_d2_n24", 1024, 2, 24, False, 1.0), ("r256_d6_n64_static_trunc", 256, 6, 64, True, 0.5)]


@pytest.mark.parametrize("tag,res,D,N,static,trunc", FULL)
def test_full_size_generator_golden(golden, tag, res, D, N, static, trunc):
    """Release-size generator on name-keyed synthetic weights vs strided samples of the reference output."""
    fx = golden("full_size")
    cfg = configs.ffhq_G_cfg(res, D)
    G = pkg.build_generator(cfg, DEV, seed=1)
    sd_cpu = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    # weights and inputs are closed-form functions of (name, seed, index): a mismatch is a bug, never a reason to skip
    assert weights.state_dict_checksum(sd_cpu) == int(fx[f"{tag}.sd_checksum"])
    zs, nb, means = weights.synth_inputs(cfg, batch=1, seed=12345)
    G.style_render_mean, G.style_decoder_mean = cu(means[0]), cu(means[1])
    e, f, n, fa, _ = Camera.generate_camera_params(64, DEV, locations=torch.tensor([[0.31, -0.08]], device=DEV))
    r = G(zs=[cu(z) for z in zs], cam_poses=e, focals=f, img_size=64, near=n, far=fa, noise_bufs=[cu(b) for b in nb],
          truncation=trunc, nerf_cfg=dict(N_samples=N, perturb=False, static_viewdirs=static), return_sdf=True,
          return_xyz=True)
    stride = int(fx["stride"])
    assert r["rgb"].shape == (1, 3, res, res)
    d_rgb = maxdiff(r["rgb"].flatten()[::stride].cpu(), fx[f"{tag}.rgb_s"])
    d_thumb = maxdiff(r["thumb_rgb"].cpu(), fx[f"{tag}.thumb_rgb"])
    print(f"{tag}: rgb diff {d_rgb:.2e} (range +-{float(fx[tag + '.rgb_absmax']):.1f}, reference fp32 noise floor "
          f"{float(fx[tag + '.noise_floor_rgb']):.1e}), thumb diff {d_thumb:.2e}")
    assert d_rgb < 1e-3 and d_thumb < 1e-3
    for k in ("mask", "depth", "xyz"):
        assert maxdiff(r[k].cpu(), fx[f"{tag}.{k}"]) < 1e-4, k
    assert maxdiff(r["sdf"].flatten()[::stride].cpu(), fx[f"{tag}.sdf_s"]) < 1e-4


@pytest.mark.parametrize("mode", ["fp32_exact"])
@pytest.mark.parametrize("tag,res,D,N,static,trunc", [FULL[2], FULL[0]])
def test_full_size_generator_golden_in_the_other_render_arithmetics(golden, mode, tag, res, D, N, static, trunc):
    """The release-size reference goldens through the whole forward in IEEE-fp32 arithmetic (Generator.set_precision("fp32_exact"):
    render kernel AND decoder on the fp32 matrix instruction): the same bars as the default path."""
    fx = golden("full_size")
    cfg = configs.ffhq_G_cfg(res, D)
    G = pkg.build_generator(cfg, DEV, seed=1)
    G.set_precision("fp32_exact")
    zs, nb, means = weights.synth_inputs(cfg, batch=1, seed=12345)
    G.style_render_mean, G.style_decoder_mean = cu(means[0]), cu(means[1])
    e, f, n, fa, _ = Camera.generate_camera_params(64, DEV, locations=torch.tensor([[0.31, -0.08]], device=DEV))
    r = G(zs=[cu(z) for z in zs], cam_poses=e, focals=f, img_size=64, near=n, far=fa, noise_bufs=[cu(b) for b in nb],
          truncation=trunc, nerf_cfg=dict(N_samples=N, perturb=False, static_viewdirs=static), return_sdf=True,
          return_xyz=True)
    stride = int(fx["stride"])
    d_rgb = maxdiff(r["rgb"].flatten()[::stride].cpu(), fx[f"{tag}.rgb_s"])
    d_thumb = maxdiff(r["thumb_rgb"].cpu(), fx[f"{tag}.thumb_rgb"])
    print(f"{tag} [{mode}]: rgb diff {d_rgb:.2e}, thumb diff {d_thumb:.2e}")
    assert d_rgb < 1e-3 and d_thumb < 1e-3
    for k in ("mask", "depth", "xyz"):
        assert maxdiff(r[k].cpu(), fx[f"{tag}.{k}"]) < 1e-4, k
    assert maxdiff(r["sdf"].flatten()[::stride].cpu(), fx[f"{tag}.sdf_s"]) < 1e-4


def test_planned_forward_equals_per_op_path(golden):
    """cips3d_generator_forward (one call) and the per-op launches run the same kernels: identical outputs."""
    fx = golden("tiny_generator")
    tag = "h32_d2"
    G = pkg.build_generator(_tiny_cfg(tag), DEV, state_dict=fx.sub(f"{tag}.sd."))
    zs = [cu(fx[f"{tag}.z0"]), cu(fx[f"{tag}.z1"])]
    e, f, n, fa, _ = Camera.generate_camera_params(8, DEV, locations=cu(fx[f"{tag}.locs"]))
    nb = [cu(fx[f"{tag}.noise{i}"]) for i in range(G.decoder.num_layers)]
    G.style_render_mean, G.style_decoder_mean = cu(fx[f"{tag}.mean_r"]), cu(fx[f"{tag}.mean_d"])
    ncfg = dict(N_samples=6, perturb=False, static_viewdirs=False)
    kw = dict(zs=zs, cam_poses=e, focals=f, img_size=8, near=n, far=fa, noise_bufs=nb, truncation=0.7, nerf_cfg=ncfg,
              return_sdf=True, return_xyz=True)
    a = G(**kw)
    assert G._plans[(2, 8, 6, False)] is not None          # the plan path was taken
    G._plans[(2, 8, 6, False)] = None                      # force the per-op path
    b = G(**kw)
    for k in ("rgb", "thumb_rgb", "sdf", "xyz", "mask", "depth"):
        assert maxdiff(a[k], b[k]) < 1e-6, k
    # explicit W+ styles bypass the mapping networks on both paths
    G._plans.clear()
    sr, sd_ = G.mapping_networks(zs, 0.7, None)
    c = G(**{**kw, "zs": [None, None], "style_render": sr, "style_decoder": sd_})
    assert maxdiff(a["rgb"], c["rgb"]) < 1e-6
    # random-noise / perturbed call runs and is finite
    d = G(zs=zs, cam_poses=e, focals=f, img_size=8, near=n, far=fa, nerf_cfg=dict(N_samples=6, perturb=True))
    assert torch.isfinite(d["rgb"]).all()


@pytest.mark.parametrize("C,H,B,last", [(32, 32, 1, True), (64, 32, 2, False), (128, 32, 1, False), (256, 32, 1, False),
                                        (32, 64, 1, False)])
def test_fused_upsampling_stage_vs_oracle(C, H, B, last):
    """cips3d_fused_up_conv = StyledConv(up) FIR part + StyledConv + ToRGB(up) of one stage, against the oracle."""
    import cips_3dplusplus_amd.decoder as dec
    torch.manual_seed(C + H)
    S = 64
    c1 = dec.StyledConv(C, C, 1, S, upsample=True)
    c2 = dec.StyledConv(C, C, 1, S)
    tr = dec.ToRGB(C, S, upsample=True)
    for m in (c1, c2):
        m.noise.weight.data.fill_(0.25)
        m.activate.bias.data = torch.randn(C) * 0.2
    tr.bias.data = torch.randn(1, 3, 1, 1) * 0.1
    sd = {}
    for nm, m in (("c1", c1), ("c2", c2), ("tr", tr)):
        sd.update({f"{nm}.{k}": v.clone() for k, v in m.state_dict().items()})
    x = torch.randn(B, C, H, H)
    st = [torch.randn(B, S) for _ in range(3)]
    n1, n2 = torch.randn(1, 1, 2 * H, 2 * H), torch.randn(B, 1, 2 * H, 2 * H)
    skip = torch.randn(B, 3, H, H)
    r1 = O.styled_conv(sd, "c1", x, st[0], n1, upsample=True)
    r2 = O.styled_conv(sd, "c2", r1, st[1], n2)
    r3 = O.to_rgb(sd, "tr", r2, st[2], skip, upsample=True)
    c1, c2, tr = c1.to(DEV), c2.to(DEV), tr.to(DEV)
    y_lo = hip.modconv1x1(cu(x), c1.conv.modulated_weight(cu(st[0]), packed=True), C, epilogue=0)
    out2, rgb = hip.fused_up_conv(y_lo, c1.conv.blur.kernel, cu(n1), c1.noise.weight, c1.activate.bias,
                                  c2.conv.modulated_weight(cu(st[1]), packed=True), cu(n2), c2.noise.weight,
                                  c2.activate.bias, tr.conv.modulated_weight(cu(st[2]), packed=False), tr.bias, cu(skip),
                                  skip_up=True, want_out2=not last)
    scale = max(1.0, float(r2.abs().max()))
    if not last:
        assert maxdiff(out2.cpu(), r2) < 3e-5 * scale
    assert maxdiff(rgb.cpu(), r3) < 3e-5 * max(1.0, float(r3.abs().max()))


@pytest.mark.parametrize("S,N,B,n_words", [(64, 24, 1, 30000), (64, 128, 1, 70001), (10, 7, 2, 1500), (64, 24, 2, 1)])
def test_render_launch_leaves_the_callers_scratch_zeroed(S, N, B, n_words):
    """cips3d_nerf_params.zero_words: the render launch clears a scratch range of its caller (the decoder's measured range rows in
    a frame of a sequence) -- inside the default kernel's fused finish, or with a small launch in front where the shape takes
    another route (ragged ray counts) -- exactly that range, and the maps do not change."""
    G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=4)
    e, f, n, fa, _ = Camera.generate_camera_params(S, DEV, locations=torch.tensor([[0.2, -0.1]] * B, device=DEV))
    styles = cu(weights.det_normal("zw.styles", (B, 3, 256), 0.5, 2))
    ref = G.renderer.render(e, f, n, fa, styles, S, N, return_sdf=True)
    buf = torch.full((n_words + 64,), 7.0, device=DEV)
    new = G.renderer.render(e, f, n, fa, styles, S, N, return_sdf=True, zero_words=buf[:n_words])
    assert float(buf[:n_words].abs().max()) == 0.0 and bool((buf[n_words:] == 7.0).all())
    for a, b in zip(ref, new):
        assert torch.equal(a, b)


@pytest.mark.parametrize("C,H,B,last", [(32, 64, 1, True), (64, 64, 2, False), (128, 64, 1, False), (256, 64, 1, False), (32, 128, 2, True)])
def test_flat_stage_vs_oracle(C, H, B, last):
    """CIPS3D_STAGE_FLAT: a block that does not up-sample -- StyledConv + StyledConv + ToRGB at one resolution (the 512 / 1024
    blocks of a 256^2 generator, model_v3.py:553-590) -- through the fused stage kernel, against the oracle's three modules."""
    import cips_3dplusplus_amd.decoder as dec
    torch.manual_seed(3 * C + H)
    S = 64
    c1 = dec.StyledConv(2 * C, C, 1, S)
    c2 = dec.StyledConv(C, C, 1, S)
    tr = dec.ToRGB(C, S, upsample=False)
    for m in (c1, c2):
        m.noise.weight.data.fill_(0.25)
        m.activate.bias.data = torch.randn(C) * 0.2
    tr.bias.data = torch.randn(1, 3, 1, 1) * 0.1
    sd = {}
    for nm, m in (("c1", c1), ("c2", c2), ("tr", tr)):
        sd.update({f"{nm}.{k}": v.clone() for k, v in m.state_dict().items()})
    x = torch.randn(B, 2 * C, H, H)
    st = [torch.randn(B, S) for _ in range(3)]
    n1, n2 = torch.randn(1, 1, H, H), torch.randn(B, 1, H, H)
    skip = torch.randn(B, 3, H, H)
    r1 = O.styled_conv(sd, "c1", x, st[0], n1)
    r2 = O.styled_conv(sd, "c2", r1, st[1], n2)
    r3 = O.to_rgb(sd, "tr", r2, st[2], skip, upsample=False)
    c1, c2, tr = c1.to(DEV), c2.to(DEV), tr.to(DEV)
    assert _lib.load().cips3d_fused_flat_conv_supported(C, H, H)
    y = hip.modconv1x1(cu(x), c1.conv.modulated_weight(cu(st[0]), packed=True), C, epilogue=0)
    out2, rgb = hip.fused_up_conv(y, None, cu(n1), c1.noise.weight, c1.activate.bias,
                                  c2.conv.modulated_weight(cu(st[1]), packed=True), cu(n2), c2.noise.weight,
                                  c2.activate.bias, tr.conv.modulated_weight(cu(st[2]), packed=False), tr.bias, cu(skip),
                                  want_out2=not last, flat=True)
    assert rgb.shape == (B, 3, H, H)
    if not last:
        assert maxdiff(out2.cpu(), r2) < 3e-5 * max(1.0, float(r2.abs().max()))
    assert maxdiff(rgb.cpu(), r3) < 3e-5 * max(1.0, float(r3.abs().max()))
    # ... and without a skip image
    _, rgb0 = hip.fused_up_conv(y, None, cu(n1), c1.noise.weight, c1.activate.bias,
                                c2.conv.modulated_weight(cu(st[1]), packed=True), cu(n2), c2.noise.weight,
                                c2.activate.bias, tr.conv.modulated_weight(cu(st[2]), packed=False), tr.bias, None,
                                want_out2=False, flat=True)
    assert maxdiff(rgb0.cpu(), r3 - skip) < 3e-5 * max(1.0, float(r3.abs().max()))


@pytest.mark.parametrize("C,mode", [(64, "fp32"), (64, "bf16"), (64, "split"), (128, "split"), (256, "fp32"), (256, "split")])
def test_flat_stage_chains_the_next_block(C, mode):
    """The flat form of cips3d_fused_up_conv_next: y_next = W_next out2 from the registers, at the block's own resolution, against
    the separate GEMM of the stored out2; rgb / out2 unchanged by the chained work; a batch-strided first noise map."""
    torch.manual_seed(11)
    H, B = 64, 2
    bf16, split = mode == "bf16", mode == "split"
    y = torch.randn(B, C, H, H, device=DEV)
    n1, n2 = torch.randn(B, 1, H, H, device=DEV), torch.randn(1, 1, H, H, device=DEV)
    nw1, nw2 = torch.full((1,), 0.3, device=DEV), torch.full((1,), -0.2, device=DEV)
    b1, b2 = torch.randn(C, device=DEV) * 0.2, torch.randn(C, device=DEV) * 0.2
    W2, Wn, Wr = torch.randn(C, C, device=DEV), torch.randn(C // 2, C, device=DEV), torch.randn(3, C, device=DEV)
    s2, sn, sr = (torch.randn(B, C, device=DEV) * 0.3 + 1 for _ in range(3))

    def mod(W, s, flags):
        out = torch.empty(B * W.shape[0] * C, device=DEV)
        _lib.check(_lib.load().cips3d_modulate_weights(W.data_ptr(), s.data_ptr(), C, out.data_ptr(), B, W.shape[0], C, 1,
                                                       1.0 / math.sqrt(C), flags, torch.cuda.current_stream().cuda_stream), "mod")
        return out

    sp16 = hip.MOD_SPLIT16 if split else 0
    wm2 = mod(W2, s2, hip.MOD_DEMODULATE | hip.MOD_PACKED | sp16)
    wmn_std = mod(Wn, sn, hip.MOD_DEMODULATE | hip.MOD_PACKED | (hip.MOD_SPLIT if split else 0))
    wmn_chn = mod(Wn, sn, hip.MOD_DEMODULATE | hip.MOD_PACKED | hip.MOD_CHAINED | sp16)
    wmr = mod(Wr, sr, 0)
    brgb = torch.randn(3, device=DEV) * 0.1
    skip = torch.randn(B, 3, H, H, device=DEV)
    kw = dict(bf16=bf16, split=split, flat=True)
    out2, rgb = hip.fused_up_conv(y, None, n1, nw1, b1, wm2, n2, nw2, b2, wmr, brgb, skip, **kw)
    ref = hip.modconv1x1(out2, wmn_std, C // 2, epilogue=0, bf16=bf16, split=split)
    o2, rgb2, y_next = hip.fused_up_conv(y, None, n1, nw1, b1, wm2, n2, nw2, b2, wmr, brgb, skip, wm_next=wmn_chn, **kw)
    assert y_next.shape == (B, C // 2, H, H)
    tol = 2e-6 if not split else 4e-6
    assert maxdiff(o2, out2) <= (0 if not split else 2e-6 * float(out2.abs().max())) and maxdiff(rgb2, rgb) <= 4e-6 * float(rgb.abs().max())
    assert maxdiff(y_next, ref) < tol * float(ref.abs().max())
    _, rgb3, y3 = hip.fused_up_conv(y, None, n1, nw1, b1, wm2, n2, nw2, b2, wmr, brgb, skip, wm_next=wmn_chn, want_out2=False, **kw)
    assert torch.equal(rgb3, rgb2) and torch.equal(y3, y_next)
    # the exact-fp32 form of the same stage is the reference of the other two arithmetics
    if mode != "fp32":
        wm2_f = mod(W2, s2, hip.MOD_DEMODULATE | hip.MOD_PACKED)
        o_f, rgb_f = hip.fused_up_conv(y, None, n1, nw1, b1, wm2_f, n2, nw2, b2, wmr, brgb, skip, flat=True)
        lim = 3e-2 if bf16 else 3e-6
        assert maxdiff(out2, o_f) < lim * float(o_f.abs().max()) and maxdiff(rgb, rgb_f) < lim * float(rgb_f.abs().max())


@pytest.mark.parametrize("res,S,B", [(256, 32, 2), (256, 48, 1), (512, 32, 1), (1024, 16, 1), (256, 16, 3)])
def test_planned_forward_at_other_nerf_resolutions(res, S, B):
    """The one-call forward against the per-op launches at NeRF resolutions other than the recipes' 64: the planes run, the chained
    up-sampling stages and the flat stages behind them pick their shapes from the plan (192^2 / 128^2 / 64^2 flat blocks, a
    1024 recipe whose last stage is 256^2)."""
    cfg = configs.ffhq_G_cfg(res, 2)
    G = pkg.build_generator(cfg, DEV, seed=3)
    zs, nb, _ = weights.synth_inputs(cfg, batch=B, seed=7, img_size=S)
    g = torch.Generator(device=DEV).manual_seed(S)
    e, f, n, fa, _ = Camera.generate_camera_params(S, DEV, locations=0.2 * torch.randn(B, 2, device=DEV, generator=g))
    kw = dict(zs=[cu(z) for z in zs], cam_poses=e, focals=f, img_size=S, near=n, far=fa, noise_bufs=[cu(b) for b in nb],
              nerf_cfg=dict(N_samples=6, perturb=False, static_viewdirs=False))
    a = G(**kw)["rgb"].clone()
    key = (B, S, 6, False)
    assert G._plans.get(key) is not None
    n_flat = sum(1 for li in G._plans[key]._layer_info if li.get("flat_head"))
    assert n_flat == {256: 2, 512: 1, 1024: 0}[res]
    G._plans[key] = None                                   # force the per-op path
    b = G(**kw)["rgb"].clone()
    up = {256: 4, 512: 8, 1024: 16}[res]
    assert a.shape == (B, 3, up * S, up * S)
    assert maxdiff(a, b) < 3e-5 * max(1.0, float(b.abs().max()))


def test_flat_stage_refuses_what_it_does_not_tile():
    lib = _lib.load()
    assert lib.cips3d_fused_flat_conv_supported(64, 256, 256) and lib.cips3d_fused_flat_conv_supported(32, 64, 64)
    assert not lib.cips3d_fused_flat_conv_supported(64, 256, 96)      # 64-pixel wave rows
    assert not lib.cips3d_fused_flat_conv_supported(64, 6, 64)        # 4-row tiles
    assert not lib.cips3d_fused_flat_conv_supported(48, 64, 64)
    y = torch.randn(1, 64, 6, 64, device=DEV)
    z = torch.zeros(64, device=DEV)
    wm = torch.zeros(64 * 64, device=DEV)
    with pytest.raises(RuntimeError):
        hip.fused_up_conv(y, None, None, None, z, wm, None, None, z, flat=True)


@pytest.mark.parametrize("res,precision", [(256, "fp32"), (512, "fp32"), (256, "fp32_exact"), (256, "bf16"), (256, "bf16_storage")])
def test_flat_blocks_of_a_low_resolution_generator(monkeypatch, res, precision):
    """A 256^2 (512^2) FFHQ generator still walks the 512 and 1024 (1024) blocks, at its final resolution: the plan runs them as
    flat stages chained behind the last up-sampling stage.  Same image as the per-layer launches (CIPS3D_FLAT_STAGES=0: two
    GEMMs + ToRGB per block), and the uint8 image leaves the last of them."""
    from cips_3dplusplus_amd import plan as planmod
    cfg = configs.ffhq_G_cfg(res, 2)
    G = pkg.build_generator(cfg, DEV, seed=2)
    G.set_precision(precision)
    B = 2
    zs, nb, _ = weights.synth_inputs(cfg, batch=B, seed=5)
    e, f, n, fa, _ = Camera.generate_camera_params(64, DEV, locations=torch.tensor([[0.2, 0.05], [-0.1, 0.1]], device=DEV))
    kw = dict(zs=[cu(z) for z in zs], cam_poses=e, focals=f, img_size=64, near=n, far=fa,
              noise_bufs=[cu(b) for b in nb], nerf_cfg=dict(N_samples=8, perturb=False, static_viewdirs=False))
    monkeypatch.setattr(planmod, "FLAT_STAGES", True)
    a = G(**kw)["rgb"].clone()
    pl = G._forward_plan(B, 64, 8, False)
    heads = [li for li in pl._layer_info if li.get("flat_head")]
    assert len(heads) == {256: 2, 512: 1}[res] and all(h.get("chained") for h in heads) and pl.u8_capable
    assert a.shape == (B, 3, res, res)
    u8 = torch.empty(B, 3, res, res, dtype=torch.uint8, device=DEV)
    with torch.no_grad():
        G(**kw, rgb_out=u8)
    assert torch.equal(u8, hip.rgb_to_uint8(a))
    monkeypatch.setattr(planmod, "FLAT_STAGES", False)
    G._plans.clear()
    b = G(**kw)["rgb"].clone()
    assert not any(li.get("flat_head") for li in G._forward_plan(B, 64, 8, False)._layer_info)
    G._plans.clear()
    # (bf16_storage: conv1's result of a flat block is one more tensor stored as bf16 -- the mode's rule for every fused stage)
    lim = {"fp32": 2e-5, "fp32_exact": 2e-5, "bf16": 2e-3, "bf16_storage": 2e-2}[precision]
    d, r = maxdiff(a, b), float(b.abs().max())
    mse = float(((a.double() - b.double()) ** 2).mean())
    psnr = 10 * math.log10(r * r / max(mse, 1e-300))
    print(f"flat stages vs per-layer launches at {res}^2 [{precision}]: {d:.2e} (max |rgb| {r:.2f}), PSNR {psnr:.1f} dB")
    assert d < lim * max(r, 1.0)
    # the flat stages' own check in the storage mode, independent of the oracle (whose bf16_store rounds conv1's result of a flat block
    # because the product does): against the per-layer launches, which keep that tensor in fp32, the image moves by ONE more
    # bf16-stored tensor per flat block -- far above the 53 dB floor test_generator_bf16_storage_vs_oracle_and_fp32 holds the whole
    # mode to against the oracle
    if precision == "bf16_storage":
        assert psnr > 50.0


@pytest.mark.parametrize("C,bf16", [(64, False), (64, True), (128, False), (128, True), (256, False), (256, True)])
def test_fused_stage_also_computes_next_low_res_gemm(C, bf16):
    """cips3d_fused_up_conv_next: y_next = W_next out2 taken from the registers that hold out2 (split K over the wave rows)
    against the separate cips3d_modconv1x1 of the stored out2; out2 / rgb unchanged by the extra work."""
    torch.manual_seed(7)
    H, B = 32, 2
    assert hip.fused_up_conv_chains(C)
    y_lo = torch.randn(B, C, H, H, device=DEV)
    fir = cu(torch.tensor([1.0, 3.0, 3.0, 1.0]).outer(torch.tensor([1.0, 3.0, 3.0, 1.0])) / 16.0)
    n1, n2 = torch.randn(1, 1, 2 * H, 2 * H, device=DEV), torch.randn(B, 1, 2 * H, 2 * H, device=DEV)
    nw1, nw2 = torch.full((1,), 0.3, device=DEV), torch.full((1,), -0.2, device=DEV)
    b1, b2 = torch.randn(C, device=DEV) * 0.2, torch.randn(C, device=DEV) * 0.2
    W2, Wn, Wr = torch.randn(C, C, device=DEV), torch.randn(C // 2, C, device=DEV), torch.randn(3, C, device=DEV)
    s2, sn, sr = (torch.randn(B, C, device=DEV) * 0.3 + 1 for _ in range(3))
    def _mod_flags(W, s, flags):
        from cips_3dplusplus_amd import _lib
        out = torch.empty(B * W.shape[0] * C, device=DEV)
        _lib.check(_lib.load().cips3d_modulate_weights(W.data_ptr(), s.data_ptr(), C, out.data_ptr(), B, W.shape[0], C, 1,
                                                       1.0 / math.sqrt(C), flags, torch.cuda.current_stream().cuda_stream), "mod")
        return out

    wm2 = _mod_flags(W2, s2, hip.MOD_DEMODULATE | hip.MOD_PACKED)
    wmn_std = _mod_flags(Wn, sn, hip.MOD_DEMODULATE | hip.MOD_PACKED)
    wmn_chn = _mod_flags(Wn, sn, hip.MOD_DEMODULATE | hip.MOD_PACKED | hip.MOD_CHAINED)
    wmr = _mod_flags(Wr, sr, 0)
    brgb = torch.randn(3, device=DEV) * 0.1
    skip = torch.randn(B, 3, H, H, device=DEV)
    out2, rgb = hip.fused_up_conv(y_lo, fir, n1, nw1, b1, wm2, n2, nw2, b2, wmr, brgb, skip, skip_up=True, bf16=bf16)
    ref = hip.modconv1x1(out2, wmn_std, C // 2, epilogue=0, bf16=bf16)
    o2, rgb2, y_next = hip.fused_up_conv(y_lo, fir, n1, nw1, b1, wm2, n2, nw2, b2, wmr, brgb, skip, skip_up=True, bf16=bf16,
                                         wm_next=wmn_chn)
    assert torch.equal(o2, out2) and torch.equal(rgb2, rgb)
    assert maxdiff(y_next, ref) < 2e-6 * float(ref.abs().max())
    # activations not stored at all
    _, rgb3, y3 = hip.fused_up_conv(y_lo, fir, n1, nw1, b1, wm2, n2, nw2, b2, wmr, brgb, skip, skip_up=True, bf16=bf16,
                                    wm_next=wmn_chn, want_out2=False)
    assert torch.equal(rgb3, rgb) and torch.equal(y3, y_next)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16_storage"])
def test_full_size_forward_repeats_bit_for_bit_at_batch_4(precision):
    """Sixty one-call forwards at 1024^2, batch 4 (fixed noise, no jitter) must produce the same bits: every kernel of the
    decoder runs with several workgroups per CU there, and the four fused up-sampling stages are compiled WITH hipcc's SLP
    vectoriser (v_pk_*_f32 in their FIR / epilogue arithmetic).  The planes kernels (csrc/chain.hip) once differed from run to
    run in exactly that situation when SLP had packed their ToRGB fold (profiles/r04_pk_fold_probe.txt, profiles/r05_slp_fold_cause.md:
    a property of that build's code, not of v_pk_fma_f32 -- the same pattern written by hand repeats); this is the tripwire for
    the rest of the decoder."""
    from cips_3dplusplus_amd.camera import Camera
    cfg = configs.ffhq_G_cfg(1024, 2)
    G = pkg.build_generator(cfg, DEV, seed=2)
    G.set_decoder_precision(precision)
    B = 4
    g = torch.Generator(device=DEV).manual_seed(5)
    zs = [torch.randn(B, 256, device=DEV, generator=g), torch.randn(B, 256, device=DEV, generator=g)]
    locs = torch.randn(B, 2, device=DEV, generator=g) * 0.2
    e, f, n, fa, _ = Camera.generate_camera_params(64, DEV, locations=locs)
    nb = [torch.randn(b.shape, device=DEV, generator=g) for b in G.create_noise_bufs(64, DEV)]
    kw = dict(zs=zs, cam_poses=e, focals=f, img_size=64, near=n, far=fa, noise_bufs=nb,
              nerf_cfg=dict(N_samples=24, perturb=False, static_viewdirs=False))
    with torch.no_grad():
        first = G(**kw)
        first = {k: first[k].clone() for k in ("rgb", "thumb_rgb")}
        assert bool(torch.isfinite(first["rgb"]).all())
        for rep in range(59):
            out = G(**kw)
            for k, v in first.items():
                assert torch.equal(out[k], v), (precision, rep, k, int((out[k] != v).sum()))


@pytest.mark.parametrize("bf16", [False, True])
def test_chained_stages_equal_unchained_full_size(bf16):
    """The one-call forward with every up-sampling stage computing the next stage's low-res GEMM (plan.CHAIN_STAGES) against
    the same forward with one GEMM launch per stage: same arithmetic up to the split-K / exchange summation order."""
    from cips_3dplusplus_amd import plan as _plan
    G = pkg.build_generator(configs.ffhq_G_cfg(1024, 2), DEV, seed=4)
    G.set_decoder_precision("bf16" if bf16 else "fp32")
    g = torch.Generator(device=DEV).manual_seed(9)
    B = 2
    zs = [torch.randn(B, 256, device=DEV, generator=g) for _ in range(2)]
    e, f, n, fa, _ = Camera.generate_camera_params(64, DEV, locations=torch.tensor([[0.2, 0.05], [-0.4, -0.1]], device=DEV))
    nb = G.create_noise_bufs(64, DEV)
    kw = dict(zs=zs, cam_poses=e, focals=f, img_size=64, near=n, far=fa, noise_bufs=nb,
              nerf_cfg=dict(N_samples=24, perturb=False, static_viewdirs=False))
    old = _plan.CHAIN_STAGES
    try:
        _plan.CHAIN_STAGES = True
        G._plans = {}
        a = G(**kw)["rgb"].clone()
        assert any(L.flags & 1 for L in list(G._plans.values())[0].plan.layers[: list(G._plans.values())[0].plan.n_dec_layers])
        _plan.CHAIN_STAGES = False
        G._plans = {}
        b = G(**kw)["rgb"].clone()
        assert not any(L.flags & 1 for L in list(G._plans.values())[0].plan.layers[: list(G._plans.values())[0].plan.n_dec_layers])
    finally:
        _plan.CHAIN_STAGES = old
        G._plans = {}
    tol = (2e-2 if bf16 else 2e-5) * float(b.abs().max())
    assert maxdiff(a, b) < tol


def test_rgb_to_uint8():
    x = torch.randn(2, 3, 37, 41) * 0.8
    x[0, 0, 0, :4] = torch.tensor([-1.0, 1.0, -3.0, 3.0])
    y = hip.rgb_to_uint8(cu(x)).cpu()
    ref = ((x.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8)
    assert y.dtype == torch.uint8 and y.shape == x.shape
    assert int((y.int() - ref.int()).abs().max()) <= 1     # ties may round differently by one ulp of the product
    assert float((y != ref).float().mean()) < 1e-3


# ------------------------------------------------------------------------------------------ Render.* stand-alone steps
def test_render_class_vs_oracle():
    """nerf_utils.Render.{get_rays_in_world,get_z_vals,get_points,normalize_points,prepare_nerf_inputs} vs the oracle."""
    from cips_3dplusplus_amd.nerf_utils import Render
    g = torch.Generator().manual_seed(4)
    B, S, N = 3, 12, 7
    cam = O.camera_params(torch.tensor([[0.3, 0.1], [-0.9, -0.2], [0.0, 0.4]]), S, 9, 0.12)
    for static in (False, True):
        ro, rd, vd = O.rays_in_world(cam[1], S, cam[0], static)
        o, d, v = Render.get_rays_in_world(cu(cam[1]), S, cu(cam[0]), static_viewdirs=static)
        assert o.shape == (B, S, S, 3)
        assert maxdiff(o.cpu(), ro) < 1e-6 and maxdiff(d.cpu(), rd) < 1e-6 and maxdiff(v.cpu(), vd) < 1e-6
    u = torch.rand(B, S, S, 1, generator=g)
    for pu in (None, u):
        zr = O.z_vals(cam[2], cam[3], B, S, S, N, pu)
        z = Render.get_z_vals(cu(cam[2]), cu(cam[3]), d, N, perturb=pu is not None, perturb_u=None if pu is None else cu(pu))
        assert z.shape == (B, S, S, N) and maxdiff(z.cpu(), zr) < 2e-7
    z = Render.get_z_vals(cu(cam[2]), cu(cam[3]), d, N, perturb=True)          # RNG site: one uniform per ray
    lo = O.z_vals(cam[2], cam[3], B, S, S, N, torch.zeros(B, S, S, 1))
    hi = O.z_vals(cam[2], cam[3], B, S, S, N, torch.ones(B, S, S, 1))
    assert bool((z.cpu() >= lo - 1e-6).all()) and bool((z.cpu() <= hi + 1e-6).all())
    pr = O.ray_points(ro, rd, zr)
    pts = Render.get_points(o, d, cu(zr))
    assert pts.shape == (B, S, S, N, 3) and maxdiff(pts.cpu(), pr) < 1e-6
    assert maxdiff(Render.normalize_points(pts, cu(cam[2]), cu(cam[3])).cpu(), O.normalize_points(pr, cam[2], cam[3])) < 1e-5
    p2, d2, v2, z2 = Render.prepare_nerf_inputs(cu(cam[1]), S, cu(cam[0]), cu(cam[2]), cu(cam[3]), N, perturb=True,
                                                static_viewdirs=True, perturb_u=cu(u))
    assert maxdiff(p2.cpu(), O.ray_points(ro, rd, O.z_vals(cam[2], cam[3], B, S, S, N, u))) < 1e-6
    assert maxdiff(v2.cpu(), vd) < 1e-6


@pytest.mark.parametrize("n,N,C", [(37, 6, 32), (130, 24, 256), (5, 1, 8)])
def test_volume_integration_vs_oracle(n, N, C):
    from cips_3dplusplus_amd.nerf_utils import Render
    g = torch.Generator().manual_seed(n + N)
    rgb, sdf, feat = torch.randn(2, n, N, 3, generator=g), 0.3 * torch.randn(2, n, N, 1, generator=g), \
        torch.randn(2, n, N, C, generator=g)
    z = torch.sort(torch.rand(2, n, N, generator=g) * 0.24 + 0.88, dim=-1).values
    rays_d, pts = torch.randn(2, n, 3, generator=g), torch.randn(2, n, N, 3, generator=g)
    beta = torch.tensor([0.1])
    ref = O.volume_integration(rgb, sdf, feat, z, rays_d, pts, beta)
    out = Render.volume_integration(cu(rgb), cu(sdf), cu(feat), cu(z), cu(rays_d), cu(pts), sigmoid_beta=cu(beta))
    assert out[4] is None
    for a, b, name in zip((out[0], out[1], out[2], out[3]), ref, ("rgb_map", "feature_map", "xyz", "mask")):
        assert a.shape == b.shape, name
        assert maxdiff(a.cpu(), b) < 2e-5 * max(1.0, float(b.abs().max())), name
    out = Render.volume_integration(cu(rgb), cu(sdf), None, cu(z), cu(rays_d), cu(pts), sigmoid_beta=0.1)
    assert out[1] is None and maxdiff(out[0].cpu(), ref[0]) < 2e-5


@pytest.mark.parametrize("hidden,D,R,N", [(32, 2, 50, 5), (256, 2, 64, 6), (32, 3, 129, 8), (256, 2, 100, 8), (64, 2, 37, 16)])
def test_renderer_explicit_points_entry_vs_oracle(hidden, D, R, N):
    """VolumeFeatureRenderer.forward(pts, rays_d, viewdirs, z_vals, near, far, styles): the reference entry with
    caller-made geometry (arbitrary ray count, rays that come from no camera)."""
    cfg = configs.tiny_G_cfg(hidden, D, 1) if hidden < 256 else configs.ffhq_G_cfg(256, D)
    G = pkg.build_generator(cfg, DEV, seed=2)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(R)
    B = 2
    S_dim = cfg["mapping_renderer_cfg"]["style_dim"]
    rays_o = 0.2 * torch.randn(B, R, 3, generator=g) + torch.tensor([0.0, 0.0, 1.0])
    rays_d = torch.randn(B, R, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -1.0])
    viewdirs = rays_d / rays_d.norm(dim=-1, keepdim=True)
    z = torch.sort(torch.rand(B, R, N, generator=g) * 0.24 + 0.88, dim=-1).values
    pts = rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z.unsqueeze(-1)
    near, far = torch.full((B, 1, 1), 0.88), torch.full((B, 1, 1), 1.12)
    styles = 0.5 * torch.randn(B, D + 1, S_dim, generator=g)
    ref = O.renderer_forward(sd, "renderer", pts, rays_d, viewdirs, z, near, far, styles, D)   # rgb, feat, sdf, mask, xyz
    out = G.renderer(cu(pts), cu(rays_d), cu(viewdirs), cu(z), cu(near), cu(far), styles=cu(styles))
    assert out[5] is None
    tol = 1e-4 if hidden == 256 else 3e-5
    for a, b, name in zip(out[:5], ref, ("rgb_map", "feature_map", "sdf", "mask", "xyz")):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        assert maxdiff(a.cpu(), b) < tol * max(1.0, float(b.abs().max())), name
    if hidden == 256:       # the exact-fp32 instantiation of the explicit-geometry kernel (csrc/nerf.hip: <.., XG, .., F32>)
        G.renderer.set_precision("fp32_exact")
        out_x = G.renderer(cu(pts), cu(rays_d), cu(viewdirs), cu(z), cu(near), cu(far), styles=cu(styles))
        G.renderer.set_precision("fp32")
        for a, b, name in zip(out_x[:5], ref, ("rgb_map", "feature_map", "sdf", "mask", "xyz")):
            assert maxdiff(a.cpu(), b) < tol * max(1.0, float(b.abs().max())), name
        assert not torch.equal(out_x[1], out[1])            # another arithmetic really ran
    # (b, h, w, ...) input layout
    if R == 64:
        o4 = G.renderer(cu(pts).view(B, 8, 8, N, 3), cu(rays_d).view(B, 8, 8, 3), cu(viewdirs).view(B, 8, 8, 3),
                        cu(z).view(B, 8, 8, N), cu(near), cu(far), styles=cu(styles))
        assert o4[1].shape == (B, 8, 8, hidden) and torch.equal(o4[1].reshape(B, R, hidden), out[1])


def test_per_point_module_forwards_vs_oracle():
    """FiLMSiren.forward / LinearLayer.forward on point tensors / SirenGenerator.points_forward / run_network, and the
    piecewise pipeline of the reference (prepare_nerf_inputs -> normalize -> run_network -> volume_integration) against the
    oracle and against the fused kernel."""
    from cips_3dplusplus_amd.nerf_utils import Render
    cfg = configs.tiny_G_cfg(32, 3, 1)
    G = pkg.build_generator(cfg, DEV, seed=6)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    net = G.renderer.network
    g = torch.Generator().manual_seed(12)
    B, S, N, D = 2, 6, 5, 3
    styles = 0.5 * torch.randn(B, D + 1, 32, generator=g)
    x3 = torch.randn(B, S * S, N, 3, generator=g)
    # one FiLM layer, K = 3 / 32 / 35 (first, hidden, view)
    y = net.pts_linears[0](cu(x3), cu(styles[:, 0]))
    assert maxdiff(y.cpu(), O.film_siren(sd, "renderer.network.pts_linears.0", x3, styles[:, 0])) < 2e-5
    xh = torch.randn(B, S, S, N, 32, generator=g)
    y = net.pts_linears[1](cu(xh), cu(styles[:, 1]))
    assert y.shape == (B, S, S, N, 32)
    assert maxdiff(y.cpu(), O.film_siren(sd, "renderer.network.pts_linears.1", xh, styles[:, 1])) < 2e-5
    xv = torch.randn(B, S * S, N, 35, generator=g)
    y = net.views_linears(cu(xv), cu(styles[:, -1]))
    assert maxdiff(y.cpu(), O.film_siren(sd, "renderer.network.views_linears", xv, styles[:, -1])) < 2e-5
    s1 = net.sigma_linear(cu(xh))
    assert s1.shape == (B, S, S, N, 1) and maxdiff(s1.cpu(), O._affine(sd, "renderer.network.sigma_linear", xh)) < 1e-5
    # whole per-point network
    cam = O.camera_params(torch.tensor([[0.2, 0.1], [-0.5, 0.0]]), S, 6, 0.12)
    pts, rays_d, viewdirs, z = Render.prepare_nerf_inputs(cu(cam[1]), S, cu(cam[0]), cu(cam[2]), cu(cam[3]), N, perturb=False)
    ptsn = Render.normalize_points(pts, cu(cam[2]), cu(cam[3]))
    rgb, sdf, feat = G.renderer.run_network(ptsn, viewdirs, styles=cu(styles))
    ref = O.siren_points(sd, "renderer.network", ptsn.cpu(), viewdirs.cpu(), styles, D)
    for a, b, name in zip((rgb, sdf, feat), ref, ("rgb", "sdf", "feat")):
        assert a.shape == b.shape and maxdiff(a.cpu(), b) < 5e-5 * max(1.0, float(b.abs().max())), name
    piece = Render.volume_integration(rgb, sdf, feat, z, rays_d, pts, sigmoid_beta=G.renderer.sigmoid_beta)
    fused = G.renderer(pts, rays_d, viewdirs, z, cu(cam[2]), cu(cam[3]), styles=cu(styles))
    for a, b, name in ((piece[0], fused[0], "rgb_map"), (piece[1], fused[1], "feature_map"), (piece[2], fused[4], "xyz"),
                       (piece[3], fused[3], "mask")):
        assert a.shape == b.shape and maxdiff(a, b) < 5e-5 * max(1.0, float(b.abs().max())), name


def test_mapping_modules_callable_like_the_reference():
    """`G.style(z)` / `G.style_decoder(z)` as plain module calls (projector_v10.py:313-315,351-353 computes the W means this
    way with 10 000 rows), `get_ws`, `mapping_networks` with truncation."""
    cfg = configs.tiny_G_cfg(32, 2, 1)
    G = pkg.build_generator(cfg, DEV, seed=4)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    z = torch.randn(300, 32, generator=g)
    wr = G.style(cu(z))
    wd = G.style_decoder(cu(z))
    ref_r = O.mapping_renderer(sd, cfg, z)[:, 0]
    ref_d = O.mapping_decoder(sd, cfg, z)[:, 0]
    assert maxdiff(wr.cpu(), ref_r) < 2e-5 and maxdiff(wd.cpu(), ref_d) < 2e-5
    mr, md = wr.mean(0, keepdim=True), wd.mean(0, keepdim=True)
    G.style_render_mean, G.style_decoder_mean = mr, md
    z2 = [cu(torch.randn(2, 32, generator=g)), cu(torch.randn(2, 32, generator=g))]
    s_r, s_d = G.mapping_networks(zs=z2, truncation=0.6, inject_index=None)
    assert maxdiff(s_r.cpu(), O.mapping_renderer(sd, cfg, z2[0].cpu(), 0.6, mr.cpu())) < 2e-5
    assert maxdiff(s_d.cpu(), O.mapping_decoder(sd, cfg, z2[1].cpu(), 0.6, md.cpu())) < 2e-5
    assert s_r.shape == (2, 3, 32) and s_d.shape == (2, G.decoder.n_latent, 32)
    assert G.z_dim == 32 and G.N_layers_renderer == 2 and "decoder" in G.module_name_list and "style" in G.module_name_list


def test_forward_is_graph_capturable():
    """cips3d_generator_forward neither allocates nor synchronises: the whole forward can be captured into a HIP graph and
    replayed bit-identically (a property, not a speed-up: replays do not overlap across streams the way eager lanes do)."""
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=9)
    e, f, n, fa, _ = Camera.generate_camera_params(8, DEV, locations=torch.tensor([[0.2, -0.1]], device=DEV))
    zs = [torch.randn(1, 32, device=DEV), torch.randn(1, 32, device=DEV)]
    nb = G.create_noise_bufs(8, DEV)
    u = torch.rand(1, 8, 8, 1, device=DEV)

    def fwd():
        return G(zs=zs, cam_poses=e, focals=f, img_size=8, near=n, far=fa, noise_bufs=nb, perturb_u=u,
                 nerf_cfg=dict(N_samples=6, perturb=True, static_viewdirs=False))["rgb"]

    ref = fwd().clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    zs[0].add_(0.5)                      # new latent in the captured input buffer -> replay renders the new view
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, fwd())


# ------------------------------------------------------------------------------------------ bf16 decoder mode (config 3)
def _psnr(a, b):
    mse = float(((a - b) ** 2).mean())
    peak = float(b.max() - b.min())
    return 10.0 * math.log10(peak * peak / max(mse, 1e-30))


@pytest.mark.parametrize("cin,cout,hw,up,B", [(32, 32, 16, False, 2), (64, 32, 16, True, 1), (512, 512, 8, False, 1),
                                               (128, 128, 16, True, 2), (256, 256, 16, True, 1)])
def test_bf16_gemm_mode_vs_bf16_oracle(cin, cout, hw, up, B):
    """bf16 compute mode of StyledConv (operands rounded to bf16, fp32 accumulate) vs the oracle with the same rounding."""
    import cips_3dplusplus_amd.decoder as dec
    torch.manual_seed(cin + cout + hw + 1)
    sc = dec.StyledConv(cin, cout, 1, 64, upsample=up)
    sc.noise.weight.data.fill_(0.3)
    sc.activate.bias.data = torch.randn(cout) * 0.2
    sd = {"m." + k: v.clone() for k, v in sc.state_dict().items()}
    x, st = torch.randn(B, cin, hw, hw), torch.randn(B, 64)
    ho = 2 * hw if up else hw
    nz = torch.randn(1, 1, ho, ho)
    sc = sc.to(DEV)
    sc.bf16 = True
    y = sc(cu(x), cu(st), noise=cu(nz))
    ref16 = O.styled_conv(sd, "m", x, st, nz, upsample=up, bf16_gemm=True)
    ref32 = O.styled_conv(sd, "m", x, st, nz, upsample=up)
    scale = max(1.0, float(ref32.abs().max()))
    # the device rounds the MODULATED weight to bf16 exactly like the oracle; what differs is the fp32 accumulation order
    # and, rarely, one-ulp ties of the fp32 modulation feeding the rounding
    assert maxdiff(y.cpu(), ref16) < 2e-3 * scale
    assert float((y.cpu() - ref16).abs().mean()) < 5e-5 * scale
    assert maxdiff(y.cpu(), ref32) > 1e-4 * scale           # and it is really the reduced-precision path
    assert _psnr(y.cpu(), ref32) > 40.0


def test_bf16_decoder_generator(golden):
    """Config 3 semantics on the tiny and the 256^2 generator: planned path == per-op path; close to the bf16 oracle;
    PSNR against the exact fp32 result reported and bounded."""
    fx, tag = golden("tiny_generator"), "h32_d2"
    cfg = _tiny_cfg(tag)
    G = pkg.build_generator(cfg, DEV, state_dict=fx.sub(f"{tag}.sd."))
    zs = [cu(fx[f"{tag}.z0"]), cu(fx[f"{tag}.z1"])]
    e, f, n, fa, _ = Camera.generate_camera_params(8, DEV, locations=cu(fx[f"{tag}.locs"]))
    nb = [cu(fx[f"{tag}.noise{i}"]) for i in range(G.decoder.num_layers)]
    ncfg = dict(N_samples=6, perturb=False, static_viewdirs=False)
    r32 = G(zs=zs, cam_poses=e, focals=f, img_size=8, near=n, far=fa, noise_bufs=nb, nerf_cfg=ncfg)["rgb"].clone()
    G.set_decoder_precision("bf16")
    r16 = G(zs=zs, cam_poses=e, focals=f, img_size=8, near=n, far=fa, noise_bufs=nb, nerf_cfg=ncfg)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    cam = O.camera_params(fx[f"{tag}.locs"], 8, 6, 0.12)
    ref16 = O.generator_forward(sd, cfg, [z.cpu() for z in zs], cam[0], cam[1], 8, cam[2], cam[3], ncfg,
                                [b.cpu() for b in nb], bf16_decoder=True)
    scale = float(ref16["rgb"].abs().max())
    assert maxdiff(r16["rgb"].cpu(), ref16["rgb"]) < 5e-3 * scale
    assert maxdiff(r16["thumb_rgb"].cpu(), ref16["thumb_rgb"]) < 1e-5          # the renderer stays fp32
    assert _psnr(r16["rgb"], r32) > 35.0 and not torch.equal(r16["rgb"], r32)
    # planned (one-call) path and per-op path agree in bf16 mode too
    s_r, s_d = G.mapping_networks(zs=zs, truncation=1, inject_index=None)
    thumb, feats, _, _, _ = G.renderer.render(e, f, n, fa, s_r, 8, 6)
    per_op = G.decoder(features=feats, styles=s_d, noise=nb)
    assert maxdiff(per_op, r16["rgb"]) < 2e-4 * scale
    G.set_decoder_precision("fp32")
    assert torch.equal(G(zs=zs, cam_poses=e, focals=f, img_size=8, near=n, far=fa, noise_bufs=nb, nerf_cfg=ncfg)["rgb"], r32)
    # release-size generator, batch 4 (the configuration of BASELINE config 3 at 256^2 to keep the test short)
    G2 = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=1)
    g = torch.Generator(device=DEV).manual_seed(5)
    z2 = [torch.randn(4, 256, device=DEV, generator=g), torch.randn(4, 256, device=DEV, generator=g)]
    e2, f2, n2, fa2, _ = Camera.generate_camera_params(64, DEV, locations=0.3 * torch.randn(4, 2, device=DEV, generator=g))
    nb2 = G2.create_noise_bufs(64, DEV)
    kw = dict(zs=z2, cam_poses=e2, focals=f2, img_size=64, near=n2, far=fa2, noise_bufs=nb2,
              nerf_cfg=dict(N_samples=24, perturb=False, static_viewdirs=False))
    a32 = G2(**kw)["rgb"].clone()
    G2.set_decoder_precision("bf16")
    a16 = G2(**kw)["rgb"]
    psnr = _psnr(a16, a32)
    print(f"bf16 decoder vs fp32, 256^2 B=4: PSNR {psnr:.1f} dB, max-abs {maxdiff(a16, a32):.3e} on range {float(a32.abs().max()):.2f}")
    assert psnr > 35.0


@pytest.mark.parametrize("hidden,D,S,N,B,static,perturb,trunc", [
    (64, 2, 8, 5, 3, False, True, 1.0), (128, 3, 12, 7, 1, True, False, 0.7), (32, 1, 16, 1, 2, False, False, 1.0),
    (64, 4, 20, 9, 2, True, True, 0.5), (32, 2, 4, 24, 5, False, True, 1.0), (32, 2, 5, 3, 2, False, False, 1.0),
    (32, 2, 7, 4, 1, True, True, 0.8)])
def test_generator_shape_sweep_vs_oracle(hidden, D, S, N, B, static, perturb, trunc):
    """Widths / depths / ray-grid sizes / sample counts / batch sizes off the released recipe: whole generator vs oracle."""
    cfg = configs.tiny_G_cfg(hidden, D, 1)
    G = pkg.build_generator(cfg, DEV, seed=hidden + D)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(S * N + B)
    zs = [torch.randn(B, hidden, generator=g), torch.randn(B, hidden, generator=g)]
    locs = torch.stack([0.5 * torch.randn(B, generator=g), 0.2 * torch.randn(B, generator=g)], 1)
    nb = [torch.randn(*b.shape, generator=g) for b in G.create_noise_bufs(S, "cpu")]
    mr, md = 0.2 * torch.randn(1, hidden, generator=g), 0.2 * torch.randn(1, 32, generator=g)
    u = torch.rand(B, S, S, 1, generator=g) if perturb else None
    ncfg = dict(N_samples=N, perturb=perturb, static_viewdirs=static)
    G.style_render_mean, G.style_decoder_mean = cu(mr), cu(md)
    e, f, n, fa, _ = Camera.generate_camera_params(S, DEV, locations=cu(locs), fov_ang=12, dist_radius=0.3)
    r = G(zs=[cu(z) for z in zs], cam_poses=e, focals=f, img_size=S, near=n, far=fa, noise_bufs=[cu(b) for b in nb],
          truncation=trunc, nerf_cfg=ncfg, return_sdf=True, return_xyz=True, perturb_u=None if u is None else cu(u))
    cam = O.camera_params(locs, S, 12, 0.3)
    ref = O.generator_forward(sd, cfg, zs, cam[0], cam[1], S, cam[2], cam[3], ncfg, nb, truncation=trunc,
                              style_render_mean=mr, style_decoder_mean=md, perturb_u=u, return_sdf=True, return_xyz=True)
    for k in ("rgb", "thumb_rgb", "sdf", "xyz", "mask", "depth"):
        assert r[k].shape == ref[k].shape, k
        assert maxdiff(r[k].cpu(), ref[k]) < 2e-4 * max(1.0, float(ref[k].abs().max())), k


@pytest.mark.parametrize("hidden,D,S,N", [(32, 2, 8, 6), (256, 2, 16, 24)])
def test_generator_with_raw_density_vs_oracle(hidden, D, S, N):
    """renderer_cfg.with_sdf = False through the whole generator (the one-call plan and the per-op path): the sigma head is a
    raw density (nerf_utils.py:288-297).  The image must also differ from the sdf reading of the same weights."""
    cfg = configs.tiny_G_cfg(hidden, D, 1) if hidden < 256 else configs.ffhq_G_cfg(256, D)
    cfg["renderer_cfg"] = dict(cfg["renderer_cfg"], with_sdf=False)
    G = pkg.build_generator(cfg, DEV, seed=11)
    assert G.renderer.with_sdf is False
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    B = 2
    zs = [torch.randn(B, G.z_dim, generator=g), torch.randn(B, G.z_dim, generator=g)]
    locs = torch.tensor([[0.4, 0.1], [-0.3, -0.15]])
    nb = [torch.randn(*b.shape, generator=g) for b in G.create_noise_bufs(S, "cpu")]
    ncfg = dict(N_samples=N, perturb=False, static_viewdirs=False)
    e, f, n, fa, _ = Camera.generate_camera_params(S, DEV, locations=cu(locs), fov_ang=12, dist_radius=0.12)
    cam = O.camera_params(locs, S, 12, 0.12)
    ref = O.generator_forward(sd, cfg, zs, cam[0], cam[1], S, cam[2], cam[3], ncfg, nb, return_sdf=True, return_xyz=True)
    kw = dict(zs=[cu(z) for z in zs], cam_poses=e, focals=f, img_size=S, near=n, far=fa, noise_bufs=[cu(b) for b in nb],
              nerf_cfg=ncfg, return_sdf=True, return_xyz=True)
    r = G(**kw)
    for k in ("rgb", "thumb_rgb", "sdf", "xyz", "mask", "depth"):
        assert r[k].shape == ref[k].shape, k
        assert maxdiff(r[k].cpu(), ref[k]) < 2e-4 * max(1.0, float(ref[k].abs().max())), k
    G.renderer.with_sdf = True                   # part of the plan's key: the one-call plan is re-made
    other = G(**kw)
    assert maxdiff(other["thumb_rgb"].cpu(), ref["thumb_rgb"]) > 1e-3


def test_full_size_properties():
    """Size-independent properties at the BASELINE size (1024^2, D=2, N=24), where the oracle is too slow to run inside the
    GPU suite: batch elements are independent (B=2 == two B=1 calls to fp32 round-off), repeat runs are bitwise identical,
    compositing weights are probabilities, thumb_rgb is inside [-1,1], depth = -|xyz|, and the same forward through the
    per-op path agrees with the one-call plan."""
    cfg = configs.ffhq_G_cfg(1024, 2)
    G = pkg.build_generator(cfg, DEV, seed=0)
    g = torch.Generator(device=DEV).manual_seed(77)
    zs = [torch.randn(2, 256, device=DEV, generator=g), torch.randn(2, 256, device=DEV, generator=g)]
    locs = torch.tensor([[0.3, 0.1], [-0.5, -0.1]], device=DEV)
    e, f, n, fa, _ = Camera.generate_camera_params(64, DEV, locations=locs)
    nb = G.create_noise_bufs(64, DEV)
    u = torch.rand(2, 64, 64, 1, device=DEV, generator=g)
    ncfg = dict(N_samples=24, perturb=True, static_viewdirs=False)

    def run(sl):
        return G(zs=[z[sl] for z in zs], cam_poses=e[sl], focals=f[sl], img_size=64, near=n[sl], far=fa[sl], noise_bufs=nb,
                 perturb_u=u[sl], nerf_cfg=ncfg, return_xyz=True, return_sdf=True)

    both = {k: v.clone() for k, v in run(slice(0, 2)).items() if v is not None}
    again = run(slice(0, 2))
    for k in both:
        assert torch.equal(both[k], again[k]), f"{k}: repeat run differs"
    for b in range(2):
        one = run(slice(b, b + 1))
        for k in both:
            # not bitwise: the sample-chunk count of the NeRF kernel depends on B (fewer chunks per ray at larger B), so the
            # chunk partials are combined in a different association
            assert maxdiff(both[k][b:b + 1], one[k]) < 2e-5 * max(1.0, float(one[k].abs().max())), \
                f"{k}: batch element {b} depends on its neighbours"
    assert float(both["thumb_rgb"].abs().max()) <= 1.0 + 1e-6
    assert float(both["mask"].min()) >= 0.0 and float(both["mask"].max()) <= 1.0 + 1e-6
    assert maxdiff(both["depth"], -both["xyz"].norm(dim=1, keepdim=True)) < 1e-6
    assert both["rgb"].shape == (2, 3, 1024, 1024) and bool(torch.isfinite(both["rgb"]).all())
    # per-op path (module by module, python launches) == one-call planned path
    s_r, s_d = G.mapping_networks(zs=zs, truncation=1, inject_index=None)
    thumb, feats, _, _, _ = G.renderer.render(e, f, n, fa, s_r, 64, 24, perturb_u=u)
    assert torch.equal(thumb, both["thumb_rgb"])
    rgb_ops = G.decoder(features=feats, styles=s_d, noise=nb)
    assert maxdiff(rgb_ops, both["rgb"]) < 2e-4 * float(both["rgb"].abs().max())


def test_config4_shape_n128_static_truncated():
    """BASELINE config 4's per-view shape (the reference demo's: 1024^2, N = 128 samples, static view directions, truncation 0.5
    with preset means, return_xyz -- render_video_web_v10.py:1806-1824): the NeRF half against the oracle on a strided subset
    of the rays (explicit-points entry of the same fused kernel), and size-independent properties of the whole forward: the
    fused render == Render.prepare_nerf_inputs + rays_forward, two batch elements independent, repeat bitwise."""
    from cips_3dplusplus_amd.nerf_utils import Render
    cfg = configs.ffhq_G_cfg(1024, 2)
    G = pkg.build_generator(cfg, DEV, seed=3)
    g = torch.Generator(device=DEV).manual_seed(5)
    zs = [torch.randn(2, 256, device=DEV, generator=g), torch.randn(2, 256, device=DEV, generator=g)]
    G.style_render_mean = 0.1 * torch.randn(1, 256, device=DEV, generator=g)
    G.style_decoder_mean = 0.1 * torch.randn(1, 512, device=DEV, generator=g)
    locs = torch.tensor([[0.77, 0.0], [-0.4, 0.0]], device=DEV)             # the yaw sweep's extreme and an inner frame
    e, f, n, fa, _ = Camera.generate_camera_params(64, DEV, locations=locs)
    nb = G.create_noise_bufs(64, DEV)
    ncfg = dict(N_samples=128, perturb=False, static_viewdirs=True)
    kw = dict(zs=zs, cam_poses=e, focals=f, img_size=64, near=n, far=fa, noise_bufs=nb, truncation=0.5, nerf_cfg=ncfg,
              return_xyz=True, return_sdf=True)
    both = {k: v.clone() for k, v in G(**kw).items() if v is not None}
    again = G(**kw)
    assert all(torch.equal(both[k], again[k]) for k in both)
    assert both["sdf"].shape == (2, 64, 64, 128, 1) and both["rgb"].shape == (2, 3, 1024, 1024)
    assert bool(torch.isfinite(both["rgb"]).all()) and float(both["thumb_rgb"].abs().max()) <= 1.0 + 1e-6
    for b in range(2):
        one = G(**{**kw, "zs": [z[b:b + 1] for z in zs], "cam_poses": e[b:b + 1], "focals": f[b:b + 1], "near": n[b:b + 1],
                   "far": fa[b:b + 1]})
        for k in both:
            assert maxdiff(both[k][b:b + 1], one[k]) < 3e-5 * max(1.0, float(one[k].abs().max())), k
    # the NeRF half against the oracle on every 37th ray (N = 128 makes the full grid slow on the CPU)
    s_r, _ = G.mapping_networks(zs=zs, truncation=0.5, inject_index=None)
    pts, rd, vd, zz = Render.prepare_nerf_inputs(f, 64, e, n, fa, N_samples=128, perturb=False, static_viewdirs=True)
    idx = torch.arange(0, 4096, 37, device=DEV)
    sub = lambda t: t.reshape(2, 4096, *t.shape[3:])[:, idx].contiguous()     # noqa: E731
    out = G.renderer(sub(pts), sub(rd), sub(vd), sub(zz), n, fa, styles=s_r)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    ref = O.renderer_forward(sd, "renderer", sub(pts).cpu(), sub(rd).cpu(), sub(vd).cpu(), sub(zz).cpu(), n.cpu(), fa.cpu(),
                             s_r.cpu(), 2)
    for a, r, k in zip(out[:5], ref, ("rgb_map", "feature_map", "sdf", "mask", "xyz")):
        assert maxdiff(a.cpu(), r) < 1e-4 * max(1.0, float(r.abs().max())), k
    thumb = both["thumb_rgb"].reshape(2, 3, 4096)[:, :, idx].transpose(1, 2)
    assert maxdiff(thumb.cpu(), ref[0]) < 1e-4                                # the camera-driven kernel == the explicit entry


def test_generator_rays_forward_equals_fused_forward():
    """Generator.rays_forward on Render.prepare_nerf_inputs == the NeRF half of Generator.forward (the reference's own
    decomposition, model_v3.py:941-1003)."""
    from cips_3dplusplus_amd.nerf_utils import Render
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=8)
    B, S, N = 2, 8, 6
    e, f, n, fa, _ = Camera.generate_camera_params(S, DEV, locations=torch.tensor([[0.3, 0.1], [-0.2, 0.0]], device=DEV))
    zs = [torch.randn(B, 32, device=DEV), torch.randn(B, 32, device=DEV)]
    nb = G.create_noise_bufs(S, DEV)
    full = G(zs=zs, cam_poses=e, focals=f, img_size=S, near=n, far=fa, noise_bufs=nb, return_xyz=True, return_sdf=True,
             nerf_cfg=dict(N_samples=N, perturb=False, static_viewdirs=False))
    s_r, s_d = G.mapping_networks(zs=zs, truncation=1, inject_index=None)
    pts, rays_d, viewdirs, z = Render.prepare_nerf_inputs(f, S, e, n, fa, N, perturb=False)
    flat = lambda t: t.reshape(B, S * S, *t.shape[3:])
    thumb, sdf, mask, xyz, feats, eik = G.rays_forward(None, flat(pts), flat(rays_d), flat(viewdirs), flat(z), n, fa, s_r)
    img = lambda t: t.transpose(1, 2).reshape(B, t.shape[-1], S, S)
    assert eik is None and feats.shape == (B, S * S, 32)
    assert maxdiff(img(thumb), full["thumb_rgb"]) < 2e-6 and maxdiff(img(xyz), full["xyz"]) < 2e-6
    assert maxdiff(img(mask)[:, 0:1], full["mask"]) < 2e-6 and maxdiff(sdf.view(B, S, S, N, 1), full["sdf"]) < 2e-6
    rgb = G.decoder(features=img(feats).contiguous(), styles=s_d, noise=nb)
    assert maxdiff(rgb, full["rgb"]) < 1e-4


def test_modconv1x1_torgb_fold_vs_oracle():
    """GEMM with the following ToRGB folded into its epilogue + the fixed-order reduction == StyledConv then ToRGB."""
    import ctypes as C
    from cips_3dplusplus_amd import _lib
    dec = _dec_mod()
    torch.manual_seed(31)
    B, cin, cout, hw = 2, 64, 128, 16
    sc = dec.StyledConv(cin, cout, 1, 32)
    sc.noise.weight.data.fill_(0.25)
    sc.activate.bias.data = torch.randn(cout) * 0.2
    tr = dec.ToRGB(cout, 32, upsample=False)
    tr.bias.data = torch.randn(1, 3, 1, 1)
    sd = {**{"c." + k: v.clone() for k, v in sc.state_dict().items()}, **{"t." + k: v.clone() for k, v in tr.state_dict().items()}}
    x, st, st2 = torch.randn(B, cin, hw, hw), torch.randn(B, 32), torch.randn(B, 32)
    nz, skip = torch.randn(1, 1, hw, hw), torch.randn(B, 3, hw, hw)
    y_ref = O.styled_conv(sd, "c", x, st, nz)
    rgb_ref = O.to_rgb(sd, "t", y_ref, st2, skip, upsample=False)
    sc, tr = sc.to(DEV), tr.to(DEV)
    wm = sc.conv.modulated_weight(cu(st), packed=True)
    wrgb = tr.conv.modulated_weight(cu(st2), packed=False)
    lib = _lib.load()
    out = torch.empty(B, cout, hw, hw, device=DEV)
    part = torch.empty(16, B, 3, hw, hw, device=DEV)
    nblk = C.c_int(0)
    xg, nzg = cu(x), cu(nz)
    _lib.check(lib.cips3d_modconv1x1_torgb(xg.data_ptr(), wm.data_ptr(), out.data_ptr(), B, cin, cout, hw * hw, 1, nzg.data_ptr(), 0,
                                           sc.noise.weight.data_ptr(), sc.activate.bias.data_ptr(), wrgb.data_ptr(),
                                           part.data_ptr(), C.byref(nblk), None, hip.stream_ptr()), "cips3d_modconv1x1_torgb")
    assert nblk.value == 1                      # Cout = 128 -> one 128-row block
    rgb = torch.empty(B, 3, hw, hw, device=DEV)
    biases = (C.c_void_p * 1)(tr.bias.data_ptr())
    skg = cu(skip)
    _lib.check(lib.cips3d_torgb_reduce(part.data_ptr(), nblk.value, biases, 1, skg.data_ptr(), rgb.data_ptr(), B, hw * hw,
                                       hip.stream_ptr()), "cips3d_torgb_reduce")
    assert maxdiff(out.cpu(), y_ref) < 3e-5 * max(1.0, float(y_ref.abs().max()))
    assert maxdiff(rgb.cpu(), rgb_ref) < 5e-5 * max(1.0, float(rgb_ref.abs().max()))


@pytest.mark.parametrize("B,hw,n_slots,with_skip,n_bias", [(1, 64, 40, True, 5), (1, 64, 8, True, 1), (2, 32, 5, False, 2),
                                                            (1, 16, 1, True, 0), (4, 64, 48, True, 6), (2, 16, 17, False, 1)])
def test_torgb_fold_riding_on_a_planes_gemm_equals_the_stand_alone_reduce(B, hw, n_slots, with_skip, n_bias):
    """cips3d_reduce_job: the ToRGB fold carried by a split-planes GEMM launch (the low-resolution GEMM of the first up-sampling
    stage in the one-call forward) writes the bits cips3d_torgb_reduce writes, and leaves the GEMM's own result untouched."""
    import ctypes as C
    from cips_3dplusplus_amd import _lib
    dec = _dec_mod()
    g = torch.Generator().manual_seed(B * 100 + hw + n_slots)
    cin, cout = 128, 64
    sc = dec.StyledConv(cin, cout, 1, 32).to(DEV)
    wm = sc.conv.modulated_weight(cu(torch.randn(B, 32, generator=g)), packed=True, split=True)
    xp = hip.to_planes(cu(torch.randn(B, cin, hw, hw, generator=g)))
    part = cu(torch.randn(n_slots, B, 3, hw * hw, generator=g))
    skip = cu(torch.randn(B, 3, hw * hw, generator=g)) if with_skip else None
    biases = [cu(torch.randn(3, generator=g)) for _ in range(n_bias)]
    ref = torch.empty(B, 3, hw * hw, device=DEV)
    lib = _lib.load()
    barr = (C.c_void_p * max(n_bias, 1))(*[b.data_ptr() for b in biases])
    _lib.check(lib.cips3d_torgb_reduce(part.data_ptr(), n_slots, barr, n_bias, skip.data_ptr() if with_skip else None, ref.data_ptr(),
                                       B, hw * hw, hip.stream_ptr()), "cips3d_torgb_reduce")
    y_plain = hip.modconv1x1_planes(xp, wm, cout, hw * hw, out_format="fp32")
    out = torch.full((B, 3, hw * hw), float("nan"), device=DEV)
    y_ride = hip.modconv1x1_planes(xp, wm, cout, hw * hw, out_format="fp32",
                                   ride=dict(part=part, biases=biases, skip=skip, out=out))
    assert torch.equal(out, ref)
    assert torch.equal(y_ride, y_plain)


def test_empty_and_degenerate_inputs():
    """Edge cases at the op boundary: empty batches are legal and launch nothing; single-sample rays; 1x1 images."""
    k = torch.tensor([[1., 3., 3., 1.]]).t() @ torch.tensor([[1., 3., 3., 1.]]) / 64
    y = op.fused_leaky_relu(torch.empty(0, 8, 4, 4, device=DEV), torch.zeros(8, device=DEV))
    assert y.shape == (0, 8, 4, 4)
    y = op.upfirdn2d(torch.empty(0, 3, 8, 8, device=DEV), cu(k), up=2, pad=(2, 1))
    assert y.shape == (0, 3, 16, 16)
    x = torch.randn(2, 3, 1, 1)
    y = op.upfirdn2d(cu(x), cu(k), up=2, pad=(2, 1))
    assert maxdiff(y.cpu(), O.upfirdn2d(x, k, 2, 1, (2, 1))) < 1e-6
    assert hip.rgb_to_uint8(torch.empty(0, 3, 4, 4, device=DEV)).shape == (0, 3, 4, 4)
    u8 = hip.rgb_to_uint8(torch.tensor([[-2.0, -1.0, 0.0, 0.5, 1.0, 3.0, float("-inf"), 1e-9]], device=DEV))
    assert u8.cpu().tolist() == [[0, 0, 128, 191, 255, 255, 0, 128]]          # clamp, round half to even on 127.5
    e, f, n, fa = hip.camera_params(torch.empty(0, 2, device=DEV), 64)
    assert e.shape == (0, 3, 4) and f.shape == (0, 1, 1)
