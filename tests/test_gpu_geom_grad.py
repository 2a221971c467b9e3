"""The gradient through the render's mask / depth / xyz maps (autograd.NerfRenderFn; cips3d_nerf_bwd_composite and
cips3d_nerf_bwd_camera of csrc/nerf_bwd.hip, reached by the fused and by the materialised backward) and the silhouette term
of the inversion loop, against torch autograd through the CPU oracle's volume_integration (oracle/path.py:150-171:
xyz = sum_k w_k p_k, mask = [w_last, -|xyz|]).  The harness is that of test_gpu_backward.py::test_nerf_render_bwd_vs_oracle."""
import ctypes
import functools

import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import _lib, autograd as AG, configs, hip, weights
from cips_3dplusplus_amd.camera import Camera
from oracle import path as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cu(t):
    return t.to(DEV).contiguous()


def close(a, b, rel=2e-4, what=""):
    a = a.detach().cpu().reshape(b.shape)
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / max(scale, 1e-30):.3e}")
    assert err <= rel * scale + 1e-6, f"{what}: err {err:.3e} vs scale {scale:.3e}"


def leaf(t):
    return t.clone().requires_grad_(True)


# ------------------------------------------------------------------------------------------------ 1. against the oracle
CASES = [(2, False, False, 6, 8), (3, True, True, 5, 8),
         (2, False, True, 2, 8),         # the smallest parallel case: the last sample is half the ray
         (2, False, True, 32, 8),        # the parallel kernel's upper edge
         (2, False, True, 36, 8)]        # the per-ray loop
TERMS = ("mask", "depth", "xyz", "all")


@functools.lru_cache(maxsize=None)
def _oracle_case(D, static, perturb, N, S):
    """One CPU-oracle graph per case; the gradients of the four losses are taken from it (retain_graph) and kept unchanged."""
    cfg = configs.tiny_G_cfg(32, D, 1)
    G = pkg.build_generator(cfg, DEV, seed=3)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(D + N)
    B, R, H = 2, S * S, 32
    locs = torch.tensor([[0.25, 0.1], [-0.4, -0.05]])
    cam = O.camera_params(locs, S, 6, 0.12)
    styles = 0.5 * torch.randn(B, D + 1, 32, generator=g)
    u = torch.rand(B, S, S, 1, generator=g) if perturb else None
    t = {"F": torch.randn(B, H, S, S, generator=g), "T": torch.randn(B, 3, S, S, generator=g),
         "M": torch.randn(B, S, S, generator=g), "D": torch.randn(B, S, S, generator=g), "X": torch.randn(B, 3, S, S, generator=g)}
    cr, sr = leaf(cam[0]), leaf(styles)
    rays_o, rays_d, viewdirs = O.rays_in_world(cam[1], S, cr, static)
    z = O.z_vals(cam[2], cam[3], B, S, S, N, u)
    pts = O.ray_points(rays_o, rays_d, z)
    thumb, feat, sdf, mask, xyz = O.renderer_forward(sd, "renderer", pts.reshape(B, R, N, 3), rays_d.reshape(B, R, 3),
                                                     viewdirs.reshape(B, R, 3), z.reshape(B, R, N), cam[2], cam[3], sr, D)
    to_img = lambda v: v.transpose(1, 2).reshape(B, v.shape[-1], S, S)
    maps = {"features": to_img(feat), "thumb": to_img(thumb), "mask": to_img(mask)[:, 0], "depth": to_img(mask)[:, 1],
            "xyz": to_img(xyz)}
    grads = {}
    for term in TERMS:
        dsty, dcam = torch.autograd.grad(_loss(term, maps, t), [sr, cr], retain_graph=True)
        grads[term] = (dsty.clone(), dcam.clone())
    return G, cam, styles, u, t, {k: v.detach() for k, v in maps.items()}, grads


def _loss(term, m, t, to=lambda v: v):
    lm = (m["mask"] * to(t["M"])).sum()
    ld = 10.0 * (m["depth"] * to(t["D"])).sum()
    lx = 10.0 * (m["xyz"] * to(t["X"])).sum()
    if term == "all":
        return lm + ld + lx + (m["features"] * to(t["F"])).sum() + 3.0 * (m["thumb"] * to(t["T"])).sum()
    return {"mask": lm, "depth": ld, "xyz": lx}[term]


@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("D,static,perturb,N,S", CASES)
def test_geometry_map_gradients_vs_oracle(D, static, perturb, N, S, term):
    """d loss / d styles and d loss / d cam_poses of each geometry map's loss ALONE (the camera gradient of the xyz term is
    dominated by the direct path through the points and would hide a wrong d loss / d w_k) and of all maps together."""
    G, cam, styles, u, t, maps, grads = _oracle_case(D, static, perturb, N, S)
    ref_s, ref_c = grads[term]
    # (close()'s absolute floor of 1e-6 must not carry the comparison)
    print(f"oracle max-abs: dstyles {float(ref_s.abs().max()):.4g} dcam {float(ref_c.abs().max()):.4g}")
    assert float(ref_s.abs().max()) >= 0.05 and float(ref_c.abs().max()) >= 0.05
    cg, sg = leaf(cu(cam[0])), leaf(cu(styles))
    film = AG.film_table(G.renderer, sg)
    f_g, t_g, xyz_g, mask_g = AG.NerfRenderFn.apply(G.renderer, cg, cu(cam[1]), cu(cam[2]), cu(cam[3]), film,
                                                    None if u is None else cu(u), S, N, static)
    assert xyz_g.requires_grad and mask_g.requires_grad
    got = {"features": f_g, "thumb": t_g, "mask": mask_g[0], "depth": mask_g[1], "xyz": xyz_g}
    for k in ("mask", "depth", "xyz"):
        close(got[k], maps[k], 1e-4, k)
    _loss(term, got, t, cu).backward()
    close(sg.grad, ref_s, 3e-4, "dstyles")
    close(cg.grad, ref_c, 3e-4, "dcam_poses")


# ------------------------------------------------------------------------------------------------ 2, 3. the two routes
def _setup(hidden, depth, B, S, seed=3):
    cfg = configs.tiny_G_cfg(hidden, depth, 1) if hidden < 256 else configs.ffhq_G_cfg(256, depth)
    G = pkg.build_generator(cfg, DEV, seed=seed)
    r = G.renderer
    locs = torch.tensor([[0.25, 0.1], [-0.4, -0.05]])[:B].to(DEV)
    cam, focal, near, far = Camera.generate_camera_params(locations=locs, img_size=S, device=DEV, fov_ang=6,
                                                          dist_radius=0.12)[:4]
    styles = (0.5 * weights.det_normal("geo.styles", (B, depth + 1, r.style_dim), 1.0, seed)).to(DEV)
    film = AG.film_table(r, styles).detach()
    return r, cam, focal, near, far, film


def _agree(f0, c0, f1, c1, tol, depth):
    for l in range(depth + 1):
        for k, nm in ((0, "gamma"), (1, "beta")):
            ref = f0[:, l, k]
            if l == depth and float(ref.abs().max()) == 0:      # the view layer feeds only the features and the thumbnail:
                assert float(f1[:, l, k].abs().max()) == 0, (l, nm)     # with their upstreams zero its gradient IS zero
                continue
            d = float((ref - f1[:, l, k]).abs().max() / ref.abs().max())
            assert d < tol, (l, nm, d)
    d = float((c0 - c1).abs().max() / c0.abs().max())
    assert d < tol, ("dcam", d)


@pytest.mark.parametrize("hidden,depth,B,S,N", [(32, 2, 2, 8, 6), (256, 2, 1, 16, 8)])
def test_fused_backward_agrees_with_the_materialised_sequence(hidden, depth, B, S, N):
    """Only the geometry upstreams are set (d_features = d_thumb = 0): both routes hand them to the same two kernels; also with
    the stash the differentiable forward filled."""
    assert hip.nerf_backward_fused_supported(hidden, depth, S, N)
    r, cam, focal, near, far, film = _setup(hidden, depth, B, S)
    H = r.hidden_dim
    u = weights.det_unit_uniform("geo.u", (B, S, S, 1), 2).to(DEV)
    dF, dT = torch.zeros(B, H, S, S, device=DEV), torch.zeros(B, 3, S, S, device=DEV)
    dM = weights.det_normal("geo.dM", (2, B, S, S), 1.0, 3).to(DEV)
    dM[1] *= 10.0
    dX = (10.0 * weights.det_normal("geo.dX", (B, 3, S, S), 1.0, 4)).to(DEV)
    packed, layer_bias = r._derived_buffers()
    args = (r.network, r.sigmoid_beta.detach(), cam, focal, near, far, u, film, layer_bias)
    fwd = hip.nerf_forward_stash(B, S, N, H, depth, DEV)
    xyz = r.render(cam, focal, near, far, None, S, N, perturb_u=u, film=film, stash=fwd)[4]
    geo = dict(d_mask=dM, d_xyz=dX, xyz=xyz)
    f0, c0 = hip.nerf_backward(*args, S, N, False, dF, dT, **geo)
    assert torch.isfinite(f0).all() and torch.isfinite(c0).all() and float(f0.abs().max()) > 0 and float(c0.abs().max()) > 0
    f1, c1 = hip.nerf_backward_fused(*args, packed, r._packed_transposed(), S, N, False, dF, dT, **geo)
    _agree(f0, c0, f1, c1, 3e-5, depth)
    f2, c2 = hip.nerf_backward_fused(*args, packed, r._packed_transposed(), S, N, False, dF, dT, fwd=fwd, **geo)
    _agree(f0, c0, f2, c2, 3e-5, depth)


def test_absent_upstreams_equal_zero_upstreams():
    """None means absent: explicit zero d_mask / d_xyz give the gradients of None, up to the atomics' reordering."""
    hidden, depth, B, S, N = 32, 2, 2, 8, 6
    r, cam, focal, near, far, film = _setup(hidden, depth, B, S)
    u = weights.det_unit_uniform("geo.u", (B, S, S, 1), 2).to(DEV)
    dF = weights.det_normal("geo.dF", (B, hidden, S, S), 1.0, 3).to(DEV)
    dT = (10.0 * weights.det_normal("geo.dT", (B, 3, S, S), 1.0, 4)).to(DEV)
    packed, layer_bias = r._derived_buffers()
    args = (r.network, r.sigmoid_beta.detach(), cam, focal, near, far, u, film, layer_bias)
    xyz = r.render(cam, focal, near, far, None, S, N, perturb_u=u, film=film)[4]
    zero = dict(d_mask=torch.zeros(2, B, S, S, device=DEV), d_xyz=torch.zeros(B, 3, S, S, device=DEV), xyz=xyz)
    for run in (lambda **kw: hip.nerf_backward(*args, S, N, False, dF, dT, **kw),
                lambda **kw: hip.nerf_backward_fused(*args, packed, r._packed_transposed(), S, N, False, dF, dT, **kw)):
        f0, c0 = run()
        f1, c1 = run(**zero)
        assert float((f1 - f0).abs().max() / f0.abs().max()) < 2e-6
        assert float((c1 - c0).abs().max() / c0.abs().max()) < 2e-6
    with pytest.raises(ValueError, match="xyz"):
        hip.nerf_backward(*args, S, N, False, dF, dT, d_mask=zero["d_mask"])


# ------------------------------------------------------------------------------------------------ 4. depth at the origin
@pytest.mark.parametrize("N", [6, 36])          # one sample per thread; the per-ray loop
def test_depth_gradient_of_a_ray_composited_to_the_origin(N):
    """depth = -|xyz| has no gradient at xyz == 0 (torch's subgradient of norm is 0): a ray whose xyz map entry is exactly 0
    gets nothing from the depth's upstream -- its outputs are those of a call without it -- and nothing is NaN."""
    lib = _lib.load()
    B, S = 2, 4
    R, P = S * S, S * S * N
    cam, focal, near, far = Camera.generate_camera_params(locations=torch.tensor([[0.25, 0.1], [-0.4, -0.05]], device=DEV),
                                                          img_size=S, device=DEV, fov_ang=6, dist_radius=0.12)[:4]
    geom = _lib.NerfBwdGeom()
    keep = [cam.float().contiguous(), focal.float().reshape(B).contiguous(), near.float().reshape(B).contiguous(),
            far.float().reshape(B).contiguous()]
    geom.cam_poses, geom.focals, geom.near_, geom.far_ = (t.data_ptr() for t in keep)
    geom.perturb_u = None
    geom.B, geom.img_size, geom.n_samples, geom.static_viewdirs = B, S, N, 0
    rnd = lambda tag, shape, s=1.0: (s * weights.det_normal("geo.origin." + tag, shape, 1.0, N)).to(DEV).contiguous()
    sdf, crgb, g, dth = rnd("sdf", (B, P), 0.05), rnd("crgb", (B, 3, P)), rnd("g", (B, P)), rnd("dth", (B, 3, R))
    beta = torch.full((1,), 0.1, device=DEV)
    d_mask = torch.zeros(2, B, R, device=DEV)
    d_mask[1] = rnd("ddepth", (B, R))
    xyz = rnd("xyz", (B, 3, R), 0.1)
    b0, ray0 = 1, 5
    xyz[b0, :, ray0] = 0.0

    def run(with_depth):
        o = {k: torch.full(shape, float("nan"), device=DEV) for k, shape in
             (("w", (B, P)), ("T", (B, P)), ("dsdf", (B, P)), ("dcrgb", (B, 3, P)), ("ddnorm", (B, R)), ("wsum", (B, R)),
              ("wzsum", (B, R)))}
        geo = (d_mask.data_ptr(), None, xyz.data_ptr(), o["wsum"].data_ptr(), o["wzsum"].data_ptr()) if with_depth \
            else (None,) * 5
        _lib.check(lib.cips3d_nerf_bwd_composite(
            ctypes.byref(geom), sdf.data_ptr(), crgb.data_ptr(), g.data_ptr(), dth.data_ptr(),
            beta.data_ptr(), o["w"].data_ptr(), o["T"].data_ptr(), o["dsdf"].data_ptr(), o["dcrgb"].data_ptr(),
            o["ddnorm"].data_ptr(), None, *geo, hip.stream_ptr()), "cips3d_nerf_bwd_composite")
        torch.cuda.synchronize()
        return o

    base, got = run(False), run(True)
    for k in ("w", "T", "dsdf", "dcrgb", "ddnorm", "wsum", "wzsum"):
        assert torch.isfinite(got[k]).all(), k
    ds0, ds1 = base["dsdf"].view(B, N, R), got["dsdf"].view(B, N, R)
    assert torch.equal(ds1[b0, :, ray0], ds0[b0, :, ray0]) and torch.equal(got["ddnorm"][b0, ray0], base["ddnorm"][b0, ray0])
    others = torch.ones(B, R, dtype=torch.bool, device=DEV)
    others[b0, ray0] = False
    assert bool(((ds1 - ds0).abs().amax(1) > 0)[others].all())            # every other ray does get the depth's share
    # the per-ray sums: sum_k w_k, and sum_k w_k z_k within the ray's depth range
    assert float((got["wsum"] - got["w"].view(B, N, R).sum(1)).abs().max()) < 1e-5
    lo, hi = near.reshape(B, 1), far.reshape(B, 1)
    assert bool((got["wzsum"] >= got["wsum"] * lo * (1 - 1e-5)).all() and (got["wzsum"] <= got["wsum"] * hi * (1 + 1e-5)).all())


# ------------------------------------------------------------------------------------------------ 5. renderer weights
def test_mask_gradient_reaches_the_renderer_weights():
    """`optim_render_params` (the materialised route): the larger d loss / d w_k flows on into d sdf and d sigmoid_beta."""
    D, static, N, S = 2, False, 8, 8
    cfg = configs.tiny_G_cfg(32, D, 1)
    G = pkg.build_generator(cfg, DEV, seed=4)
    g = torch.Generator().manual_seed(D + N)
    sd = {k: leaf(v.detach().cpu()) if k.startswith("renderer.") else v.detach().cpu() for k, v in G.state_dict().items()}
    B, R = 2, S * S
    cam = O.camera_params(torch.tensor([[0.25, 0.1], [-0.4, -0.05]]), S, 6, 0.12)
    styles = 0.5 * torch.randn(B, D + 1, 32, generator=g)
    u = torch.rand(B, S, S, 1, generator=g)
    tM = torch.randn(B, S, S, generator=g)
    rays_o, rays_d, viewdirs = O.rays_in_world(cam[1], S, cam[0], static)
    z = O.z_vals(cam[2], cam[3], B, S, S, N, u)
    pts = O.ray_points(rays_o, rays_d, z)
    mask = O.renderer_forward(sd, "renderer", pts.reshape(B, R, N, 3), rays_d.reshape(B, R, 3), viewdirs.reshape(B, R, 3),
                              z.reshape(B, R, N), cam[2], cam[3], styles, D)[3]
    (mask[..., 0].reshape(B, S, S) * tM).sum().backward()
    G.requires_grad_(False)
    G.renderer.requires_grad_(True)
    film = AG.film_table(G.renderer, cu(styles))
    rp = [p for _, p in AG.nerf_named_parameters(G.renderer)]
    mask_g = AG.NerfRenderFn.apply(G.renderer, cu(cam[0]), cu(cam[1]), cu(cam[2]), cu(cam[3]), film, cu(u), S, N, static, *rp)[3]
    (mask_g[0] * cu(tM)).sum().backward()
    for name, p in (("network.sigma_linear.weight", G.renderer.network.sigma_linear.weight),
                    ("sigmoid_beta", G.renderer.sigmoid_beta)):
        ref = sd["renderer." + name].grad
        assert ref is not None and p.grad is not None and float(ref.abs().max()) > 0, name
        close(p.grad, ref, 3e-4, name)


# ------------------------------------------------------------------------------------------------ 6. generator surface
def test_generator_maps_carry_a_graph():
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=1)
    loc = torch.tensor([[0.2, 0.05], [-0.2, 0.05]], device=DEV).requires_grad_(True)
    e, f, n, fa, _ = Camera.generate_camera_params(8, DEV, locations=loc, fov_ang=6, dist_radius=0.12)
    assert e.requires_grad
    g = torch.Generator().manual_seed(5)
    style_render = leaf(cu(0.5 * torch.randn(2, 3, 32, generator=g)))
    style_decoder = cu(0.5 * torch.randn(2, G.decoder.n_latent, 32, generator=g))
    ret = G(zs=[None, None], style_render=style_render, style_decoder=style_decoder, cam_poses=e, focals=f, img_size=8, near=n,
            far=fa, nerf_cfg=dict(N_samples=6, perturb=False), noise_bufs=G.create_noise_bufs(8, DEV), return_xyz=True)
    assert ret["mask"].shape == (2, 1, 8, 8) and ret["depth"].shape == (2, 1, 8, 8) and ret["xyz"].shape == (2, 3, 8, 8)
    assert ret["mask"].requires_grad and ret["depth"].requires_grad and ret["xyz"].requires_grad
    ret["mask"].sum().backward()
    for t in (style_render, loc):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 7. the loop
def test_silhouette_term_drives_the_pose_phase_like_the_oracle_loop():
    """project_wplus with the silhouette term alone (surrogate loss of weight 0): the loss falls over 30 pose steps towards a
    mask rendered at another azimuth, and the first 5 steps follow the same loop written with torch autograd over the CPU oracle
    and torch's Adam (the construction of test_gpu_backward.py::test_pose_phase_trajectory_matches_the_oracle_loop)."""
    from cips_3dplusplus_amd.projector import FlipProjector, surrogate_loss, cur_lr
    cfg = configs.tiny_G_cfg(32, 2, 1)
    G = pkg.build_generator(cfg, DEV, seed=13)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    mr, md = 0.3 * torch.randn(1, 32, generator=g), 0.3 * torch.randn(1, 32, generator=g)
    t_rgb, t_thumb = torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 8, 8)
    N, lr_cam, lr_w, az0 = 30, 0.02, 0.01, (0.15, -0.15)
    cam_cfg = {"img_size": 8, "fov_ang": 6, "dist_radius": 0.12}
    ncfg = {"N_samples": 6, "perturb": False, "static_viewdirs": True}
    G.get_mean_latent = lambda n, dev: (cu(mr), cu(md))        # (the projector draws its means on the device otherwise)
    w_d = md.reshape(1, 1, -1).repeat(2, G.decoder.n_latent, 1)
    with torch.no_grad():
        e, f, n, fa, _ = Camera.generate_camera_params(8, DEV, locations=torch.tensor([[0.35, 0.0], [-0.35, 0.0]], device=DEV),
                                                       fov_ang=6, dist_radius=0.12)
        tgt = G(zs=[None, None], style_render=cu(mr.reshape(1, 1, -1).repeat(2, 3, 1)), style_decoder=cu(w_d), cam_poses=e,
                focals=f, img_size=8, near=n, far=fa, nerf_cfg=ncfg, noise_bufs=[torch.zeros_like(b) for b in G.create_noise_bufs(8, DEV)])
        target_masks = (1 - tgt["mask"]).clone()               # foreground
    traj = []
    FlipProjector(G, DEV).project_wplus(cam_cfg, ncfg, surrogate_loss(cu(t_rgb), cu(t_thumb), rgb_weight=0.0, thumb_weight=0.0),
                                        N_steps_pose=N, N_steps_app=0, lr_cam=lr_cam, lr_render_w=lr_w, azim_init=az0,
                                        w_avg_samples=8, silhouette_weight=1.0, target_masks=target_masks,
                                        on_step=lambda s_, l, a, e_: traj.append((float(l.detach()), a.detach().cpu().clone(),
                                                                                  e_.detach().cpu().clone())))
    losses = [t[0] for t in traj]
    print("silhouette losses:", " ".join(f"{v:.5e}" for v in losses))
    assert len(traj) == N and all(v == v and abs(v) != float("inf") for v in losses)
    assert losses[-1] < losses[1], (losses[1], losses[-1])
    # the same loop on the CPU oracle, 5 steps
    bg = 1 - target_masks.cpu()
    azim = torch.tensor([[az0[0]], [az0[1]]], requires_grad=True)
    elev = torch.zeros(2, 1, requires_grad=True)
    w_r = mr.reshape(1, 1, -1).repeat(1, 3, 1).clone().requires_grad_(True)
    nb = [torch.zeros(*b.shape) for b in G.create_noise_bufs(8, "cpu")]
    o_cam = torch.optim.Adam([{"params": [azim, elev], "lr": lr_cam, "betas": (0.9, 0.999)}])
    o_w = torch.optim.Adam([{"params": [w_r], "lr": lr_w, "betas": (0.9, 0.999)}])
    for step in range(5):
        m = cur_lr(step, N)
        o_cam.param_groups[0]["lr"], o_w.param_groups[0]["lr"] = lr_cam * m, lr_w * m
        cam = O.camera_params(torch.cat([azim, elev], 1), 8, 6, 0.12)
        r = O.generator_forward(sd, cfg, [None, None], cam[0], cam[1], 8, cam[2], cam[3], ncfg, nb, style_render=w_r.repeat(2, 1, 1),
                                style_decoder=w_d)
        loss = 0.0 * ((r["rgb"] - t_rgb) ** 2).mean() + 0.0 * ((r["thumb_rgb"] - t_thumb) ** 2).mean() \
            + ((r["mask"] - bg) ** 2).mean()
        o_cam.zero_grad(); o_w.zero_grad()
        loss.backward()
        o_cam.step(); o_w.step()
        l_hip, a_hip, e_hip = traj[step]
        print(f"step {step}: loss hip {l_hip:.6e} oracle {float(loss.detach()):.6e}  d azim {float((a_hip - azim.detach()).abs().max()):.2e}"
              f" d elev {float((e_hip - elev.detach()).abs().max()):.2e}")
        assert abs(l_hip - float(loss.detach())) < 2e-4 * abs(float(loss.detach())), (step, l_hip)
        assert float((a_hip - azim.detach()).abs().max()) < 2e-4 and float((e_hip - elev.detach()).abs().max()) < 2e-4, step
    assert abs(float(azim.detach()[0]) - az0[0]) > 1e-3            # the camera moved
