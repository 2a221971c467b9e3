"""The free camera of flip inversion on the GPU: the axis-angle pose kernel and its backward (csrc/camera_free.hip) against float64
matrix_exp, the gradient of the render with respect to the focal length (the camera chain's second instantiation,
csrc/nerf_bwd.hip, on both NeRF backward routes) against torch autograd through the CPU oracle, the autograd nodes, and the
loop: an in-plane roll that the axis-angle camera recovers and the look-at camera cannot.  Cases and references:
tests/_free_camera_cases.py."""
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import autograd as AG, configs, hip, weights
from cips_3dplusplus_amd.camera import Camera, cameras_around_pose
from cips_3dplusplus_amd.projector import FlipProjector, cur_lr, surrogate_loss
import _free_camera_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cu(t):
    return t.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ 1. the pose kernel
@pytest.mark.parametrize("B", [1, 3, 65])
def test_pose_forward_vs_float64_matrix_exp(B):
    """One rounding of an fp64 result with entries <= 1: |extr - ref| <= 2^-23; R is a rotation to 1e-6."""
    rot, trans, fov = FC.pose_table(B)
    extr, focal, near, far = hip.camera_axis_angle(cu(rot), cu(trans), 64, cu(fov), 0.12)
    assert extr.shape == (B, 3, 4) and focal.shape == near.shape == far.shape == (B, 1, 1)
    ref = FC.pose64(rot, trans)
    err = float((extr.cpu().double() - ref).abs().max())
    print(f"B {B}: max |extr - ref| {err:.3e} (bar {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23
    R = extr[:, :, :3].cpu().double()
    assert float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
    assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-6
    fref = FC.focal64(fov, 64)
    # (focal is cips3d_camera_params' fp32 expression -- angle, tanf, division: four roundings and tanf's own ulp)
    assert float(((focal.cpu().reshape(B).double() - fref) / fref).abs().max()) <= 8 * 2.0 ** -23
    assert bool((near == 1 - 0.12).all()) and bool((far == 1 + 0.12).all())
    # a scalar field of view is the [B] tensor of that value
    e2, f2, _, _ = hip.camera_axis_angle(cu(rot), cu(trans), 64, 6.0, 0.12)
    e3, f3, _, _ = hip.camera_axis_angle(cu(rot), cu(trans), 64, torch.full((B,), 6.0, device=DEV), 0.12)
    assert torch.equal(e2, extr) and torch.equal(e2, e3) and torch.equal(f2, f3)


def test_start_point_is_the_frontal_look_at_camera_bit_for_bit():
    rot, trans = torch.zeros(2, 3, device=DEV), torch.tensor([[0.0, 0.0, 1.0]] * 2, device=DEV)
    got = hip.camera_axis_angle(rot, trans, 64, 6.0, 0.12)
    ref = Camera.generate_camera_params(64, DEV, locations=torch.zeros(2, 2, device=DEV), fov_ang=6, dist_radius=0.12)[:4]
    for a, b, name in zip(got, ref, ("extrinsics", "focal", "near", "far")):
        assert a.shape == b.shape and torch.equal(a, b), name
    eye = torch.eye(3, 4, device=DEV)
    eye[2, 3] = 1.0
    assert torch.equal(got[0][0], eye)
    # the one-launch front end and the reference-named torch expression give the same pose
    e = Camera.free_camera_params(64, DEV, rot, trans)[0]
    assert torch.equal(e, got[0])
    assert torch.equal(Camera.get_camera2world(rot, trans), got[0])
    assert Camera.get_camera2world(rot, trans, homo=True).shape == (2, 4, 4)


@pytest.mark.parametrize("B", [1, 3, 65])
def test_pose_backward_vs_float64_autograd(B):
    """Random dextr / dfocal; per output |got - ref| <= 2^-22 sum_i |g_i d_i| (the result is rounded once from fp64; the bound
    leaves a factor 4 for the oracle's own fp64 evaluation of nearly cancelling terms).  Finite at theta = 0, where
    d R / d r_i = [e_i]x; dtrans is orthogonal to trans above the clamp of F.normalize."""
    rot, trans, fov = FC.pose_table(B)
    Jr, Jt, Jf = FC.pose_jacobian(B)
    g = torch.Generator().manual_seed(B)
    dextr = torch.randn(B, 3, 4, generator=g)
    dfocal = torch.randn(B, generator=g)
    drot, dtrans, dfov = hip.camera_axis_angle_bwd(cu(rot), cu(trans), 64, cu(fov), cu(dextr), cu(dfocal))
    gd = dextr.reshape(B, 12, 1).double()
    for name, got, J in (("drot", drot, Jr), ("dtrans", dtrans, Jt)):
        got = got.cpu().double()
        assert bool(torch.isfinite(got).all()), name
        ref, bar = (gd * J).sum(1), 2.0 ** -22 * (gd * J).abs().sum(1)
        worst = float(((got - ref).abs() / bar.clamp_min(1e-300)).max())
        print(f"B {B} {name}: max |got - ref| / bar {worst:.3f}")
        assert bool(((got - ref).abs() <= bar).all()), (name, worst)
    ref = dfocal.double() * Jf
    assert bool(((dfov.cpu().double() - ref).abs() <= 2.0 ** -22 * ref.abs()).all())
    # theta = 0 (row 0): the generators
    G0 = dextr[0, :, :3].double()
    lim = torch.stack([G0[2, 1] - G0[1, 2], G0[0, 2] - G0[2, 0], G0[1, 0] - G0[0, 1]])
    assert float((drot[0].cpu().double() - lim).abs().max()) <= 2.0 ** -22 * float(G0.abs().sum())
    big = trans.norm(dim=1) > 1e-6
    dots = (dtrans.cpu().double() * trans.double()).sum(1)[big]
    scale = (dtrans.cpu().double().abs() * trans.double().abs()).sum(1)[big]
    assert bool((dots.abs() <= 1e-6 * scale + 1e-12).all())
    # absent upstreams are zeros
    z = hip.camera_axis_angle_bwd(cu(rot), cu(trans), 64, cu(fov), None, cu(dfocal))
    assert float(z[0].abs().max()) == 0 and float(z[1].abs().max()) == 0 and torch.equal(z[2], dfov)
    z = hip.camera_axis_angle_bwd(cu(rot), cu(trans), 64, 6.0, cu(dextr), None)
    assert torch.equal(z[0], drot) and torch.equal(z[1], dtrans) and z[2] is None


def test_camera_axis_angle_fn_is_the_kernel_pair():
    rot, trans, fov = (FC.leaf(cu(t)) for t in FC.pose_table(3))
    extr, focal, near, far = Camera.free_camera_params(64, DEV, rot, trans, fov_ang=fov)
    assert extr.requires_grad and focal.requires_grad and not near.requires_grad and not far.requires_grad
    g = torch.Generator().manual_seed(1)
    dextr, dfocal = cu(torch.randn(3, 3, 4, generator=g)), cu(torch.randn(3, 1, 1, generator=g))
    ((extr * dextr).sum() + (focal * dfocal).sum()).backward()
    ref = hip.camera_axis_angle_bwd(rot, trans, 64, fov, dextr, dfocal)
    for t, r in zip((rot, trans, fov), ref):
        assert t.grad is not None and torch.equal(t.grad, r.reshape(t.shape))
    # a constant field of view: focal carries no graph, so the render's focal instantiation is never asked for
    e2, f2, _, _ = Camera.free_camera_params(64, DEV, rot, trans, fov_ang=6)
    assert e2.requires_grad and not f2.requires_grad


# ------------------------------------------------------------------------------------------------ 2. d loss / d focals
@pytest.mark.parametrize("term", FC.FOCAL_TERMS)
@pytest.mark.parametrize("D,static,perturb,N,S", FC.FOCAL_CASES)
def test_focal_gradient_vs_oracle(D, static, perturb, N, S, term):
    """d loss / d focals [B] of `features + 3 thumb` and of all five maps' loss against torch autograd through the CPU oracle with
    `focal` a leaf of rays_in_world.  The bar is the harness's bar for dcam_poses (3e-4 of the reference's maximum): d focals is
    a contraction of the same per-ray sums.  Measured on an MI355X: see DESIGN 8.6."""
    case = FC.focal_oracle_case(D, static, perturb, N, S, DEV)
    G, _, cam, styles, u, t, grads = case
    ref_f, ref_c = grads[term]
    print(f"oracle: dfocal {[float(v) for v in ref_f]} max |dcam| {float(ref_c.abs().max()):.4g}")
    assert float(ref_f.abs().max()) >= 0.05
    cg, fg, sg = FC.leaf(cu(cam[0])), FC.leaf(cu(cam[1])), cu(styles)
    film = AG.film_table(G.renderer, sg)
    f_g, t_g, xyz_g, mask_g = AG.NerfRenderFn.apply(G.renderer, cg, fg, cu(cam[2]), cu(cam[3]), film,
                                                    None if u is None else cu(u), S, N, static)
    got = {"features": f_g, "thumb": t_g, "mask": mask_g[0], "depth": mask_g[1], "xyz": xyz_g}
    FC.focal_loss(term, got, t, cu).backward()
    assert fg.grad is not None and fg.grad.shape == fg.shape
    scale = float(ref_f.abs().max())
    err = float((fg.grad.cpu().reshape(-1) - ref_f).abs().max())
    errc = float((cg.grad.cpu() - ref_c).abs().max()) / float(ref_c.abs().max())
    print(f"dfocal: err {err:.3e} scale {scale:.3e} ratio {err / scale:.3e} (bar 3e-4); dcam ratio {errc:.3e}")
    assert errc <= 3e-4
    assert err <= 3e-4 * scale + 1e-6, f"dfocal: err {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------------------------------------ 3. both routes
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


@pytest.mark.parametrize("hidden,depth,B,S,N", [(32, 2, 2, 8, 6), (256, 2, 1, 16, 8)])
def test_focal_gradient_of_both_routes_and_nothing_else_moves(hidden, depth, B, S, N):
    """d focals of the fused backward (with and without the forward's stash) agrees with the materialised sequence's to 3e-5
    relative; asking for it changes nothing else: at S = 8 (one workgroup per view) dfilm and dcam are the bits of the call
    without it, at S = 16 they agree within 2e-6 relative (the atomics' order).  One exception at S = 8: the FUSED backward sums
    d film with LDS atomics of the waves of a workgroup and global atomics of several workgroups per view at every size
    (nerf_bwd_kernel: accumulate_sums and the flush of s_sum), so two identical calls already differ in the last bits; its
    dfilm is held to the 2e-6 of the atomics' order, its dcam -- one camera-chain workgroup per view -- to the bits."""
    assert hip.nerf_backward_fused_supported(hidden, depth, S, N)
    r, cam, focal, near, far, film = _setup(hidden, depth, B, S)
    H = r.hidden_dim
    u = weights.det_unit_uniform("free.u", (B, S, S, 1), 2).to(DEV)
    dF = weights.det_normal("free.dF", (B, H, S, S), 1.0, 3).to(DEV)
    dT = (3.0 * weights.det_normal("free.dT", (B, 3, S, S), 1.0, 4)).to(DEV)
    dM = weights.det_normal("free.dM", (2, B, S, S), 1.0, 5).to(DEV)
    dX = (10.0 * weights.det_normal("free.dX", (B, 3, S, S), 1.0, 6)).to(DEV)
    packed, layer_bias = r._derived_buffers()
    args = (r.network, r.sigmoid_beta.detach(), cam, focal, near, far, u, film, layer_bias)
    fwd = hip.nerf_forward_stash(B, S, N, H, depth, DEV)
    xyz = r.render(cam, focal, near, far, None, S, N, perturb_u=u, film=film, stash=fwd)[4]
    geo = dict(d_mask=dM, d_xyz=dX, xyz=xyz)
    routes = {"materialised": lambda **kw: hip.nerf_backward(*args, S, N, False, dF, dT, **geo, **kw),
              "fused": lambda **kw: hip.nerf_backward_fused(*args, packed, r._packed_transposed(), S, N, False, dF, dT, **geo, **kw),
              "fused+stash": lambda **kw: hip.nerf_backward_fused(*args, packed, r._packed_transposed(), S, N, False, dF, dT,
                                                                  fwd=fwd, **geo, **kw)}
    dfoc = {}
    for name, run in routes.items():
        base = run()
        assert len(base) == 2                                  # the default arity stays
        with_f = run(d_focal=True)
        assert len(with_f) == 3 and with_f[2].shape == (B,) and bool(torch.isfinite(with_f[2]).all())
        for a, b, what in zip(base, with_f, ("dfilm", "dcam")):
            if S == 8 and not (what == "dfilm" and name != "materialised"):
                assert torch.equal(a, b), (name, what)
            else:
                assert float((a - b).abs().max() / a.abs().max()) < 2e-6, (name, what)
        dfoc[name] = with_f[2]
    ref = dfoc["materialised"]
    assert float(ref.abs().max()) > 0
    for name in ("fused", "fused+stash"):
        d = float((dfoc[name] - ref).abs().max() / ref.abs().max())
        print(f"{name}: dfocal vs materialised {d:.3e}")
        assert d < 3e-5, (name, d)
    out = hip.nerf_backward(*args, S, N, False, dF, dT, need_params=True, d_focal=True, **geo)
    assert len(out) == 4 and isinstance(out[2], dict) and float((out[3] - ref).abs().max() / ref.abs().max()) < 2e-6


# ------------------------------------------------------------------------------------------------ 4. autograd through G
@pytest.mark.parametrize("hidden,S,N", [(32, 8, 6), (256, 16, 8)])
def test_generator_returns_the_focal_gradient(hidden, S, N, monkeypatch):
    """G(..., focals=leaf, cam_poses=leaf, differentiable=True): focals.grad is finite, non-zero and the direct hip call's
    result (up to the atomics' order); a focal that does not ask for a gradient gets None from the node."""
    B, depth = 2, 2
    G = pkg.build_generator(configs.tiny_G_cfg(hidden, depth, 1), DEV, seed=5)
    r = G.renderer
    cam, focal, near, far = Camera.generate_camera_params(locations=torch.tensor([[0.25, 0.1], [-0.4, -0.05]], device=DEV),
                                                          img_size=S, device=DEV, fov_ang=6, dist_radius=0.12)[:4]
    g = torch.Generator().manual_seed(hidden)
    style_render = cu(0.5 * torch.randn(B, depth + 1, r.style_dim, generator=g))
    style_decoder = cu(0.5 * torch.randn(B, G.decoder.n_latent, 32, generator=g))
    tT, tM, tD = (cu(torch.randn(*s, generator=g)) for s in ((B, 3, S, S), (B, 1, S, S), (B, 1, S, S)))
    ncfg = dict(N_samples=N, perturb=False, static_viewdirs=True)
    cg, fg = FC.leaf(cam), FC.leaf(focal)
    ret = G(zs=[None, None], style_render=style_render, style_decoder=style_decoder, cam_poses=cg, focals=fg, img_size=S,
            near=near, far=far, nerf_cfg=ncfg, noise_bufs=G.create_noise_bufs(S, DEV), differentiable=True)
    ((ret["thumb_rgb"] * tT).sum() + (ret["mask"] * tM).sum() + 10.0 * (ret["depth"] * tD).sum()).backward()
    assert fg.grad is not None and fg.grad.shape == fg.shape and bool(torch.isfinite(fg.grad).all())
    assert float(fg.grad.abs().min()) > 0
    film = AG.film_table(r, style_render, batch=B).detach()
    packed, layer_bias = r._derived_buffers()
    fwd = hip.nerf_forward_stash(B, S, N, r.hidden_dim, depth, DEV)
    xyz = r.render(cam, focal, near, far, None, S, N, static_viewdirs=True, film=film, stash=fwd)[4]
    _, dcam, dfoc = hip.nerf_backward_fused(r.network, r.sigmoid_beta.detach(), cam, focal, near, far, None, film, layer_bias,
                                            packed, r._packed_transposed(), S, N, True, torch.zeros(B, r.hidden_dim, S, S, device=DEV),
                                            tT, fwd=fwd, d_mask=torch.cat([tM, 10.0 * tD], 1).transpose(0, 1).contiguous(),
                                            xyz=xyz, d_focal=True)
    assert float((fg.grad.reshape(-1) - dfoc).abs().max() / dfoc.abs().max()) < 2e-6
    assert float((cg.grad - dcam).abs().max() / dcam.abs().max()) < 2e-6
    # the node alone, with a focal that asks for nothing: None, and the focal instantiation is not asked for
    seen = []
    for name in ("nerf_backward", "nerf_backward_fused"):
        orig = getattr(hip, name)
        monkeypatch.setattr(hip, name, lambda *a, _o=orig, **kw: (seen.append(kw.get("d_focal", False)), _o(*a, **kw))[1])
    c2, f2 = FC.leaf(cam), focal.clone()
    out = AG.NerfRenderFn.apply(r, c2, f2, near, far, film, None, S, N, True)
    (out[1] * tT).sum().backward()
    assert c2.grad is not None and f2.grad is None and seen == [False]
    f3 = FC.leaf(focal)
    out = AG.NerfRenderFn.apply(r, cam, f3, near, far, film, None, S, N, True)
    (out[1] * tT).sum().backward()
    assert f3.grad is not None and seen == [False, True]


# ------------------------------------------------------------------------------------------------ 5. the loop
def _loop_generator():
    L = FC.LOOP
    G = pkg.build_generator(configs.tiny_G_cfg(L["hidden"], L["depth"], 1), DEV, seed=L["seed"])
    sr, g = FC.loop_inputs()
    sd = 0.5 * torch.randn(1, G.decoder.n_latent, 32, generator=g)
    nb = [torch.zeros_like(b) for b in G.create_noise_bufs(L["img_size"], DEV)]
    cam_cfg = {"img_size": L["img_size"], "fov_ang": 6, "dist_radius": 0.12}
    ncfg = {"N_samples": L["N_samples"], "perturb": False, "static_viewdirs": True}
    return G, cu(sr), cu(sd), nb, cam_cfg, ncfg


def _run_loop(proj, G, sr, sd, nb, cam_cfg, ncfg, target, camera):
    L = FC.LOOP
    if camera == "axis_angle":
        p = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 1.0]], device=DEV, requires_grad=True)
        kw = lambda: dict(rot=p[:, :3], trans=p[:, 3:], camera="axis_angle")
    else:
        p = torch.zeros(1, 2, device=DEV, requires_grad=True)
        kw = lambda: dict(rot=p)
    opt = torch.optim.Adam([p], lr=L["lr"], betas=(0.9, 0.999))
    losses = []
    for step in range(L["steps"] + 1):                   # (the last pass only evaluates)
        thumb = proj.g_forward(G, sr, sd, nb, cam_cfg, ncfg, **kw())[1]
        loss = 50.0 * ((thumb - target) ** 2).mean()
        losses.append(loss.detach())
        if step == L["steps"]:
            break
        opt.param_groups[0]["lr"] = L["lr"] * cur_lr(step, L["steps"])
        opt.zero_grad()
        loss.backward()
        opt.step()
    losses = [float(v) for v in torch.stack(losses).cpu()]
    return losses, p.detach().cpu()


def test_axis_angle_camera_recovers_an_in_plane_roll_and_look_at_cannot():
    """Target: the generator's own thumbnail at rot = (0, 0, 0.2), trans = (0, 0, 1).  80 Adam steps at lr 0.02 with cur_lr's ramp
    over the camera leaves only, loss 50 MSE(thumb): the free camera ends at <= 1/100 of its initial loss with |rot_z - 0.2| <=
    0.01; the look-at camera stays at >= 0.9 of it.  (The fp32 CPU-oracle run of this set-up: 2.64e-3 -> 9.9e-8, rot_z 0.2005;
    look-at 0.947.)"""
    G, sr, sd, nb, cam_cfg, ncfg = _loop_generator()
    proj = FlipProjector(G, DEV)
    with torch.no_grad():
        target = proj.g_forward(G, sr, sd, nb, cam_cfg, ncfg, rot=torch.tensor([[0.0, 0.0, FC.ROLL]], device=DEV),
                                trans=torch.tensor([[0.0, 0.0, 1.0]], device=DEV), camera="axis_angle")[1].clone()
    free, p = _run_loop(proj, G, sr, sd, nb, cam_cfg, ncfg, target, "axis_angle")
    print(f"axis_angle: {free[0]:.4e} -> {free[-1]:.4e} (ratio {free[-1] / free[0]:.3e}), rot {p[0, :3].tolist()} trans {p[0, 3:].tolist()}")
    look, q = _run_loop(proj, G, sr, sd, nb, cam_cfg, ncfg, target, "look_at")
    print(f"look_at: {look[0]:.4e} -> {look[-1]:.4e} (ratio {look[-1] / look[0]:.3f}), (azim, elev) {q[0].tolist()}")
    assert free[0] > 0 and free[-1] <= free[0] / 100
    assert abs(float(p[0, 2]) - FC.ROLL) <= 0.01
    assert look[0] == free[0]                                 # the same start: the frontal camera, bit for bit
    assert look[-1] >= 0.9 * look[0]
    with pytest.raises(ValueError, match="camera"):
        proj.g_forward(G, sr, sd, nb, cam_cfg, ncfg, rot=torch.zeros(1, 3, device=DEV), trans=torch.zeros(1, 3, device=DEV),
                       camera="euler")


def test_project_wplus_with_the_free_camera():
    G, _, _, _, cam_cfg, ncfg = _loop_generator()
    proj = FlipProjector(G, DEV)
    g = torch.Generator().manual_seed(3)
    S = cam_cfg["img_size"]
    t_rgb, t_thumb = cu(torch.randn(2, 3, 4 * S, 4 * S, generator=g)).clamp(-1, 1), cu(torch.randn(2, 3, S, S, generator=g)).clamp(-1, 1)
    loss_fn = surrogate_loss(t_rgb, t_thumb)
    out = proj.project_wplus(cam_cfg, ncfg, loss_fn, N_steps_pose=3, N_steps_app=2, w_avg_samples=64, camera="axis_angle",
                             optim_fov=True)
    assert out["azim"] is None and out["elev"] is None
    assert out["rot"].shape == (2, 3) and out["trans"].shape == (2, 3) and out["fov"].shape == (2,)
    assert out["cam_poses"].shape == (2, 3, 4)
    assert out["loss_history"].shape == (5,) and bool(torch.isfinite(out["loss_history"]).all())
    start_t = torch.tensor([[0.0, 0.0, 1.0]] * 2, device=DEV)
    assert float(out["rot"].abs().max()) > 0 and not torch.equal(out["trans"], start_t)
    assert float((out["fov"] - 6.0).abs().min()) > 0
    # trans is the optimiser's own value -- not renormalised in place -- and cam_poses shows its normalised form
    ref = hip.camera_axis_angle(out["rot"], out["trans"], S, out["fov"], 0.12)[0]
    assert torch.equal(out["cam_poses"], ref)
    n = out["trans"] / out["trans"].norm(dim=1, keepdim=True)
    assert float((out["cam_poses"][:, :, 3] - n).abs().max()) < 1e-6
    base = proj.project_wplus(cam_cfg, ncfg, loss_fn, N_steps_pose=3, N_steps_app=2, w_avg_samples=64)
    assert not ({"rot", "trans", "fov", "cam_poses"} & set(base)) and base["azim"].shape == (2, 1)
    assert set(out) - set(base) == {"rot", "trans", "fov", "cam_poses"}


# ------------------------------------------------------------------------------------------------ 6. new views of a pose
def test_cameras_around_the_frontal_pose_are_the_trajectory_cameras():
    traj = torch.tensor([[0.3, 0.1, 6.0], [-0.77, 0.0, 8.0], [0.0, -0.15, 12.0]])
    frontal = torch.eye(3, 4)
    frontal[2, 3] = 1.0
    got = cameras_around_pose(frontal, traj, 64, DEV)
    ref = Camera.generate_camera_params(64, DEV, locations=cu(traj[:, :2]), fov_ang=cu(traj[:, 2]), dist_radius=0.12)[:4]
    assert float((got[0] - ref[0]).abs().max()) < 1e-6            # (fp32 rounding of entries <= 1: a few ulps of products and sums)
    assert float(((got[1] - ref[1]) / ref[1]).abs().max()) < 1e-6
    assert torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])


def test_multi_view_around_the_frontal_base_pose_is_the_plain_sequence():
    from cips_3dplusplus_amd.multiview import sample_multi_view
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=6)
    g = torch.Generator().manual_seed(8)
    zs = [cu(torch.randn(1, 32, generator=g)), cu(torch.randn(1, 32, generator=g))]
    G.style_render_mean, G.style_decoder_mean = cu(0.2 * torch.randn(1, 32, generator=g)), cu(0.2 * torch.randn(1, 32, generator=g))
    nb = [cu(torch.randn(*b.shape, generator=g)) for b in G.create_noise_bufs(8, "cpu")]
    cam_cfg = {"img_size": 8, "fov_ang": 6, "dist_radius": 0.12}
    kw = dict(view_mode="yaw", N_frames=2, truncation_ratio=0.5, N_samples=6, noise_bufs=nb, gather=("rgb",))
    a = sample_multi_view(G, cam_cfg, {"static_viewdirs": True}, zs, **kw)
    frontal = torch.eye(3, 4, device=DEV)
    frontal[2, 3] = 1.0
    b = sample_multi_view(G, cam_cfg, {"static_viewdirs": True}, zs, base_pose=frontal, base_fov=6.0, **kw)
    assert a["rgb"].dtype == torch.uint8 and a["rgb"].shape == b["rgb"].shape and a["rgb"].shape[0] == 2
    assert int((a["rgb"].int() - b["rgb"].int()).abs().max()) <= 1
    # a rolled base pose is another picture
    rolled = hip.camera_axis_angle(torch.tensor([[0.0, 0.0, 0.5]], device=DEV), torch.tensor([[0.0, 0.0, 1.0]], device=DEV), 8)[0]
    c = sample_multi_view(G, cam_cfg, {"static_viewdirs": True}, zs, base_pose=rolled, **kw)
    assert int((a["rgb"].int() - c["rgb"].int()).abs().max()) > 1
    with pytest.raises(ValueError, match="base_pose"):
        sample_multi_view(G, cam_cfg, {"static_viewdirs": True}, zs, base_pose=frontal, **{**kw, "view_mode": "translate_rotate"})
