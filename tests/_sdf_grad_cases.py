"""Shared recipe of the SDF-gradient tests (test_sdf_grad_host.py, test_gpu_sdf_grad.py, golden/make_sdf_grad_golden.py):
formula-generated renderer weights and inputs, and the oracle's gradient by autograd in a chosen precision."""
import torch

from cips_3dplusplus_amd import weights
from oracle import path as O

H = 256
NEAR, FAR = (0.88, 0.80, 0.95), (1.12, 1.25, 1.10)      # per view, distinct


def renderer_shapes(D, hidden=H):
    """state-dict shapes of VolumeFeatureRenderer(N_layers_renderer=D, hidden_dim = style_dim = hidden), names under renderer."""
    s = {"renderer.sigmoid_beta": (1,)}

    def film(prefix, cin):
        s[prefix + ".weight"], s[prefix + ".bias"] = (hidden, cin), (hidden,)
        for head in ("gamma", "beta"):
            s[f"{prefix}.{head}.weight"], s[f"{prefix}.{head}.bias"] = (hidden, hidden), (hidden,)
    film("renderer.network.pts_linears.0", 3)
    for i in range(1, D):
        film(f"renderer.network.pts_linears.{i}", hidden)
    film("renderer.network.views_linears", hidden + 3)
    s["renderer.network.rgb_linear.weight"], s["renderer.network.rgb_linear.bias"] = (3, hidden), (3,)
    s["renderer.network.sigma_linear.weight"], s["renderer.network.sigma_linear.bias"] = (1, hidden), (1,)
    return s


def synth_renderer_sd(D, hidden=H, seed=0):
    return weights.synth_state_dict(renderer_shapes(D, hidden), seed=seed)


def explicit_inputs(B, R, N, D, tag="sg", hidden=H):
    """Explicit-geometry inputs: distinct styles and near / far per view, jittered depths, rays around -z."""
    near = torch.tensor(NEAR[:B]).view(B, 1, 1)
    far = torch.tensor(FAR[:B]).view(B, 1, 1)
    rays_d = torch.nn.functional.normalize(weights.det_normal(tag + ".d", (B, R, 3), 0.2, R) + torch.tensor([0.0, 0.0, -1.0]), dim=-1) * 1.1
    viewdirs = torch.nn.functional.normalize(rays_d, dim=-1)
    rays_o = torch.tensor([0.0, 0.0, 1.0]).expand(B, R, 3) + weights.det_normal(tag + ".o", (B, R, 3), 0.05, R)
    u = weights.det_unit_uniform(tag + ".u", (B, R, 1, 1), R)
    z = O.z_vals(near, far, B, R, 1, N, perturb_u=u).reshape(B, R, N)
    pts = (rays_o.unsqueeze(-2) + rays_d.unsqueeze(-2) * z.unsqueeze(-1)).contiguous()
    styles = weights.det_normal(tag + ".styles", (B, D + 1, hidden), 0.5, D)
    return dict(pts=pts, rays_d=rays_d, viewdirs=viewdirs, z=z, near=near, far=far, styles=styles)


def oracle_sdf_grad(sd, inp, D, dt):
    """(sdf (B,R,N,1), d sdf / d pts (B,R,N,3)) of oracle.path.renderer_forward by autograd, everything in dtype dt."""
    sdd = {k: v.to(dt) if v.is_floating_point() else v for k, v in sd.items()}
    c = {k: v.detach().to(dt) for k, v in inp.items()}
    with torch.enable_grad():
        pts = c["pts"].clone().requires_grad_(True)
        sdf = O.renderer_forward(sdd, "renderer", pts, c["rays_d"], c["viewdirs"], c["z"], c["near"], c["far"], c["styles"], D)[2]
        g, = torch.autograd.grad(sdf, pts, torch.ones_like(sdf))
    return sdf.detach(), g.detach()


def camera_inputs(cam, S, N, perturb_u, static, dt, D, styles):
    """The oracle's rays / depths / points for a camera tuple (extr, focal, near, far, ...), as explicit inputs in dtype dt."""
    c = [t.to(dt) for t in cam[:4]]
    B = c[0].shape[0]
    ro, rd, vd = O.rays_in_world(c[1], S, c[0], static)
    z = O.z_vals(c[2], c[3], B, S, S, N, perturb_u=None if perturb_u is None else perturb_u.to(dt).view(B, S, S, 1))
    pts = O.ray_points(ro, rd, z)
    R = S * S
    return dict(pts=pts.reshape(B, R, N, 3), rays_d=rd.reshape(B, R, 3), viewdirs=vd.reshape(B, R, 3), z=z.reshape(B, R, N),
                near=c[2], far=c[3], styles=styles.to(dt))


def err_stats(x, ref64):
    """(max, rms) of x - ref64, in fp64."""
    d = x.double().reshape(ref64.shape) - ref64
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())
