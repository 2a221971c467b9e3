"""Shared cases and float64 references of the free-camera tests (test_free_camera_host.py, test_gpu_free_camera.py): the pose
table of the axis-angle kernel with its matrix_exp oracle, the CPU-oracle graphs of the focal gradient, and the set-up of the
roll-recovery loop.  Nothing here touches a device; references are computed once (lru_cache) and handed out unchanged."""
import functools
import math

import torch
import torch.nn.functional as F

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs
from oracle import path as O

SERIES_THETA = 0.5              # sqrt(SERIES_S) of csrc/camera_free.hip: below it the Taylor series in s = theta^2
ANGLES = (0.0, 1e-8, SERIES_THETA - 1e-3, SERIES_THETA + 1e-3, 0.5, math.pi - 1e-3, 4.0)
AXES = ((0.0, 0.0, 1.0), (0.36, -0.48, 0.8), (-0.6, 0.0, 0.8), (1.0, 0.0, 0.0))          # unit vectors
TRANS = ((0.0, 0.0, 1.0), (0.3, -0.7, 1.9), (6e-14, 0.0, 8e-14))                         # start, generic, below the eps clamp
FOVS = (6.0, 12.0, 3.5)


@functools.lru_cache(maxsize=None)
def pose_table(B):
    """rot [B,3], trans [B,3], fov [B] (float32).  Row 0 is the start point of every inversion; the rows walk ANGLES fastest, so
    the first 3 hold 0, 1e-8 and the lower side of the threshold, and 65 rows hold every (angle, axis, trans) combination that
    matters at least once (7 x 4 x 3 = 84 > 65: the axis and the trans cycle with different periods)."""
    rot, trans, fov = [], [], []
    for i in range(B):
        th, ax, tr = ANGLES[i % len(ANGLES)], AXES[(i // len(ANGLES) + i) % len(AXES)], TRANS[(i // 2 + i // 7) % len(TRANS)]
        if i == 0:
            ax, tr = AXES[0], TRANS[0]
        rot.append([th * a for a in ax])
        trans.append(list(tr))
        fov.append(FOVS[i % len(FOVS)])
    return (torch.tensor(rot, dtype=torch.float32), torch.tensor(trans, dtype=torch.float32),
            torch.tensor(fov, dtype=torch.float32))


def skew64(r):
    z = torch.zeros_like(r[:, 0])
    return torch.stack([z, -r[:, 2], r[:, 1], r[:, 2], z, -r[:, 0], -r[:, 1], r[:, 0], z], -1).reshape(-1, 3, 3)


def pose64(rot, trans):
    """float64 oracle of the pose: [matrix_exp([rot]x) | trans / max(|trans|, 1e-12)] (what pytorch3d's axis_angle_to_matrix and
    F.normalize compute)."""
    R = torch.linalg.matrix_exp(skew64(rot.double()))
    return torch.cat([R, F.normalize(trans.double(), p=2, dim=1, eps=1e-12).unsqueeze(-1)], -1)


def focal64(fov, img_size):
    return 0.5 * img_size / torch.tan(fov.double() * math.pi / 180)


@functools.lru_cache(maxsize=None)
def pose_jacobian(B, img_size=64):
    """(J_rot [B,12,3], J_trans [B,12,3], J_fov [B]) in float64: d extrinsics / d rot, / d trans per view (torch autograd through
    matrix_exp and F.normalize) and d focal / d fov."""
    rot, trans, fov = (t.double() for t in pose_table(B))
    f = lambda r, t: pose64(r, t).reshape(B, 12)
    Jr, Jt = torch.autograd.functional.jacobian(f, (rot, trans))         # [B,12,B,3] each
    idx = torch.arange(B)
    Jf = torch.autograd.functional.jacobian(lambda v: focal64(v, img_size), fov)[idx, idx]
    return Jr[idx, :, idx, :], Jt[idx, :, idx, :], Jf


# ------------------------------------------------------------------------------------------------ focal gradient vs the oracle
FOCAL_CASES = [(2, False, False, 6, 8),
               (3, True, True, 5, 8),           # static view directions: the dV term
               (2, False, True, 2, 8),          # all but the first slices of the camera chain empty
               (2, False, True, 17, 8),         # the last slices empty
               (2, False, True, 36, 8),
               (2, False, False, 6, 12)]        # R = 144: a ragged third workgroup
FOCAL_TERMS = ("ft", "all")


def leaf(t):
    return t.clone().requires_grad_(True)


def focal_loss(term, m, t, to=lambda v: v):
    ft = (m["features"] * to(t["F"])).sum() + 3.0 * (m["thumb"] * to(t["T"])).sum()
    if term == "ft":
        return ft
    return ft + (m["mask"] * to(t["M"])).sum() + 10.0 * (m["depth"] * to(t["D"])).sum() + 10.0 * (m["xyz"] * to(t["X"])).sum()


def _oracle_grads(sd, cam, styles, u, t, D, static, N, S, dtype):
    B, R = 2, S * S
    c = lambda v: None if v is None else v.to(dtype)
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    cr, fr = leaf(c(cam[0])), leaf(c(cam[1]))
    rays_o, rays_d, viewdirs = O.rays_in_world(fr, S, cr, static)
    z = O.z_vals(c(cam[2]), c(cam[3]), B, S, S, N, c(u))
    pts = O.ray_points(rays_o, rays_d, z)
    thumb, feat, sdf, mask, xyz = O.renderer_forward(sdd, "renderer", pts.reshape(B, R, N, 3), rays_d.reshape(B, R, 3),
                                                     viewdirs.reshape(B, R, 3), z.reshape(B, R, N), c(cam[2]), c(cam[3]),
                                                     c(styles), D)
    to_img = lambda v: v.transpose(1, 2).reshape(B, v.shape[-1], S, S)
    maps = {"features": to_img(feat), "thumb": to_img(thumb), "mask": to_img(mask)[:, 0], "depth": to_img(mask)[:, 1],
            "xyz": to_img(xyz)}
    grads = {}
    for term in FOCAL_TERMS:
        dfoc, dcam = torch.autograd.grad(focal_loss(term, maps, t, c), [fr, cr], retain_graph=True)
        grads[term] = (dfoc.reshape(B).clone(), dcam.clone())
    return grads


@functools.lru_cache(maxsize=None)
def focal_oracle_case(D, static, perturb, N, S, device):
    """The harness of test_gpu_geom_grad.py::_oracle_case with `focal` a leaf of O.rays_in_world: one fp32 CPU-oracle graph per
    case, d loss / d focals [B] (and d cam_poses) of both losses taken from it and kept."""
    cfg = configs.tiny_G_cfg(32, D, 1)
    G = pkg.build_generator(cfg, device, seed=3)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(D + N)
    B, H = 2, 32
    locs = torch.tensor([[0.25, 0.1], [-0.4, -0.05]])
    cam = O.camera_params(locs, S, 6, 0.12)
    styles = 0.5 * torch.randn(B, D + 1, 32, generator=g)
    u = torch.rand(B, S, S, 1, generator=g) if perturb else None
    t = {"F": torch.randn(B, H, S, S, generator=g), "T": torch.randn(B, 3, S, S, generator=g),
         "M": torch.randn(B, S, S, generator=g), "D": torch.randn(B, S, S, generator=g), "X": torch.randn(B, 3, S, S, generator=g)}
    grads = _oracle_grads(sd, cam, styles, u, t, D, static, N, S, torch.float32)
    return G, sd, cam, styles, u, t, grads


# ------------------------------------------------------------------------------------------------ the roll-recovery loop
ROLL = 0.2
LOOP = dict(hidden=32, depth=2, seed=2, img_size=8, N_samples=6, steps=80, lr=0.02)


def loop_inputs():
    """Fixed styles of the loop test (CPU float32): (style_render [1,3,32], style_decoder [1,n_latent,32] is built by the caller
    from the generator's n_latent with the same generator)."""
    g = torch.Generator().manual_seed(11)
    return 0.5 * torch.randn(1, LOOP["depth"] + 1, 32, generator=g), g
