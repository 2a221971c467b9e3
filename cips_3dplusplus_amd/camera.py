"""Camera sampling and demo trajectories (host-side front end of the generator call).

`Camera.generate_camera_params` keeps the reference signature and return tuple
(/root/reference/exp/cips3d/nerf_utils.py:344-436; `_v1` with a custom up vector :466-564): the
random draws (azim/elev) are made with torch's device RNG exactly where the reference makes them,
the pose arithmetic runs in csrc/camera.hip.  Trajectories restate the three view modes of
`_sample_multi_view_web` (exp/cips3d/models/render_video_web_v10.py:1587-1649,1732-1783).
"""
import math

import torch

from . import hip


class Camera(object):
    @staticmethod
    def _angles(batch, device, locations, sweep, uniform, azim_range, elev_range):
        if locations is not None:
            return locations[:, 0].reshape(-1, 1), locations[:, 1].reshape(-1, 1), None
        if sweep:
            if isinstance(azim_range, list) and isinstance(elev_range, list):
                azim = (azim_range[0] + (azim_range[1] - azim_range[0]) / 7 * torch.arange(8, device=device)).view(-1, 1).repeat(batch, 1)
                elev = elev_range[0] + (elev_range[1] - elev_range[0]) * torch.rand(batch, 1, device=device).repeat(1, 8).view(-1, 1)
            else:
                azim = (-azim_range + (2 * azim_range / 7) * torch.arange(8, device=device)).view(-1, 1).repeat(batch, 1)
                elev = -elev_range + 2 * elev_range * torch.rand(batch, 1, device=device).repeat(1, 8).view(-1, 1)
            return azim, elev, 8
        if uniform:
            if isinstance(azim_range, list) and isinstance(elev_range, list):
                azim = azim_range[0] + (azim_range[1] - azim_range[0]) * torch.rand(batch, 1, device=device)
                elev = elev_range[0] + (elev_range[1] - elev_range[0]) * torch.rand(batch, 1, device=device)
            else:
                azim = -azim_range + 2 * azim_range * torch.rand(batch, 1, device=device)
                elev = -elev_range + 2 * elev_range * torch.rand(batch, 1, device=device)
        else:
            azim = azim_range * torch.randn(batch, 1, device=device)
            elev = elev_range * torch.randn(batch, 1, device=device)
        return azim, elev, None

    @staticmethod
    def generate_camera_params_v1(img_size, device, batch=1, locations=None, sweep=False, uniform=False,
                                  azim_range=0.3, elev_range=0.15, fov_ang=6, dist_radius=0.12, up=None):
        if locations is not None and locations.dim() == 2 and locations.shape[1] == 2:
            # (azim, elev) given: they ARE the viewpoint -- no column selects and re-concatenation (seven launches of autograd
            # plumbing per inversion step when `locations` carries gradients)
            viewpoint = locations.float()
        else:
            azim, elev, _ = Camera._angles(batch, device, locations, sweep, uniform, azim_range, elev_range)
            viewpoint = torch.cat([azim, elev], 1).float()
        n = viewpoint.shape[0]
        fov = fov_ang
        if torch.is_tensor(fov_ang) and fov_ang.numel() not in (1, n):
            raise RuntimeError("fov_ang tensor must have 1 or B elements")
        if torch.is_grad_enabled() and viewpoint.requires_grad:
            # inversion: the pose is optimised through `locations` (projector_v10.py:227-232)
            from .autograd import CameraFn
            extr, focal, near, far = CameraFn.apply(viewpoint.to(device), img_size, fov, dist_radius, up)
        else:
            extr, focal, near, far = hip.camera_params(viewpoint.to(device), img_size, fov, dist_radius, up=up)
        return extr, focal, near, far, viewpoint

    @staticmethod
    def generate_camera_params(img_size, device, batch=1, locations=None, sweep=False, uniform=False,
                               azim_range=0.3, elev_range=0.15, fov_ang=6, dist_radius=0.12):
        return Camera.generate_camera_params_v1(img_size, device, batch, locations, sweep, uniform, azim_range,
                                                elev_range, fov_ang, dist_radius, up=None)

    @staticmethod
    def get_camera2world(cam2world, trans, homo=False):
        """cips3d/nerf_utils.py:439-463: cam2world [..., 3] axis-angle, trans [..., 3] -> [..., 3, 4] = [exp([r]x) | trans]
        (or [..., 4, 4] with the row (0, 0, 0, 1)).  Nothing is normalised here -- the reference's projector normalises `trans`
        before the call.  The rotation is Rodrigues' formula as a torch expression (what pytorch3d's axis_angle_to_matrix
        computes), on any device and differentiable; the loop's one-launch form is `free_camera_params`."""
        assert cam2world.shape[:-1] == trans.shape[:-1]
        prefix = cam2world.shape[:-1]
        r = cam2world.reshape(-1, 3)
        s = (r * r).sum(-1)
        small = s < 1e-4                          # (the series there: the quotients' rounding would be divided by s)
        s_ = torch.where(small, torch.ones_like(s), s)
        t = torch.sqrt(s_)
        a = torch.where(small, 1 - s / 6 + s * s / 120, torch.sin(t) / t)
        b = torch.where(small, 0.5 - s / 24 + s * s / 720, (1 - torch.cos(t)) / s_)
        z = torch.zeros_like(s)
        K = torch.stack([z, -r[:, 2], r[:, 1], r[:, 2], z, -r[:, 0], -r[:, 1], r[:, 0], z], -1).reshape(-1, 3, 3)
        rot_m = torch.eye(3, dtype=r.dtype, device=r.device) + a.view(-1, 1, 1) * K + b.view(-1, 1, 1) * (K @ K)
        extr = torch.cat((rot_m.view(*prefix, 3, 3), trans.view(*prefix, 3, 1)), dim=-1)
        if homo:
            extend = torch.zeros(*prefix, 1, 4, dtype=extr.dtype, device=extr.device)
            extend[..., 0, 3] = 1.
            extr = torch.cat((extr, extend), dim=-2)
        return extr

    @staticmethod
    def free_camera_params(img_size, device, rot, trans, fov_ang=6, dist_radius=0.12):
        """The free camera of the axis-angle projector in ONE launch (hip.camera_axis_angle): rot [B,3] axis-angle, trans [B,3]
        (normalised onto the unit sphere inside, F.normalize) -> (extrinsics [B,3,4], focal, near, far [B,1,1]).  Differentiable
        w.r.t. rot, trans and a tensor fov_ang when one of them requires grad (autograd.CameraAxisAngleFn)."""
        rot, trans = rot.to(device), trans.to(device)
        if torch.is_tensor(fov_ang):
            if fov_ang.numel() not in (1, rot.shape[0]):
                raise RuntimeError("fov_ang tensor must have 1 or B elements")
            fov_ang = fov_ang.to(device)
        if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (rot, trans, fov_ang)):
            from .autograd import CameraAxisAngleFn
            return CameraAxisAngleFn.apply(rot, trans, img_size, fov_ang, dist_radius)
        return hip.camera_axis_angle(rot, trans, img_size, fov_ang, dist_radius)


# ---------------------------------------------------------------------------------------- trajectories
def yaw_trajectory(n_frames, azim_range=(-0.77, 0.77), elev=0.0, fov=6.0):
    """render_video_web_v10.py:1733-1739: azim = a0 + (a1-a0) sin(pi t); columns (azim, elev, fov)."""
    t = torch.linspace(0, 1, n_frames, dtype=torch.float64)
    traj = torch.zeros(n_frames, 3, dtype=torch.float32)
    traj[:, 0] = (azim_range[0] + (azim_range[1] - azim_range[0]) * torch.sin(t * math.pi)).float()
    traj[:, 1] = elev
    traj[:, 2] = fov
    return traj


def circle_trajectory(n_frames, azim_range=0.5, elev=0.0, fov_range=(6.0, 8.0)):
    """render_video_web_v10.py:1764-1775."""
    t = torch.linspace(0, 1, n_frames, dtype=torch.float64)
    traj = torch.zeros(n_frames, 3, dtype=torch.float32)
    traj[:, 0] = (azim_range * torch.sin(t * 2 * math.pi)).float()
    traj[:, 1] = elev
    traj[:, 2] = (fov_range[0] + (fov_range[1] - fov_range[0]) * torch.sin(t * math.pi)).float()
    return traj


def roll_up_vectors(n_frames):
    """render_video_web_v10.py:1625-1633: up = (cos a, sin a, 0), a = 2 pi t + pi/2 (in-plane roll)."""
    t = torch.linspace(0, 1, n_frames)
    a = t * 2 * math.pi + 0.5 * math.pi
    return torch.stack([torch.cos(a), torch.sin(a), torch.zeros(n_frames)], dim=1)


def cameras_from_trajectory(traj, img_size, device, dist_radius=0.12, up=None):
    """(azim, elev, fov) rows -> (extrinsics, focal, near, far) on `device`."""
    traj = traj.to(device)
    e, f, n, fa, _ = Camera.generate_camera_params_v1(img_size, device, locations=traj[:, :2].contiguous(),
                                                      fov_ang=traj[:, 2].contiguous(), dist_radius=dist_radius,
                                                      up=None if up is None else up.to(device))
    return e, f, n, fa


def cameras_around_pose(base_extr, traj, img_size, device, dist_radius=0.12):
    """Rows (d azim, d elev, fov) of `traj` as offsets around a given pose base_extr [3,4] (an inverted subject's camera): row i
    gives Ry(d azim) Rx(-d elev) base -- a WORLD rotation of the whole camera, applied to its axes and to its origin -- with the
    row's field of view.  For the frontal base (identity, origin (0,0,1)) this is the pose cameras_from_trajectory makes.
    -> (extrinsics [n,3,4], focal, near, far [n,1,1]) on `device`; a torch expression of a dozen small ops per call (a
    sequence calls it once), the intrinsics as everywhere else."""
    traj = traj.to(device=device, dtype=torch.float32)
    base = base_extr.detach().to(device=device, dtype=torch.float32).reshape(3, 4)
    n = traj.shape[0]
    az, el = traj[:, 0], traj[:, 1]
    ca, sa, ce, se = torch.cos(az), torch.sin(az), torch.cos(el), torch.sin(el)
    z, o = torch.zeros_like(az), torch.ones_like(az)
    ry = torch.stack([ca, z, sa, z, o, z, -sa, z, ca], -1).reshape(n, 3, 3)
    rx = torch.stack([o, z, z, z, ce, se, z, -se, ce], -1).reshape(n, 3, 3)       # Rx(-d elev)
    extr = (ry @ rx) @ base.unsqueeze(0)
    fov = traj[:, 2].double() * math.pi / 180
    focal = (0.5 * img_size / torch.tan(fov)).float().reshape(n, 1, 1)
    near = torch.full((n, 1, 1), 1.0 - dist_radius, device=traj.device)
    far = torch.full((n, 1, 1), 1.0 + dist_radius, device=traj.device)
    return extr.contiguous(), focal, near, far


def translate_rotate_cameras(n_frames, trans_max, img_size, device, fov_ang=6.0, dist_radius=0.12):
    """render_video_web_v10.py:1587-1649: first a sideways translation of a frontal camera at z = 1
    (x = trans_max sin(2 pi t), identity rotation), then an in-plane roll of the frontal camera (custom up vectors).
    Returns (extrinsics [2n,3,4], trajectory [2n,3], focal, near, far)."""
    t = torch.linspace(0, 1, n_frames)
    ext_t = torch.zeros(n_frames, 3, 4, device=device)
    ext_t[:, :, :3] = torch.eye(3, device=device)
    ext_t[:, 0, 3] = (trans_max * torch.sin(t * 2 * math.pi)).to(device)
    ext_t[:, 2, 3] = 1
    traj = torch.zeros(n_frames, 3)
    traj[:, 2] = fov_ang
    _, f_t, n_t, fa_t = cameras_from_trajectory(traj, img_size, device, dist_radius)
    ext_r, f_r, n_r, fa_r = cameras_from_trajectory(traj, img_size, device, dist_radius, up=roll_up_vectors(n_frames))
    cat = lambda a, b: torch.cat([a, b], 0)
    return cat(ext_t, ext_r), cat(traj, traj).to(device), cat(f_t, f_r), cat(n_t, n_r), cat(fa_t, fa_r)
