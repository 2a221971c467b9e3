"""Host checks of the free camera (csrc/camera_free.hip, the focal entry points of csrc/nerf_bwd.hip / nerf_bwd_fused.hip, and
the Python surface on them): the C ABI's declarations and argument checks, the knobs' errors, the checkpoint keys, and the torch
expressions that run without a device.  Nothing here launches a kernel."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from cips_3dplusplus_amd import _lib, build, checkpoint, configs, projector as P
from cips_3dplusplus_amd.camera import Camera, cameras_around_pose
from oracle import path as O
import _free_camera_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cips3d_camera_axis_angle", "cips3d_camera_axis_angle_bwd", "cips3d_nerf_bwd_camera",
                "cips3d_nerf_bwd_fused")


def test_abi_exports_and_version():
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    for s in ENTRY_POINTS:
        assert s in _lib.EXPORTED and s in _lib._SIGS and hasattr(raw, s), s
        assert re.search(r"\b%s\(" % s, header), s
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 48
    # the focal gradient of the fused route is an argument of the entry point: the params struct keeps its layout
    assert lib.cips3d_sizeof_struct(7) == ctypes.sizeof(_lib.NerfBwdFusedParams)
    assert "camera_free.hip" in build.SOURCES


def test_library_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    one = ctypes.cast(ctypes.pointer(ctypes.c_float(0.0)), ctypes.c_void_p).value       # a non-null host address: never read
    fwd, bwd = lib.cips3d_camera_axis_angle, lib.cips3d_camera_axis_angle_bwd
    ok_f = [one, one, None, 6.0, 0.12, 8, 1, one, one, one, one, None]
    for i in (0, 1, 7, 8, 9, 10):                                                       # rot, trans, the four outputs
        a = list(ok_f)
        a[i] = None
        assert fwd(*a) == -1, i
    assert fwd(*(ok_f[:6] + [-1] + ok_f[7:])) == -1                                     # B < 0
    assert fwd(*(ok_f[:5] + [0] + ok_f[6:])) == -1                                      # img_size
    assert fwd(*(ok_f[:6] + [0] + ok_f[7:])) == 0                                       # an empty batch is a no-op
    ok_b = [one, one, None, 6.0, 8, None, None, 1, one, one, None, None]
    for i in (0, 1, 8, 9):                                                              # rot, trans, drot, dtrans
        a = list(ok_b)
        a[i] = None
        assert bwd(*a) == -1, i
    assert bwd(*(ok_b[:7] + [-3] + ok_b[8:])) == -1
    assert bwd(*(ok_b[:7] + [0] + ok_b[8:])) == 0
    geom = _lib.NerfBwdGeom()
    geom.cam_poses = geom.focals = geom.near_ = geom.far_ = one
    geom.B, geom.img_size, geom.n_samples, geom.static_viewdirs = 1, 2, 4, 0
    gp = ctypes.byref(geom)
    cam = lib.cips3d_nerf_bwd_camera                                                    # (dfocal non-null throughout)
    assert cam(None, one, one, one, None, None, None, None, None, 0, one, one, None) == -1
    assert cam(gp, one, one, one, None, None, None, None, None, 0, None, one, None) == -1      # no dcam
    assert cam(gp, one, one, one, one, None, None, one, one, 0, one, one, None) == -1          # d_mask without xyz
    geom.B = -1
    assert cam(gp, one, one, one, None, None, None, None, None, 0, one, one, None) == -1
    geom.B = 0
    assert cam(gp, one, one, one, None, None, None, None, None, 1, one, one, None) == 0
    assert lib.cips3d_nerf_bwd_fused(None, one, None) == -1
    assert lib.cips3d_nerf_bwd_fused(ctypes.byref(_lib.NerfBwdFusedParams()), one, None) == -1


def test_default_surfaces_are_unchanged():
    sig = inspect.signature(P.FlipProjector.project_wplus).parameters
    assert sig["camera"].default == "look_at" and sig["optim_fov"].default is False
    assert sig["rot_init"].default is None and sig["trans_init"].default is None and sig["lr_fov"].default > 0
    g = inspect.signature(P.FlipProjector.g_forward).parameters
    assert g["camera"].default == "look_at" and g["fov"].default is None
    assert list(g)[:10] == ["self", "G", "style_render", "style_decoder", "noise_bufs", "cam_cfg", "nerf_cfg", "rot", "trans",
                            "flip_w_decoder"]
    from cips_3dplusplus_amd import hip, multiview
    for f in (hip.nerf_backward, hip.nerf_backward_fused):
        assert inspect.signature(f).parameters["d_focal"].default is False
    mv = inspect.signature(multiview.sample_multi_view).parameters
    assert mv["base_pose"].default is None and mv["base_fov"].default is None
    assert inspect.signature(Camera.get_camera2world).parameters["homo"].default is False
    assert list(inspect.signature(Camera.free_camera_params).parameters) == ["img_size", "device", "rot", "trans", "fov_ang",
                                                                              "dist_radius"]
    assert checkpoint.INVERSION_KEYS == ("azim", "elev", "w_render_opt", "w_decoder_opt", "render_state_dict",
                                         "decoder_state_dict", "noise_bufs", "padding")


@pytest.mark.parametrize("kw", [dict(camera="euler"), dict(camera=None), dict(optim_fov=True),
                                dict(camera="look_at", optim_fov=True)])
def test_project_wplus_refuses_unknown_cameras_before_anything_is_built(kw):
    proj = P.FlipProjector(G=None, device="cpu")                             # (raises before the generator is touched)
    with pytest.raises(ValueError, match="camera"):
        proj.project_wplus({"img_size": 8, "fov_ang": 6, "dist_radius": 0.12}, {"N_samples": 4}, lambda rgb, thumb: rgb.sum(),
                           N_steps_pose=1, **kw)


def test_checkpoint_keys_and_the_camera_of_a_file(tmp_path):
    import cips_3dplusplus_amd as pkg
    G = pkg.Generator(**configs.tiny_G_cfg(32, 2, 1))
    w_r, w_d = torch.zeros(1, 3, 32), torch.zeros(2, G.decoder.n_latent, 32)
    azim, elev = torch.tensor([[0.3], [-0.3]]), torch.tensor([[0.1], [0.1]])
    p0 = checkpoint.save_inversion(str(tmp_path / "look_at.pth"), azim, elev, w_r, w_d, G)
    assert tuple(torch.load(p0, weights_only=True)) == checkpoint.INVERSION_KEYS       # exactly, and in order
    assert len(checkpoint.load_inversion(p0)) == 7
    pose, fov = checkpoint.load_inversion_camera(p0, w_idx=1)
    assert pose.shape == (1, 3, 4) and fov is None
    assert float((pose - O.camera_params(torch.tensor([[-0.3, 0.1]]), 64, 6, 0.12)[0]).abs().max()) < 1e-6
    rot, trans = torch.tensor([[0.0, 0.0, 0.2], [0.1, -0.2, 0.3]]), torch.tensor([[0.0, 0.0, 1.3], [0.2, 0.1, 0.9]])
    fv = torch.tensor([6.5, 5.5])
    p1 = checkpoint.save_inversion(str(tmp_path / "free.pth"), None, None, w_r, w_d, G, rot=rot, trans=trans, fov=fv)
    kw = torch.load(p1, weights_only=True)
    assert tuple(kw) == checkpoint.INVERSION_KEYS + ("rot", "trans", "fov") and kw["azim"] is None
    pose, fov = checkpoint.load_inversion_camera(p1, w_idx=1)
    assert fov == 5.5 and float((pose.double() - FC.pose64(rot[1:], trans[1:])).abs().max()) <= 2.0 ** -23
    p2 = checkpoint.save_inversion(str(tmp_path / "free_nofov.pth"), None, None, w_r, w_d, G, rot=rot, trans=trans)
    assert "fov" not in torch.load(p2, weights_only=True) and checkpoint.load_inversion_camera(p2)[1] is None


def test_get_camera2world_is_rodrigues_without_normalisation():
    """The reference's name and signature (a torch expression: it runs here on the CPU), against float64 matrix_exp."""
    rot, trans, _ = FC.pose_table(65)
    ref = FC.pose64(rot, trans)
    got = Camera.get_camera2world(rot.double(), trans.double())
    assert got.shape == (65, 3, 4)
    assert float((got[:, :, :3] - ref[:, :, :3]).abs().max()) < 1e-12
    assert torch.equal(got[:, :, 3], trans.double())                        # trans as given
    h = Camera.get_camera2world(rot.reshape(5, 13, 3), trans.reshape(5, 13, 3), homo=True)
    assert h.shape == (5, 13, 4, 4) and torch.equal(h[..., 3, :], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(5, 13, 4))
    assert float((h[..., :3, :3].reshape(65, 3, 3).double() - ref[:, :, :3]).abs().max()) < 1e-6
    r = torch.zeros(1, 3, requires_grad=True)
    Camera.get_camera2world(r, torch.zeros(1, 3))[0, 1, 0].backward()      # d R_10 / d r = e_z at the identity
    assert torch.equal(r.grad, torch.tensor([[0.0, 0.0, 1.0]]))


def test_cameras_around_the_frontal_pose_vs_the_oracle_cpu():
    """CPU tensors through cameras_around_pose's torch expression (the function is not device-only) against
    oracle.path.camera_params at three (azim, elev) rows."""
    traj = torch.tensor([[0.3, 0.1, 6.0], [-0.77, 0.0, 8.0], [0.0, -0.15, 12.0]])
    frontal = torch.eye(3, 4)
    frontal[2, 3] = 1.0
    extr, focal, near, far = cameras_around_pose(frontal, traj, 64, "cpu")
    for i in range(3):
        ref = O.camera_params(traj[i:i + 1, :2], 64, float(traj[i, 2]), 0.12)
        assert float((extr[i] - ref[0][0]).abs().max()) < 1e-6
        assert abs(float(focal[i]) / float(ref[1]) - 1) < 1e-6
        assert float(near[i]) == float(ref[2]) and float(far[i]) == float(ref[3])
    # a world rotation of the whole camera: a rolled base keeps its roll in the camera frame
    c, s = math.cos(0.4), math.sin(0.4)
    rolled = torch.tensor([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 1.0]])
    e2 = cameras_around_pose(rolled, traj, 64, "cpu")[0]
    assert float((e2[:, :, :3] - extr[:, :, :3] @ rolled[:, :3]).abs().max()) < 1e-6
    assert float((e2[:, :, 3] - extr[:, :, 3]).abs().max()) < 1e-6


def test_pose_oracle_of_the_gpu_tests_is_a_rotation_with_the_analytic_limit():
    """The float64 reference the GPU tests hold the kernel to: matrix_exp gives rotations, the start row is the frontal camera,
    and its Jacobian at theta = 0 is the generators [e_i]x."""
    rot, trans, fov = FC.pose_table(65)
    ref = FC.pose64(rot, trans)
    R = ref[:, :, :3]
    assert float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-14
    eye = torch.eye(3, 4, dtype=torch.float64)
    eye[2, 3] = 1.0
    assert torch.equal(ref[0], eye)
    assert {float(v) for v in rot.norm(dim=1).double().round(decimals=4)} >= {0.0, 0.499, 0.501, 0.5, 4.0}
    assert bool((trans.norm(dim=1) < 1e-12).any()) and float(F.normalize(trans.double(), dim=1, eps=1e-12).norm(dim=1).min()) < 0.2
    Jr, Jt, Jf = FC.pose_jacobian(3)
    gens = torch.stack([FC.skew64(torch.eye(3, dtype=torch.float64)[i:i + 1])[0] for i in range(3)], -1)      # [3,3,i]
    assert float((Jr[0].reshape(3, 4, 3)[:, :3] - gens).abs().max()) < 1e-14
    assert float(Jr[0].reshape(3, 4, 3)[:, 3].abs().max()) == 0 and bool((Jf < 0).all())
