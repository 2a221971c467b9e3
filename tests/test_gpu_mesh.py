"""Geometry export on the GPU (csrc/mesh.hip, cips_3dplusplus_amd/mesh.py): frustum alignment against the reference's
recorded output, marching cubes against the numpy oracle of tests/test_mesh_host.py, and the renderer-only surface
extraction against the renderer and the CPU oracle."""
import numpy as np
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, hip, mesh
from cips_3dplusplus_amd.camera import Camera
from conftest import maxdiff
from oracle import path as O
from test_mesh_host import assert_closed_oriented, euler, mc_numpy, random_field, sphere, torus

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def cu(t):
    return t.to(DEV)


def _mc(A, level=0.0, affine=None):
    v, f = hip.marching_cubes(cu(torch.from_numpy(np.ascontiguousarray(A))), level, affine)
    assert f.dtype == torch.int64 and v.dtype == torch.float32
    return v.cpu().numpy(), f.cpu().numpy()


# ------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("tag", ["a", "b"])
def test_align_volume_matches_reference(golden, tag):
    fx = golden("mesh_align")
    vin, ref = fx[f"align.{tag}.in"], fx[f"align.{tag}.out"]
    near, far = float(fx[f"align.{tag}.near"]), float(fx[f"align.{tag}.far"])
    out = mesh.align_volume(cu(vin), near, far).cpu()
    assert out.shape == ref.shape
    # out-of-frustum mask bit for bit: the reference writes exactly 1 there; the inside values are samples
    mask = (ref == 1.0)
    assert mask.any() and (~mask).any()
    assert torch.equal(out[mask], ref[mask])
    assert maxdiff(out, ref) < 1e-6
    out4 = mesh.align_volume(cu(vin[..., 0]), near, far).cpu()
    assert torch.equal(out4, out[..., 0])


def test_reference_vertex_frame(golden):
    fx = golden("mesh_align")
    sdf = fx["mc.in"]
    _, h, w, d, _ = sdf.shape
    # the array the reference meshes is sdf[0, ..., 0].permute(1, 0, 2): x <-> w, y <-> h, z <-> d
    assert torch.equal(fx["mc.sdf_vol"], sdf[0, ..., 0].permute(1, 0, 2))
    vi = fx["mc.verts_index"].numpy()
    aff = mesh.reference_affine(h, w, d)
    ours = np.stack([vi[:, a] * np.float32(aff[a][0]) + np.float32(aff[a][1]) for a in range(3)], 1)
    assert np.abs(ours - fx["mc.verts_out"].numpy()).max() < 1e-6


# ------------------------------------------------------------------------------------------------ marching cubes = oracle
FIELDS = {
    "random_12": lambda: random_field((12, 12, 12), 0),
    "random_nc": lambda: random_field((9, 17, 13), 1),
    "random_big": lambda: random_field((40, 33, 70), 2),
    "sphere_nc": lambda: sphere(24, 30, 20, 8.3),
    "torus": lambda: torus(32, 9.0, 3.5),
    "noisy": lambda: np.random.default_rng(5).standard_normal((7, 5, 6)).astype(np.float32),
}


@pytest.mark.parametrize("name", list(FIELDS))
def test_marching_cubes_equals_oracle(name):
    A = FIELDS[name]()
    h, w, d = A.shape
    for affine in (None, mesh.reference_affine(h, w, d)):
        v, f = _mc(A, 0.0, affine)
        rv, rf = mc_numpy(A, 0.0, affine)
        assert v.shape == rv.shape and f.shape == rf.shape
        assert len(f) > 0
        assert np.abs(v - rv).max() < 1e-6
        assert np.array_equal(f, rf)


def test_marching_cubes_level():
    A = sphere(20, 20, 20, 4.0)
    v, f = _mc(A, 2.5)
    rv, rf = mc_numpy(A, 2.5)
    assert np.array_equal(f, rf) and np.abs(v - rv).max() < 1e-6
    r = np.linalg.norm(v - 9.5, axis=1)
    assert np.abs(r - 6.5).max() < 0.5


def test_sphere_geometry():
    r = 20.0
    v, f = _mc(sphere(64, 64, 64, r))
    c = 31.5
    assert np.abs(np.linalg.norm(v - c, axis=1) - r).max() < 0.5
    tri = v[f].astype(np.float64) - c
    vol = np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6
    exact = 4 / 3 * np.pi * r ** 3
    assert vol > 0 and abs(vol - exact) < 0.01 * exact
    assert_closed_oriented(f)
    assert euler(v, f) == 2


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_planes_land_on_their_axis(axis):
    h, w, d = 10, 12, 14
    i, j, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(d), indexing="ij")
    coord = (j, i, k)[axis].astype(np.float32)         # x <-> j, y <-> i, z <-> k
    v, f = _mc(coord - 4.25)
    assert len(f) > 0
    assert np.abs(v[:, axis] - 4.25).max() < 1e-6
    # the reference frame maps that index plane to the expected coordinate
    vr, _ = _mc(coord - 4.25, 0.0, mesh.reference_affine(h, w, d))
    n = (w, h, d)[axis]
    want = (4.25 / n - 0.5) * 0.24 * (1 if axis == 0 else -1)
    assert np.abs(vr[:, axis] - want).max() < 1e-6


def test_empty_volumes_and_refusals():
    for val in (1.0, -1.0):
        A = cu(torch.full((1, 6, 7, 8, 1), val))
        v, f = hip.marching_cubes(A[0, ..., 0].contiguous())
        assert v.shape == (0, 3) and f.shape == (0, 3)
        assert mesh.extract_mesh_with_marching_cubes(A) is None
    with pytest.raises(RuntimeError):
        hip.marching_cubes(cu(torch.zeros(1, 8, 8)))
    with pytest.raises(RuntimeError):
        hip.marching_cubes(cu(torch.zeros(8, 8, 1)))


def test_two_runs_are_bit_identical():
    A = cu(torch.from_numpy(random_field((48, 40, 56), 9)))
    v1, f1 = hip.marching_cubes(A, 0.1, mesh.reference_affine(48, 40, 56))
    v2, f2 = hip.marching_cubes(A, 0.1, mesh.reference_affine(48, 40, 56))
    assert torch.equal(v1, v2) and torch.equal(f1, f2)
    a1, a2 = mesh.align_volume(A[None]), mesh.align_volume(A[None])
    assert torch.equal(a1, a2)


# ------------------------------------------------------------------------------------------------ surface_mesh
def test_surface_mesh_tiny_generator():
    cfg = configs.tiny_G_cfg(hidden=32, N_layers_renderer=2)
    G = pkg.build_generator(cfg, DEV, seed=5)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    zs = [torch.randn(1, 32, generator=g), torch.randn(1, 32, generator=g)]
    nb = O.create_noise_bufs(cfg, 8, generator=g)
    ncfg = dict(N_samples=6, perturb=False, static_viewdirs=False)
    e, f, n, fa, _ = Camera.generate_camera_params(8, DEV, locations=cu(torch.tensor([[0.2, -0.05]])))

    def forward():
        return G(zs=[cu(z) for z in zs], cam_poses=e, focals=f, img_size=8, near=n, far=fa,
                 noise_bufs=[cu(b) for b in nb], nerf_cfg=ncfg, return_xyz=True)

    before = forward()
    S, N = 12, 10
    style_r, _ = G.mapping_renderer([cu(zs[0])], 1, None)
    locs = torch.zeros(1, 2)
    cam = Camera.generate_camera_params(S, DEV, locations=cu(locs))
    _, _, sdf_r, _, _ = G.renderer.render(cam[0], cam[1], cam[2], cam[3], style_r, S, N, return_sdf=True)
    aligned_r = mesh.align_volume(sdf_r)
    inside = aligned_r[0, ..., 0][aligned_r[0, ..., 0] != 1.0]
    level = float(inside.median())

    out = mesh.surface_mesh(G, zs=[cu(zs[0])], resolution=S, N_samples=N, level=level)
    assert torch.equal(out["sdf"], sdf_r)
    # the volume agrees with the CPU oracle's renderer
    D = cfg["renderer_cfg"]["N_layers_renderer"]
    st = style_r.cpu()
    ocam = O.camera_params(locs, S, 6, 0.12)
    rays_o, rays_d, vd = O.rays_in_world(ocam[1], S, ocam[0], False)
    z = O.z_vals(ocam[2], ocam[3], 1, S, S, N, None)
    pts = O.ray_points(rays_o, rays_d, z)
    R = S * S
    r_sdf = O.renderer_forward(sd, "renderer", pts.reshape(1, R, N, 3), rays_d.reshape(1, R, 3), vd.reshape(1, R, 3),
                               z.reshape(1, R, N), ocam[2], ocam[3], st, D)[2]
    assert maxdiff(out["sdf"].cpu(), r_sdf.reshape(1, S, S, N, 1)) < 5e-5
    # the mesh is the oracle's on the aligned volume
    assert torch.equal(out["aligned"], aligned_r)
    A = aligned_r[0, ..., 0].cpu().numpy()
    rv, rf = mc_numpy(A, level, mesh.reference_affine(S, S, N))
    assert out["meshes"][0] is not None and len(rf) > 0
    v, fc = out["meshes"][0]
    assert np.abs(v.cpu().numpy() - rv).max() < 1e-6
    assert np.array_equal(fc.cpu().numpy(), rf)
    # nothing leaks into the forward's plans or tables
    after = forward()
    for k in ("rgb", "thumb_rgb", "xyz", "mask", "depth"):
        assert torch.equal(before[k], after[k]), k


def test_surface_mesh_ffhq_d2_at_128():
    G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=1)
    out = mesh.surface_mesh(G, zs=[torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(0)).to(DEV)])
    assert out["sdf"].shape == (1, 128, 128, 128, 1)
    assert torch.isfinite(out["aligned"]).all()
    vol = out["aligned"][0, ..., 0]
    level = float(vol[vol != 1.0].median())
    for lv in (0.0, level):
        m = mesh.extract_mesh_with_marching_cubes(out["aligned"], lv)
        if m is None:
            assert lv == 0.0 and ((vol < 0).all() or (vol >= 0).all())
            continue
        v, f = m
        assert f.min() >= 0 and f.max() < v.shape[0]
        assert torch.isfinite(v).all()
        assert v.abs().max() <= 0.12 + 1e-6
