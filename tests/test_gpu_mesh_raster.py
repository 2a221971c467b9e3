"""The mesh rasteriser on the GPU (csrc/mesh_raster.hip, mesh.py): parity with the fp64 brute-force yardstick of
_mesh_raster_cases.py under the ratio rule, the edges of the contract, reproducibility, attributes, the Phong mesh frame,
NoiseProjector, Generator.forward(project_noise=True), the projected multi-view sequence and marching cubes -> mesh frames.

Measured ratios (kernel error / fp32 restatement's error against fp64, max / RMS) are printed by every ratio check."""
import numpy as np
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, gen_images, mesh

import _mesh_raster_cases as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -12345.5
PAD = 64


def cu(a, dtype=None):
    t = torch.tensor(np.asarray(a)) if not torch.is_tensor(a) else a
    return t.to(DEV, dtype).contiguous()


def spheres(kind):
    v, f, n, attr = MR.two_spheres(kind)
    return cu(v), cu(f), cu(n), cu(attr)


def padded(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    sent = {torch.float32: SENTINEL, torch.int32: -777, torch.uint8: 201}[dtype]
    buf = torch.full((PAD + n + PAD,), sent, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(*shape), sent


def one_triangle_views(tri, S, faces=((0, 1, 2),), **kw):
    """Vertices given as (x, y, z) in the frontal camera's image frame -- x right, y up, both in [-1, 1] across the frame, z the
    view depth -- for a camera at (0, 0, 1) with fov 90 degrees (s = 1): world p = (x z, y z, 1 - z).  -> (outputs on the CPU,
    world vertices, faces)."""
    tri = np.asarray(tri, np.float64)
    world = np.stack([tri[:, 0] * tri[:, 2], tri[:, 1] * tri[:, 2], 1 - tri[:, 2]], 1).astype(np.float32)
    f = torch.tensor(faces, dtype=torch.int64).reshape(-1, 3)
    out = mesh.rasterize_mesh(cu(world), cu(f), 0.0, 0.0, S, fov_deg=90.0, dist=1.0, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}, world, f.numpy()


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("kind,S", [("coarse", 32), ("coarse", 64), ("subpixel", 32)])
def test_parity_with_fp64(kind, S):
    v, f, _, _ = spheres(kind)
    az, el = [a for a, _ in MR.VIEWS], [e for _, e in MR.VIEWS]
    out = mesh.rasterize_mesh(v, f, az, el, S)
    torch.cuda.synchronize()
    assert out["face"].dtype == torch.int32 and tuple(out["bary"].shape) == (2, S, S, 3)
    for view in range(2):
        r64, r32 = MR.case(kind, view, S, "float64"), MR.case(kind, view, S, "float32")
        keep = ~MR.excluded(r64)
        face, zbuf, bary = (out[k][view].cpu().numpy() for k in ("face", "zbuf", "bary"))
        bad = (face != r64["face"]) & keep
        print(f"{kind} S={S} view {view}: {int(bad.sum())} face mismatches outside the excluded {int((~keep).sum())} pixels, "
              f"{int((face != r64['face']).sum())} inside or outside")
        assert not bad.any()
        empty = face < 0
        assert (zbuf[empty] == -1).all() and (bary[empty] == -1).all() and (face[empty] == -1).all()
        same = keep & (face == r64["face"]) & ~empty
        MR.check_ratio(f"{kind} S={S} view {view} zbuf", zbuf, r32["zbuf"], r64["zbuf"], same)
        MR.check_ratio(f"{kind} S={S} view {view} bary", bary, r32["bary"], r64["bary"], same)
        assert np.abs(bary[~empty].sum(-1) - 1).max() < 1e-4


def test_frontal_view_at_even_size():
    v, f, _, _ = spheres("coarse")
    out = mesh.rasterize_mesh(v, f, 0.0, 0.0, 32)
    r64 = MR.case("coarse", (0.0, 0.0), 32, "float64")
    keep = ~MR.excluded(r64)
    assert (~keep).mean() <= 0.01
    assert not ((out["face"][0].cpu().numpy() != r64["face"]) & keep).any()


# ------------------------------------------------------------------------------------------------ 2. edges of the contract
def test_single_pixel_frame_and_no_faces():
    out, _, _ = one_triangle_views([(-0.5, -0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.6, 0.5)], 1)
    assert out["face"].tolist() == [[[0]]] and abs(float(out["zbuf"]) - 0.5) < 1e-6
    assert abs(float(out["bary"].sum()) - 1) < 1e-5
    v = torch.zeros(3, 3, device=DEV)
    for verts, faces in ((v, torch.zeros(0, 3, dtype=torch.int64, device=DEV)), (v[:0], torch.zeros(0, 3, dtype=torch.int64, device=DEV))):
        out = mesh.rasterize_mesh(verts, faces, [0.1, 0.2], 0.0, 8, attrs=torch.ones(verts.shape[0], 2, device=DEV), fill=0.25)
        torch.cuda.synchronize()
        assert bool((out["face"] == -1).all()) and bool((out["zbuf"] == -1).all()) and bool((out["bary"] == -1).all())
        assert tuple(out["attr"].shape) == (2, 2, 8, 8) and bool((out["attr"] == 0.25).all())


@pytest.mark.parametrize("S", [64, 1024])
def test_two_triangles_cover_the_frame(S):
    """A quad larger than the frame at depth 0.5: every pixel is covered (the boxes are the whole frame: the wave path)."""
    quad = [(-1.5, -1.4, 0.5), (1.6, -1.4, 0.5), (1.6, 1.7, 0.5), (-1.5, 1.7, 0.5)]
    out, _, _ = one_triangle_views(quad, S, faces=((0, 1, 2), (0, 2, 3)))
    face, z = out["face"][0], out["zbuf"][0]
    assert bool(((face == 0) | (face == 1)).all()) and 0.2 < float((face == 0).float().mean()) < 0.8
    assert float((z - 0.5).abs().max()) < 1e-5
    assert float((out["bary"][0].sum(-1) - 1).abs().max()) < 1e-4
    # the diagonal from the lower left to the upper right: image rows grow downwards, so face 0 (below it) holds the last row
    assert int(face[S - 1, S // 2]) == 0 and int(face[0, S // 2]) == 1


def test_faces_off_the_frame_behind_znear_and_degenerate():
    tris = [(0.2, -0.3, 0.5), (1.8, -0.3, 0.5), (0.2, 0.9, 0.5),            # 0: partly off the frame (to the right)
            (1.2, 1.2, 0.5), (2.5, 1.2, 0.5), (1.2, 2.5, 0.5),              # 1: wholly off
            (-0.8, -0.8, 0.4), (0.8, -0.8, 0.4), (0.0, 0.8, 0.005),         # 2: one vertex behind znear = 0.01: dropped whole
            (-0.9, 0.5, 0.3), (-0.5, 0.5, 0.3), (-0.1, 0.5, 0.3),           # 3: zero area
            (-0.9, -0.9, 0.7), (-0.2, -0.9, 0.7), (-0.9, -0.2, 0.7),        # 4, 5: coincident: the lower index wins
            (-0.9, -0.9, 0.7), (-0.2, -0.9, 0.7), (-0.9, -0.2, 0.7)]
    faces = [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(6)]
    S = 32
    out, world, f = one_triangle_views(tris, S, faces=faces)
    face = out["face"][0].numpy()
    assert set(np.unique(face)) == {-1, 0, 4}
    ref = MR.rasterize(world, f, 0.0, 0.0, S, fov_deg=90.0)
    keep = ref["edge"] >= MR.EDGE_TOL
    assert np.array_equal(face[keep], ref["face"][keep])
    assert (face[:, S - 1] == 0).any() and (face[:, :S // 2] != 0).all()     # clipped at the right border, not wrapped


def test_permuted_faces_give_the_same_depths():
    """Two parallel quads (four triangles); the face order permuted: zbuf identical, face equal up to the permutation."""
    quad = lambda z, dx: [(-0.7 + dx, -0.6, z), (0.5 + dx, -0.6, z), (0.5 + dx, 0.7, z), (-0.7 + dx, 0.7, z)]   # noqa: E731
    verts = quad(0.5, 0.0) + quad(0.6, 0.3)
    faces = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)]
    perm = [2, 0, 3, 1]
    a, _, _ = one_triangle_views(verts, 48, faces=faces)
    b, _, _ = one_triangle_views(verts, 48, faces=[faces[p] for p in perm])
    assert torch.equal(a["zbuf"], b["zbuf"])
    fb = b["face"][0].numpy()
    mapped = np.where(fb >= 0, np.asarray(perm)[np.maximum(fb, 0)], -1)
    assert np.array_equal(mapped, a["face"][0].numpy())
    assert set(np.unique(a["face"][0].numpy())) == {-1, 0, 1, 2, 3}


def test_padded_outputs_are_untouched_past_their_ends():
    v, f, n, attr = spheres("coarse")
    S, nv = 17, 2
    bufs = {"face": padded((nv, S, S), torch.int32), "zbuf": padded((nv, S, S)), "bary": padded((nv, S, S, 3)),
            "attr": padded((nv, 3, S, S)), "shade": padded((nv, S, S)), "shade_u8": padded((nv, 3, S, S), torch.uint8)}
    light = cu(np.stack([MR.light_of(a) for a, _ in MR.VIEWS]), torch.float32)
    mesh.rasterize_mesh(v, f, [a for a, _ in MR.VIEWS], [e for _, e in MR.VIEWS], S, attrs=attr, normals=n, light=light,
                        want=(), out={k: b[1] for k, b in bufs.items()})
    torch.cuda.synchronize()
    for k, (buf, view, sent) in bufs.items():
        assert bool((buf[:PAD] == sent).all()) and bool((buf[-PAD:] == sent).all()), f"{k}: store outside the output"
        if buf.dtype != torch.uint8:
            assert not bool((view == sent).any()), f"{k}: an element was not written"


# ------------------------------------------------------------------------------------------------ 3. reproducibility
def test_runs_are_bit_equal_and_views_are_independent():
    v, f, n, attr = spheres("subpixel")
    az, el = [0.4, -0.77, 0.0], [0.1, 0.2, -0.15]
    light = cu(np.stack([MR.light_of(a) for a in az]), torch.float32)
    kw = dict(attrs=attr, normals=n)
    a = mesh.rasterize_mesh(v, f, az, el, 40, light=light, **kw)
    b = mesh.rasterize_mesh(v, f, az, el, 40, light=light, **kw)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for i in range(3):
        one = mesh.rasterize_mesh(v, f, az[i], el[i], 40, light=light[i:i + 1].contiguous(), **kw)
        for k in a:
            assert torch.equal(one[k][0], a[k][i]), (k, i)


# ------------------------------------------------------------------------------------------------ 4. attributes, 5. mesh frame
def test_attributes_and_shade_against_fp64():
    v, f, n, attr = spheres("coarse")
    S = 32
    for view, (az, el) in enumerate(MR.VIEWS):
        r64, r32 = MR.case("coarse", view, S, "float64", True), MR.case("coarse", view, S, "float32", True)
        light = cu(MR.light_of(az)[None], torch.float32)
        base = torch.randn(1, 3, S, S, device=DEV)
        out = mesh.rasterize_mesh(v, f, az, el, S, attrs=attr, base=base, normals=n, light=light)
        one = mesh.rasterize_mesh(v, f, az, el, S, attrs=attr[:, :1].contiguous(), fill=-3.5)
        torch.cuda.synchronize()
        face = out["face"][0].cpu().numpy()
        same = ~MR.excluded(r64) & (face == r64["face"]) & (face >= 0)
        empty = torch.from_numpy(face < 0).to(DEV)
        got = out["attr"][0].cpu().numpy()
        m3 = np.broadcast_to(same, got.shape)
        MR.check_ratio(f"view {view} attr C=3", got, r32["attr"], r64["attr"], m3)
        MR.check_ratio(f"view {view} attr C=1", one["attr"][0].cpu().numpy(), r32["attr"][:1], r64["attr"][:1], m3[:1])
        assert torch.equal(out["attr"][0][:, empty], base[0][:, empty])                   # base: bit-exact on empty pixels
        assert bool((one["attr"][0, 0][empty] == -3.5).all())                             # fill
        assert torch.equal(one["attr"][0, 0][~empty], out["attr"][0, 0][~empty])
        MR.check_ratio(f"view {view} shade", out["shade"][0].cpu().numpy(), r32["shade"], r64["shade"], same)
        sh = out["shade"][0]
        u8 = torch.floor(255 * sh.clamp(0, 1) + 0.5).to(torch.uint8)
        assert torch.equal(out["shade_u8"][0], u8[None].expand(3, S, S))
        assert bool((sh[empty] == 1).all()) and bool((out["shade_u8"][0][:, empty] == 255).all())    # white background
        assert float(sh[~empty].min()) >= 0.1 - 1e-6 and float(sh[~empty].max()) > 0.5


def test_render_mesh_frames_matches_rasterize_mesh():
    v, f, n, _ = spheres("coarse")
    traj = torch.tensor([[0.4, 0.1, 6.0], [-0.77, 0.2, 7.0]])
    frames = mesh.render_mesh_frames(v, f, n, traj, image_size=32)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 3, 32, 32)
    light = cu(np.stack([MR.light_of(0.4), MR.light_of(-0.77)]), torch.float32)
    ref = mesh.rasterize_mesh(v, f, traj[:, 0], traj[:, 1], 32, fov_deg=2 * traj[:, 2], normals=n, light=light)
    assert torch.equal(frames, ref["shade_u8"])
    assert int((frames[0, 0] < 255).sum()) != int((frames[1, 0] < 255).sum())           # fov 12 and 14: different footprints


# ------------------------------------------------------------------------------------------------ 6. NoiseProjector
def test_noise_projector_against_the_restatement():
    v, f, _, _ = spheres("coarse")
    sizes = [16, 32, 32]
    g = torch.Generator(device=DEV).manual_seed(3)
    vn = [torch.randn(v.shape[0], device=DEV, generator=g) for _ in sizes]
    proj = mesh.NoiseProjector(v, f, sizes, vert_noise=vn)
    assert proj.levels == [0, 0, 0]
    bufs = [torch.randn(1, 1, s, s, device=DEV, generator=g) for s in sizes]
    keep = [b.clone() for b in bufs]
    az, el = MR.VIEWS[0]
    out = proj.project(bufs, az, el)
    again = proj.project(bufs, torch.tensor([az], device=DEV), torch.tensor([el], device=DEV))
    torch.cuda.synchronize()
    for i, s in enumerate(sizes):
        assert torch.equal(bufs[i], keep[i]) and torch.equal(out[i], again[i])
        kw = dict(attrs=vn[i].cpu().numpy()[:, None])
        r64 = MR.rasterize(v.cpu().numpy(), f.cpu().numpy(), az, el, s, **kw)
        r32 = MR.rasterize(v.cpu().numpy(), f.cpu().numpy(), az, el, s, dt=np.float32, **kw)
        face = mesh.rasterize_mesh(v, f, az, el, s)["face"][0].cpu().numpy()
        same = ~MR.excluded(r64) & (face == r64["face"]) & (face >= 0)
        MR.check_ratio(f"layer {i} ({s}^2)", out[i][0].cpu().numpy(), r32["attr"], r64["attr"], same[None])
        empty = torch.from_numpy(face < 0).to(DEV)
        assert torch.equal(out[i][0, 0][empty], bufs[i][0, 0][empty])                     # the caller's values, bit for bit
        assert 0.2 < float((~empty).float().mean()) < 0.8
    assert abs(proj.absmax() - max(float(t.abs().max()) for t in vn)) == 0


def test_noise_projector_level_one():
    """A 256^2 layer takes the once-subdivided mesh: same surface, so the covered set is the level-0 one and the values are
    the interpolated noise of the subdivided vertices."""
    v, f, _, _ = spheres("coarse")
    proj = mesh.NoiseProjector(v, f, [256], generator=torch.Generator(device=DEV).manual_seed(5))
    assert proj.levels == [1]
    v1, f1 = mesh.subdivide(v, f)
    assert proj.vert_noise[0].shape[0] == v1.shape[0] == v.shape[0] + 3 * f.shape[0] // 2
    buf = torch.randn(1, 1, 256, 256, device=DEV)
    az, el = MR.VIEWS[1]
    out = proj.project([buf], az, el)[0]
    ref = mesh.rasterize_mesh(v1, f1, az, el, 256, attrs=proj.vert_noise[0], base=buf)
    assert torch.equal(out, ref["attr"])
    hit0 = mesh.rasterize_mesh(v, f, az, el, 256)["face"] >= 0
    assert float(((ref["face"] >= 0) != hit0).float().mean()) < 2e-3
    assert torch.equal(out[0, 0][~(ref["face"][0] >= 0)], buf[0, 0][~(ref["face"][0] >= 0)])
    assert float(out[0, 0][ref["face"][0] >= 0].abs().max()) <= proj.absmax()


# ------------------------------------------------------------------------------------------------ 7. Generator, 8. sequence
def tiny_generator():
    from cips_3dplusplus_amd.decoder import NoiseInjection
    G = pkg.build_generator(configs.tiny_G_cfg(hidden=32, N_layers_renderer=2), DEV, seed=7)
    with torch.no_grad():
        for i, m in enumerate(mod for mod in G.modules() if isinstance(mod, NoiseInjection)):
            m.weight.fill_(0.3 + 0.05 * i)                # the noise must show in the image
    g = torch.Generator(device=DEV).manual_seed(0)
    zs = [torch.randn(1, 32, device=DEV, generator=g), torch.randn(1, 32, device=DEV, generator=g)]
    nb = [torch.randn(b.shape, device=DEV, generator=g) for b in G.create_noise_bufs(8, DEV)]
    return G, zs, nb


def test_generator_project_noise(tmp_path):
    from cips_3dplusplus_amd.camera import cameras_from_trajectory, yaw_trajectory
    G, zs, nb = tiny_generator()
    v, f, _, _ = spheres("coarse")
    S, N = 8, 6
    traj = yaw_trajectory(3, (-0.5, 0.4), 0.15, 6)
    ext, foc, near, far = cameras_from_trajectory(traj, S, torch.device(DEV), 0.12)
    az, el = mesh.view_angles(ext)
    assert float((az.cpu() - traj[:, 0].float()).abs().max()) <= 1e-6 and float((el.cpu() - traj[:, 1].float()).abs().max()) <= 1e-6
    j = 1
    kw = dict(zs=zs, cam_poses=ext[j:j + 1].contiguous(), focals=foc[j:j + 1].contiguous(), img_size=S, near=near[j:j + 1].contiguous(),
              far=far[j:j + 1].contiguous(), nerf_cfg=dict(N_samples=N, perturb=False, static_viewdirs=False))
    plain = G(noise_bufs=nb, **kw)
    assert set(G(noise_bufs=nb, project_noise=False, **kw)) == set(plain)
    got = G(noise_bufs=nb, project_noise=True, mesh_path=(v, f), **kw)
    assert set(got) == set(plain)
    projector = G.noise_projector((v, f), [b.shape[-1] for b in nb])
    maps = projector.project(nb, az[j:j + 1], el[j:j + 1])
    assert any(not torch.equal(m, b) for m, b in zip(maps, nb))
    ref = G(noise_bufs=maps, **kw)
    assert torch.equal(got["rgb"], ref["rgb"]) and torch.equal(got["thumb_rgb"], ref["thumb_rgb"])
    assert not torch.equal(got["rgb"], plain["rgb"])
    # an OBJ path gives the result of the pair it holds, given that pair's vertex noise (each projector draws its own)
    sizes = [b.shape[-1] for b in nb]
    path = gen_images.write_obj(str(tmp_path / "m.obj"), v.cpu().numpy(), f.cpu().numpy())
    rv, rf = mesh.read_obj(path, device=DEV)
    p_pair = G.noise_projector((rv, rf), sizes)
    assert p_pair is not projector and G.noise_projector((rv, rf), sizes) is p_pair
    vn = p_pair.vert_noise
    from_pair = G(noise_bufs=nb, project_noise=True, mesh_path=(rv, rf), **kw)
    p_path = G.noise_projector(path, sizes)
    assert p_path is not p_pair
    p_path.vert_noise = vn
    from_path = G(noise_bufs=nb, project_noise=True, mesh_path=path, **kw)
    assert torch.equal(from_path["rgb"], from_pair["rgb"]) and not torch.equal(from_path["rgb"], plain["rgb"])
    with pytest.raises(ValueError, match="mesh_path"):
        G(noise_bufs=nb, project_noise=True, **kw)


@pytest.mark.parametrize("hoist,lanes", [(True, 1), (True, 2), (False, 1), (False, 2)])
def test_sample_multi_view_projects_per_frame(hoist, lanes):
    from cips_3dplusplus_amd.camera import cameras_from_trajectory
    from cips_3dplusplus_amd.multiview import sample_multi_view
    G, zs, nb = tiny_generator()
    v, f, _, _ = spheres("coarse")
    S, N, n = 8, 6, 4
    cam_cfg = {"img_size": S, "fov_ang": 6, "dist_radius": 0.12}
    kw = dict(view_mode="yaw", N_frames=n, truncation_ratio=1, N_samples=N, noise_bufs=nb, to_uint8=False, gather=("rgb",))
    out = sample_multi_view(G, cam_cfg, {"static_viewdirs": False}, zs, project_noise=(v, f), hoist=hoist, lanes=lanes, **kw)
    plain = sample_multi_view(G, cam_cfg, {"static_viewdirs": False}, zs, hoist=hoist, lanes=lanes, **kw)
    torch.cuda.synchronize()
    assert set(out) == set(plain) and not torch.equal(out["rgb"], plain["rgb"])
    traj = out["trajectory"]
    ext, foc, near, far = cameras_from_trajectory(traj, S, torch.device(DEV), 0.12)
    projector = G.noise_projector((v, f), [b.shape[-1] for b in nb])
    bound = max([projector.absmax()] + [float(b.abs().max()) for b in nb])
    for j in range(n):
        one = G(zs=zs, cam_poses=ext[j:j + 1].contiguous(), focals=foc[j:j + 1].contiguous(), img_size=S, near=near[j:j + 1].contiguous(),
                far=far[j:j + 1].contiguous(), noise_bufs=nb, truncation=1, project_noise=True, mesh_path=(v, f), noise_bound=bound,
                nerf_cfg=dict(N_samples=N, perturb=False, static_viewdirs=False))
        assert torch.equal(one["rgb"], out["rgb"][j:j + 1]), j


# ------------------------------------------------------------------------------------------------ 9. end to end
def test_marching_cubes_to_mesh_frames():
    """An analytic sphere SDF in 24^3 -> extract_mesh_with_marching_cubes(normals=True) -> render_mesh_frames at 64^2: a closed
    mesh always shows a front face, so every covered pixel's depth lies between the near pole and the silhouette."""
    n = 24
    ax = torch.arange(n, dtype=torch.float32, device=DEV)
    i, j, k = torch.meshgrid(ax, ax, ax, indexing="ij")
    r_idx = 7.3
    sdf = ((i - 11.4) ** 2 + (j - 11.7) ** 2 + (k - 11.5) ** 2).sqrt() - r_idx
    v, f, nrm = mesh.extract_mesh_with_marching_cubes(sdf[None], normals=True)
    cell = mesh.FRAME_SCALE / n
    r = r_idx * cell
    traj = torch.tensor([[-0.5, 0.1, 6.0], [0.0, 0.0, 6.0], [0.6, -0.2, 6.0]])
    frames = mesh.render_mesh_frames(v, f, nrm, traj, image_size=64)
    out = mesh.rasterize_mesh(v, f, traj[:, 0], traj[:, 1], 64, fov_deg=12.0)
    torch.cuda.synchronize()
    hit = out["face"] >= 0
    assert tuple(frames.shape) == (3, 3, 64, 64) and bool((frames[:, 0][~hit] == 255).all())
    assert bool((frames[:, 0][hit] < 255).any())
    share = hit.float().mean(dim=(1, 2))
    assert bool((share > 0.15).all()) and bool((share < 0.8).all())
    z = out["zbuf"][hit]
    assert float(z.min()) >= 1 - r - cell and float(z.max()) < 1
