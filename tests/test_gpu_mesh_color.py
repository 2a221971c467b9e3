"""Mesh colours on the GPU (csrc/mesh_color.hip, mesh.py): parity with the fp64 yardstick of _mesh_color_cases.py under the ratio
rule, the edge inputs of the contract, convexity, reproducibility, the albedo frame, and the way from a generator to a coloured
mesh, its frames and its files.

Measured ratios (kernel error / fp32 restatement's error against fp64, max / RMS) are printed by every ratio check."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, hip, mesh

import _mesh_color_cases as MC
import _mesh_raster_cases as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0.375


def cu(a, dtype=None):
    t = torch.tensor(np.asarray(a)) if not torch.is_tensor(a) else a
    return t.to(DEV, dtype).contiguous()


def run_case(name, **kw):
    """mesh.vertex_colors on CASES[name] -> its dict, on the CPU as numpy."""
    kind, views, S, R, power, depth_tol, znear = MC.CASES[name]
    v, f, n, _ = MR.two_spheres(kind)
    out = mesh.vertex_colors(cu(v), cu(f), cu(n), cu(MC.images(len(views), R)), [a for a, _ in views], [e for _, e in views],
                             znear=znear, raster_size=S, depth_tol=depth_tol, power=power, fill=FILL, **kw)
    torch.cuda.synchronize()
    assert out["colors"].dtype == torch.float32 and out["weight"].dtype == torch.float32 and out["seen"].dtype == torch.int32
    assert tuple(out["colors"].shape) == (len(v), 3) and tuple(out["weight"].shape) == tuple(out["seen"].shape) == (len(v),)
    return {k: t.cpu().numpy() for k, t in out.items()}


def check_case(name):
    """`seen` exact outside the excluded pairs; weight and colours under the ratio rule on the vertices without such a pair;
    an unseen vertex carries weight 0 and the fill colour exactly."""
    got = run_case(name)
    r64, r32 = MC.case(name, "float64"), MC.case(name, "float32")
    keep = ~r64["tie"].any(0)
    bad = (got["seen"] != r64["seen"]) & keep
    print(f"{name}: {int(bad.sum())} `seen` mismatches outside the {int((~keep).sum())} excluded vertices of {len(keep)}")
    assert not bad.any()
    MR.check_ratio(f"{name} weight", got["weight"], r32["weight"], r64["weight"], keep)
    lit = keep & (r64["seen"] > 0) & (r64["weight"] > 0)
    MR.check_ratio(f"{name} colors", got["colors"], r32["colors"], r64["colors"], np.broadcast_to(lit[:, None], got["colors"].shape))
    dark = keep & (r64["seen"] == 0)
    assert (got["weight"][dark] == 0).all() and (got["colors"][dark] == np.float32(FILL)).all()
    assert ((got["weight"] > 0) == (got["colors"] != np.float32(FILL)).any(1))[keep].all()
    return got, r64


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", ["coarse", "subpixel"])
def test_parity_with_fp64(name):
    got, r64 = check_case(name)
    assert (r64["seen"] == 2).any() and (r64["seen"] == 1).any() and (r64["seen"] == 0).any()
    assert len(got["seen"]) == {"coarse": 158, "subpixel": 2720}[name]


# ------------------------------------------------------------------------------------------------ 2. edge inputs
@pytest.mark.parametrize("name", ["one_view", "power1", "power8", "R1", "S1"])
def test_edge_case_against_fp64(name):
    got, r64 = check_case(name)
    assert (got["seen"] > 0).any()
    if name == "R1":                        # one texel per view: a seen vertex carries a mean of the views' texels
        img = MC.images(2, 1)[:, :, 0, 0]
        one = r64["faces_view"][0] & ~r64["faces_view"][1] & ~r64["tie"].any(0)
        assert one.any() and np.abs(got["colors"][one] - img[0]).max() <= 2.0 ** -23


def test_near_plane_drops_vertices():
    got, r64 = check_case("znear")
    v = MR.two_spheres("coarse")[0]
    dropped = np.ones(len(v), bool)
    for az, el in MR.VIEWS:
        _, _, vz, kept, _ = MC.project(v, az, el, 64, 12.0, 1.0, 0.95, np.float64)
        dropped &= ~kept & (np.abs(vz - 0.95) >= MC.TIE_Z)
    assert dropped.sum() >= 10 and (~dropped).sum() >= 10
    assert (got["weight"][dropped] == 0).all() and (got["seen"][dropped] == 0).all()
    assert (got["colors"][dropped] == np.float32(FILL)).all()


def flat_patch():
    """A 3 x 3 grid in the plane z = 0, its normals (0, 0, 1): seen from the front only."""
    g = np.linspace(-0.05, 0.05, 3)
    v = np.array([(x, y, 0.0) for y in g for x in g], np.float32)
    f = np.array([t for r in range(2) for c in range(2) for t in ((3 * r + c, 3 * r + c + 1, 3 * r + c + 4), (3 * r + c, 3 * r + c + 4, 3 * r + c + 3))])
    return v, f, np.tile(np.array([[0, 0, 1]], np.float32), (9, 1))


def test_single_vertex_and_view_from_behind():
    img = MC.images(1, 40)
    # one vertex: a face of zero area draws nothing, so no pixel hides it
    v = np.array([[0.01, -0.02, 0.03]], np.float32)
    n = np.array([[0.0, 0.0, 1.0]], np.float32)
    f = np.zeros((1, 3), np.int64)
    out = mesh.vertex_colors(cu(v), cu(f), cu(n), cu(img), 0.3, 0.1, raster_size=32, fill=FILL)
    ref = MC.vertex_colors(v, f, n, img, ((0.3, 0.1),), 32, fill=FILL)
    assert int(out["seen"][0]) == 1 == int(ref["seen"][0]) and not ref["tie"].any()
    assert abs(float(out["weight"][0]) - ref["weight"][0]) <= 1e-6
    # x_p carries a few ulp of S / 2 = 16 px (< 1e-5 px), u = x_p R / S as much in texels; neighbouring texels differ by at
    # most 2, in two directions: < 4e-5
    assert np.abs(out["colors"].cpu().numpy() - ref["colors"]).max() <= 1e-4
    pv, pf, pn = flat_patch()
    for azim, lit in ((0.3, True), (2.8, False)):
        out = mesh.vertex_colors(cu(pv), cu(pf), cu(pn), cu(img), azim, 0.2, raster_size=32, fill=FILL)
        if lit:
            assert bool((out["seen"] == 1).all()) and bool((out["weight"] > 0).all())
        else:                              # from behind: n . d < 0 everywhere
            assert bool((out["seen"] == 0).all()) and bool((out["weight"] == 0).all()) and bool((out["colors"] == FILL).all())
    with pytest.raises(ValueError, match="without faces"):
        mesh.vertex_colors(cu(pv), cu(pf[:0]), cu(pn), cu(img), 0.3, 0.2, raster_size=32)
    with pytest.raises(RuntimeError, match="cips3d_mesh_vertex_colors failed"):
        mesh.vertex_colors(cu(pv), cu(pf), cu(pn), cu(img), 0.3, 0.2, raster_size=32, power=9)
    with pytest.raises(ValueError, match="images"):
        mesh.vertex_colors(cu(pv), cu(pf), cu(pn), cu(MC.images(2, 40)), 0.3, 0.2, raster_size=32)


# ------------------------------------------------------------------------------------------------ 3. convexity
@pytest.mark.parametrize("name", ["coarse", "subpixel", "power8"])
def test_colours_are_convex_combinations(name):
    """A colour is a convex combination of K = 4 n texels (four taps in each of the n views).  Its fp32 evaluation rounds at
    most 2 n + 5 times on the way (1 - f, two products and a sum per lerp level: 3 + 3; w x rgb; n - 1 additions in each of
    the two sums; the division), which K + 2 = 4 n + 2 covers for n >= 2: the colour leaves [min, max] of its channel by at
    most (K + 2) 2^-24 of the largest magnitude."""
    got = run_case(name)
    kind, views, S, R = MC.CASES[name][:4]
    img = MC.images(len(views), R)
    K = 4 * len(views)
    allow = (K + 2) * 2.0 ** -24 * float(np.abs(img).max())
    seen = got["weight"] > 0
    assert seen.sum() > 50
    for c in range(3):
        lo, hi = float(img[:, c].min()), float(img[:, c].max())
        col = got["colors"][seen, c].astype(np.float64)
        print(f"{name} channel {c}: colours in [{col.min():.7f}, {col.max():.7f}], texels in [{lo:.7f}, {hi:.7f}]")
        assert col.min() >= lo - allow and col.max() <= hi + allow


def test_constant_images_give_the_constant():
    """Every texel of channel c is q_c: the weighted mean is q_c to the rounding of the sums, whatever the weights."""
    v, f, n, _ = MR.two_spheres("coarse")
    q = np.array([0.7231, -0.3117, 0.0519], np.float32)
    img = np.broadcast_to(q[None, :, None, None], (2, 3, 17, 17)).copy()
    out = mesh.vertex_colors(cu(v), cu(f), cu(n), cu(img), [a for a, _ in MR.VIEWS], [e for _, e in MR.VIEWS], raster_size=64,
                             power=3, fill=FILL)
    seen = (out["weight"] > 0).cpu().numpy()
    col = out["colors"].cpu().numpy()
    assert seen.sum() > 50 and np.abs(col[seen] - q).max() <= 10 * 2.0 ** -24 and (col[~seen] == np.float32(FILL)).all()


# ------------------------------------------------------------------------------------------------ 4. reproducibility
def test_runs_are_bit_equal_and_buffers_can_be_reused():
    kind, views, S, R, power, tol, znear = MC.CASES["subpixel"]
    v, f, n, _ = (cu(a) for a in MR.two_spheres(kind))
    img = cu(MC.images(len(views), R))
    az, el = [a for a, _ in views], [e for _, e in views]
    kw = dict(raster_size=S, depth_tol=tol, power=power)
    a = mesh.vertex_colors(v, f, n, img, az, el, **kw)
    b = mesh.vertex_colors(v, f, n, img, az, el, **kw)
    ws, keys = hip.mesh_raster_workspace(v.shape[0], f.shape[0], len(views), S, v.device)
    ws.fill_(0x5a)
    keys.fill_(12345)
    c = mesh.vertex_colors(v, f, n, img, az, el, ws=ws, keys=keys, **kw)
    d = mesh.vertex_colors(v, f, n, img, az, el, ws=ws, keys=keys, **kw)
    for k in ("colors", "weight", "seen"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and torch.equal(a[k], d[k]), k
    # every view alone: its weights add up to the joint call's, in the views' order
    w = torch.zeros_like(a["weight"])
    for i in range(len(views)):
        one = mesh.vertex_colors(v, f, n, img[i:i + 1].contiguous(), az[i], el[i], **kw)
        w = w + one["weight"]
    assert torch.equal(w, a["weight"])
    # outputs on request, written into the caller's tensors, nothing past their ends
    buf = torch.full((64 + v.shape[0] + 64,), -7.5, device=DEV)
    ws, keys = hip.mesh_rasterize(v, f.to(torch.int32), mesh.camera_rows(az, el, device=DEV), S)
    only = hip.mesh_vertex_colors(v, n, img, ws, keys, S, power=power, depth_tol=tol, want=(), out={"weight": buf[64:-64]})
    assert set(only) == {"weight"} and torch.equal(only["weight"], a["weight"])
    assert bool((buf[:64] == -7.5).all()) and bool((buf[-64:] == -7.5).all())


# ------------------------------------------------------------------------------------------------ 5. albedo frame
def test_albedo_frame_against_fp64():
    v, f, n, _ = (cu(a) for a in MR.two_spheres("coarse"))
    S = 64
    colors = cu(np.random.RandomState(4).uniform(-1.1, 1.1, (v.shape[0], 3)).astype(np.float32))
    az, el = [a for a, _ in MR.VIEWS], [e for _, e in MR.VIEWS]
    light = cu(np.stack([MR.light_of(a) for a in az]), torch.float32)
    maps = mesh.rasterize_mesh(v, f, az, el, S, attrs=colors, normals=n, light=light, want=("face", "shade", "attr"))
    got = hip.mesh_albedo_frame(maps["face"], maps["shade"], maps["attr"])
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, S, S)
    ref, near = MC.albedo_u8(*(maps[k].cpu().numpy() for k in ("face", "shade", "attr")))
    got = got.cpu().numpy()
    print(f"albedo frame: {int(near.sum())} of {near.size} values within 2^-10 of a half-integer, "
          f"{int((got != ref).sum())} bytes differ")
    assert near.mean() <= 0.01
    assert np.array_equal(got[~near], ref[~near])
    assert (np.abs(got.astype(int) - ref.astype(int))[near] <= 1).all()
    empty = (maps["face"] < 0).cpu().numpy()
    assert empty.any() and (got[np.broadcast_to(empty[:, None], got.shape)] == 255).all()
    hit = ~empty
    assert len(np.unique(got[:, 0][hit])) > 20 and not np.array_equal(got[:, 0], got[:, 1])          # coloured, not grey
    # the frames call is this pipeline
    traj = torch.tensor([[a, e, 6.0] for a, e in MR.VIEWS])
    frames = mesh.render_mesh_frames(v, f, n, traj, image_size=S, colors=colors)
    assert torch.equal(frames.cpu(), torch.from_numpy(got))


# ------------------------------------------------------------------------------------------------ 6. end to end
VIEWS2 = ((0.25, 0.05), (-0.3, 0.0))


def tiny_mesh_inputs():
    G = pkg.build_generator(configs.tiny_G_cfg(hidden=32, N_layers_renderer=2), DEV, seed=5)
    g = torch.Generator().manual_seed(3)
    zs = [torch.randn(1, 32, generator=g).to(DEV), torch.randn(1, 32, generator=g).to(DEV)]
    kw = dict(resolution=32, N_samples=16, normals=True)
    vol = mesh.surface_mesh(G, zs=zs, **kw)["aligned"][0, ..., 0]
    kw["level"] = float(vol[vol != 1.0].median())        # synthetic weights: the SDF's zero level need not cross the volume
    return G, zs, kw


def test_surface_mesh_with_colours_end_to_end():
    from cips_3dplusplus_amd.camera import Camera
    G, zs, kw = tiny_mesh_inputs()
    color_kw = dict(views=VIEWS2, img_size=8, N_samples=6, raster_size=48)
    plain = mesh.surface_mesh(G, zs=zs, **kw)
    torch.manual_seed(11)
    out = mesh.surface_mesh(G, zs=zs, colors=True, color_kw=color_kw, **kw)
    assert set(out) == set(plain) | {"color_weight", "color_seen"}
    v, f, n, col = out["meshes"][0]
    for a, b in zip(plain["meshes"][0], (v, f, n)):
        assert torch.equal(a, b)                          # the geometry is the uncoloured call's
    V = v.shape[0]
    weight, seen = out["color_weight"][0], out["color_seen"][0]
    assert tuple(col.shape) == (V, 3) and tuple(weight.shape) == (V,) and tuple(seen.shape) == (V,) and V > 100
    assert bool(torch.isfinite(col).all()) and bool(torch.isfinite(weight).all())
    assert int(seen.max()) >= 1 and int(seen.max()) <= 2 and bool((seen[weight > 0] > 0).all())
    # the pictures the colours were taken from: the same seed draws the same noise maps
    torch.manual_seed(11)
    nb = G.create_noise_bufs(8, DEV)
    imgs = []
    for az, el in VIEWS2:
        cam = Camera.generate_camera_params(8, DEV, locations=torch.tensor([[az, el]], device=DEV))
        imgs.append(G(zs=zs, cam_poses=cam[0], focals=cam[1], img_size=8, near=cam[2], far=cam[3], noise_bufs=nb,
                      nerf_cfg=dict(N_samples=6, perturb=False))["rgb"])
    imgs = torch.cat(imgs, 0)
    lit = weight > 0
    allow = (4 * 2 + 2) * 2.0 ** -24 * float(imgs.abs().max())
    for c in range(3):
        assert float(col[lit, c].min()) >= float(imgs[:, c].min()) - allow and float(col[lit, c].max()) <= float(imgs[:, c].max()) + allow
    assert bool((col[~lit] == 0).all())                   # the default fill
    direct = mesh.color_mesh(G, v, f, n, zs=zs, noise_bufs=nb, **color_kw)
    for k, t in (("colors", col), ("weight", weight), ("seen", seen)):
        assert torch.equal(direct[k], t), k
    # the same seed: the same bits; another seed: other noise maps, other colours
    torch.manual_seed(11)
    again = mesh.surface_mesh(G, zs=zs, colors=True, color_kw=color_kw, **kw)
    assert torch.equal(again["meshes"][0][3], col) and torch.equal(again["color_weight"][0], weight)
    torch.manual_seed(12)
    other = mesh.surface_mesh(G, zs=zs, colors=True, color_kw=color_kw, **kw)
    assert torch.equal(other["color_seen"][0], seen) and not torch.equal(other["meshes"][0][3], col)
    # frames: coloured where the plain panel is drawn, white exactly where it is white
    traj = torch.tensor([[0.25, 0.05, 6.0], [-0.5, 0.1, 7.0]])
    grey = mesh.render_mesh_frames(v, f, n, traj, image_size=40)
    hit = mesh.rasterize_mesh(v, f, traj[:, 0], traj[:, 1], 40, fov_deg=2 * traj[:, 2], want=("face",))["face"] >= 0
    painted = mesh.render_mesh_frames(v, f, n, traj, image_size=40, colors=col)
    assert painted.dtype == torch.uint8 and tuple(painted.shape) == (2, 3, 40, 40)
    white = ~hit[:, None].expand(-1, 3, -1, -1)
    assert bool((painted[white] == 255).all()) and bool((grey[white] == 255).all()) and bool(hit.any()) and bool((~hit).any())
    assert not torch.equal(painted[:, 0], painted[:, 1]) and not torch.equal(painted, grey)           # coloured, not grey
    with pytest.raises(ValueError, match="normals"):
        mesh.surface_mesh(G, zs=zs, colors=True, resolution=32, N_samples=16)
    with pytest.raises(ValueError, match="decoder"):
        mesh.surface_mesh(G, zs=zs[:1], colors=True, **kw)


def test_extract_mesh_tool_writes_colours(tmp_path):
    path = str(tmp_path / "m.obj")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--resolution", "32", "--colors", "--ply",
                        "--color-views", "0,0;0.35,0.05", "--out", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "coloured from 2 views" in r.stdout
    rows = [ln.split() for ln in open(path).read().splitlines() if ln.startswith("v ")]
    assert len(rows) > 0 and all(len(row) == 7 for row in rows)
    rgb = np.array([[float(x) for x in row[4:]] for row in rows])
    assert rgb.min() >= 0 and rgb.max() <= 1 and len(np.unique(rgb.round(3), axis=0)) > 10
    ov, of = mesh.read_obj(path)
    ply = mesh.read_ply(str(tmp_path / "m.ply"))
    assert set(ply) == {"verts", "faces", "normals", "colors"}
    assert torch.equal(ply["faces"], of) and ply["verts"].shape == ov.shape and float((ply["verts"] - ov).abs().max()) <= 1e-6
    assert np.abs(ply["colors"].numpy() / 255.0 - rgb).max() <= 1 / 255 + 1e-6
