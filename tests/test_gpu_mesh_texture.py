"""The mesh texture atlas on the GPU (csrc/mesh_texture.hip, mesh.py): the bake's parity with the fp64 yardstick of
_mesh_texture_cases.py under the ratio rule, the edge inputs of the contract, the fill's bit equality with its restatement,
the bake's fallback to the filled vertex colours, the textured frame (no bleed across a face's border), reproducibility, and the
way from a generator to a textured OBJ, its MTL and PNG and its frames.

Measured ratios (kernel error / fp32 restatement's error against fp64, max / RMS) are printed by every ratio check."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, gen_images, hip, mesh

import _mesh_color_cases as MC
import _mesh_raster_cases as MR
import _mesh_texture_cases as MT

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = MT.FILL


def cu(a, dtype=None):
    t = torch.tensor(np.asarray(a)) if not torch.is_tensor(a) else a
    return t.to(DEV, dtype).contiguous()


def case_inputs(name):
    c = dict(MT.CASES[name])
    v, f, n, _ = MR.two_spheres(c["kind"])
    f = f[c.get("face0", 0):][:c.get("n_faces")]
    views = c["views"]
    args = (cu(v), cu(f), cu(n), cu(MC.images(len(views), c["R"])), [a for a, _ in views], [e for _, e in views])
    kw = dict(texels=c["T"], cols=c.get("cols"), znear=c.get("znear", 0.01), raster_size=c["S"],
              depth_tol=c.get("depth_tol", MC.DEFAULT_DEPTH_TOL), power=c.get("power", 2), fill=FILL)
    return args, kw


def run_case(name, **extra):
    """mesh.bake_texture on CASES[name] -> (its dict on the CPU as numpy, the atlas)."""
    args, kw = case_inputs(name)
    out = mesh.bake_texture(*args, **kw, **extra)
    torch.cuda.synchronize()
    atlas = out.pop("atlas")
    Ht, Wt = atlas["height"], atlas["width"]
    assert out["texture"].dtype == torch.float32 and out["weight"].dtype == torch.float32 and out["seen"].dtype == torch.int32
    assert tuple(out["texture"].shape) == (3, Ht, Wt) and tuple(out["weight"].shape) == tuple(out["seen"].shape) == (Ht, Wt)
    return {k: t.cpu().numpy() for k, t in out.items()}, atlas


def check_against(name, got, r64, r32):
    """`seen` exact outside the excluded pairs; weight and colours under the ratio rule on the texels without such a pair; an
    unseen texel carries weight 0; an unowned texel holds fill, weight 0 and seen 0 exactly."""
    owned = r64["owned"]
    assert got["seen"].shape == owned.shape == (r64["layout"][3], r64["layout"][2])
    keep = owned & ~r64["tie"].any(0)
    bad = (got["seen"] != r64["seen"]) & keep
    print(f"{name}: {int(bad.sum())} `seen` mismatches outside the {int((owned & ~keep).sum())} excluded texels of {int(owned.sum())}; "
          f"excluded pairs {100 * r64['tie'][:, owned].mean():.2f} %")
    assert r64["tie"][:, owned].mean() <= MC.CAP
    assert not bad.any()
    MR.check_ratio(f"{name} weight", got["weight"], r32["weight"], r64["weight"], keep)
    lit = keep & (r64["seen"] > 0) & (r64["weight"] > 0)
    if lit.any():
        MR.check_ratio(f"{name} texture", got["texture"], r32["texture"], r64["texture"], np.broadcast_to(lit[None], got["texture"].shape))
    dark = keep & (r64["seen"] == 0)
    assert (got["weight"][dark] == 0).all()
    assert (got["texture"][:, ~owned] == np.float32(FILL)).all() and (got["weight"][~owned] == 0).all() and (got["seen"][~owned] == 0).all()
    return keep, lit, dark


def check_case(name):
    got, atlas = run_case(name)
    r64, r32 = MT.case(name, "float64"), MT.case(name, "float32")
    assert (atlas["cols"], atlas["rows"], atlas["width"], atlas["height"]) == r64["layout"]
    keep, lit, dark = check_against(name, got, r64, r32)
    assert (got["texture"][:, dark] == np.float32(FILL)).all()           # no fallback colours given: the constant fill
    return got, r64


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", MT.PARITY)
def test_parity_with_fp64(name):
    got, r64 = check_case(name)
    seen = r64["seen"][r64["owned"]]
    assert (seen == 2).any() and (seen == 1).any() and (seen == 0).any()


# ------------------------------------------------------------------------------------------------ 2. edge inputs
@pytest.mark.parametrize("name", ["odd_F", "cols1", "cols7", "one_view", "znear", "power8", "R1", "S1", "F1"])
def test_edge_case_against_fp64(name):
    got, r64 = check_case(name)
    assert (got["seen"] > 0).any()
    if name == "odd_F":                                  # the last cell's upper half: nobody's
        assert int((~r64["owned"]).sum()) >= 4 * 5 // 2
    if name == "cols1":                                  # one cell per row: the default layout's texels, elsewhere
        base = MT.case("coarse_T4", "float64")
        assert r64["layout"] == (1, 154, 5, 616)
        assert sorted(r64["seen"][r64["owned"]].tolist()) == sorted(base["seen"][base["owned"]].tolist())
    if name == "cols7":                                  # 150 cells: the last of the 22 rows holds 3, four cells are nobody's
        assert r64["layout"] == (7, 22, 35, 88) and int((~r64["owned"]).sum()) == 4 * 20
    if name == "znear":
        assert (r64["seen"][r64["owned"]] == 0).sum() > (MT.case("coarse_T4", "float64")["seen"][r64["owned"]] == 0).sum()


def test_outputs_on_request_inside_guarded_buffers():
    args, kw = case_inputs("coarse_T4")
    v, f, n, img, az, el = args
    full = mesh.bake_texture(*args, **kw)
    atlas = full["atlas"]
    Ht, Wt, S = atlas["height"], atlas["width"], kw["raster_size"]
    ws, keys = hip.mesh_rasterize(v, f.to(torch.int32), mesh.camera_rows(az, el, znear=kw["znear"], device=DEV), S)
    common = dict(power=kw["power"], depth_tol=kw["depth_tol"], fill=FILL)
    G = 257
    for name, per, dtype, guard in (("texture", 3, torch.float32, -7.5), ("weight", 1, torch.float32, -7.5), ("seen", 1, torch.int32, -77)):
        buf = torch.full((G + per * Ht * Wt + G,), guard, dtype=dtype, device=DEV)
        shape = (3, Ht, Wt) if per == 3 else (Ht, Wt)
        only = hip.mesh_texture_bake(v, f.to(torch.int32), n, img, ws, keys, S, atlas["T"], atlas["cols"], atlas["rows"], want=(),
                                     out={name: buf[G:-G].view(shape)}, **common)
        assert set(only) == {name} and torch.equal(only[name], full[name]), name
        assert bool((buf[:G] == guard).all()) and bool((buf[-G:] == guard).all()), name
    with pytest.raises(RuntimeError, match="cips3d_mesh_texture_bake failed"):
        mesh.bake_texture(*args, **dict(kw, power=9))
    with pytest.raises(RuntimeError):
        mesh.bake_texture(*args, **dict(kw, texels=2))
    with pytest.raises(ValueError, match="without faces"):
        mesh.bake_texture(v, f[:0], n, img, az, el, raster_size=S)


# ------------------------------------------------------------------------------------------------ 3. fill
def coarse_one_view_colours():
    v, f, n, _ = MR.two_spheres("coarse")
    az, el = MR.VIEWS[0]
    out = mesh.vertex_colors(cu(v), cu(f), cu(n), cu(MC.images(1, 40)), az, el, raster_size=64, fill=FILL)
    return f, out["colors"], out["weight"]


@pytest.mark.parametrize("iters", [0, 1, 3, 64])
def test_fill_is_bit_equal_to_the_restatement(iters):
    f, col, w = coarse_one_view_colours()
    got = mesh.fill_colors(col, w, cu(f), iters=iters)
    again = mesh.fill_colors(col, w, cu(f), iters=iters)
    torch.cuda.synchronize()
    assert got["colors"].dtype == torch.float32 and got["filled"].dtype == torch.int32
    ref_c, ref_f = MT.fill(col.cpu().numpy(), w.cpu().numpy(), f, iters)
    unseen = int((w == 0).sum())
    print(f"fill iters {iters}: {unseen} unseen of {len(ref_f)} vertices, {int((ref_f > 0).sum())} filled, {int((ref_f < 0).sum())} left, "
          f"last ring {int(ref_f.max())}")
    assert unseen > 20
    assert np.array_equal(got["filled"].cpu().numpy(), ref_f)
    assert np.array_equal(got["colors"].cpu().numpy().view(np.int32), ref_c.view(np.int32))
    assert torch.equal(got["colors"], again["colors"]) and torch.equal(got["filled"], again["filled"])
    seen = (w > 0)
    assert torch.equal(got["colors"][seen], col[seen])                   # seen vertices keep their bits
    if iters == 0:
        assert torch.equal(got["colors"], col) and int((got["filled"] > 0).sum()) == 0
    if iters == 64:                                      # both spheres hold seen vertices: everything is reached, well before ring 64
        assert int((got["filled"] < 0).sum()) == 0 and int(got["filled"].max()) < 64


def test_fill_ring_is_graph_distance_and_islands_stay():
    v, f = MT.strip(300)                                  # 602 vertices: more than one block
    f = np.concatenate([f, np.array([[602, 603, 604]])])  # an island no seen vertex touches
    V = 605
    col = np.full((V, 3), FILL, np.float32)
    w = np.zeros(V, np.float32)
    src = [0, 401]
    col[0], col[401] = (0.25, -0.5, 1.0), (-1.0, 0.125, 0.5)
    w[src] = 1.0
    dist = MT.graph_distance(V, f, src)
    for iters in (7, 400):
        got = mesh.fill_colors(cu(col), cu(w), cu(f), iters=iters)
        filled = got["filled"].cpu().numpy()
        want = np.where((dist >= 0) & (dist <= iters), dist, -1)
        assert np.array_equal(filled, want), iters
        ref_c, ref_f = MT.fill(col, w, f, iters)
        assert np.array_equal(ref_f, want) and np.array_equal(got["colors"].cpu().numpy().view(np.int32), ref_c.view(np.int32))
        out = got["colors"].cpu().numpy()
        assert (out[602:] == np.float32(FILL)).all() and (filled[602:] == -1).all()
        assert (out[filled < 0] == np.float32(FILL)).all()
    assert dist.max() > 64 and (want[:602] >= 0).all()
    # no faces: nothing grows; bad ring counts are refused
    none = mesh.fill_colors(cu(col), cu(w), cu(f[:0]), iters=5)
    assert torch.equal(none["colors"], cu(col)) and none["filled"].cpu().tolist() == np.where(w > 0, 0, -1).tolist()
    for bad in (-1, 4097):
        with pytest.raises(RuntimeError):
            mesh.fill_colors(cu(col), cu(w), cu(f), iters=bad)


# ------------------------------------------------------------------------------------------------ 4. fallback
def test_unseen_texels_take_the_filled_vertex_colours():
    name = "coarse_T4"
    v, f, n, attr = MR.two_spheres("coarse")
    vc = np.clip(attr * 0.5, -1, 1).astype(np.float32)
    filled = np.where(np.arange(len(v)) % 5 == 0, -1, 1).astype(np.int32)
    got, _ = run_case(name, vertex_colors=cu(vc), filled=cu(filled))
    r64, r32 = (MT.bake(fill_value=FILL, vertex_colors=vc, filled=filled, dt=dt, **MT.CASES[name]) for dt in (np.float64, np.float32))
    keep, lit, dark = check_against(name, got, r64, r32)
    fb = dark & r64["fallback"]
    rest = dark & ~r64["fallback"]
    print(f"fallback: {int(fb.sum())} unseen texels take vertex colours, {int(rest.sum())} have an unfilled corner")
    assert fb.sum() > 100 and rest.sum() > 100
    MR.check_ratio("fallback texture", got["texture"], r32["texture"], r64["texture"], np.broadcast_to(fb[None], got["texture"].shape))
    assert (got["texture"][:, rest] == np.float32(FILL)).all()
    assert (got["texture"][:, fb] != np.float32(FILL)).any(0).all()
    plain, _ = run_case(name)
    assert np.array_equal(plain["texture"][:, lit], got["texture"][:, lit]) and np.array_equal(plain["weight"], got["weight"])
    args, kw = case_inputs(name)
    with pytest.raises(RuntimeError, match="together"):
        hip.mesh_texture_bake(args[0], args[1].to(torch.int32), args[2], args[3], *hip.mesh_raster_workspace(158, 308, 2, 64, DEV), 64,
                              4, 12, 13, vertex_colors=cu(vc))


# ------------------------------------------------------------------------------------------------ 5. textured frame
@pytest.mark.parametrize("S", [33, 64])
@pytest.mark.parametrize("T", [3, 8])
def test_textured_frame_against_fp64(S, T):
    v, f, n, _ = (cu(a) for a in MR.two_spheres("coarse"))
    F = f.shape[0]
    az, el = [a for a, _ in MR.VIEWS], [e for _, e in MR.VIEWS]
    light = cu(np.stack([MR.light_of(a) for a in az]), torch.float32)
    maps = mesh.rasterize_mesh(v, f, az, el, S, normals=n, light=light, want=("face", "bary", "shade"))
    atlas = mesh.texture_atlas(F, texels=T)
    tex, c = MT.synthetic_texture(F, T, atlas["cols"], atlas["rows"], seed=S + T)
    got = hip.mesh_textured_frame(maps["face"], maps["bary"], maps["shade"], cu(tex), F, T, atlas["cols"], atlas["rows"])
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, S, S)
    face = maps["face"].cpu().numpy()
    attr = np.moveaxis(c[np.maximum(face, 0)], -1, 1)                     # [n,3,S,S]: every pixel's own face's constant
    ref, near = MC.albedo_u8(face, maps["shade"].cpu().numpy(), attr)
    got = got.cpu().numpy()
    print(f"textured frame S {S} T {T}: {int(near.sum())} of {near.size} values within 2^-10 of a half-integer, "
          f"{int((got != ref).sum())} bytes differ, {int((face >= 0).sum())} hit pixels on {len(np.unique(face)) - 1} faces")
    assert near.mean() <= 0.01
    assert np.array_equal(got[~near], ref[~near])                         # any bleed across a diagonal or a cell border fails here
    assert (np.abs(got.astype(int) - ref.astype(int))[near] <= 1).all()
    empty = face < 0
    plain = mesh.rasterize_mesh(v, f, az, el, S, normals=n, light=light, want=("shade_u8",))["shade_u8"].cpu().numpy()
    assert empty.any() and (got[np.broadcast_to(empty[:, None], got.shape)] == 255).all()
    assert (plain[np.broadcast_to(empty[:, None], got.shape)] == 255).all()
    assert len(np.unique(face)) > 20 and not np.array_equal(got[:, 0], got[:, 1])
    # the frames call is this pipeline
    traj = torch.tensor([[a, e, 6.0] for a, e in MR.VIEWS])
    frames = mesh.render_textured_frames(v, f, n, traj, cu(tex), atlas, image_size=S)
    assert torch.equal(frames.cpu(), torch.from_numpy(got))


def test_texture_to_uint8_takes_a_non_square_map():
    x = cu(np.random.RandomState(2).uniform(-1.2, 1.2, (3, 52, 60)).astype(np.float32))
    got = mesh.texture_to_uint8(x)
    want = np.rint((np.clip(x.cpu().numpy(), -1, 1) + np.float32(1)) * np.float32(127.5)).astype(np.uint8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 52, 60) and np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 6. reproducibility
def test_runs_are_bit_equal_and_buffers_can_be_reused():
    args, kw = case_inputs("subpixel_T3")
    v, f, n, img, az, el = args
    a = mesh.bake_texture(*args, **kw)
    b = mesh.bake_texture(*args, **kw)
    ws, keys = hip.mesh_raster_workspace(v.shape[0], f.shape[0], len(az), kw["raster_size"], DEV)
    ws.fill_(0x5a)
    keys.fill_(12345)
    c = mesh.bake_texture(*args, ws=ws, keys=keys, **kw)
    d = mesh.bake_texture(*args, ws=ws, keys=keys, atlas=a["atlas"], **kw)
    for k in ("texture", "weight", "seen"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and torch.equal(a[k], d[k]), k
    traj = torch.tensor([[x, e, 6.0] for x, e in MR.VIEWS])
    fa = mesh.render_textured_frames(v, f, n, traj, a["texture"], a["atlas"], image_size=48)
    fb = mesh.render_textured_frames(v, f, n, traj, a["texture"], a["atlas"], image_size=48)
    assert torch.equal(fa, fb) and bool((fa != 255).any())


# ------------------------------------------------------------------------------------------------ 7. end to end
VIEWS2 = ((0.25, 0.05), (-0.3, 0.0))


def tiny_mesh_inputs():
    G = pkg.build_generator(configs.tiny_G_cfg(hidden=32, N_layers_renderer=2), DEV, seed=5)
    g = torch.Generator().manual_seed(3)
    zs = [torch.randn(1, 32, generator=g).to(DEV), torch.randn(1, 32, generator=g).to(DEV)]
    kw = dict(resolution=32, N_samples=16, normals=True)
    vol = mesh.surface_mesh(G, zs=zs, **kw)["aligned"][0, ..., 0]
    kw["level"] = float(vol[vol != 1.0].median())        # synthetic weights: the SDF's zero level need not cross the volume
    return G, zs, kw


def test_surface_mesh_with_texture_end_to_end(tmp_path):
    from PIL import Image
    G, zs, kw = tiny_mesh_inputs()
    color_kw = dict(views=VIEWS2, img_size=8, N_samples=6, raster_size=48)
    torch.manual_seed(11)
    coloured = mesh.surface_mesh(G, zs=zs, colors=True, color_kw=color_kw, **kw)
    torch.manual_seed(11)
    out = mesh.surface_mesh(G, zs=zs, colors=True, texture=True, color_kw=color_kw, texture_kw=dict(texels=3), **kw)
    assert set(out) == set(coloured) | {"textures"}
    v, f, n, col = out["meshes"][0]
    for a, b in zip(coloured["meshes"][0], (v, f, n, col)):
        assert torch.equal(a, b)                          # geometry and colours are the untextured call's
    t = out["textures"][0]
    atlas = t["atlas"]
    F, V = f.shape[0], v.shape[0]
    Ht, Wt = atlas["height"], atlas["width"]
    assert atlas["T"] == 3 and atlas["n_faces"] == F and tuple(t["texture"].shape) == (3, Ht, Wt) and F > 100
    assert tuple(t["colors"].shape) == (V, 3) and tuple(t["filled"].shape) == (V,)
    assert bool(torch.isfinite(t["texture"]).all())
    seen, filled, never = mesh.texel_counts(t, t["filled"], f)
    owned = int((mesh.atlas_texels(atlas)["face"] >= 0).sum())
    print(f"end to end: V {V} F {F}, atlas {Wt} x {Ht}, texels seen {seen} filled {filled} never {never} of {owned}")
    assert seen + filled + never == owned == F * 6 and seen > 0
    assert bool((t["filled"][t["color_weight"] > 0] == 0).all()) and torch.equal(t["seen_colors"], col)
    # without the fill behind it, the same texels are seen; the unseen ones hold the constant
    torch.manual_seed(11)
    direct = mesh.texture_mesh(G, v, f, n, zs=zs, texels=3, fill_iters=0, **color_kw)
    assert torch.equal(direct["weight"], t["weight"]) and torch.equal(direct["texture"][:, t["weight"] > 0], t["texture"][:, t["weight"] > 0])
    # files
    u8 = mesh.texture_to_uint8(t["texture"])
    png = gen_images.write_texture_png(str(tmp_path / "m.png"), u8.cpu().numpy())
    gen_images.write_mtl(str(tmp_path / "m.mtl"), "m.png")
    obj = gen_images.write_textured_obj(str(tmp_path / "m.obj"), v.cpu().numpy(), f.cpu().numpy(), atlas["uv"].numpy(), Wt, Ht,
                                        normals=n.cpu().numpy(), mtl="m.mtl")
    vt = np.array([[float(x) for x in ln.split()[1:]] for ln in open(obj) if ln.startswith("vt ")])
    assert vt.shape == (3 * F, 2) and vt.min() >= 0 and vt.max() <= 1
    with Image.open(png) as im:
        assert im.size == (Wt, Ht)
    rv, rf = mesh.read_obj(obj)
    assert torch.equal(rf, f.cpu()) and rv.shape == v.shape
    # frames
    traj = torch.tensor([[0.25, 0.05, 6.0], [-0.5, 0.1, 7.0]])
    frames = mesh.render_textured_frames(v, f, n, traj, t["texture"], atlas, image_size=40)
    grey = mesh.render_mesh_frames(v, f, n, traj, image_size=40)
    hit = mesh.rasterize_mesh(v, f, traj[:, 0], traj[:, 1], 40, fov_deg=2 * traj[:, 2], want=("face",))["face"] >= 0
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 3, 40, 40)
    white = ~hit[:, None].expand(-1, 3, -1, -1)
    assert bool((frames[white] == 255).all()) and bool((grey[white] == 255).all()) and bool(hit.any()) and bool((~hit).any())
    assert not torch.equal(frames, grey)
    with pytest.raises(ValueError, match="normals"):
        mesh.surface_mesh(G, zs=zs, texture=True, resolution=32, N_samples=16)
    with pytest.raises(ValueError, match="decoder"):
        mesh.surface_mesh(G, zs=zs[:1], texture=True, **kw)


def test_extract_mesh_tool_writes_a_textured_obj(tmp_path):
    from PIL import Image
    path = str(tmp_path / "m.obj")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_mesh.py"), "--resolution", "32", "--colors", "--texture",
                        "--texels", "3", "--fill-iters", "8", "--color-views", "0,0;0.35,0.05", "--out", path],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"texture"' in ln]
    assert len(line) == 1
    import json
    info = json.loads(line[0])["texture"]
    lines = open(path).read().splitlines()
    n_f = sum(ln.startswith("f ") for ln in lines)
    assert lines[0] == "mtllib m.mtl" and sum(ln.startswith("vt ") for ln in lines) == 3 * n_f and n_f > 0
    assert "map_Kd m.png" in open(str(tmp_path / "m.mtl")).read()
    with Image.open(str(tmp_path / "m.png")) as im:
        assert list(im.size) == info["atlas"] and info["texels"] == 3
    assert info["seen"] + info["filled"] + info["never_filled"] == n_f * 6 and info["seen"] > 0
