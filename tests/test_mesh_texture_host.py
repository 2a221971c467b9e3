"""The mesh texture atlas without a GPU: the entry points are exported under the bumped ABI version, their argument contracts
(negative codes are decided on the host, nothing is launched), the atlas layout against its numpy restatement, the
bilinear-footprint property of the layout, the fill's restatement on a hand-computed strip, the yardstick's excluded share on
every case the GPU test uses, and the OBJ / MTL / PNG writers' round trips."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _mesh_color_cases as MC
import _mesh_raster_cases as MR
import _mesh_texture_cases as MT
from cips_3dplusplus_amd import _lib, gen_images, hip, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cips3d_mesh_fill_colors", "cips3d_mesh_fill_workspace_bytes", "cips3d_mesh_texture_bake",
                "cips3d_mesh_textured_frame", "cips3d_mesh_atlas_layout", "cips3d_mesh_atlas_uv", "cips3d_mesh_atlas_texels")
P = 64                                                  # a non-null pointer that is never dereferenced on the host


def test_library_declares_and_exports_the_texture_pass():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED and getattr(lib, name) is not None, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 44
    which = [k for k, st in _lib._struct_table().items() if st is _lib.MeshTextureParams]
    assert len(which) == 1 and lib.cips3d_sizeof_struct(which[0]) == C.sizeof(_lib.MeshTextureParams) == 136
    from cips_3dplusplus_amd import build
    assert "mesh_texture.hip" in build.SOURCES


# ------------------------------------------------------------------------------------------------ argument errors
def _good_bake():
    p = _lib.MeshTextureParams()
    p.verts = p.faces = p.normals = p.images = p.workspace = p.keys = p.texture = P
    p.V, p.F, p.n_views, p.S, p.R, p.power, p.T, p.cols, p.rows = 3, 4, 1, 8, 4, 2, 8, 2, 1
    return p


def test_bake_bad_arguments_launch_nothing():
    bake = _lib.load().cips3d_mesh_texture_bake
    assert bake(None, None) == -1
    assert bake(C.byref(_lib.MeshTextureParams()), None) == -1
    for field in ("verts", "faces", "normals", "images", "workspace", "keys"):
        p = _good_bake()
        setattr(p, field, None)
        assert bake(C.byref(p), None) == -1, field
    p = _good_bake()
    p.texture = None
    assert bake(C.byref(p), None) == -1                                           # no output at all
    for field in ("vertex_colors", "filled"):                                     # one of the pair without the other
        p = _good_bake()
        setattr(p, field, P)
        assert bake(C.byref(p), None) == -1, field
    for field, bad in (("V", -1), ("F", -1), ("n_views", -1), ("S", 0), ("R", 0), ("power", 0), ("power", 9), ("T", 2), ("T", 65),
                       ("cols", 0), ("rows", -1), ("cols", 1)):                   # (cols 1 x rows 1 holds two faces, not four)
        p = _good_bake()
        setattr(p, field, bad)
        assert bake(C.byref(p), None) == -1, (field, bad)
    for field, big in (("S", 16385), ("R", 16385), ("n_views", 65537), ("cols", 1821), ("rows", 2049)):
        p = _good_bake()                                                          # 1821 x 9 = 16389, 2049 x 8 = 16392 texels
        setattr(p, field, big)
        assert bake(C.byref(p), None) == -2, (field, big)
    p = _good_bake()
    p.cols, p.power = 1821, 0
    assert bake(C.byref(p), None) == -1                                           # a bad argument wins over an unsupported size
    for field in ("V", "F"):
        p = _good_bake()
        setattr(p, field, 0)
        p.verts = p.faces = p.normals = p.images = None
        assert bake(C.byref(p), None) == 0, field                                 # nothing to do


def test_fill_bad_arguments_launch_nothing():
    lib = _lib.load()
    fill = lib.cips3d_mesh_fill_colors
    good = [P, P, P, 3, 1, 4, 2 * P, P, P, None]
    for k in (0, 1, 2, 6, 7, 8):
        args = list(good)
        args[k] = None
        assert fill(*args) == -1, k
    for k, bad in ((3, -1), (4, -1), (5, -1), (5, 4097)):
        args = list(good)
        args[k] = bad
        assert fill(*args) == -1, (k, bad)
    args = list(good)
    args[6] = P
    assert fill(*args) == -1                                                      # in place
    for k in (3, 4):
        args = list(good)
        args[k] = 2 ** 31
        assert fill(*args) == -2, k
    assert fill(None, None, None, 0, 1, 4, None, None, None, None) == 0 and fill(P, P, None, 3, 0, 4, 2 * P, P, P, None) == 0
    assert lib.cips3d_mesh_fill_workspace_bytes(-1) == -1 and lib.cips3d_mesh_fill_workspace_bytes(2 ** 31) == -2
    assert lib.cips3d_mesh_fill_workspace_bytes(10) >= 10 * 32 + 4097 * 4


def test_textured_frame_bad_arguments_launch_nothing():
    frame = _lib.load().cips3d_mesh_textured_frame
    good = [P, P, P, P, P, 1, 8, 4, 8, 2, 1, None]
    for k in range(5):
        args = list(good)
        args[k] = None
        assert frame(*args) == -1, k
    for k, bad in ((5, -1), (6, 0), (7, -1), (8, 2), (8, 65), (9, 0), (10, -1), (9, 1)):
        args = list(good)
        args[k] = bad
        assert frame(*args) == -1, (k, bad)
    for k, big in ((5, 65537), (6, 16385), (9, 1821), (10, 2049), (7, 2 ** 31)):
        args = list(good)
        args[k] = big
        if k == 7:
            args[9], args[10] = 1820, 2048                                        # (too few cells for 2^31 faces: a bad argument)
            assert frame(*args) == -1
        else:
            assert frame(*args) == -2, (k, big)
    for k in (5, 7):
        args = list(good)
        args[k] = 0
        assert frame(*args) == 0, k                                               # no views / no faces: nothing to do


def test_uint8_step_bad_arguments_launch_nothing():
    """The texture -> uint8 step is cips3d_rgb_to_uint8, which takes a flat element count: any map size."""
    u8 = _lib.load().cips3d_rgb_to_uint8
    assert u8(None, P, 16, None) == -1 and u8(P, None, 16, None) == -1 and u8(P, P, -1, None) == -1
    assert u8(P + 4, P, 16, None) == -2                                           # a misaligned pointer
    assert u8(None, None, 0, None) == 0


def test_atlas_calls_bad_arguments():
    lib = _lib.load()
    o = [C.c_int32(0) for _ in range(4)]
    refs = [C.byref(x) for x in o]
    assert lib.cips3d_mesh_atlas_layout(10, 8, 0, *refs) == 0 and o[0].value * o[1].value >= 5
    assert lib.cips3d_mesh_atlas_layout(10, 2, 0, *refs) == -1 and lib.cips3d_mesh_atlas_layout(10, 65, 0, *refs) == -1
    assert lib.cips3d_mesh_atlas_layout(-1, 8, 0, *refs) == -1 and lib.cips3d_mesh_atlas_layout(10, 8, -1, *refs) == -1
    assert lib.cips3d_mesh_atlas_layout(10, 8, 0, None, *refs[1:]) == -1
    assert lib.cips3d_mesh_atlas_layout(10, 8, 1821, *refs) == -2                 # too wide
    assert lib.cips3d_mesh_atlas_layout(2 * 2049, 8, 1, *refs) == -2              # too tall
    assert lib.cips3d_mesh_atlas_layout(2 ** 31, 8, 0, *refs) == -2
    assert lib.cips3d_mesh_atlas_uv(4, 8, 2, None) == -1 and lib.cips3d_mesh_atlas_uv(4, 2, 2, P) == -1
    assert lib.cips3d_mesh_atlas_texels(4, 8, 1, 1, None, None, None) == -1       # two cells needed
    with pytest.raises(RuntimeError):
        mesh.texture_atlas(100, texels=2)
    with pytest.raises(RuntimeError):
        mesh.texture_atlas(2 * 2049, texels=8, cols=1)


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("T", [3, 4, 8])
@pytest.mark.parametrize("F", [1, 2, 7, 308])
@pytest.mark.parametrize("cols", [None, 1, 7])
def test_atlas_layout(T, F, cols):
    atlas = mesh.texture_atlas(F, texels=T, cols=cols)
    c, r, Wt, Ht = MT.layout(F, T, cols)
    assert (atlas["T"], atlas["cols"], atlas["rows"], atlas["width"], atlas["height"], atlas["n_faces"]) == (T, c, r, Wt, Ht, F)
    assert atlas["uv"].dtype == torch.float32 and np.array_equal(atlas["uv"].numpy(), MT.corner_uv(F, T, c).astype(np.float32))
    face, gutter, li, lj = MT.classify(F, T, c, r)
    tex = mesh.atlas_texels(atlas)
    assert np.array_equal(tex["face"].numpy(), face) and np.array_equal(tex["gutter"].numpy(), gutter)
    b32 = np.stack(MT.bary(li, lj, T, np.float32), -1) * (face >= 0)[..., None]
    assert np.array_equal(tex["bary"].numpy(), b32)
    # every texel has exactly one classification: unowned, or one face as owned or gutter; the counts per face
    assert face.shape == (Ht, Wt) and face.min() >= -1 and face.max() == F - 1
    for f in range(F):
        mine = face == f
        assert int((mine & ~gutter).sum()) == T * (T - 1) // 2 and int((mine & gutter).sum()) == T, f
    assert int((face < 0).sum()) == Ht * Wt - F * (T * (T - 1) // 2 + T)
    if F % 2:                                            # the last cell's upper half is unowned
        oc = (F - 1) // 2
        cell = face[(oc // c) * T:(oc // c + 1) * T, (oc % c) * (T + 1):(oc % c + 1) * (T + 1)]
        assert int((cell == F - 1).sum()) == int((cell < 0).sum()) == T * (T + 1) // 2
    # a texel's lattice point is where its centre lies in the face's UV triangle; the corners have b = unit vectors
    uv = MT.corner_uv(F, T, c)
    b = np.stack(MT.bary(li, lj, T, np.float64), -1)
    ys, xs = np.nonzero((face >= 0) & ~gutter)
    pos = np.einsum("nk,nkc->nc", b[ys, xs], uv[face[ys, xs]])
    assert np.abs(pos - np.stack([xs + 0.5, ys + 0.5], -1)).max() <= 1e-12
    assert np.abs(b[ys, xs].sum(-1) - 1).max() <= 1e-12


@pytest.mark.parametrize("T,F,cols", [(3, 7, None), (4, 7, 1), (8, 7, None), (5, 308, 7), (64, 3, None)])
def test_bilinear_fetch_stays_inside_the_face(T, F, cols):
    """A bilinear fetch at any point of a face's UV triangle reads, with non-zero weight, only texels the face owns or its own
    gutter: exhaustively over a barycentric lattice of step 1/16 (every product below is exact in fp64, so points on the
    triangle's edges sit exactly on them), and at random interior points."""
    c, r, Wt, Ht = MT.layout(F, T, cols)
    face, _, _, _ = MT.classify(F, T, c, r)
    uv = MT.corner_uv(F, T, c)
    rng = np.random.RandomState(T * 1000 + F)
    N = 16
    lattice = [(p / N, q / N) for p in range(N + 1) for q in range(N + 1 - p)]
    n_taps = 0
    for f in range(F):
        rnd = rng.uniform(0, 1, (40, 2))
        rnd = np.where((rnd.sum(1) > 1)[:, None], 1 - rnd, rnd)
        for b1, b2 in lattice + [tuple(x) for x in rnd]:
            x = uv[f, 0, 0] + b1 * (uv[f, 1, 0] - uv[f, 0, 0]) + b2 * (uv[f, 2, 0] - uv[f, 0, 0])
            y = uv[f, 0, 1] + b1 * (uv[f, 1, 1] - uv[f, 0, 1]) + b2 * (uv[f, 2, 1] - uv[f, 0, 1])
            for tx, ty in MT.bilinear_footprint(x, y, Wt, Ht):
                assert face[ty, tx] == f, (f, b1, b2, tx, ty, int(face[ty, tx]))
                n_taps += 1
    assert n_taps >= F * len(lattice)


# ------------------------------------------------------------------------------------------------ fill
def test_fill_restatement_on_a_hand_computed_strip():
    """Four columns; only vertex 0 is seen, colour (1, 0.5, -0.25).  Ring 1 reaches 1 and 2 (the corners of face 0), ring 2
    vertex 3, ring 3 vertex 4 and 5 ... and a copy of one colour stays that colour: its multiples of 2^-20 are exact."""
    v, f = MT.strip(4)
    col = np.zeros((10, 3), np.float32)
    col[0] = (1.0, 0.5, -0.25)
    w = np.zeros(10, np.float32)
    w[0] = 2.0
    out, filled = MT.fill(col, w, f, 64)
    assert filled.tolist() == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5] == MT.graph_distance(10, f, [0]).tolist()
    assert (out == col[0]).all()
    # two sources of different colour: vertex 2 of (0, 2, 1), (1, 2, 3), (2, 4, 3) takes (c0 + c1 + c1) / 3 in ring 1 -- the pair
    # (face, corner) counts, so vertex 1, which shares two faces with it, counts twice
    col[1] = (0.0, 0.25, 0.5)
    w[1] = 1.0
    out, filled = MT.fill(col, w, f, 1)
    assert filled.tolist() == [0, 0, 1, 1, -1, -1, -1, -1, -1, -1]
    q = lambda x: np.rint(np.float32(x) * np.float32(2 ** 20)).astype(np.int64)      # noqa: E731
    want2 = ((q(col[0]) + 2 * q(col[1])).astype(np.float64) / (3 * 1048576.0)).astype(np.float32)
    assert np.array_equal(out[2], want2) and np.array_equal(out[3], col[1]) and (out[4:] == 0).all()
    assert abs(float(out[2][0]) - 1 / 3) < 1e-6
    # iters = 0: the identity; an unreachable component keeps its colour and -1
    out0, filled0 = MT.fill(col, w, f, 0)
    assert np.array_equal(out0, col) and filled0.tolist() == [0, 0] + [-1] * 8
    f2 = np.concatenate([f, f[:2] + 10])
    col2, w2 = np.concatenate([col, np.full((4, 3), 0.375, np.float32)]), np.concatenate([w, np.zeros(4, np.float32)])
    out2, filled2 = MT.fill(col2, w2, f2, 64)
    assert (filled2[10:] == -1).all() and (out2[10:] == np.float32(0.375)).all() and (filled2[:10] >= 0).all()


# ------------------------------------------------------------------------------------------------ the bake's yardstick
@pytest.mark.parametrize("name", list(MT.CASES))
def test_yardstick_excludes_little_and_fp32_agrees(name):
    r64, r32 = MT.case(name, "float64"), MT.case(name, "float32")
    tie, owned = r64["tie"], r64["owned"]
    share = tie[:, owned].mean()
    hist = np.bincount(r64["seen"][owned], minlength=3).tolist()
    print(f"{name}: atlas {r64['layout']}, excluded pairs {int(tie.sum())} of {tie[:, owned].size} ({100 * share:.2f} %), "
          f"seen histogram {hist}")
    assert share <= MC.CAP
    keep = owned & ~tie.any(0)
    assert np.array_equal(r32["seen"][keep], r64["seen"][keep])
    assert not tie[:, ~owned].any() and (r64["seen"][~owned] == 0).all() and (r64["texture"][:, ~owned] == MT.FILL).all()
    if name in MT.PARITY:
        assert all(h > 0 for h in hist[:3])              # texels seen by 0, 1 and 2 views


# ------------------------------------------------------------------------------------------------ writers
def test_textured_obj_mtl_png_round_trip(tmp_path):
    from PIL import Image
    v, f, n, _ = MR.two_spheres("coarse")
    atlas = mesh.texture_atlas(len(f), texels=4)
    Wt, Ht = atlas["width"], atlas["height"]
    tex = np.random.RandomState(0).randint(0, 256, (3, Ht, Wt)).astype(np.uint8)
    png = gen_images.write_texture_png(str(tmp_path / "m.png"), tex)
    with Image.open(png) as im:
        assert im.size == (Wt, Ht) and im.mode == "RGB" and np.array_equal(np.asarray(im), tex.transpose(1, 2, 0))
    mtl = gen_images.write_mtl(str(tmp_path / "m.mtl"), "m.png")
    text = open(mtl).read()
    assert "newmtl textured" in text and "map_Kd m.png" in text
    for normals in (None, n):
        path = gen_images.write_textured_obj(str(tmp_path / "m.obj"), v, f, atlas["uv"].numpy(), Wt, Ht, normals=normals, mtl="m.mtl")
        rv, rf = mesh.read_obj(path)
        assert np.array_equal(rf.numpy(), f) and rv.shape == v.shape and np.abs(rv.numpy() - v).max() <= 1e-6
        lines = open(path).read().splitlines()
        assert lines[0] == "mtllib m.mtl" and "usemtl textured" in lines
        vt = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("vt ")])
        assert vt.shape == (3 * len(f), 2) and vt.min() >= 0 and vt.max() <= 1
        uv = atlas["uv"].numpy().reshape(-1, 2).astype(np.float64)
        assert np.abs(vt[:, 0] - uv[:, 0] / Wt).max() <= 1e-7 and np.abs(vt[:, 1] - (1 - uv[:, 1] / Ht)).max() <= 1e-7
        faces = [ln.split()[1:] for ln in lines if ln.startswith("f ")]
        assert lines.index("usemtl textured") < lines.index("f " + " ".join(faces[0]))
        for k, tri in enumerate(faces):
            for c, item in enumerate(tri):
                parts = item.split("/")
                assert len(parts) == (2 if normals is None else 3) and int(parts[1]) == 3 * k + c + 1
                assert int(parts[0]) == f[k, c] + 1 and (normals is None or parts[2] == parts[0])
        assert sum(ln.startswith("vn ") for ln in lines) == (0 if normals is None else len(v))
    with pytest.raises(ValueError):
        gen_images.write_textured_obj(str(tmp_path / "bad.obj"), v, f, atlas["uv"].numpy()[:5], Wt, Ht)
    with pytest.raises(ValueError):
        gen_images.write_texture_png(str(tmp_path / "bad.png"), tex.astype(np.float32))


def test_new_signatures_and_defaults():
    sm = inspect.signature(mesh.surface_mesh).parameters
    assert sm["texture"].default is False and sm["texture_kw"].default is None
    ta = inspect.signature(mesh.texture_atlas).parameters
    assert list(ta) == ["n_faces", "texels", "cols"] and ta["texels"].default == 8 and ta["cols"].default is None
    assert inspect.signature(mesh.fill_colors).parameters["iters"].default == 64
    bt = inspect.signature(mesh.bake_texture).parameters
    assert (bt["texels"].default, bt["raster_size"].default, bt["depth_tol"].default, bt["power"].default, bt["fill"].default,
            bt["znear"].default) == (8, 512, None, 2, 0.0, 0.01)
    tm = inspect.signature(mesh.texture_mesh).parameters
    assert tm["fill_iters"].default == 64 and tm["texels"].default == 8 and tm["views"].default == mesh.DEFAULT_COLOR_VIEWS
    assert hip.mesh_atlas_layout(453278, 8) == (449, 505, 4041, 4040)
