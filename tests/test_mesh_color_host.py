"""Mesh colours without a GPU: the entry points are exported under the bumped ABI version, their argument contracts (negative
codes are decided on the host, nothing is launched), the numpy yardstick's excluded share on every case the GPU test uses, the
OBJ / PLY writers' round trips, and the defaults of the signatures that gained arguments."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _mesh_color_cases as MC
import _mesh_raster_cases as MR
from cips_3dplusplus_amd import _lib, gen_images, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cips3d_mesh_vertex_colors", "cips3d_mesh_albedo_frame")


def test_library_declares_and_exports_the_colour_pass():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED and getattr(lib, name) is not None, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 43
    which = [k for k, st in _lib._struct_table().items() if st is _lib.MeshColorParams]
    assert len(which) == 1 and lib.cips3d_sizeof_struct(which[0]) == C.sizeof(_lib.MeshColorParams) == 96
    from cips_3dplusplus_amd import build
    assert "mesh_color.hip" in build.SOURCES


def _good_params(P=64):
    p = _lib.MeshColorParams()
    p.verts = p.normals = p.images = p.workspace = p.keys = p.colors = P          # (never dereferenced on the host)
    p.V, p.n_views, p.S, p.R, p.power = 3, 1, 8, 4, 2
    return p


def test_vertex_colors_bad_arguments_launch_nothing():
    lib = _lib.load()
    col = lib.cips3d_mesh_vertex_colors
    assert col(None, None) == -1
    assert col(C.byref(_lib.MeshColorParams()), None) == -1                       # everything null, S = 0
    for field in ("verts", "normals", "images", "workspace", "keys"):
        p = _good_params()
        setattr(p, field, None)
        assert col(C.byref(p), None) == -1, field
    p = _good_params()
    p.colors = None
    assert col(C.byref(p), None) == -1                                            # no output at all
    for field, bad in (("V", -1), ("n_views", -1), ("S", 0), ("R", 0), ("power", 0), ("power", 9), ("power", -2)):
        p = _good_params()
        setattr(p, field, bad)
        assert col(C.byref(p), None) == -1, (field, bad)
    for field, big in (("S", 16385), ("R", 16385), ("n_views", 65537)):
        p = _good_params()
        setattr(p, field, big)
        assert col(C.byref(p), None) == -2, (field, big)
    p = _good_params()
    p.S, p.power = 16385, 0
    assert col(C.byref(p), None) == -1                                            # a bad argument wins over an unsupported size
    p = _good_params()
    p.V = 0
    p.verts = p.normals = p.images = None
    assert col(C.byref(p), None) == 0                                             # no vertices: nothing to do


def test_albedo_frame_bad_arguments_launch_nothing():
    alb = _lib.load().cips3d_mesh_albedo_frame
    P = 64
    for k in range(4):
        args = [P, P, P, P]
        args[k] = None
        assert alb(*args, 1, 8, None) == -1, k
    assert alb(P, P, P, P, -1, 8, None) == -1 and alb(P, P, P, P, 1, 0, None) == -1
    assert alb(P, P, P, P, 1, 16385, None) == -2 and alb(P, P, P, P, 65537, 8, None) == -2
    assert alb(P, P, P, P, 0, 8, None) == 0                                       # no views: nothing to do


@pytest.mark.parametrize("name", list(MC.CASES))
def test_yardstick_excludes_little_and_fp32_agrees(name):
    """At most 3 % of the (view, vertex) pairs sit on a tie, and outside them the fp32 run of the same code takes every
    decision the fp64 run takes: the exclusion bands are wider than fp32's uncertainty on these cases."""
    r64, r32 = MC.case(name, "float64"), MC.case(name, "float32")
    tie = r64["tie"]
    print(f"{name}: excluded pairs per view {tie.sum(1).tolist()} of {tie.shape[1]} ({100 * tie.mean():.2f} %), "
          f"seen histogram {np.bincount(r64['seen']).tolist()}")
    assert tie.mean() <= MC.CAP
    assert np.array_equal(r32["faces_view"][~tie], r64["faces_view"][~tie])
    keep = ~tie.any(0)
    assert np.array_equal(r32["seen"][keep], r64["seen"][keep])
    if name in ("coarse", "subpixel"):
        # not trivial: some vertices are seen by both views, some by one, some by none
        assert (r64["seen"] == 0).any() and (r64["seen"] == 1).any() and (r64["seen"] == 2).any()
    assert (r64["seen"] > 0).any()


def test_yardstick_covers_the_cases_the_issue_names():
    """The coarse case holds off-frame vertices and vertices of the large sphere hidden by the small one."""
    v, f, n, _ = MR.two_spheres("coarse")
    S = MC.CASES["coarse"][2]
    r64 = MC.case("coarse", "float64")
    off = 0
    for k, (az, el) in enumerate(MR.VIEWS):
        sx, sy, _, kept, _ = MC.project(v, az, el, S, 12.0, 1.0, 0.01, np.float64)
        off += int((~((np.rint(sx) >= 0) & (np.rint(sx) <= S - 1) & (np.rint(sy) >= 0) & (np.rint(sy) <= S - 1))).sum())
    print(f"off-frame (view, vertex) pairs: {off}")
    assert off >= 1
    # on the large sphere (its 128 vertices come first), squarely facing view 0 (no grazing angle), yet unseen by it: hidden by
    # the small sphere
    C0 = MR.camera(*MR.VIEWS[0], 12.0, 1.0, np.float64)[0]
    d = (C0 - v) / np.linalg.norm(C0 - v, axis=1, keepdims=True)
    facing = (d * n).sum(1) > 0.6
    hidden = facing[:128] & ~r64["faces_view"][0][:128]
    print(f"large-sphere vertices hidden from view 0 by the small sphere: {int(hidden.sum())}")
    assert hidden.any()


def test_obj_round_trip_with_colours(tmp_path):
    v, f, n, attr = MR.two_spheres("coarse")
    colors = np.clip(attr, -1.5, 1.5)                                             # some beyond [-1, 1]: clamped
    for normals in (None, n):
        path = gen_images.write_obj(str(tmp_path / "m.obj"), v, f, normals, colors)
        rv, rf = mesh.read_obj(path)
        assert np.array_equal(rf.numpy(), f)
        # the writer prints positions with 7 significant digits (unchanged): half a unit of the last printed digit, and the
        # reader's rounding to fp32
        digit = 10.0 ** (np.floor(np.log10(np.maximum(np.abs(v.astype(np.float64)), 1e-30))) - 6)
        assert (np.abs(rv.numpy().astype(np.float64) - v) <= 0.5 * digit + np.abs(v) * 2.0 ** -24).all()
        rows = [line.split() for line in open(path) if line.startswith("v ")]
        assert all(len(r) == 7 for r in rows)
        rgb = np.array([[float(x) for x in r[4:]] for r in rows])
        assert rgb.min() >= 0 and rgb.max() <= 1
        assert np.abs(rgb - np.clip((colors.astype(np.float64) + 1) / 2, 0, 1)).max() <= 0.5e-6      # the printed precision
    plain = gen_images.write_obj(str(tmp_path / "p.obj"), v, f, n)
    assert all(len(line.split()) == 4 for line in open(plain) if line.startswith("v "))              # without colours: as before


def test_ply_round_trip(tmp_path):
    v, f, n, attr = MR.two_spheres("coarse")
    colors = np.clip(attr, -1.5, 1.5)
    for normals, cols in ((None, None), (n, None), (None, colors), (n, colors)):
        path = gen_images.write_ply(str(tmp_path / "m.ply"), v, f, normals, cols)
        assert open(path, "rb").read(4) == b"ply\n"
        got = mesh.read_ply(path)
        assert set(got) == {"verts", "faces"} | ({"normals"} if normals is not None else set()) | ({"colors"} if cols is not None else set())
        assert got["verts"].dtype == torch.float32 and got["faces"].dtype == torch.int64
        assert np.array_equal(got["verts"].numpy(), v) and np.array_equal(got["faces"].numpy(), f)
        if normals is not None:
            assert np.array_equal(got["normals"].numpy(), n)
        if cols is not None:
            assert got["colors"].dtype == torch.uint8
            want = np.clip((cols.astype(np.float64) + 1) / 2, 0, 1)
            assert np.abs(got["colors"].numpy() / 255.0 - want).max() <= 1 / 255
    size = os.path.getsize(path)
    assert size < 300 + len(v) * 27 + len(f) * 13
    with pytest.raises(ValueError):
        gen_images.write_ply(str(tmp_path / "bad.ply"), v, f + len(v))
    with pytest.raises(ValueError):
        gen_images.write_ply(str(tmp_path / "bad.ply"), v, f, colors=colors[:5])


def test_signatures_keep_their_defaults():
    sm = inspect.signature(mesh.surface_mesh).parameters
    assert sm["colors"].default is False and sm["color_kw"].default is None and sm["normals"].default is False
    assert [k for k in sm][:4] == ["G", "zs", "style_render", "truncation"] and sm["resolution"].default == 128
    rf = inspect.signature(mesh.render_mesh_frames).parameters
    assert list(rf) == ["verts", "faces", "normals", "trajectory", "image_size", "light", "colors"]
    assert rf["colors"].default is None and rf["image_size"].default == 512 and rf["light"].default is None
    vc = inspect.signature(mesh.vertex_colors).parameters
    assert (vc["fov_deg"].default, vc["dist"].default, vc["znear"].default, vc["raster_size"].default, vc["depth_tol"].default,
            vc["power"].default, vc["fill"].default) == (12.0, 1.0, 0.01, 512, None, 2, 0.0)
    cm = inspect.signature(mesh.color_mesh).parameters
    assert cm["views"].default == ((0, 0), (0.4, 0), (-0.4, 0)) and cm["img_size"].default == 64 and cm["N_samples"].default == 24
    wo = inspect.signature(gen_images.write_obj).parameters
    assert list(wo) == ["path", "verts", "faces", "normals", "colors"] and wo["colors"].default is None
    assert MC.DEFAULT_DEPTH_TOL == mesh.FRAME_SCALE / 128
