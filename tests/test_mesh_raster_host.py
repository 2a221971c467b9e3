"""The mesh rasteriser without a GPU: the entry points are exported under the bumped ABI version, their argument contracts,
the torch-op mesh helpers (subdivide, the subdivision ladder, the OBJ reader), and two facts about the numpy yardstick the GPU
tests lean on: its excluded share stays under 1 % and its fp32 run picks the fp64 run's face on every pixel."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _mesh_raster_cases as MR
from cips_3dplusplus_amd import _lib, gen_images, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cips3d_mesh_raster_workspace_bytes", "cips3d_mesh_rasterize", "cips3d_mesh_resolve")


def test_library_declares_and_exports_the_rasteriser():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED and getattr(lib, name) is not None, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 34
    assert lib.cips3d_sizeof_struct(11) == C.sizeof(_lib.MeshResolveParams)


def test_bad_arguments_launch_nothing():
    """Negative codes are decided on the host before any GPU call."""
    lib = _lib.load()
    ws = lib.cips3d_mesh_raster_workspace_bytes
    assert ws(10, 20, 2, 64) >= 16 * 10 * 2
    assert ws(0, 0, 0, 1) >= 0
    assert ws(-1, 0, 1, 8) == -1 and ws(1, -1, 1, 8) == -1 and ws(1, 1, -1, 8) == -1 and ws(1, 1, 1, 0) == -1
    assert ws(2 ** 31, 1, 1, 8) == -2 and ws(1, 2 ** 31, 1, 8) == -2 and ws(1, 1, 1, 16385) == -2
    ras = lib.cips3d_mesh_rasterize
    P = 64                                                                       # (never dereferenced on the host)
    assert ras(None, 3, P, 1, P, 1, 8, P, P, None) == -1                         # vertices
    assert ras(P, 3, None, 1, P, 1, 8, P, P, None) == -1                         # faces
    assert ras(P, 3, P, 1, None, 1, 8, P, P, None) == -1                         # cameras
    assert ras(P, 3, P, 1, P, 1, 8, None, P, None) == -1                         # workspace
    assert ras(P, 3, P, 1, P, 1, 8, P, None, None) == -1                         # keys
    assert ras(P, 3, P, 1, P, 1, 0, P, P, None) == -1                            # S < 1
    assert ras(P, 3, P, 1, P, 1, 16385, P, P, None) == -2
    assert ras(P, 3, P, 1, P, 0, 8, P, P, None) == 0                             # no views: nothing to do
    res = lib.cips3d_mesh_resolve
    assert res(None, None) == -1
    p = _lib.MeshResolveParams()
    assert res(C.byref(p), None) == -1                                           # everything null, S = 0
    p.V, p.F, p.n_views, p.S = 3, 1, 1, 8
    assert res(C.byref(p), None) == -1
    p.verts = p.faces = p.workspace = P
    assert res(C.byref(p), None) == -1                                           # no keys
    p.keys = p.attr_out = P
    assert res(C.byref(p), None) == -1                                           # attr_out without attr
    p.attr, p.n_attr = P, 0
    assert res(C.byref(p), None) == -1                                           # ... without a channel count
    p.attr_out, p.shade = None, P
    assert res(C.byref(p), None) == -1                                           # shade without normals / light
    p.normals = P
    assert res(C.byref(p), None) == -1                                           # ... still no light
    p.light, p.n_views = P, 0
    assert res(C.byref(p), None) == 0                                            # no views: nothing to do


OCTA_V = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)
OCTA_F = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], np.int64)


def _area(v, f):
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum()


def _edge_counts(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def test_subdivide_matches_the_numpy_restatement():
    v, f = torch.from_numpy(OCTA_V), torch.from_numpy(OCTA_F)
    rv, rf = OCTA_V, OCTA_F
    for level, (n_v, n_f) in enumerate(((18, 32), (66, 128))):
        v, f = mesh.subdivide(v, f)
        rv, rf = MR.subdivide_np(rv, rf)
        assert tuple(v.shape) == (n_v, 3) and tuple(f.shape) == (n_f, 3) and f.dtype == torch.int64
        assert np.array_equal(f.numpy(), rf) and np.array_equal(v.numpy(), rv)
        assert (_edge_counts(f.numpy()) == 2).all()                               # closed in, closed out
        assert abs(_area(v.numpy(), f.numpy()) - _area(OCTA_V, OCTA_F)) <= 1e-6
    assert np.array_equal(v[:6].numpy(), OCTA_V)                                  # originals first


def test_subdivide_a_lone_triangle():
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    nv, nf = mesh.subdivide(v, torch.tensor([[0, 1, 2]]))
    assert tuple(nv.shape) == (6, 3) and tuple(nf.shape) == (4, 3)
    # midpoints in ascending (min, max) order: (0,1), (0,2), (1,2)
    assert torch.equal(nv[3:], torch.tensor([[0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0]]))
    assert nf.tolist() == [[0, 3, 4], [3, 1, 5], [4, 5, 2], [3, 5, 4]]
    assert abs(_area(nv.numpy(), nf.numpy()) - 0.5) <= 1e-6


def test_subdivision_levels_is_the_reference_ladder():
    assert [mesh.subdivision_levels(s) for s in (4, 64, 128, 256, 512, 1024)] == [0, 0, 0, 1, 3, 3]


def test_read_obj_after_write_obj(tmp_path):
    v, f, n, _ = MR.two_spheres("coarse")
    for normals in (None, n):
        path = gen_images.write_obj(str(tmp_path / "m.obj"), v, f, normals)
        rv, rf = mesh.read_obj(path)
        assert rv.dtype == torch.float32 and rf.dtype == torch.int64
        assert np.array_equal(rf.numpy(), f)
        assert np.abs(rv.numpy() - v).max() <= 1e-6


def test_camera_rows_broadcasts():
    c = mesh.camera_rows([0.1, 0.2], 0.3, fov_deg=torch.tensor([12.0, 14.0]))
    assert tuple(c.shape) == (2, 5) and c.dtype == torch.float32
    assert torch.allclose(c, torch.tensor([[0.1, 0.3, 12.0, 1.0, 0.01], [0.2, 0.3, 14.0, 1.0, 0.01]]))
    with pytest.raises(ValueError):
        mesh.camera_rows([0.1, 0.2], [0.1, 0.2, 0.3])


def test_noise_injection_stores_the_project_flag():
    from cips_3dplusplus_amd.decoder import NoiseInjection
    assert NoiseInjection(project=True).project is True and NoiseInjection().project is False


@pytest.mark.parametrize("kind,S", [("coarse", 32), ("coarse", 64), ("subpixel", 32)])
def test_yardstick_excludes_little_and_fp32_agrees(kind, S):
    """The excluded share stays under 1 %, and the fp32 run of the same code picks the fp64 run's face on EVERY pixel, inside
    the excluded set or not: the exclusion band is wider than fp32's uncertainty on these cases."""
    v, f = MR.two_spheres(kind)[:2]
    assert (len(v), len(f)) == {"coarse": (158, 308), "subpixel": (2720, 5432)}[kind]
    for view in range(len(MR.VIEWS)):
        r64, r32 = MR.case(kind, view, S, "float64"), MR.case(kind, view, S, "float32")
        share = MR.excluded(r64).mean()
        print(f"{kind} S={S} view {view}: excluded {100 * share:.2f} %, covered {100 * r64['hit'].mean():.1f} %")
        assert share <= 0.01
        assert r64["hit"].mean() > 0.2
        assert np.array_equal(r32["face"], r64["face"])
        assert len(np.unique(r64["face"][r64["face"] >= len(f) - {"coarse": 56, "subpixel": 1064}[kind]])) > 3   # the small sphere shows
