"""Surface normals without a GPU: the new entry points are exported under the bumped ABI version, the OBJ writer's `vn` form,
and the wrapper's refusal of a shade request it cannot serve."""
import os
import re

import numpy as np
import pytest
import torch

from cips_3dplusplus_amd import _lib, gen_images, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_normals_entry_points():
    lib = _lib.load()
    for name in ("cips3d_nerf_normals", "cips3d_marching_cubes_normals"):
        assert name in _lib.EXPORTED and getattr(lib, name) is not None, name


def test_abi_version_is_bumped_everywhere():
    lib = _lib.load()
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "cips3d_hip.h")).read())
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION
    assert _lib.ABI_VERSION >= 33


def test_bad_arguments_launch_nothing():
    """CIPS3D_E_BADARG is decided on the host before any GPU call: null required pointers, N < 1, no output, a shade output
    without xyz / eye / light."""
    import ctypes as C
    lib = _lib.load()
    p = _lib.NormalsParams()
    assert lib.cips3d_nerf_normals(None, None) == -1
    assert lib.cips3d_nerf_normals(C.byref(p), None) == -1                       # everything null
    p.sdf = p.grad = p.sigmoid_beta = p.x_z_vals = p.x_rays_d = p.normal = 64    # (never dereferenced on the host)
    p.B, p.n_rays, p.n_samples = 1, 4, 0
    assert lib.cips3d_nerf_normals(C.byref(p), None) == -1                       # N < 1
    p.n_samples, p.normal = 3, None
    assert lib.cips3d_nerf_normals(C.byref(p), None) == -1                       # no output
    p.shade = 64
    assert lib.cips3d_nerf_normals(C.byref(p), None) == -1                       # shade without xyz / eye / light
    p.xyz = p.eye = 64
    assert lib.cips3d_nerf_normals(C.byref(p), None) == -1                       # ... still no light
    assert lib.cips3d_marching_cubes_normals(None, 4, 4, 4, 0.0, None, None, None, 0, None) == -1


def test_write_obj_with_and_without_normals(tmp_path):
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int64)
    normals = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0, 0.8]], np.float32)
    plain = gen_images.write_obj(str(tmp_path / "a.obj"), verts, faces)
    # today's bytes
    assert open(plain).read() == "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1.5\nf 1 2 3\nf 1 3 4\n"
    assert open(gen_images.write_obj(str(tmp_path / "b.obj"), verts, faces, None)).read() == open(plain).read()
    lines = open(gen_images.write_obj(str(tmp_path / "c.obj"), verts, faces, normals=normals)).read().splitlines()
    v = [ln for ln in lines if ln.startswith("v ")]
    vn = [ln for ln in lines if ln.startswith("vn ")]
    f = [ln for ln in lines if ln.startswith("f ")]
    assert len(v) == len(vn) == 4 and v == open(plain).read().splitlines()[:4]
    assert vn[3] == "vn 0.6 0 0.8" and f == ["f 1//1 2//2 3//3", "f 1//1 3//3 4//4"]
    with pytest.raises(ValueError):
        gen_images.write_obj(str(tmp_path / "d.obj"), verts, faces, normals=normals[:3])


def test_wrapper_refuses_a_shade_request_without_xyz():
    sdf, grad, beta = torch.zeros(1, 4, 3), torch.zeros(1, 4, 3, 3), torch.ones(1)
    geom = dict(x_z_vals=torch.zeros(1, 4, 3), x_rays_d=torch.zeros(1, 4, 3), n_rays=4)
    with pytest.raises(RuntimeError, match="xyz"):
        hip.nerf_normals(sdf=sdf, grad=grad, sigmoid_beta=beta, B=1, n_samples=3, want=("normal", "shade"), **geom)
    with pytest.raises(RuntimeError, match="xyz"):
        hip.nerf_normals(sdf=sdf, grad=grad, sigmoid_beta=beta, B=1, n_samples=3, want=("shade_u8",), eye=torch.zeros(1, 3),
                         light=torch.zeros(1, 3), **geom)
    with pytest.raises(RuntimeError, match="want"):
        hip.nerf_normals(sdf=sdf, grad=grad, sigmoid_beta=beta, B=1, n_samples=3, want=(), **geom)
