"""Golden vectors of the reference's mesh utilities (CPU, this container only): writes tests/golden/mesh_align.npz and
tests/golden/mesh_align_sizes.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mesh_golden.py

Records (data only, no reference source):
  align.{a,b}.in / .out / near / far   align_volume (exp/cips3d/utils.py:183-203) on non-cubic volumes.  The reference
                                       builds a batch-1 sampling grid, so a batch of 2 is aligned one sample at a time.
  mc.in / mc.sdf_vol                   extract_mesh_with_marching_cubes (utils.py:206-224): its input and the array it
                                       hands to skimage's marching_cubes
  mc.verts_index / mc.verts_out        the fixed index-space vertices a recorder returned in place of marching_cubes, and
                                       the vertices the reference passed on to trimesh.Trimesh

mesh_align_sizes.npz: align_volume at the production size and at degenerate sizes.  The inputs are closed-form
(weights.det_normal(name, shape, 1.0, seed)), so only their recipe is stored:
  cases                                the tags, in order
  <tag>.name / shape / seed / near / far
  large cases (LARGE):  <tag>.mask     np.packbits(out == 1): the out-of-frustum mask, whole volume
                        <tag>.stride / <tag>.vals            out.reshape(-1)[::stride]
                        <tag>.plane_stride / <tag>.plane.<p> the border planes i0, i1, j0, j1, k0, k1 (first / last index of
                                                             h, w, d), each .reshape(-1)[::plane_stride]
  small cases (SMALL):  <tag>.out      the whole output (a batch is aligned one sample at a time, as case "b" above)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]
from _ref_import import import_reference  # noqa: E402

import_reference()
from exp.cips3d import utils as ref_utils  # noqa: E402

sys.path.append(os.path.dirname(os.path.dirname(HERE)))
from cips_3dplusplus_amd import weights  # noqa: E402

torch.set_grad_enabled(False)

# tag: (shape, near, far, seed[, stride, plane_stride]); the strides are primes, so the samples walk through all three axes
LARGE = {
    "p128": ((1, 128, 128, 128, 1), 0.88, 1.12, 11, 31, 5),
    "nc": ((1, 96, 129, 64, 1), 0.8, 1.2, 12, 17, 5),
}
SMALL = {
    "h1": ((1, 1, 5, 4, 1), 0.9, 1.1, 21),
    "w1": ((1, 6, 1, 4, 1), 0.9, 1.1, 22),
    "d1": ((1, 6, 5, 1, 1), 0.9, 1.1, 23),
    "two": ((1, 2, 2, 2, 1), 0.88, 1.12, 24),
    "flat": ((1, 7, 6, 5, 1), 1.0, 1.0, 25),           # near = far: nothing outside the frustum
    "inv": ((1, 5, 7, 6, 1), 1.12, 0.88, 26),          # far < near: nothing outside the frustum
    "b3": ((3, 7, 9, 6, 1), 0.8, 1.2, 27),
}


def planes(vol):
    """The six border planes of vol [h, w, d], by name."""
    return {"i0": vol[0], "i1": vol[-1], "j0": vol[:, 0], "j1": vol[:, -1], "k0": vol[:, :, 0], "k1": vol[:, :, -1]}


def sizes():
    out = {"_src": np.array("exp/cips3d/utils.py:183-203"), "cases": np.array(list(LARGE) + list(SMALL))}
    for tag, case in {**LARGE, **SMALL}.items():
        shape, near, far, seed = case[:4]
        name = "mesh_align_sizes." + tag
        vol = weights.det_normal(name, shape, 1.0, seed)
        aligned = torch.cat([ref_utils.align_volume(vol[b:b + 1], near=near, far=far) for b in range(shape[0])], 0).numpy()
        assert np.isfinite(aligned).all()
        out[f"{tag}.name"] = np.array(name)
        out[f"{tag}.shape"] = np.array(shape, np.int64)
        out[f"{tag}.seed"] = np.int64(seed)
        out[f"{tag}.near"] = np.float64(near)
        out[f"{tag}.far"] = np.float64(far)
        if tag in SMALL:
            out[f"{tag}.out"] = aligned
            continue
        stride, plane_stride = case[4:]
        out[f"{tag}.mask"] = np.packbits(aligned == 1.0)
        out[f"{tag}.stride"] = np.int64(stride)
        out[f"{tag}.vals"] = aligned.reshape(-1)[::stride].copy()
        out[f"{tag}.plane_stride"] = np.int64(plane_stride)
        for p, a in planes(aligned[0, ..., 0]).items():
            out[f"{tag}.plane.{p}"] = a.reshape(-1)[::plane_stride].copy()
    path = os.path.join(HERE, "mesh_align_sizes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def main():
    g = torch.Generator().manual_seed(1234)
    out = {"_src": np.array("exp/cips3d/utils.py:183-224")}
    cases = {"a": ((1, 20, 24, 16, 1), 0.88, 1.12), "b": ((2, 12, 12, 10, 1), 0.8, 1.2)}
    for tag, (shape, near, far) in cases.items():
        vol = torch.randn(shape, generator=g)
        aligned = torch.cat([ref_utils.align_volume(vol[b:b + 1], near=near, far=far) for b in range(shape[0])], 0)
        out[f"align.{tag}.in"] = vol.numpy()
        out[f"align.{tag}.out"] = aligned.numpy()
        out[f"align.{tag}.near"] = np.float64(near)
        out[f"align.{tag}.far"] = np.float64(far)

    rec = {}
    verts_index = (torch.rand(64, 3, generator=g) * torch.tensor([24.0, 20.0, 16.0])).numpy().astype(np.float32)

    def marching_cubes(vol, level):
        rec["sdf_vol"] = np.array(vol)
        rec["level"] = level
        return verts_index.copy(), np.zeros((0, 3), np.int64), None, None

    class Trimesh:
        def __init__(self, verts, faces):
            rec["verts_out"] = np.array(verts)

    ref_utils.marching_cubes = marching_cubes
    ref_utils.trimesh = type("trimesh", (), {"Trimesh": Trimesh})
    sdf = torch.randn(1, 20, 24, 16, 1, generator=g)
    ref_utils.extract_mesh_with_marching_cubes(sdf)
    out["mc.in"] = sdf.numpy()
    out["mc.sdf_vol"] = rec["sdf_vol"]
    out["mc.level"] = np.float64(rec["level"])
    out["mc.verts_index"] = verts_index
    out["mc.verts_out"] = rec["verts_out"]
    path = os.path.join(HERE, "mesh_align.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
    sizes()
