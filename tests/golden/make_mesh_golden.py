"""Golden vectors of the reference's mesh utilities (CPU, this container only): writes tests/golden/mesh_align.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mesh_golden.py

Records (data only, no reference source):
  align.{a,b}.in / .out / near / far   align_volume (exp/cips3d/utils.py:183-203) on non-cubic volumes.  The reference
                                       builds a batch-1 sampling grid, so a batch of 2 is aligned one sample at a time.
  mc.in / mc.sdf_vol                   extract_mesh_with_marching_cubes (utils.py:206-224): its input and the array it
                                       hands to skimage's marching_cubes
  mc.verts_index / mc.verts_out        the fixed index-space vertices a recorder returned in place of marching_cubes, and
                                       the vertices the reference passed on to trimesh.Trimesh
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

torch.set_grad_enabled(False)


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
