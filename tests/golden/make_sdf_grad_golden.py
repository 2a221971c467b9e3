"""Golden vectors of the reference's eikonal term (CPU, this container only): writes tests/golden/sdf_grad.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sdf_grad_golden.py

The reference's VolumeFeatureRenderer (hidden 256, D = 2 and D = 6) is loaded with the formula-generated weights of
weights.synth_state_dict (tests/_sdf_grad_cases.py: the fixture stores none) and called as
forward(pts, rays_d, viewdirs, z_vals, near, far, styles, return_eikonal=True) on B = 2 views with distinct styles and
near / far, R = 37 rays, N = 5 samples.  Records (data only, no reference source), per depth tag d2 / d6:
  <tag>.pts / rays_d / viewdirs / z / near / far / styles     the inputs
  <tag>.sdf / <tag>.eikonal_term                              its outputs (B, R, N, 1) / (B, R, N, 3)
  <tag>.eikonal_loss / <tag>.minimal_surface_loss             exp/stylesdf/losses.py:13-24 on them, beta = 100
  <tag>.eikonal_loss_nosdf                                    the same call with sdf=None (first value)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]
from _ref_import import import_reference  # noqa: E402

import_reference()
from exp.cips3d import volume_renderer as ref_vr  # noqa: E402
from exp.stylesdf import losses as ref_losses  # noqa: E402

sys.path.append(os.path.dirname(os.path.dirname(HERE)))
sys.path.append(os.path.dirname(HERE))
import _sdf_grad_cases as SG  # noqa: E402

B, R, N = 2, 37, 5


def main():
    out = {"_src": "cips3d/volume_renderer.py:192-303 (return_eikonal=True); cips3d/nerf_utils.py:221-228; stylesdf/losses.py:13-24"}
    for D in (2, 6):
        tag = f"d{D}"
        ren = ref_vr.VolumeFeatureRenderer(N_layers_renderer=D, input_dim=3, hidden_dim=SG.H, style_dim=SG.H, view_dim=3,
                                           with_sdf=True, output_features=True)
        sd = SG.synth_renderer_sd(D)
        missing = ren.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()}, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        inp = SG.explicit_inputs(B, R, N, D, tag="sgfix")
        ret = ren(inp["pts"].clone(), inp["rays_d"], inp["viewdirs"], inp["z"], inp["near"], inp["far"], styles=inp["styles"],
                  return_eikonal=True)
        sdf, eik = ret[2].detach(), ret[5].detach()
        assert eik.shape == (B, R, N, 3) and sdf.shape == (B, R, N, 1)
        le, lm = ref_losses.eikonal_loss(eik, sdf=sdf, beta=100)
        le0, lm0 = ref_losses.eikonal_loss(eik, sdf=None, beta=100)
        assert float(lm0) == 0.0
        out.update({f"{tag}.{k}": v for k, v in inp.items()})
        out.update({f"{tag}.sdf": sdf, f"{tag}.eikonal_term": eik, f"{tag}.eikonal_loss": le.detach(),
                    f"{tag}.minimal_surface_loss": lm.detach(), f"{tag}.eikonal_loss_nosdf": le0.detach()})
        print(tag, "max |eikonal_term|", float(eik.abs().max()), "losses", float(le), float(lm))
    path = os.path.join(HERE, "sdf_grad.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else np.array(v)) for k, v in out.items()})
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
