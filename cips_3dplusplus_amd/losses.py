"""Diagnostics on the SDF gradient field: the eikonal and minimal-surface terms (exp/stylesdf/losses.py:13-24).

Plain torch ops on whatever device the tensors live on (CPU included): these are two reductions over tensors the gradient
kernel has already written (`VolumeFeatureRenderer.sdf_gradient`, `ret_maps["eikonal_term"]`), not a hot path.
"""
import torch


def eikonal_loss(eikonal_term, sdf=None, beta=100):
    """-> (eikonal, minimal_surface): ((|g| - 1)^2).mean() over the gradient field g = eikonal_term (.., 3), which is 0 for a
    distance field, and exp(-beta |sdf|).mean(), which penalises values near the zero level away from the surface.
    eikonal_term None gives 0 for the first, sdf None a zero tensor for the second, as in the reference."""
    eikonal = 0 if eikonal_term is None else ((eikonal_term.norm(dim=-1) - 1) ** 2).mean()
    if sdf is None:
        minimal_surface = torch.tensor(0.0, device=eikonal_term.device)
    else:
        minimal_surface = torch.exp(-beta * torch.abs(sdf)).mean()
    return eikonal, minimal_surface
