"""Closed-surface export: the renderer's SDF volume -> frustum alignment -> marching cubes, on the GPU.

Follows exp/cips3d/utils.py:183-224 (`align_volume`, `extract_mesh_with_marching_cubes`) and the surface extraction of
exp/stylesdf/scripts/generate_shapes_and_images.py:116-163,226-235 (a renderer-only pass at 128^2 rays x 128 samples,
perturbation off).  Both steps run as HIP kernels (csrc/mesh.hip); the reference hands the second to skimage's
`marching_cubes` (Lewiner) and wraps the result in a `trimesh.Trimesh`.  Here the result is `(verts [V,3] fp32,
faces [F,3] int64)` on the device.

Marching cubes differs from skimage's Lewiner variant in how ambiguous cells are resolved: here every cube face whose
corners form a checkerboard separates its inside corners (tools/gen_mc_table.py), and no interior points are added.  The
vertex set -- one point on every lattice edge whose ends change sign, linearly interpolated -- is the one both methods
interpolate; the triangles of ambiguous cells can differ.
"""
import torch

from . import hip

FRAME_SCALE = 0.24          # utils.py:215-221: X = (x / w - 0.5) * 0.24, Y = -(y / h - 0.5) * 0.24, Z = -(z / d - 0.5) * 0.24


def reference_affine(h, w, d):
    """Per-axis (scale, offset) of the reference's output frame for index-space positions (x <-> w, y <-> h, z <-> d)."""
    s = FRAME_SCALE
    return ((s / w, -0.5 * s), (-s / h, 0.5 * s), (-s / d, 0.5 * s))


def _as_4d(volume):
    if volume.dim() == 5:
        if volume.shape[-1] != 1:
            raise ValueError("volume must be (B, h, w, d) or (B, h, w, d, 1)")
        return volume[..., 0]
    if volume.dim() != 4:
        raise ValueError("volume must be (B, h, w, d) or (B, h, w, d, 1)")
    return volume


def align_volume(volume, near=0.88, far=1.12):
    """utils.py:183-203: resample a renderer SDF volume (B, h, w, d[, 1]) into the frustum-aligned grid; same shape out."""
    v = _as_4d(volume).float().contiguous()
    out = hip.align_volume(v, near, far)
    return out.view(volume.shape)


def extract_mesh_with_marching_cubes(sdf, level=0.0, normals=False):
    """utils.py:206-224 on the aligned volume's first sample: (verts [V,3] fp32, faces [F,3] int64) in the reference's
    output frame, or None when the volume has no crossing (the reference's caller gets None from its ValueError).
    normals=True: (verts, faces, normals [V,3] fp32) -- unit vertex normals in the same frame, the volume's lattice gradient
    interpolated along each vertex's edge (skimage's grid normals, which the reference drops); they point towards larger
    values, the side the triangles' winding faces (the reference frame mirrors two axes: positive determinant)."""
    v = _as_4d(sdf)[0].float().contiguous()
    h, w, d = v.shape
    out = hip.marching_cubes(v, level, affine=reference_affine(h, w, d), normals=normals)
    if out[1].shape[0] == 0:
        return None
    return out


@torch.no_grad()
def surface_mesh(G, zs=None, style_render=None, truncation=1, resolution=128, N_samples=None, locations=None, fov_ang=6,
                 dist_radius=0.12, near=0.88, far=1.12, level=0.0, normals=False):
    """The reference's surface extraction on the renderer only (the decoder is not run): mapping network ->
    `G.renderer.render(..., return_sdf=True)` at resolution^2 rays x N_samples (default: resolution) with perturbation off
    -> align_volume -> marching cubes per view.

    zs: a list whose first entry is the renderer's z (B, z_dim), or that tensor; ignored when `style_render` (B, D+1, S) is
    given; both None: one random z.  locations: (B, 2) azimuth / elevation, default the frontal view.
    Returns {"sdf": (B, S, S, N, 1), "aligned": the same shape, "meshes": [(verts, faces) or None per view]}; with
    normals=True each mesh is (verts, faces, normals).

    Runs on the caller's stream through the renderer's lane-0 tables: do not issue it from inside a `ViewPipeline` lane
    (pipeline.py) while that pipeline has views in flight."""
    from .camera import Camera
    dev = next(G.parameters()).device
    if style_render is None:
        if zs is None:
            zs = [torch.randn(1, G.z_dim, device=dev)]
        z = zs[0] if isinstance(zs, (list, tuple)) else zs
        mean_r = None
        if truncation < 1:
            if not hasattr(G, "style_render_mean"):
                G.style_render_mean, G.style_decoder_mean = G.get_mean_latent(10000, dev)
            mean_r = G.style_render_mean
        style_render, _ = G.mapping_renderer([z.to(dev)], truncation, mean_r)
    B = style_render.shape[0]
    if locations is None:
        locations = torch.zeros(B, 2, device=dev)
    N = int(N_samples) if N_samples is not None else int(resolution)
    cam, focal, near_c, far_c, _ = Camera.generate_camera_params(resolution, dev, batch=B, locations=locations.to(dev),
                                                                 fov_ang=fov_ang, dist_radius=dist_radius)
    _, _, sdf, _, _ = G.renderer.render(cam, focal, near_c, far_c, style_render, resolution, N, perturb_u=None,
                                        return_sdf=True)
    aligned = align_volume(sdf, near, far)
    meshes = [extract_mesh_with_marching_cubes(aligned[b:b + 1], level, normals=normals) for b in range(B)]
    return {"sdf": sdf, "aligned": aligned, "meshes": meshes}
