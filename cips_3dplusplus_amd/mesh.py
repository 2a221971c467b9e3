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

The second half rasterises that mesh (csrc/mesh_raster.hip; the reference uses pytorch3d): `rasterize_mesh`, the Phong
`render_mesh_frames` of exp/cips3d/utils.py:260-308, and `NoiseProjector`, the surface-bound decoder noise of
models/model_v3.py:344-415 (`NoiseInjection.project_noise`), with the midpoint `subdivide` its mesh ladder needs.

The third colours the mesh (csrc/mesh_color.hip; an extension, the reference exports a grey surface): `vertex_colors` gathers
pictures of the mesh onto its vertices through the rasteriser's own visibility, `color_mesh` takes those pictures from the
generator, and `render_mesh_frames(colors=)` draws the result.

The fourth gives it a texture (csrc/mesh_texture.hip): `texture_atlas` lays two faces into every cell of an arithmetic atlas,
`fill_colors` grows the vertex colours into the vertices no view saw, `bake_texture` applies `vertex_colors`' rule to every
texel, `texture_mesh` does all of it from the generator's pictures, and `render_textured_frames` draws the result.
"""
import math

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
                 dist_radius=0.12, near=0.88, far=1.12, level=0.0, normals=False, colors=False, color_kw=None, texture=False,
                 texture_kw=None):
    """The reference's surface extraction on the renderer only (the decoder is not run): mapping network ->
    `G.renderer.render(..., return_sdf=True)` at resolution^2 rays x N_samples (default: resolution) with perturbation off
    -> align_volume -> marching cubes per view.

    zs: a list whose first entry is the renderer's z (B, z_dim), or that tensor; ignored when `style_render` (B, D+1, S) is
    given; both None: one random z.  locations: (B, 2) azimuth / elevation, default the frontal view.
    Returns {"sdf": (B, S, S, N, 1), "aligned": the same shape, "meshes": [(verts, faces) or None per view]}; with
    normals=True each mesh is (verts, faces, normals).
    colors=True (needs normals=True and a decoder latent: zs = [z_renderer, z_decoder]): every mesh is coloured by
    `color_mesh(G, ..., **color_kw)` from its own sample's latents and becomes (verts, faces, normals, colors); the dict gains
    "color_weight" and "color_seen", one entry per view (None where there is no mesh).
    texture=True (the same needs): every mesh gets a texture atlas by `texture_mesh(G, ..., **color_kw, **texture_kw)`; the dict
    gains "textures", one `texture_mesh` dict per view (None where there is no mesh).  With colors=True as well the pictures are
    rendered once, and the colours are the ones colors=True alone gives.

    Runs on the caller's stream through the renderer's lane-0 tables: do not issue it from inside a `ViewPipeline` lane
    (pipeline.py) while that pipeline has views in flight."""
    from .camera import Camera
    dev = next(G.parameters()).device
    if colors or texture:
        what = "colors=True" if colors else "texture=True"
        if not normals:
            raise ValueError(f"surface_mesh({what}) needs normals=True: the colours are weighted by the vertex normals")
        if style_render is not None or not isinstance(zs, (list, tuple)) or len(zs) < 2:
            raise ValueError(f"surface_mesh({what}) needs the decoder's latent too: zs = [z_renderer, z_decoder]")
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
    out = {"sdf": sdf, "aligned": aligned, "meshes": meshes}
    if colors or texture:
        kw = dict(fov_ang=fov_ang, dist_radius=dist_radius, truncation=truncation)
        kw.update(color_kw or {})
        if colors:
            out["color_weight"], out["color_seen"] = [None] * B, [None] * B
        if texture:
            kw.update(texture_kw or {})
            out["textures"] = [None] * B
        for b, m in enumerate(meshes):
            if m is None:
                continue
            zb = [z[b:b + 1].to(dev) for z in zs[:2]]
            if texture:
                t = out["textures"][b] = texture_mesh(G, m[0], m[1], m[2], zs=zb, **kw)
                c = {"colors": t["seen_colors"], "weight": t["color_weight"], "seen": t["color_seen"]}
            else:
                c = color_mesh(G, m[0], m[1], m[2], zs=zb, **kw)
            if colors:
                meshes[b] = (m[0], m[1], m[2], c["colors"])
                out["color_weight"][b], out["color_seen"][b] = c["weight"], c["seen"]
    return out


# ------------------------------------------------------------------------------------------------ rasterisation
def camera_rows(azim, elev, fov_deg=12.0, dist=1.0, znear=0.01, device=None):
    """cams [n,5] fp32 = (azim, elev, fov_deg, dist, znear) per view, the rasteriser's camera input (the reference's
    create_cameras arguments; angles in radians).  Every argument is a number, a sequence or a tensor of n values; device
    tensors stay on the device (no synchronisation)."""
    cols = [torch.as_tensor(c, dtype=torch.float32, device=device).reshape(-1) for c in (azim, elev, fov_deg, dist, znear)]
    n = max(c.numel() for c in cols)
    if any(c.numel() not in (1, n) for c in cols):
        raise ValueError("camera_rows: every argument must hold one value or one per view")
    return torch.stack([c.expand(n) for c in cols], 1).contiguous()


def _faces_i32(faces):
    if faces.numel() and int(faces.shape[0]) > 2 ** 31 - 1:
        raise ValueError("more than 2^31 - 1 faces")
    return faces.to(torch.int32).contiguous()


def rasterize_mesh(verts, faces, azim, elev, image_size, fov_deg=12.0, dist=1.0, znear=0.01, attrs=None, base=None, fill=0.0,
                   normals=None, light=None, want=None, ws=None, keys=None, out=None):
    """Hard z-buffer rasterisation of (verts [V,3] fp32, faces [F,3] int32 / int64) from the cameras (azim, elev) [radians; one
    value or n], the reference's create_cameras(azim, elev, dist, fov, znear) -> dict:
      face [n,S,S] int32, zbuf [n,S,S] fp32 (view-space depth), bary [n,S,S,3] fp32 (perspective-correct): -1 where empty;
      attrs [V,C] given: attr [n,C,S,S], the interpolated vertex attributes; empty pixels take `base` [n,C,S,S] or `fill`;
      normals [V,3] and light [n,3] given: shade [n,S,S] fp32 and shade_u8 [n,3,S,S], the Phong frame on a white background.
    `want` restricts the outputs; ws / keys: buffers of hip.mesh_raster_workspace to reuse; out: tensors to write into.
    Contract: include/cips3d_hip.h (cips3d_mesh_rasterize)."""
    verts = verts.float().contiguous()
    f32 = _faces_i32(faces)
    cams = camera_rows(azim, elev, fov_deg, dist, znear, device=verts.device)
    if want is None:
        want = ["face", "zbuf", "bary"] + (["attr"] if attrs is not None else []) + \
               (["shade", "shade_u8"] if normals is not None and light is not None else [])
    ws, keys = hip.mesh_rasterize(verts, f32, cams, image_size, ws=ws, keys=keys)
    return hip.mesh_resolve(verts, f32, ws, keys, want=want, attr=None if attrs is None else attrs.float().contiguous(), base=base,
                           fill=fill, normals=None if normals is None else normals.float().contiguous(),
                           light=None if light is None else light.float().contiguous(), out=out)


def render_mesh_frames(verts, faces, normals, trajectory, image_size=512, light=None, colors=None):
    """The reference's mesh panel (create_cameras / create_mesh_renderer, utils.py:260-308, as the frame loops call it): the
    Phong picture of the mesh from every row (azim, elev, fov / 2) of `trajectory`, camera fov = 2 trajectory[:,2] degrees at
    distance 1, point light (5 sin az, 0, 5 cos az) unless `light` [n,3] is given -> uint8 [n,3,S,S], white where empty.
    The rasteriser is hard (one face per pixel); pytorch3d's soft blending is not reproduced.
    colors [V,3] in [-1, 1] (vertex_colors / color_mesh): the same frames with the interpolated vertex colour as albedo,
    floor(255 clamp(shade (colour + 1) / 2, 0, 1) + 0.5); white exactly where the plain panel is white."""
    traj = torch.as_tensor(trajectory, dtype=torch.float32).to(verts.device)
    az, el = traj[:, 0], traj[:, 1]
    if light is None:
        light = torch.stack([5 * torch.sin(az), torch.zeros_like(az), 5 * torch.cos(az)], 1)
    if colors is not None:
        if tuple(colors.shape) != (verts.shape[0], 3):
            raise ValueError("render_mesh_frames: colors must be [V, 3]")
        out = rasterize_mesh(verts, faces, az, el, image_size, fov_deg=2.0 * traj[:, 2], dist=1.0, attrs=colors, normals=normals,
                             light=light.float().contiguous(), want=("face", "shade", "attr"))
        return hip.mesh_albedo_frame(out["face"], out["shade"], out["attr"])
    out = rasterize_mesh(verts, faces, az, el, image_size, fov_deg=2.0 * traj[:, 2], dist=1.0, normals=normals,
                         light=light.float().contiguous(), want=("shade_u8",))
    return out["shade_u8"]


def vertex_colors(verts, faces, normals, images, azim, elev, fov_deg=12.0, dist=1.0, znear=0.01, raster_size=512, depth_tol=None,
                  power=2, fill=0.0, ws=None, keys=None):
    """Colours of the vertices of (verts [V,3], faces [F,3]) from `images` [n,3,R,R], pictures of the mesh taken by the cameras
    (azim, elev) [radians; one value or n] of `rasterize_mesh`: the mesh is rasterised at raster_size^2 from every camera, and
    every vertex takes, from each view whose z-buffer shows it (vertex depth <= the depth of its pixel + depth_tol) and that it
    faces (c = normal . direction to the eye > 0), the bilinear sample of that view's image at its projection, weighted by
    c^power (an integer 1..8).  normals [V,3]: unit, outward (extract_mesh_with_marching_cubes(normals=True)).
    -> {"colors": [V,3] fp32, the weighted mean, `fill` where no view sees the vertex; "weight": [V] fp32, the sum of the
    weights; "seen": [V] int32, the number of views that see the vertex}.
    depth_tol=None: FRAME_SCALE / 128, one cell of the default 128^3 volume in the output frame.  depth_tol, power and
    raster_size are design defaults, not measured optima.  ws / keys: buffers of hip.mesh_raster_workspace to reuse.
    Visibility is quantised to the z-buffer's pixels: a front-facing vertex at a grazing angle can be hidden by
    the nearer surface that owns its pixel centre.  Contract: include/cips3d_hip.h (cips3d_mesh_vertex_colors)."""
    verts = verts.float().contiguous()
    f32 = _faces_i32(faces)
    cams = camera_rows(azim, elev, fov_deg, dist, znear, device=verts.device)
    images = images.float().contiguous()
    if images.dim() != 4 or images.shape[0] != cams.shape[0]:
        raise ValueError(f"vertex_colors: {cams.shape[0]} cameras need images [{cams.shape[0]}, 3, R, R]")
    if depth_tol is None:
        depth_tol = FRAME_SCALE / 128
    if f32.shape[0] == 0 and verts.shape[0]:
        raise ValueError("vertex_colors: a mesh without faces has no surface to colour (the rasteriser projects nothing)")
    ws, keys = hip.mesh_rasterize(verts, f32, cams, raster_size, ws=ws, keys=keys)
    return hip.mesh_vertex_colors(verts, normals.float().contiguous(), images, ws, keys, raster_size, power=power,
                                  depth_tol=depth_tol, fill=fill)


DEFAULT_COLOR_VIEWS = ((0, 0), (0.4, 0), (-0.4, 0))       # (azim, elev): frontal and two side views; a design default


@torch.no_grad()
def color_mesh(G, verts, faces, normals, zs=None, style_render=None, style_decoder=None, truncation=1, views=DEFAULT_COLOR_VIEWS,
               img_size=64, N_samples=24, fov_ang=6, dist_radius=0.12, noise_bufs=None, **vertex_colors_kw):
    """Colours the mesh of a latent with the generator's own pictures of that latent: one full forward (renderer and decoder,
    perturbation off) per (azim, elev) of `views` at img_size^2 rays x N_samples, then `vertex_colors` from the same cameras
    (`view_angles`' correspondence: fov_deg = 2 fov_ang at distance 1) -> its dict.
    zs: [z_renderer, z_decoder], each (1, z_dim); or style_render and style_decoder, both.  noise_bufs: the decoder's noise
    maps, shared by the views; default `G.create_noise_bufs`, drawn from torch's generator on the device, so that a seed
    reproduces the colours.  The default views are a design default, not a measured optimum.  vertex_colors_kw: raster_size,
    depth_tol, power, fill, znear, ws, keys.

    Runs on the caller's stream through the generator's lane-0 plans and tables, like `surface_mesh`: do not issue it from
    inside a `ViewPipeline` lane (pipeline.py) while that pipeline has views in flight."""
    images, locs = _color_views(G, verts.device, zs, style_render, style_decoder, truncation, views, img_size, N_samples, fov_ang,
                                dist_radius, noise_bufs)
    return vertex_colors(verts, faces, normals, images, locs[:, 0], locs[:, 1], fov_deg=2.0 * float(fov_ang), dist=1.0,
                         **vertex_colors_kw)


def _color_views(G, dev, zs, style_render, style_decoder, truncation, views, img_size, N_samples, fov_ang, dist_radius, noise_bufs):
    """The generator's pictures of one latent from `views` (color_mesh's renders) -> (images [n,3,R,R] fp32, locs [n,2])."""
    from .camera import Camera
    if (style_render is None) != (style_decoder is None):
        raise ValueError("color_mesh: give style_render and style_decoder together")
    if style_render is None and (not isinstance(zs, (list, tuple)) or len(zs) < 2):
        raise ValueError("color_mesh needs zs = [z_renderer, z_decoder] or both styles")
    locs = torch.as_tensor(views, dtype=torch.float32).reshape(-1, 2).to(dev)
    if noise_bufs is None:
        noise_bufs = G.create_noise_bufs(img_size, dev)
    images = []
    for k in range(locs.shape[0]):
        cam, focal, near, far, _ = Camera.generate_camera_params(img_size, dev, locations=locs[k:k + 1].contiguous(),
                                                                 fov_ang=fov_ang, dist_radius=dist_radius)
        out = G(zs=zs if style_render is None else [None, None], cam_poses=cam, focals=focal, img_size=img_size, near=near, far=far,
                truncation=truncation, style_render=style_render, style_decoder=style_decoder, noise_bufs=noise_bufs,
                nerf_cfg=dict(N_samples=N_samples, perturb=False))
        images.append(out["rgb"].float())
    return torch.cat(images, 0), locs


# ------------------------------------------------------------------------------------------------ texture atlas
def texture_atlas(n_faces, texels=8, cols=None):
    """The atlas of a mesh of n_faces faces (csrc/mesh_texture.h; pure arithmetic, no unwrap): faces 2c and 2c + 1 share cell c
    of (T + 1) x T texels, T = texels in 3..64; `cols` cells per row (default: the atlas about square) ->
    {"T", "cols", "rows", "width", "height", "n_faces", "uv": [F,3,2] fp32 on the CPU, the faces' corner UVs in continuous
    texel coordinates (the centre of texel k is k + 1/2; gen_images.write_textured_obj turns them into `vt` lines)}.
    Every face owns T (T - 1) / 2 texels and T gutter texels; a bilinear fetch inside a face's UV triangle touches only those.
    Raises RuntimeError when a side would exceed 16384 texels."""
    c, r, w, h = hip.mesh_atlas_layout(n_faces, texels, cols)
    return {"T": int(texels), "cols": c, "rows": r, "width": w, "height": h, "n_faces": int(n_faces),
            "uv": torch.from_numpy(hip.mesh_atlas_uv(n_faces, texels, c))}


def atlas_texels(atlas):
    """Per texel of `atlas` (texture_atlas), on the CPU: {"face": [Ht,Wt] int32, -1 where no face owns the texel; "bary":
    [Ht,Wt,3] fp32, the texel's barycentrics in its face; "gutter": [Ht,Wt] bool} -- the bake kernel's own decisions."""
    face, bary, gutter = hip.mesh_atlas_texels(atlas["n_faces"], atlas["T"], atlas["cols"], atlas["rows"])
    return {"face": torch.from_numpy(face), "bary": torch.from_numpy(bary), "gutter": torch.from_numpy(gutter)}


def fill_colors(colors, weight, faces, iters=64):
    """Grows the colours of the vertices some view saw (weight > 0: vertex_colors' outputs) into the others, ring by ring over
    the faces' edges: a vertex unfilled at the start of ring r takes the mean of the corners, filled before ring r, of the faces
    it belongs to (one term per (face, corner) pair) -> {"colors": [V,3] fp32, "filled": [V] int32: 0 seen, r filled in ring r,
    -1 never reached (it keeps its input colour)}.  iters in 0..4096, a design default; the sums are integers (2^-20 steps), so
    the result is exact and bit-reproducible.  Contract: include/cips3d_hip.h (cips3d_mesh_fill_colors)."""
    return hip.mesh_fill_colors(colors.float().contiguous(), weight.float().contiguous(), _faces_i32(faces), iters=iters)


def bake_texture(verts, faces, normals, images, azim, elev, texels=8, cols=None, vertex_colors=None, filled=None, fov_deg=12.0,
                 dist=1.0, znear=0.01, raster_size=512, depth_tol=None, power=2, fill=0.0, ws=None, keys=None, atlas=None):
    """A texture for the mesh from `images` [n,3,R,R], pictures of it taken by the cameras (azim, elev) -- `vertex_colors`'
    inputs and rule, applied to every texel of `texture_atlas(F, texels, cols)` instead of every vertex: the texel's surface
    point and normal come from its barycentrics in its face, the point is projected with the rasteriser's arithmetic, and
    visibility, facing, weight and the bilinear sample follow vertex_colors word for word.
    vertex_colors [V,3] / filled [V] (fill_colors' outputs), both or neither: a texel no view sees takes the barycentric mix
    of its corners' colours when all three are filled, else `fill`.
    -> {"texture": [3,Ht,Wt] fp32 in [-1, 1], "weight": [Ht,Wt] fp32, "seen": [Ht,Wt] int32, "atlas": the atlas dict}.
    Contract: include/cips3d_hip.h (cips3d_mesh_texture_bake)."""
    verts = verts.float().contiguous()
    f32 = _faces_i32(faces)
    cams = camera_rows(azim, elev, fov_deg, dist, znear, device=verts.device)
    images = images.float().contiguous()
    if images.dim() != 4 or images.shape[0] != cams.shape[0]:
        raise ValueError(f"bake_texture: {cams.shape[0]} cameras need images [{cams.shape[0]}, 3, R, R]")
    if depth_tol is None:
        depth_tol = FRAME_SCALE / 128
    if f32.shape[0] == 0:
        raise ValueError("bake_texture: a mesh without faces has no surface to texture")
    if atlas is None:
        atlas = texture_atlas(f32.shape[0], texels, cols)
    elif atlas["n_faces"] != f32.shape[0]:
        raise ValueError(f"bake_texture: the atlas was laid out for {atlas['n_faces']} faces, the mesh has {f32.shape[0]}")
    ws, keys = hip.mesh_rasterize(verts, f32, cams, raster_size, ws=ws, keys=keys)
    out = hip.mesh_texture_bake(verts, f32, normals.float().contiguous(), images, ws, keys, raster_size, atlas["T"], atlas["cols"],
                                atlas["rows"], power=power, depth_tol=depth_tol, fill=fill,
                                vertex_colors=None if vertex_colors is None else vertex_colors.float().contiguous(),
                                filled=None if filled is None else filled.to(torch.int32).contiguous())
    out["atlas"] = atlas
    return out


@torch.no_grad()
def texture_mesh(G, verts, faces, normals, zs=None, style_render=None, style_decoder=None, truncation=1, views=DEFAULT_COLOR_VIEWS,
                 img_size=64, N_samples=24, fov_ang=6, dist_radius=0.12, noise_bufs=None, texels=8, cols=None, fill_iters=64,
                 **vertex_colors_kw):
    """`color_mesh`'s pictures, rendered once, used three times: vertex colours -> `fill_colors` (fill_iters rings) ->
    `bake_texture` with the filled colours behind the texels no view sees.  One rasterisation serves the colours and the bake.
    -> {"texture", "weight", "seen", "atlas" (bake_texture), "colors", "filled" (fill_colors), "seen_colors", "color_weight",
    "color_seen" (vertex_colors' colors, weight, seen), "images"}.  vertex_colors_kw: raster_size, depth_tol, power, fill, znear.  Counts of seen / filled / unfilled
    texels: `texel_counts`.  Runs on the caller's stream, like `color_mesh`."""
    images, locs = _color_views(G, verts.device, zs, style_render, style_decoder, truncation, views, img_size, N_samples, fov_ang,
                                dist_radius, noise_bufs)
    kw = dict(fov_deg=2.0 * float(fov_ang), dist=1.0, **vertex_colors_kw)
    S = kw.get("raster_size", 512)
    verts = verts.float().contiguous()
    ws, keys = hip.mesh_raster_workspace(verts.shape[0], faces.shape[0], locs.shape[0], S, verts.device)
    col = vertex_colors(verts, faces, normals, images, locs[:, 0], locs[:, 1], ws=ws, keys=keys, **kw)
    grown = fill_colors(col["colors"], col["weight"], faces, iters=fill_iters)
    out = bake_texture(verts, faces, normals, images, locs[:, 0], locs[:, 1], texels=texels, cols=cols, vertex_colors=grown["colors"],
                       filled=grown["filled"], ws=ws, keys=keys, **kw)
    out.update(colors=grown["colors"], filled=grown["filled"], seen_colors=col["colors"], color_weight=col["weight"],
               color_seen=col["seen"], images=images)
    return out


def texel_counts(baked, filled, faces):
    """(seen, filled, never) texel counts of a baked atlas (one synchronisation): owned and gutter texels some view sees; those
    none sees whose three corners `fill_colors` reached; those left at the constant fill.  Unowned texels are not counted."""
    tex = atlas_texels(baked["atlas"])
    face = tex["face"].to(baked["seen"].device)
    owned = face >= 0
    seen = owned & (baked["weight"] > 0)
    ok = (filled[faces.long()] >= 0).all(1)[face.clamp_min(0).long()]
    return int(seen.sum()), int((owned & ~seen & ok).sum()), int((owned & ~seen & ~ok).sum())


def texture_to_uint8(texture):
    """[3,Ht,Wt] fp32 in [-1, 1] -> uint8 with the image pipeline's rounding (cips3d_rgb_to_uint8 takes any map size)."""
    return hip.rgb_to_uint8(texture)


def render_textured_frames(verts, faces, normals, trajectory, texture, atlas, image_size=512, light=None):
    """`render_mesh_frames` at texture resolution: the Phong shade of every pixel times the bilinear fetch of `texture`
    [3,Ht,Wt] (bake_texture) at the pixel's point in its face's UV triangle of `atlas` -> uint8 [n,3,S,S], white exactly where
    the plain panel is white.  Contract: include/cips3d_hip.h (cips3d_mesh_textured_frame)."""
    traj = torch.as_tensor(trajectory, dtype=torch.float32).to(verts.device)
    az, el = traj[:, 0], traj[:, 1]
    if light is None:
        light = torch.stack([5 * torch.sin(az), torch.zeros_like(az), 5 * torch.cos(az)], 1)
    if atlas["n_faces"] != faces.shape[0]:
        raise ValueError(f"render_textured_frames: the atlas was laid out for {atlas['n_faces']} faces, the mesh has {faces.shape[0]}")
    out = rasterize_mesh(verts, faces, az, el, image_size, fov_deg=2.0 * traj[:, 2], dist=1.0, normals=normals,
                         light=light.float().contiguous(), want=("face", "bary", "shade"))
    return hip.mesh_textured_frame(out["face"], out["bary"], out["shade"], texture.float().contiguous(), atlas["n_faces"], atlas["T"],
                                   atlas["cols"], atlas["rows"])


def subdivide(verts, faces):
    """Midpoint subdivision (trimesh.remesh.subdivide's result up to vertex order), torch ops only, any device: the
    original vertices first, then one midpoint per undirected edge in ascending (min, max) order; face k = (a, b, c) becomes
    faces 4k .. 4k+3 = (a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca).  -> (verts [V + E, 3], faces [4F, 3] int64)."""
    faces = faces.long()
    V, F = verts.shape[0], faces.shape[0]
    ends = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 0)              # ab | bc | ca
    lo, hi = ends.min(1).values, ends.max(1).values
    uniq, inv = torch.unique(lo * V + hi, sorted=True, return_inverse=True)                   # one sorted 64-bit key per edge
    mid = (verts[uniq // V] + verts[uniq % V]) * 0.5
    ab, bc, ca = (V + inv).view(3, F)
    a, b, c = faces.unbind(1)
    new = torch.stack([torch.stack(t, 1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))], 1)
    return torch.cat([verts, mid], 0), new.reshape(4 * F, 3)


def subdivision_levels(im_res):
    """Subdivision steps of the reference's mesh ladder for a noise map of im_res^2 (model_v3.py:360-385): <= 128: 0, 256: 1,
    above: 3.  The reference tests `im_res == 256` a second time where 512 was meant, so 512 and 1024 both fall through to
    three steps; kept as written."""
    if im_res <= 128:
        return 0
    if im_res == 256:
        return 1
    return 3


def read_obj(path, device=None):
    """(verts [V,3] fp32, faces [F,3] int64, zero-based) from the `v` and `f` lines of an OBJ file; `f` entries may carry
    /vt/vn suffixes (gen_images.write_obj writes v//vn), everything else is ignored."""
    vs, fs = [], []
    with open(path) as fh:
        for line in fh:
            if line.startswith("v "):
                vs.append([float(x) for x in line.split()[1:4]])
            elif line.startswith("f "):
                fs.append([int(x.split("/")[0]) - 1 for x in line.split()[1:4]])
    verts = torch.tensor(vs, dtype=torch.float32).reshape(-1, 3)
    faces = torch.tensor(fs, dtype=torch.int64).reshape(-1, 3)
    return verts.to(device), faces.to(device)


def read_ply(path, device=None):
    """The binary little-endian PLY that gen_images.write_ply writes -> {"verts": [V,3] fp32, "faces": [F,3] int64, and, where
    the file holds them, "normals": [V,3] fp32 and "colors": [V,3] uint8}."""
    import numpy as np
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        counts, props, elem = {}, {}, None
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            tok = line.decode("ascii").split()
            if tok[:1] == ["end_header"]:
                break
            if tok[:1] == ["format"] and tok[1] != "binary_little_endian":
                raise ValueError(f"{path}: only binary_little_endian is read")
            if tok[:1] == ["element"]:
                elem = tok[1]
                counts[elem], props[elem] = int(tok[2]), []
            elif tok[:1] == ["property"]:
                props[elem].append(tok[1:])
        kinds = {"float": "<f4", "uchar": "u1"}
        if list(counts) != ["vertex", "face"] or props["face"] != [["list", "uchar", "int", "vertex_indices"]] or \
                any(len(p) != 2 or p[0] not in kinds for p in props["vertex"]):
            raise ValueError(f"{path}: not the layout gen_images.write_ply writes")
        vt = np.dtype([(p[1], kinds[p[0]]) for p in props["vertex"]])
        v = np.frombuffer(fh.read(vt.itemsize * counts["vertex"]), vt)
        ft = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
        f = np.frombuffer(fh.read(ft.itemsize * counts["face"]), ft)
    if len(v) != counts["vertex"] or len(f) != counts["face"] or (f["n"] != 3).any():
        raise ValueError(f"{path}: truncated, or a face that is not a triangle")
    cols = lambda names: torch.from_numpy(np.stack([v[n] for n in names], 1).copy()).to(device)      # noqa: E731
    out = {"verts": cols(("x", "y", "z")), "faces": torch.from_numpy(f["idx"].astype(np.int64)).to(device)}
    if "nx" in vt.names:
        out["normals"] = cols(("nx", "ny", "nz"))
    if "red" in vt.names:
        out["colors"] = cols(("red", "green", "blue"))
    return out


class NoiseProjector:
    """NoiseInjection.project_noise for every noise layer of a decoder (model_v3.py:344-415): the mesh, subdivided
    `subdivision_levels(size)` times for a layer of size^2, carries one N(0,1) value per vertex (`vert_noise[i]` [V_L], drawn
    once); per frame the mesh is rasterised from the frame's camera at every layer size and the covered pixels of the
    layer's screen-space map are replaced by the interpolated vertex noise, so the noise sticks to the surface.
    sizes: the layers' map sizes (noise_bufs[i].shape[-1]); generator: torch generator of the draw; vert_noise: the values
    themselves (tests).  Workspaces are kept per stream: projections on different streams may be in flight together."""

    def __init__(self, verts, faces, sizes, generator=None, vert_noise=None):
        self.sizes = [int(s) for s in sizes]
        verts, faces = verts.float().contiguous(), faces.long()
        self.meshes = {0: (verts, _faces_i32(faces))}
        v, f = verts, faces
        for lvl in range(1, max(subdivision_levels(s) for s in self.sizes) + 1 if self.sizes else 1):
            v, f = subdivide(v, f)
            self.meshes[lvl] = (v.contiguous(), _faces_i32(f))
        self.levels = [subdivision_levels(s) for s in self.sizes]
        if vert_noise is None:
            vert_noise = [torch.randn(self.meshes[l][0].shape[0], generator=generator,
                                      device=verts.device if generator is None else generator.device).to(verts.device)
                          for l in self.levels]
        self.vert_noise = [t.float().reshape(-1, 1).contiguous() for t in vert_noise]
        for t, l in zip(self.vert_noise, self.levels):
            if t.shape[0] != self.meshes[l][0].shape[0]:
                raise ValueError(f"vert_noise holds {t.shape[0]} values for a mesh of {self.meshes[l][0].shape[0]} vertices")
        self._ws = {}
        self._absmax = None

    def absmax(self):
        """max |vert_noise| over all layers (one synchronisation, once): interpolation is convex, so no projected value
        exceeds it."""
        if self._absmax is None:
            self._absmax = max([float(t.abs().max()) for t in self.vert_noise if t.numel()] or [0.0])
        return self._absmax

    def project(self, noise_bufs, azim, elev, fov_deg=12.0, out=None):
        """One projected map per layer: noise_bufs[i] [1,1,s,s] with its covered pixels replaced; every other pixel is the
        caller's value bit for bit.  azim / elev: numbers or one-element tensors (device tensors: no synchronisation).  The
        reference fixes fov = 12 degrees here whatever the trajectory's fov is; batch 1, as there."""
        if len(noise_bufs) != len(self.sizes):
            raise ValueError(f"expected {len(self.sizes)} noise buffers, got {len(noise_bufs)}")
        dev = self.meshes[0][0].device
        cams = camera_rows(azim, elev, fov_deg, 1.0, 0.01, device=dev)
        if cams.shape[0] != 1:
            raise ValueError("project_noise runs at batch 1 (model_v3.py:389)")
        stream = hip.stream_ptr()
        done = {}
        res = []
        for i, (nb, s, lvl) in enumerate(zip(noise_bufs, self.sizes, self.levels)):
            if nb is None or tuple(nb.shape) != (1, 1, s, s):
                raise ValueError(f"noise_bufs[{i}] must be a (1, 1, {s}, {s}) tensor")
            v, f = self.meshes[lvl]
            if s not in done:                     # one rasterisation per map size, shared by the layers of that size
                ws, keys = self._ws.get((stream, s), (None, None))
                self._ws[(stream, s)] = done[s] = hip.mesh_rasterize(v, f, cams, s, ws=ws, keys=keys)
            ws, keys = done[s]
            o = None if out is None else out[i]
            r = hip.mesh_resolve(v, f, ws, keys, want=("attr",), attr=self.vert_noise[i], base=nb.float().contiguous(),
                                 out=None if o is None else {"attr": o})
            res.append(r["attr"])
        return res


def view_angles(cam_poses):
    """(azim, elev) [B] of camera-to-world poses [B,3,4] from the camera position C = cam_poses[:, :, 3]:
    azim = atan2(C_x, C_z), elev = asin(C_y / |C|) -- the trajectory row the pose was made from."""
    c = cam_poses[:, :, 3].double()
    return torch.atan2(c[:, 0], c[:, 2]).float(), torch.asin(c[:, 1] / c.norm(dim=1)).float()
