"""Rank-sharded bulk generation and depth-map surface extraction.

`gen_images` follows /root/reference/exp/cips3d/scripts/gen_images.py:33-92: every rank renders `batch_gpu`
random views per round (fresh z pair, camera drawn from `cam_cfg`), image `i` of round `b` is saved as
`{b * batch_gpu * world + i * world + rank:05d}.jpg`; there is no exchange step — the file system is the gather.
The images leave the GPU as uint8 (`cips3d_rgb_to_uint8`, the clamp[-1,1] -> [0,255] of `save_image(normalize=True,
value_range=(-1,1))`), 4x fewer bytes over PCIe than the fp32 tensor.

`xyz_to_mesh` follows exp/cips3d/utils.py:228-243 (`xyz2mesh`): vertices = the compositing-weighted surface points
of the `xyz` map, faces = a triangulation of the pixel grid with inverted normals.  The reference triangulates the
(degenerate, co-circular) regular grid with scipy's Delaunay, whose diagonal choice per cell is arbitrary; here every
cell is split along the same diagonal, which is one of the valid Delaunay triangulations of that grid.
"""
import os

import numpy as np
import torch


def mixing_noise(batch, latent_dim, device, n_noise=2, generator=None):
    """exp/cips3d/utils.py:84-105: `n_noise` independent z of shape (batch, latent_dim) from one randn call."""
    return list(torch.randn(n_noise, batch, latent_dim, device=device, generator=generator).unbind(0))


def image_index(round_idx, idx_in_batch, rank, world_size, batch_gpu):
    """gen_images.py:83: global index of image `idx_in_batch` rendered by `rank` in round `round_idx`."""
    return round_idx * batch_gpu * world_size + idx_in_batch * world_size + rank


def n_rounds(num_imgs, world_size, batch_gpu):
    return (num_imgs + batch_gpu * world_size - 1) // (batch_gpu * world_size)


def _save_uint8_chw(img_u8, path):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img_u8.permute(1, 2, 0).cpu().numpy())).save(path, quality=95)


def gen_images(rank, world_size, generator, G_kwargs, fake_dir, num_imgs, batch_gpu, truncation=1, to_uint8=None,
               save_fn=_save_uint8_chw, ext="jpg", barrier=None, seed=None, camera_fn=None):
    """Returns the list of files this rank wrote.  `G_kwargs` = {"cam_cfg": {...img_size...}, "nerf_cfg": {...}}
    (train_cips3d_ffhq_v10.yaml:129-140).  `to_uint8` defaults to the HIP image post-step."""
    if camera_fn is None:
        from .camera import Camera
        camera_fn = Camera.generate_camera_params
    if to_uint8 is None:
        from .hip import rgb_to_uint8 as to_uint8
    if rank == 0:
        os.makedirs(fake_dir, exist_ok=True)
    if barrier is not None:
        barrier()
    cam_cfg = dict(G_kwargs["cam_cfg"])
    nerf_cfg = dict(G_kwargs["nerf_cfg"])
    img_size = cam_cfg.pop("img_size")
    device = next(generator.parameters()).device
    gen = None
    if seed is not None:
        gen = torch.Generator(device=device).manual_seed(int(seed) + rank)
    written = []
    generator.eval()
    with torch.no_grad():
        for b in range(n_rounds(num_imgs, world_size, batch_gpu)):
            zs = mixing_noise(batch_gpu, generator.z_dim, device, generator=gen)
            cam, focal, near, far, _ = camera_fn(img_size, device, batch=batch_gpu, **cam_cfg)
            ret = generator(zs=zs, cam_poses=cam, focals=focal, img_size=img_size, near=near, far=far,
                            truncation=truncation, nerf_cfg=nerf_cfg)
            imgs = to_uint8(ret["rgb"])
            for i in range(imgs.shape[0]):
                idx = image_index(b, i, rank, world_size, batch_gpu)
                path = os.path.join(fake_dir, f"{idx:0>5}.{ext}")
                save_fn(imgs[i], path)
                written.append(path)
    if barrier is not None:
        barrier()
    return written


def grid_faces(h, w):
    """Two triangles per pixel cell, vertex index = row * w + col.  Winding as in the reference after its
    "invert normals" swap: scipy's simplices are counter-clockwise in (col, row), the world frame has y = -row, so
    after the swap the normals of a fronto-parallel depth map point at the camera (+z for the frontal view)."""
    r, c = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")
    v00 = (r * w + c).reshape(-1)
    v01 = v00 + 1
    v10 = v00 + w
    v11 = v10 + 1
    return np.concatenate([np.stack([v00, v10, v01], 1), np.stack([v01, v10, v11], 1)], 0).astype(np.int64)


def xyz_to_mesh(xyz):
    """`xyz` (1,3,h,w) -> (vertices [h*w,3] float32, faces [2*(h-1)*(w-1),3] int64)."""
    if xyz.dim() != 4 or xyz.shape[0] != 1 or xyz.shape[1] != 3:
        raise ValueError("xyz must be (1,3,h,w)")
    _, _, h, w = xyz.shape
    verts = xyz[0].permute(1, 2, 0).reshape(h * w, 3).detach().float().cpu().numpy()
    return verts, grid_faces(h, w)


def vertex_normals(verts, faces):
    """Area-weighted vertex normals (what trimesh's `vertex_normals` provides to the mesh renderer,
    render_video_web_v10.py:1843-1850)."""
    tri = verts[faces]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    vn = np.zeros_like(verts)
    for k in range(3):
        np.add.at(vn, faces[:, k], fn)
    n = np.linalg.norm(vn, axis=1, keepdims=True)
    return vn / np.maximum(n, 1e-20)


def _unit_colors(colors, n_verts, what):
    """[V,3] colours in [-1, 1] (the generator's image range) -> numpy fp64 in [0, 1]."""
    c = np.asarray(colors, np.float64)
    if c.shape != (n_verts, 3):
        raise ValueError(f"{what}: colors of shape {c.shape} for {n_verts} vertices")
    return np.clip((c + 1) / 2, 0, 1)


def write_obj(path, verts, faces, normals=None, colors=None):
    """normals [V,3] (one per vertex): written as `vn` lines, and the faces as `f a//a b//b c//c`.
    colors [V,3] in [-1, 1]: every vertex line becomes `v x y z r g b`, r g b = (c + 1) / 2 clamped to [0, 1] (the common
    vertex-colour extension; mesh.read_obj ignores the extra columns)."""
    if normals is not None and len(normals) != len(verts):
        raise ValueError(f"write_obj: {len(normals)} normals for {len(verts)} vertices")
    rgb = None if colors is None else _unit_colors(colors, len(verts), "write_obj")
    with open(path, "w") as f:
        for i, v in enumerate(verts):
            tail = "" if rgb is None else f" {rgb[i][0]:.6f} {rgb[i][1]:.6f} {rgb[i][2]:.6f}"
            f.write(f"v {v[0]:.7g} {v[1]:.7g} {v[2]:.7g}{tail}\n")
        if normals is None:
            for t in faces + 1:
                f.write(f"f {t[0]} {t[1]} {t[2]}\n")
        else:
            for n in normals:
                f.write(f"vn {n[0]:.7g} {n[1]:.7g} {n[2]:.7g}\n")
            for t in faces + 1:
                f.write(f"f {t[0]}//{t[0]} {t[1]}//{t[1]} {t[2]}//{t[2]}\n")
    return path


def write_textured_obj(path, verts, faces, uv, width, height, normals=None, mtl=None, material="textured"):
    """The OBJ of a mesh with a texture atlas (mesh.texture_atlas): uv [F,3,2], the faces' corner UVs in continuous texel
    coordinates of a width x height atlas, become 3F `vt` lines, u = x / width, v = 1 - y / height (OBJ's v points up, the
    atlas' row 0 is its top); the faces are `f a/t/a b/t/b c/t/c` with normals [V,3], `f a/t b/t c/t` without.  mtl: the name
    of the material file (write_mtl) for the `mtllib` line, with `usemtl <material>` before the faces.  mesh.read_obj reads
    the positions and faces back."""
    uv = np.asarray(uv, np.float64).reshape(-1, 3, 2)
    if len(uv) != len(faces):
        raise ValueError(f"write_textured_obj: {len(uv)} UV triangles for {len(faces)} faces")
    if normals is not None and len(normals) != len(verts):
        raise ValueError(f"write_textured_obj: {len(normals)} normals for {len(verts)} vertices")
    with open(path, "w") as f:
        if mtl is not None:
            f.write(f"mtllib {mtl}\n")
        for v in verts:
            f.write(f"v {v[0]:.7g} {v[1]:.7g} {v[2]:.7g}\n")
        for tri in uv:
            for x, y in tri:
                f.write(f"vt {x / width:.7f} {1.0 - y / height:.7f}\n")
        if normals is not None:
            for n in normals:
                f.write(f"vn {n[0]:.7g} {n[1]:.7g} {n[2]:.7g}\n")
        if mtl is not None:
            f.write(f"usemtl {material}\n")
        for k, t in enumerate(np.asarray(faces) + 1):
            a, b, c = 3 * k + 1, 3 * k + 2, 3 * k + 3
            if normals is None:
                f.write(f"f {t[0]}/{a} {t[1]}/{b} {t[2]}/{c}\n")
            else:
                f.write(f"f {t[0]}/{a}/{t[0]} {t[1]}/{b}/{t[1]} {t[2]}/{c}/{t[2]}\n")
    return path


def write_mtl(path, texture_file, material="textured"):
    """A one-material MTL file whose diffuse map is `texture_file` (a path relative to the MTL file): white Kd, so that a viewer
    shows the texture as it is."""
    with open(path, "w") as f:
        f.write(f"newmtl {material}\nKa 0 0 0\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {texture_file}\n")
    return path


def write_texture_png(path, texture_u8):
    """uint8 [3,Ht,Wt] (mesh.texture_to_uint8 of a baked texture) -> an RGB PNG of Wt x Ht."""
    from PIL import Image
    t = np.asarray(texture_u8)
    if t.ndim != 3 or t.shape[0] != 3 or t.dtype != np.uint8:
        raise ValueError("write_texture_png: the texture must be uint8 [3, Ht, Wt]")
    Image.fromarray(np.ascontiguousarray(t.transpose(1, 2, 0))).save(path)
    return path


def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY: float x y z, float nx ny nz with `normals` [V,3], uchar red green blue with `colors` [V,3] in
    [-1, 1] (floor(255 clamp((c + 1) / 2, 0, 1) + 0.5)), then the triangles as `list uchar int`.  mesh.read_ply reads it back."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces)
    if faces.size and (faces.min() < 0 or faces.max() >= len(verts)):
        raise ValueError("write_ply: a face names a vertex that is not there")
    fields = [(n, "<f4") for n in "xyz"]
    if normals is not None:
        if len(normals) != len(verts):
            raise ValueError(f"write_ply: {len(normals)} normals for {len(verts)} vertices")
        fields += [(n, "<f4") for n in ("nx", "ny", "nz")]
    if colors is not None:
        rgb = np.floor(255 * _unit_colors(colors, len(verts), "write_ply") + 0.5).astype(np.uint8)
        fields += [(n, "u1") for n in ("red", "green", "blue")]
    v = np.zeros(len(verts), np.dtype(fields))
    for k, n in enumerate("xyz"):
        v[n] = verts[:, k]
    if normals is not None:
        for k, n in enumerate(("nx", "ny", "nz")):
            v[n] = np.asarray(normals, np.float32)[:, k]
    if colors is not None:
        for k, n in enumerate(("red", "green", "blue")):
            v[n] = rgb[:, k]
    f = np.zeros(len(faces), np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    f["n"] = 3
    f["idx"] = faces.reshape(-1, 3)
    names = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + \
           [f"property {names[t]} {n}" for n, t in fields] + \
           [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(f.tobytes())
    return path
