"""Frontal marching-cubes mesh of a generator (cips_3dplusplus_amd.mesh.surface_mesh), written as an OBJ file.

    python tools/extract_mesh.py [--ckpt DIR] [--depth 2] [--seed 0] [--resolution 128] [--out mesh.obj] [--normals] [--time]
                                 [--frames N [--frames-out DIR] [--image-size 512]]
                                 [--colors [--color-views "az,el;az,el;..."] [--ply]]
                                 [--texture [--texels 8] [--fill-iters 64]]

--normals writes the vertex normals too (`vn` lines, `f a//a b//b c//c`).  Without --ckpt the generator is the FFHQ 256^2 configuration with synthetic weights (`--depth` renderer layers).  With
--time it prints one JSON line of device-event timings (ms, median of --reps runs) of the renderer-only SDF pass, the
alignment, the two marching-cubes calls and the whole surface_mesh call, with V and F; and the same three mesh steps on
an analytic sphere (radius 0.3 n) in an n^3 volume, n = --resolution, whose triangle count does not depend on weights.
--frames N rasterises the mesh from the N-frame yaw trajectory (mesh.render_mesh_frames: the reference's Phong mesh panel) and
writes frame_000.png ... into --frames-out (default: next to --out); with --time the JSON line gains `raster_ms` / `resolve_ms`
of those N frames in one call on the sphere mesh at --image-size, and `levels`: V / F of the production mesh after 0, 1 and 3
midpoint subdivisions (mesh.subdivision_levels) with the one-view rasterise / resolve times of a noise projection at every
layer size that uses the level.
--colors colours the mesh from the generator's own pictures of the same latent (mesh.color_mesh; --color-views: the (azim, elev)
of those pictures in radians): the OBJ's vertex lines become `v x y z r g b`, --ply writes a binary PLY with uchar colours next
to it, and the --frames are the coloured ones.  With --time the JSON line gains `color`: one cips3d_mesh_vertex_colors call at
the production mesh's V, 3 views, S = 512, R = 1024, against the same gather written with torch's grid_sample on the device.
--texture bakes a texture atlas from the same pictures (mesh.texture_mesh: vertex colours -> --fill-iters rings of fill -> bake at
--texels texels per cell side; needs no --colors): the OBJ gets `vt` lines, `f a/t/a` faces and `mtllib` / `usemtl`, with an MTL
and a PNG of the same stem next to it; one JSON line `{"texture": {...}}` gives the atlas size and the seen / filled /
never-filled texel counts, and the --frames are the textured ones.  With --time that entry moves into the timing line and gains
`time`: the bake at the production mesh's F, 3 views, S = 512, R = 1024, the fill, one textured frame at --image-size, and the
same bake written in torch ops on the device.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import cips_3dplusplus_amd as pkg  # noqa: E402
from cips_3dplusplus_amd import configs, hip, mesh  # noqa: E402
from cips_3dplusplus_amd.camera import Camera  # noqa: E402
from cips_3dplusplus_amd.gen_images import write_mtl, write_obj, write_ply, write_texture_png, write_textured_obj  # noqa: E402


def timed(fn, reps):
    """(result of the last run, median ms) over `reps` runs, each bracketed by events on the current stream."""
    ts, out = [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return out, ts[len(ts) // 2]


def mesh_steps(vol, level, affine, reps):
    """align is timed by the caller; here count (classify + scan) and emit of one [h,w,d] volume, device time only."""
    (ws, totals), t_count = timed(lambda: hip.marching_cubes_count(vol, level), reps)
    n_v, n_f = (int(v) for v in totals.cpu())
    (v, f), t_emit = timed(lambda: hip.marching_cubes_emit(vol, level, ws, n_v, n_f, affine), reps)
    return v, f, t_count, t_emit


def raster_steps(verts, faces, cams, size, reps, **resolve_kw):
    """median device ms of (cips3d_mesh_rasterize, cips3d_mesh_resolve) on preallocated buffers."""
    f32 = faces.to(torch.int32).contiguous()
    (ws, keys), t_raster = timed(lambda: hip.mesh_rasterize(verts, f32, cams, size), 1)
    _, t_raster = timed(lambda: hip.mesh_rasterize(verts, f32, cams, size, ws=ws, keys=keys), reps)
    out, _ = timed(lambda: hip.mesh_resolve(verts, f32, ws, keys, **resolve_kw), 1)
    _, t_resolve = timed(lambda: hip.mesh_resolve(verts, f32, ws, keys, out=out, **resolve_kw), reps)
    return round(t_raster, 4), round(t_resolve, 4)


def color_steps(verts, faces, normals, reps, views=mesh.DEFAULT_COLOR_VIEWS, S=512, R=1024, power=2):
    """median device ms of one cips3d_mesh_vertex_colors call, and of the same gather in torch ops (the visibility test on the
    resolved z-buffer, grid_sample for the bilinear taps), both after the rasterisation, on preallocated inputs."""
    import torch.nn.functional as F
    dev = verts.device
    f32 = faces.to(torch.int32).contiguous()
    az, el = (torch.tensor([v[k] for v in views], dtype=torch.float32) for k in (0, 1))
    cams = mesh.camera_rows(az, el, 12.0, device=dev)
    n, V = cams.shape[0], verts.shape[0]
    images = torch.rand(n, 3, R, R, device=dev) * 2 - 1
    tol = mesh.FRAME_SCALE / 128
    ws, keys = hip.mesh_rasterize(verts, f32, cams, S)
    out, _ = timed(lambda: hip.mesh_vertex_colors(verts, normals, images, ws, keys, S, power=power, depth_tol=tol), 1)
    _, t_kernel = timed(lambda: hip.mesh_vertex_colors(verts, normals, images, ws, keys, S, power=power, depth_tol=tol, out=out), reps)
    zbuf = hip.mesh_resolve(verts, f32, ws, keys, want=("zbuf",))["zbuf"]
    zbuf = torch.where(zbuf < 0, torch.full_like(zbuf, float("inf")), zbuf)
    nbytes = -(-n * 16 * 4 // 256) * 256                 # the derived cameras, then proj [n,V,4] (csrc/mesh_raster.h)
    eye = ws[:n * 64].view(torch.float32).view(n, 16)[:, :3]
    proj = ws[nbytes:nbytes + n * V * 16].view(torch.float32).view(n, V, 4)

    def torch_gather():
        x, y, z = proj[..., 0], proj[..., 1], proj[..., 2]
        j, i = torch.round(x), torch.round(y)
        on = (proj[..., 3] > 0) & (j >= 0) & (j <= S - 1) & (i >= 0) & (i <= S - 1)
        pix = (i.clamp(0, S - 1) * S + j.clamp(0, S - 1)).long()
        vis = on & (z <= torch.gather(zbuf.view(n, -1), 1, pix) + tol)
        d = F.normalize(eye[:, None] - verts[None], dim=-1)
        c = (d * normals[None]).sum(-1)
        w = torch.where(vis & (c > 0), c ** power, torch.zeros_like(c))
        grid = torch.stack([(x + 0.5) * (2.0 / S) - 1, (y + 0.5) * (2.0 / S) - 1], -1)[:, :, None]
        rgb = F.grid_sample(images, grid, mode="bilinear", padding_mode="border", align_corners=False)[..., 0]
        wsum = w.sum(0)
        return torch.where(wsum[:, None] > 0, (w[:, None] * rgb).sum(0).t() / wsum[:, None].clamp_min(1e-30), torch.zeros(V, 3, device=dev))
    ref, _ = timed(torch_gather, 2)
    _, t_torch = timed(torch_gather, reps)
    return {"V": V, "views": n, "S": S, "R": R, "kernel_ms": round(t_kernel, 4), "grid_sample_ms": round(t_torch, 4),
            "max_abs_diff": round(float((ref - out["colors"]).abs().max()), 6)}


def texture_steps(verts, faces, normals, reps, views=mesh.DEFAULT_COLOR_VIEWS, S=512, R=1024, power=2, texels=8, fill_iters=64,
                  image_size=512):
    """median device ms of one cips3d_mesh_texture_bake call, of cips3d_mesh_fill_colors at fill_iters rings, of one textured
    frame at image_size^2, and of the same bake in torch ops (texel points from the atlas maps, the visibility test on the resolved
    z-buffer, grid_sample for the bilinear taps), all after the rasterisation, on preallocated inputs."""
    import torch.nn.functional as F
    dev = verts.device
    f32 = faces.to(torch.int32).contiguous()
    az, el = (torch.tensor([v[k] for v in views], dtype=torch.float32) for k in (0, 1))
    cams = mesh.camera_rows(az, el, 12.0, device=dev)
    n, V = cams.shape[0], verts.shape[0]
    images = torch.rand(n, 3, R, R, device=dev) * 2 - 1
    tol = mesh.FRAME_SCALE / 128
    atlas = mesh.texture_atlas(f32.shape[0], texels)
    T, cols, rows = atlas["T"], atlas["cols"], atlas["rows"]
    ws, keys = hip.mesh_rasterize(verts, f32, cams, S)
    bake = lambda out=None: hip.mesh_texture_bake(verts, f32, normals, images, ws, keys, S, T, cols, rows, power=power,      # noqa: E731
                                                  depth_tol=tol, out=out)
    out, _ = timed(bake, 1)
    _, t_bake = timed(lambda: bake(out), reps)
    col = hip.mesh_vertex_colors(verts, normals, images, ws, keys, S, power=power, depth_tol=tol)
    fws = torch.empty(int(hip._lib.load().cips3d_mesh_fill_workspace_bytes(V)), dtype=torch.uint8, device=dev)
    grown, _ = timed(lambda: hip.mesh_fill_colors(col["colors"], col["weight"], f32, iters=fill_iters, ws=fws), 1)
    _, t_fill = timed(lambda: hip.mesh_fill_colors(col["colors"], col["weight"], f32, iters=fill_iters, ws=fws, out=grown), reps)
    light = torch.tensor([[0.0, 0.0, 5.0]], device=dev)
    maps = mesh.rasterize_mesh(verts, faces, 0.0, 0.0, image_size, normals=normals, light=light, want=("face", "bary", "shade"))
    frame = lambda o=None: hip.mesh_textured_frame(maps["face"], maps["bary"], maps["shade"], out["texture"], f32.shape[0], T, cols,      # noqa: E731
                                                   rows, out=o)
    fr, _ = timed(frame, 1)
    _, t_frame = timed(lambda: frame(fr), reps)
    # the same bake in torch ops
    zbuf = hip.mesh_resolve(verts, f32, ws, keys, want=("zbuf",))["zbuf"]
    zbuf = torch.where(zbuf < 0, torch.full_like(zbuf, float("inf")), zbuf)
    cam = ws[:n * 64].view(torch.float32).view(n, 16)                   # the derived cameras (csrc/mesh_raster.h)
    tex = mesh.atlas_texels(atlas)
    owned = (tex["face"] >= 0).to(dev)
    tri = faces.long()[tex["face"].to(dev).long()[owned]]
    b = tex["bary"].to(dev)[owned]
    mix = lambda a: (b[:, 0:1] * a[tri[:, 0]] + b[:, 1:2] * a[tri[:, 1]]) + b[:, 2:3] * a[tri[:, 2]]      # noqa: E731

    def torch_bake():
        P, N = mix(verts), F.normalize(mix(normals), dim=-1)
        d = P[None] - cam[:, None, 0:3]
        vx, vy, vz = ((d * cam[:, None, 3 + 3 * k:6 + 3 * k]).sum(-1) for k in range(3))
        x = (1 - cam[:, 12:13] * vx / vz) * (0.5 * S) - 0.5
        y = (1 - cam[:, 12:13] * vy / vz) * (0.5 * S) - 0.5
        j, i = torch.round(x), torch.round(y)
        on = (vz >= cam[:, 13:14]) & (vz > 0) & (j >= 0) & (j <= S - 1) & (i >= 0) & (i <= S - 1)
        pix = (i.clamp(0, S - 1) * S + j.clamp(0, S - 1)).long()
        vis = on & (vz <= torch.gather(zbuf.view(n, -1), 1, pix) + tol)
        c = (F.normalize(-d, dim=-1) * N[None]).sum(-1)
        w = torch.where(vis & (c > 0), c ** power, torch.zeros_like(c))
        grid = torch.stack([(x + 0.5) * (2.0 / S) - 1, (y + 0.5) * (2.0 / S) - 1], -1)[:, :, None]
        rgb = F.grid_sample(images, grid, mode="bilinear", padding_mode="border", align_corners=False)[..., 0]
        wsum = w.sum(0)
        t = torch.zeros(3, atlas["height"], atlas["width"], device=dev)
        t[:, owned] = torch.where(wsum[None] > 0, (w[:, None] * rgb).sum(0) / wsum[None].clamp_min(1e-30), torch.zeros_like(rgb[0]))
        return t
    ref, _ = timed(torch_bake, 2)
    _, t_torch = timed(torch_bake, reps)
    return {"F": int(f32.shape[0]), "views": n, "S": S, "R": R, "texels": T, "atlas": [atlas["width"], atlas["height"]],
            "bake_ms": round(t_bake, 4), "fill_ms": round(t_fill, 4), "fill_iters": fill_iters,
            "fill_rings_used": int(grown["filled"].max()), "frame_ms": round(t_frame, 4), "frame_size": image_size,
            "torch_bake_ms": round(t_torch, 4), "max_abs_diff": round(float((ref - out["texture"]).abs().max()), 6)}


def parse_views(text):
    return tuple(tuple(float(x) for x in pair.split(",")) for pair in text.split(";") if pair.strip())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--out", default="mesh.obj")
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--frames-out", default=None)
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--colors", action="store_true")
    ap.add_argument("--color-views", default=None)
    ap.add_argument("--ply", action="store_true")
    ap.add_argument("--texture", action="store_true")
    ap.add_argument("--texels", type=int, default=8)
    ap.add_argument("--fill-iters", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.ckpt:
        from cips_3dplusplus_amd.checkpoint import load_generator
        G, _ = load_generator(args.ckpt, dev)
    else:
        G = pkg.build_generator(configs.ffhq_G_cfg(256, args.depth), dev, seed=args.seed)
    S = args.resolution
    gen = torch.Generator().manual_seed(args.seed)
    z = torch.randn(1, G.z_dim, generator=gen).to(dev)
    zs = [z]
    color_kw = {}
    if args.colors or args.texture:
        zs.append(torch.randn(1, G.z_dim, generator=gen).to(dev))
        torch.manual_seed(args.seed)                    # the decoder's noise maps are drawn from torch's generator
        if args.color_views:
            color_kw["views"] = parse_views(args.color_views)
    out = mesh.surface_mesh(G, zs=zs, resolution=S, normals=args.normals or args.frames > 0 or args.colors or args.texture,
                            colors=args.colors, color_kw=color_kw, texture=args.texture,
                            texture_kw=dict(texels=args.texels, fill_iters=args.fill_iters))
    m = out["meshes"][0]
    colors = m[3] if m is not None and args.colors else None
    baked = out["textures"][0] if m is not None and args.texture else None
    tex_info = None
    if m is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        v_np, f_np = m[0].cpu().numpy(), m[1].cpu().numpy()
        n_np = m[2].cpu().numpy() if args.normals or args.colors or args.texture else None
        c_np = None if colors is None else colors.cpu().numpy()
        if baked is None:
            write_obj(args.out, v_np, f_np, n_np, c_np)
        else:
            atlas = baked["atlas"]
            stem = os.path.splitext(args.out)[0]
            write_texture_png(stem + ".png", mesh.texture_to_uint8(baked["texture"]).cpu().numpy())
            write_mtl(stem + ".mtl", os.path.basename(stem) + ".png")
            write_textured_obj(args.out, v_np, f_np, atlas["uv"].numpy(), atlas["width"], atlas["height"], normals=n_np,
                               mtl=os.path.basename(stem) + ".mtl")
            seen, grown, never = mesh.texel_counts(baked, baked["filled"], m[1])
            tex_info = {"atlas": [atlas["width"], atlas["height"]], "texels": atlas["T"], "fill_iters": args.fill_iters, "seen": seen,
                        "filled": grown, "never_filled": never}
            print(f"wrote {stem}.mtl and {stem}.png: atlas {atlas['width']} x {atlas['height']}, {seen} texels seen, {grown} filled "
                  f"from their corners, {never} left at the fill colour")
        print(f"wrote {args.out}: {m[0].shape[0]} vertices, {m[1].shape[0]} faces")
        if args.ply:
            ply = os.path.splitext(args.out)[0] + ".ply"
            write_ply(ply, v_np, f_np, n_np, c_np)
            print(f"wrote {ply}")
        if colors is not None:
            unseen = int((out["color_seen"][0] == 0).sum())
            print(f"coloured from {len(color_kw.get('views', mesh.DEFAULT_COLOR_VIEWS))} views: {unseen} of {m[0].shape[0]} "
                  "vertices are seen by none and keep the fill colour")
    else:
        print("no surface: the SDF volume has no zero crossing")
    traj = None
    if args.frames > 0:
        from cips_3dplusplus_amd.camera import yaw_trajectory
        traj = yaw_trajectory(args.frames)
        if m is not None:
            from PIL import Image
            if baked is not None:
                frames = mesh.render_textured_frames(m[0], m[1], m[2], traj, baked["texture"], baked["atlas"],
                                                     image_size=args.image_size)
            else:
                frames = mesh.render_mesh_frames(m[0], m[1], m[2], traj, image_size=args.image_size, colors=colors)
            fdir = args.frames_out or os.path.dirname(os.path.abspath(args.out))
            os.makedirs(fdir, exist_ok=True)
            for i, fr in enumerate(frames.permute(0, 2, 3, 1).cpu().numpy()):
                Image.fromarray(fr).save(os.path.join(fdir, f"frame_{i:03d}.png"))
            print(f"wrote {args.frames} mesh frames of {args.image_size}^2 to {fdir}")
    if not args.time:
        if tex_info is not None:
            print(json.dumps({"texture": tex_info}))
        return
    reps = args.reps
    for _ in range(3):                       # warm-up: plans, film tables, code objects
        mesh.surface_mesh(G, zs=[z], resolution=S)
    torch.cuda.synchronize()
    style_r, _ = G.mapping_renderer([z], 1, None)
    cam = Camera.generate_camera_params(S, dev, locations=torch.zeros(1, 2, device=dev))
    (_, _, sdf, _, _), t_render = timed(lambda: G.renderer.render(cam[0], cam[1], cam[2], cam[3], style_r, S, S,
                                                                   return_sdf=True), reps)
    aligned, t_align = timed(lambda: mesh.align_volume(sdf), reps)
    vol = aligned[0, ..., 0].contiguous()
    v, f, t_count, t_emit = mesh_steps(vol, 0.0, mesh.reference_affine(S, S, S), reps)
    _, t_total = timed(lambda: mesh.surface_mesh(G, zs=[z], resolution=S), reps)
    # analytic sphere in an S^3 volume
    ax = torch.arange(S, device=dev, dtype=torch.float32) - (S - 1) / 2
    sph = (torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.3 * S).contiguous()
    _, t_salign = timed(lambda: mesh.align_volume(sph[None]), reps)
    sv, sf, t_scount, t_semit = mesh_steps(sph, 0.0, None, reps)
    extra = {}
    if traj is not None:
        # the N mesh frames in one call, on the sphere mesh in the reference's output frame
        sv_f, sf_f, sn_f = hip.marching_cubes(sph, 0.0, affine=mesh.reference_affine(S, S, S), normals=True)
        cams = mesh.camera_rows(traj[:, 0], traj[:, 1], 2.0 * traj[:, 2], device=dev)
        light = torch.stack([5 * torch.sin(traj[:, 0]), torch.zeros(len(traj)), 5 * torch.cos(traj[:, 0])], 1).to(dev).contiguous()
        t_r, t_s = raster_steps(sv_f, sf_f, cams, args.image_size, reps, want=("shade_u8",), normals=sn_f, light=light)
        extra.update({"raster_ms": t_r, "resolve_ms": t_s, "frames": args.frames, "image_size": args.image_size})
        # the production mesh along the reference's subdivision ladder: one view, one noise layer per size
        levels = []
        if m is not None:
            lv, lf = m[0], m[1]
            cam1 = mesh.camera_rows(0.3, 0.1, 12.0, device=dev)
            for lvl in range(4):
                if lvl:
                    lv, lf = mesh.subdivide(lv, lf)
                sizes = [s for s in (64, 128, 256, 512, 1024) if mesh.subdivision_levels(s) == lvl]
                if not sizes:
                    continue
                noise = torch.randn(lv.shape[0], 1, device=dev)
                row = {"level": lvl, "V": int(lv.shape[0]), "F": int(lf.shape[0]), "sizes": {}}
                for s in sizes:
                    t_r, t_s = raster_steps(lv.contiguous(), lf, cam1, s, reps, want=("attr",), attr=noise,
                                            base=torch.randn(1, 1, s, s, device=dev))
                    row["sizes"][str(s)] = {"raster_ms": t_r, "resolve_ms": t_s}
                levels.append(row)
        extra["levels"] = levels
    if args.colors and m is not None:
        extra["color"] = color_steps(m[0], m[1], m[2], reps)
    if tex_info is not None:
        extra["texture"] = dict(tex_info, time=texture_steps(m[0], m[1], m[2], reps, texels=args.texels, fill_iters=args.fill_iters,
                                                             image_size=args.image_size))
    print(json.dumps({
        "workload": f"surface_mesh depth={args.depth} {S}^2 rays x {S} samples, frontal", "device": torch.cuda.get_device_name(0),
        "render_ms": round(t_render, 4), "align_ms": round(t_align, 4), "count_ms": round(t_count, 4),
        "emit_ms": round(t_emit, 4), "end_to_end_ms": round(t_total, 4), "V": int(v.shape[0]), "F": int(f.shape[0]),
        "sphere": {"n": S, "radius": 0.3 * S, "align_ms": round(t_salign, 4), "count_ms": round(t_scount, 4),
                   "emit_ms": round(t_semit, 4), "V": int(sv.shape[0]), "F": int(sf.shape[0])},
        "reps": reps, **extra}))


if __name__ == "__main__":
    main()
