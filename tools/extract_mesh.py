"""Frontal marching-cubes mesh of a generator (cips_3dplusplus_amd.mesh.surface_mesh), written as an OBJ file.

    python tools/extract_mesh.py [--ckpt DIR] [--depth 2] [--seed 0] [--resolution 128] [--out mesh.obj] [--normals] [--time]

--normals writes the vertex normals too (`vn` lines, `f a//a b//b c//c`).  Without --ckpt the generator is the FFHQ 256^2 configuration with synthetic weights (`--depth` renderer layers).  With
--time it prints one JSON line of device-event timings (ms, median of --reps runs) of the renderer-only SDF pass, the
alignment, the two marching-cubes calls and the whole surface_mesh call, with V and F; and the same three mesh steps on
an analytic sphere (radius 0.3 n) in an n^3 volume, n = --resolution, whose triangle count does not depend on weights.
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
from cips_3dplusplus_amd.gen_images import write_obj  # noqa: E402


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
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.ckpt:
        from cips_3dplusplus_amd.checkpoint import load_generator
        G, _ = load_generator(args.ckpt, dev)
    else:
        G = pkg.build_generator(configs.ffhq_G_cfg(256, args.depth), dev, seed=args.seed)
    S = args.resolution
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(args.seed)).to(dev)
    out = mesh.surface_mesh(G, zs=[z], resolution=S, normals=args.normals)
    m = out["meshes"][0]
    if m is not None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        write_obj(args.out, m[0].cpu().numpy(), m[1].cpu().numpy(), m[2].cpu().numpy() if args.normals else None)
        print(f"wrote {args.out}: {m[0].shape[0]} vertices, {m[1].shape[0]} faces")
    else:
        print("no surface: the SDF volume has no zero crossing")
    if not args.time:
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
    print(json.dumps({
        "workload": f"surface_mesh depth={args.depth} {S}^2 rays x {S} samples, frontal", "device": torch.cuda.get_device_name(0),
        "render_ms": round(t_render, 4), "align_ms": round(t_align, 4), "count_ms": round(t_count, 4),
        "emit_ms": round(t_emit, 4), "end_to_end_ms": round(t_total, 4), "V": int(v.shape[0]), "F": int(f.shape[0]),
        "sphere": {"n": S, "radius": 0.3 * S, "align_ms": round(t_salign, 4), "count_ms": round(t_scount, 4),
                   "emit_ms": round(t_semit, 4), "V": int(sv.shape[0]), "F": int(sf.shape[0])},
        "reps": reps}))


if __name__ == "__main__":
    main()
