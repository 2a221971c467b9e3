"""Composited surface normals and the Phong-shaded geometry frame of a generator's frontal view, as PNG files.

    python tools/normals.py [--ckpt DIR] [--depth 2] [--seed 0] [--img-size 64] [--samples 24] [--out-prefix PREFIX] [--time] [--reps 11]

Without --ckpt the generator is the FFHQ 256^2 configuration with synthetic weights (`--depth` renderer layers).  One frontal
camera, perturbation off, the light at the reference's (5 sin azim, 0, 5 cos azim) = (0, 0, 5).  Writes PREFIXnormal.png (the
unit normal as RGB, 127.5 (n + 1)) and PREFIXshaded.png (`VolumeFeatureRenderer.normal_map`'s shade_u8), and prints ONE JSON
object last.  With --time it holds the device-event medians (ms, --reps runs) of the gradient kernel (`sdf_grad_ms`), of the
normals kernel (`normals_ms`, events around the launch itself) and of a device copy of a tensor as large as the normals kernel's
inputs, sdf + grad: 16 bytes per point (`copy_ms`).  All GPU work happens in this one process; nothing is retried.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import cips_3dplusplus_amd as pkg  # noqa: E402
from cips_3dplusplus_amd import configs, hip  # noqa: E402
from cips_3dplusplus_amd.camera import Camera  # noqa: E402
from cips_3dplusplus_amd.gen_images import _save_uint8_chw  # noqa: E402


def kernel_median_ms(name, fn, reps):
    """Median device time of the launch `name` (hip.KERNEL_EVENTS: an event pair around the launch) over `reps` calls of fn."""
    hip.KERNEL_EVENTS[name] = []
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in hip.KERNEL_EVENTS[name])
    finally:
        del hip.KERNEL_EVENTS[name]
    return ts[len(ts) // 2]


def event_median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--img-size", type=int, default=64)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--out-prefix", default="")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.ckpt:
        from cips_3dplusplus_amd.checkpoint import load_generator
        G, _ = load_generator(args.ckpt, dev)
    else:
        G = pkg.build_generator(configs.ffhq_G_cfg(256, args.depth), dev, seed=args.seed)
    ren = G.renderer
    S, N, D = args.img_size, args.samples, ren.N_layers_renderer
    z = torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(args.seed)).to(dev)
    style_r, _ = G.mapping_renderer([z], 1, None)
    cam = Camera.generate_camera_params(S, dev, batch=1, locations=torch.zeros(1, 2, device=dev))
    xyz = ren.render(cam[0], cam[1], cam[2], cam[3], style_r, S, N)[4]
    light = torch.tensor([[0.0, 0.0, 5.0]], device=dev)
    grad_call = lambda: ren.sdf_gradient(cam[0], cam[1], cam[2], cam[3], style_r, S, N)      # noqa: E731
    sdf, grad = grad_call()
    normals_call = lambda: ren.normal_map(cam[0], cam[1], cam[2], cam[3], None, S, N, grad=grad, sdf=sdf,      # noqa: E731
                                          shade=dict(light=light, xyz=xyz))
    out_maps = normals_call()
    normal_u8 = torch.floor(127.5 * (out_maps["normal"][0] + 1) + 0.5).clamp(0, 255).to(torch.uint8)
    files = [args.out_prefix + "normal.png", args.out_prefix + "shaded.png"]
    for f in files:
        if os.path.dirname(f):
            os.makedirs(os.path.dirname(f), exist_ok=True)
    _save_uint8_chw(normal_u8, files[0])
    _save_uint8_chw(out_maps["shade_u8"][0], files[1])
    length = out_maps["normal_raw"].norm(dim=1)
    out = {"workload": f"normal_map depth={D} {S}^2 rays x {N} samples, frontal", "device": torch.cuda.get_device_name(0),
           "points": S * S * N, "files": files,
           "normal_raw_norm": {"min": float(length.min()), "mean": float(length.mean()), "max": float(length.max())},
           "shade": {"min": float(out_maps["shade"].min()), "mean": float(out_maps["shade"].mean()),
                     "max": float(out_maps["shade"].max())}}
    if args.time:
        for _ in range(3):                       # warm-up: tables, weight streams, code objects
            grad_call()
            normals_call()
        out["sdf_grad_ms"] = round(kernel_median_ms("nerf_sdf_grad", grad_call, args.reps), 4)
        out["normals_ms"] = round(kernel_median_ms("nerf_normals", normals_call, args.reps), 4)
        src = torch.empty(S * S * N * 4, device=dev)             # sdf + grad: 4 floats per point
        dst = torch.empty_like(src)
        for _ in range(3):
            dst.copy_(src)
        out["copy_ms"] = round(event_median_ms(lambda: dst.copy_(src), args.reps), 4)
        out["normals_over_sdf_grad"] = round(out["normals_ms"] / out["sdf_grad_ms"], 4)
        out["normals_over_copy"] = round(out["normals_ms"] / out["copy_ms"], 3)
        out["reps"] = args.reps
    print(json.dumps(out))


if __name__ == "__main__":
    main()
