"""SDF gradient diagnostics of a generator: is the renderer's SDF a distance field?

    python tools/sdf_grad.py [--ckpt DIR] [--depth 2] [--seed 0] [--img-size 64] [--samples 24] [--batch 1] [--time] [--reps 11]
                             [--loss]

Without --ckpt the generator is the FFHQ 256^2 configuration with synthetic weights (`--depth` renderer layers).  One frontal
camera per view (views differ in their latent), perturbation off.  Prints ONE JSON object: the eikonal and minimal-surface terms
(cips_3dplusplus_amd.losses.eikonal_loss, beta 100) of `VolumeFeatureRenderer.sdf_gradient`, min / mean / max of |grad sdf|,
and with --time the device-event medians (ms, --reps runs, events around the launch itself) of the gradient kernel and of the
exact-fp32 render kernel at the same shape, their ratio, and the ratio the work predicts (4 (D - 1) / D: four B columns per point
over D - 1 of the render kernel's D matrix layers).  --loss adds "loss": the two terms from the differentiable node
(`VolumeFeatureRenderer.eikonal_loss`, csrc/nerf_eikonal.hip: values and the gradient to the styles) and the norm of d (eikonal +
minimal surface) / d styles; with --time also the wall-clock medians (ms, synchronised) of one forward + backward of the node
and of its torch partner (CIPS3D_FUSED_EIKONAL=0: double backward through torch ops), and the kernel's own device time.
All GPU work happens in this one process; nothing is retried.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import cips_3dplusplus_amd as pkg  # noqa: E402
from cips_3dplusplus_amd import configs, hip, losses  # noqa: E402
from cips_3dplusplus_amd.camera import Camera  # noqa: E402


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


def loss_report(ren, cam, style_r, S, N, args):
    """The differentiable eikonal / minimal-surface node on the same shape; with --time against its torch partner."""
    import time

    def fwd_bwd():
        st = style_r.detach().clone().requires_grad_(True)
        total, eik, ms = ren.eikonal_loss(cam[0], cam[1], cam[2], cam[3], st, S, N, weights=(1.0, 1.0))
        total.backward()
        return eik, ms, st.grad

    def wall_ms(fn, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]

    eik, ms, g = fwd_bwd()
    rep = {"eikonal": float(eik), "minimal_surface": float(ms), "dstyles_norm": float(g.norm())}
    if args.time:
        for _ in range(2):
            fwd_bwd()
        rep["fused_fwd_bwd_ms"] = round(wall_ms(fwd_bwd, args.reps), 4)
        rep["kernel_ms"] = round(kernel_median_ms("nerf_eikonal_loss", fwd_bwd, args.reps), 4)
        prev = os.environ.get("CIPS3D_FUSED_EIKONAL")
        os.environ["CIPS3D_FUSED_EIKONAL"] = "0"
        try:
            e2, m2, g2 = fwd_bwd()
            rep["torch_fwd_bwd_ms"] = round(wall_ms(fwd_bwd, max(3, args.reps // 3)), 4)
        finally:
            if prev is None:
                del os.environ["CIPS3D_FUSED_EIKONAL"]
            else:
                os.environ["CIPS3D_FUSED_EIKONAL"] = prev
        rep["torch_eikonal"], rep["torch_minimal_surface"] = float(e2), float(m2)
        rep["dstyles_rel_diff"] = float((g - g2).norm() / g2.norm().clamp_min(1e-30))
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--img-size", type=int, default=64)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--loss", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.ckpt:
        from cips_3dplusplus_amd.checkpoint import load_generator
        G, _ = load_generator(args.ckpt, dev)
    else:
        G = pkg.build_generator(configs.ffhq_G_cfg(256, args.depth), dev, seed=args.seed)
    ren = G.renderer
    B, S, N, D = args.batch, args.img_size, args.samples, ren.N_layers_renderer
    z = torch.randn(B, G.z_dim, generator=torch.Generator().manual_seed(args.seed)).to(dev)
    style_r, _ = G.mapping_renderer([z], 1, None)
    cam = Camera.generate_camera_params(S, dev, batch=B, locations=torch.zeros(B, 2, device=dev))
    grad_call = lambda: ren.sdf_gradient(cam[0], cam[1], cam[2], cam[3], style_r, S, N)      # noqa: E731
    sdf, grad = grad_call()
    eik, msurf = losses.eikonal_loss(grad, sdf=sdf, beta=100)
    norm = grad.norm(dim=-1)
    out = {"workload": f"sdf_gradient depth={D} batch={B} {S}^2 rays x {N} samples, frontal",
           "device": torch.cuda.get_device_name(0), "points": B * S * S * N,
           "eikonal_loss": float(eik), "minimal_surface_loss": float(msurf),
           "grad_norm": {"min": float(norm.min()), "mean": float(norm.mean()), "max": float(norm.max())}}
    if args.time:
        for _ in range(3):                       # warm-up: tables, weight streams, code objects
            grad_call()
        out["sdf_grad_ms"] = round(kernel_median_ms("nerf_sdf_grad", grad_call, args.reps), 4)
        ren.set_precision("fp32_exact")
        render_call = lambda: ren.render(cam[0], cam[1], cam[2], cam[3], style_r, S, N)      # noqa: E731
        for _ in range(3):
            render_call()
        out["render_exact_ms"] = round(kernel_median_ms("nerf_render", render_call, args.reps), 4)
        ren.set_precision("fp32")
        out["ratio"] = round(out["sdf_grad_ms"] / out["render_exact_ms"], 3)
        out["expected_ratio"] = round(4.0 * (D - 1) / D, 3)
        out["reps"] = args.reps
    if args.loss:
        out["loss"] = loss_report(ren, cam, style_r, S, N, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
