"""PSNR and SSIM of two image files on the GPU (cips_3dplusplus_amd/metrics.py: scikit-image's defaults for 8-bit images).

    python tools/image_metrics.py A.png B.png [--gray] [--time [--reps 11]] [--lpips VGG_PTH LIN_PTH] [--gaussian]
    python tools/image_metrics.py --size 1024 [--gray] [--time [--reps 11]]      (a seeded random pair, +-3 grey levels apart)

Both files are read with PIL as 8-bit RGB (`--gray`: as 8-bit luminance) and must have the same size.  The last stdout line is
one JSON object: {"psnr", "ssim", "sse", "size", "channels"}.  `--time` adds, for this image size, the median wall time (a
synchronise on both sides) of `metrics.image_metrics` on device-resident uint8 images (`gpu_ms`, its one read included) and of
the host route it replaces for an fp32 image -- `hip.rgb_to_uint8` -> `.cpu()` -> a float64 numpy / scipy SSIM (`host_ms`).
`--lpips VGG_PTH LIN_PTH` adds "lpips": LPIPS v0.1 (net = 'vgg') of the pair from torchvision's vgg16 checkpoint and the lpips
package's vgg.pth (perceptual.LPIPS; RGB only, both sides multiples of 16).  `--gaussian` adds "ssim_gaussian": the Gaussian-window
SSIM (metrics.ssim_gaussian: 11 taps, sigma 1.5, population covariance) of the images as continuous values x / 127.5 - 1 with
data range 2; with `--time` also its wall time, `gaussian_gpu_ms`."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from cips_3dplusplus_amd import hip, metrics


def host_route(fa, fb):
    """The float64 definition on the host, from fp32 device images."""
    from scipy.ndimage import uniform_filter
    a = hip.rgb_to_uint8(fa).cpu().numpy()[0].astype(np.float64)
    b = hip.rgb_to_uint8(fb).cpu().numpy()[0].astype(np.float64)
    C1, C2, out = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2, []
    for x, y in zip(a, b):
        f = lambda v: uniform_filter(v, size=7)[3:-3, 3:-3]           # noqa: E731
        ux, uy = f(x), f(y)
        vx, vy, vxy = (f(x * x) - ux * ux) * 49 / 48, (f(y * y) - uy * uy) * 49 / 48, (f(x * y) - ux * uy) * 49 / 48
        out.append((((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))).mean())
    return metrics.psnr_from_sse(float(((a - b) ** 2).sum()), a.size), float(np.mean(out))


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("a", nargs="?"); ap.add_argument("b", nargs="?")
    ap.add_argument("--size", type=int, default=0)
    ap.add_argument("--gray", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--lpips", nargs=2, metavar=("VGG_PTH", "LIN_PTH"))
    ap.add_argument("--gaussian", action="store_true")
    args = ap.parse_args()
    mode = "L" if args.gray else "RGB"
    if args.size > 0:
        rng = np.random.default_rng(0)
        base = rng.integers(0, 256, (args.size, args.size, 1 if args.gray else 3))
        imgs = [base.astype(np.uint8), np.clip(base + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8)]
    elif args.a and args.b:
        imgs = [np.asarray(Image.open(p).convert(mode)) for p in (args.a, args.b)]
    else:
        ap.error("two image files or --size N")
    if imgs[0].shape != imgs[1].shape:
        sys.exit(f"the images differ in size: {imgs[0].shape} and {imgs[1].shape}")
    ta, tb = (torch.from_numpy(np.ascontiguousarray(im.reshape(im.shape[0], im.shape[1], -1).transpose(2, 0, 1))).unsqueeze(0).cuda()
              for im in imgs)
    sse, ssim = metrics.image_sse_ssim(ta, tb)
    out = {"psnr": metrics.psnr_from_sse(int(sse[0]), ta[0].numel()), "ssim": float(ssim[0]), "sse": int(sse[0]),
           "size": [int(ta.shape[2]), int(ta.shape[3])], "channels": int(ta.shape[1])}
    if args.lpips:
        if args.gray:
            ap.error("--lpips needs RGB images")
        from cips_3dplusplus_amd.perceptual import LPIPS
        out["lpips"] = float(LPIPS("vgg", weights=args.lpips[0], lin_weights=args.lpips[1])(ta, tb)[0])
    if args.gaussian:
        ga, gb = ta.float() / 127.5 - 1.0, tb.float() / 127.5 - 1.0
        out["ssim_gaussian"] = float(metrics.ssim_gaussian(ga, gb)[0])
        if args.time:
            out["gaussian_gpu_ms"] = median_ms(lambda: metrics.ssim_gaussian(ga, gb), args.reps)
    if args.time:
        fa, fb = ta.float() / 127.5 - 1.0, tb.float() / 127.5 - 1.0
        out["gpu_ms"] = median_ms(lambda: metrics.image_metrics(ta, tb), args.reps)
        out["host_ms"] = median_ms(lambda: host_route(fa, fb), args.reps)
        out["host_ssim"] = host_route(fa, fb)[1]
    print(json.dumps(out))
