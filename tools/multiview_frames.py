"""Writes the panels of a multi-view sequence -- rgb | thumbnail | geometry, the picture the reference's demo shows per frame
(render_video_web_v10.py:1825-1890) -- as PNG files, composed on the GPU (multiview.sample_multi_view(gather=(..., "panel")),
frames.compose_panels, csrc/frame_resample.hip); optionally the single panes too.  Text overlay and video encoding are not
done here.

    python tools/multiview_frames.py --out DIR [--res 1024] [--frames 8] [--view-mode yaw] [--resample lanczos] [--panes]
    python tools/multiview_frames.py --time [--rounds 7]

--time prints the figures of DESIGN.md section 11 (medians over --rounds, variants interleaved in one process):
  (a) the demo's panel, 1024^2 rgb + 64^2 fp32 thumbnail + 512^2 geometry -> 1024 x 3072, per frame: device time of
      compose_panels against the reference's way -- the three panes copied to the host, Pillow's resizes, the paste.  The
      second is HOST time (copy + Pillow on one core): a host time beside a device time, not two device times.
  (b) the fused route against the two-launch route, 64^2 -> 1024^2 and 512^2 -> 1024^2, 3 channels, lanczos.
  (c) sample_multi_view frames/s at 1024^2 (yaw, N = 128) with and without "panel" in `gather`.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cips_3dplusplus_amd as pkg  # noqa: E402
from cips_3dplusplus_amd import configs, frames  # noqa: E402
from cips_3dplusplus_amd.multiview import sample_multi_view  # noqa: E402

DEV = "cuda"


def sequence_setup(res, n_samples):
    G = pkg.build_generator(configs.ffhq_G_cfg(res, 2), DEV, seed=0)
    g = torch.Generator(device=DEV).manual_seed(4)
    zs = [torch.randn(1, 256, device=DEV, generator=g), torch.randn(1, 256, device=DEV, generator=g)]
    cam_cfg = {"img_size": 64, "fov_ang": configs.FFHQ_CAM_CFG["fov_ang"], "dist_radius": configs.FFHQ_CAM_CFG["dist_radius"]}
    ncfg = {"N_samples": n_samples, "perturb": False, "static_viewdirs": False}
    return G, zs, cam_cfg, ncfg, G.create_noise_bufs(64, DEV)


def device_us(fn, reps):
    """Median-ready device time of one fn() in us: `reps` calls between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def pillow_panel(panes_dev, size, flt):
    """The reference's way: panes to the host, Pillow's resize of each, the paste."""
    from PIL import Image
    code = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[flt]
    out = Image.new("RGB", (size * len(panes_dev), size))
    for i, p in enumerate(panes_dev):
        a = p[0].cpu()
        if a.dtype != torch.uint8:
            a = ((a.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8)
        im = Image.fromarray(np.ascontiguousarray(a.permute(1, 2, 0).numpy()), "RGB")
        if im.size != (size, size):
            im = im.resize((size, size), code)
        out.paste(im, (i * size, 0))
    return out


def time_all(a):
    g = torch.Generator(device=DEV).manual_seed(1)
    rgb = torch.randint(0, 256, (1, 3, 1024, 1024), device=DEV, generator=g, dtype=torch.uint8)
    thumb = 2 * torch.rand(1, 3, 64, 64, device=DEV, generator=g) - 1
    shaded = torch.randint(0, 256, (1, 3, 512, 512), device=DEV, generator=g, dtype=torch.uint8)
    panes = [rgb, thumb, shaded]
    block = torch.empty(1, 3, 1024, 3072, dtype=torch.uint8, device=DEV)
    got = frames.compose_panels(panes, resample="lanczos", out=block)
    ref = torch.from_numpy(np.asarray(pillow_panel(panes, 1024, "lanczos"))).permute(2, 0, 1)
    print(f"panel equals Pillow's: {int((got[0].cpu() != ref).sum())} differing bytes of {ref.numel()}")
    dev_t, host_t = [], []
    for _ in range(a.rounds):
        dev_t.append(device_us(lambda: frames.compose_panels(panes, resample="lanczos", out=block), 20))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pillow_panel(panes, 1024, "lanczos")
        host_t.append((time.perf_counter() - t0) * 1e6)
    print(f"(a) panel 1024x3072 per frame: device {statistics.median(dev_t):9.1f} us (compose_panels, 3 launches)   |   "
          f"host {statistics.median(host_t):9.1f} us (device-to-host copies + Pillow; HOST time)")
    for H in (64, 512):
        src = torch.randint(0, 256, (1, 3, H, H), device=DEV, generator=g, dtype=torch.uint8)
        out = torch.empty(1, 3, 1024, 1024, dtype=torch.uint8, device=DEV)
        assert torch.equal(frames.resize_u8(src, 1024, "lanczos", route="fused"), frames.resize_u8(src, 1024, "lanczos", route="two_launch"))
        t = {"fused": [], "two_launch": []}
        for _ in range(a.rounds):
            for r in t:
                t[r].append(device_us(lambda: frames.resize_u8(src, 1024, "lanczos", out=out, route=r), 20))
        print(f"(b) {H}^2 -> 1024^2 x 3 lanczos: fused {statistics.median(t['fused']):8.1f} us   two_launch "
              f"{statistics.median(t['two_launch']):8.1f} us")
    if a.no_sequence:
        return
    G, zs, cam_cfg, ncfg, nb = sequence_setup(1024, 128)
    variants = {"without panel": ("rgb", "thumb_rgb", "shaded"), "with panel": ("rgb", "thumb_rgb", "shaded", "panel")}
    run = lambda ga: sample_multi_view(G, cam_cfg, ncfg, zs, view_mode="yaw", N_frames=a.frames, truncation_ratio=0.5,   # noqa: E731
                                       N_samples=128, noise_bufs=nb, gather=ga)
    for ga in variants.values():
        run(ga)
        run(ga)
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, ga in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                run(ga)
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) / 3 / a.frames)
    for k, v in ts.items():
        print(f"(c) sample_multi_view 1024^2, gather rgb + thumb_rgb + shaded, {k:13s}: median {statistics.median(v) * 1e6:8.1f} us/frame "
              f"-> {1 / statistics.median(v):7.1f} frames/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--n-samples", type=int, default=128)
    ap.add_argument("--view-mode", default="yaw")
    ap.add_argument("--resample", default="lanczos", choices=frames.FILTERS)
    ap.add_argument("--panes", action="store_true", help="also write rgb, thumb_rgb and shaded of every frame")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-sequence", action="store_true", help="--time: skip (c)")
    a = ap.parse_args()
    if a.time:
        return time_all(a)
    if not a.out:
        ap.error("--out DIR (or --time)")
    from PIL import Image
    os.makedirs(a.out, exist_ok=True)
    G, zs, cam_cfg, ncfg, nb = sequence_setup(a.res, a.n_samples)
    names = ("rgb", "thumb_rgb", "shaded")
    out = sample_multi_view(G, cam_cfg, ncfg, zs, view_mode=a.view_mode, N_frames=a.frames, truncation_ratio=0.5, N_samples=a.n_samples,
                            noise_bufs=nb, gather=(names if a.panes else ()) + ("panel",), panel=names, panel_resample=a.resample)
    torch.cuda.synchronize()

    def save(t, path):
        Image.fromarray(np.ascontiguousarray(t.cpu().permute(1, 2, 0).numpy()), "RGB").save(path)

    for i in range(out["panel"].shape[0]):
        save(out["panel"][i], os.path.join(a.out, f"panel_{i:04d}.png"))
        if a.panes:
            for k in names:
                t = out[k][i:i + 1]
                save((t if t.dtype == torch.uint8 else frames.resize_u8(t, t.shape[-2:]))[0], os.path.join(a.out, f"{k}_{i:04d}.png"))
    print(f"wrote {out['panel'].shape[0]} panels of {tuple(out['panel'].shape[2:])} to {a.out}")


if __name__ == "__main__":
    main()
