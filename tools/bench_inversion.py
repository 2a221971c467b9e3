"""BASELINE config 5: CompCars 256^2 generator + pose phase of the flip-inversion loop (steps/s).

    python tools/bench_inversion.py [--depth 6] [--steps 200] [--res 256] [--loss surrogate|vgg16_conv_random]
                                     [--vgg-precision fp32_exact|split_fp16]
                                     [--optim-noise-bufs] [--mask-background] [--mse-weight W] [--metrics-every K]
                                     [--lpips random] [--ssim-weight W] [--silhouette-weight W]
                                     [--camera look_at|axis_angle] [--optim-fov]
                                     [--eikonal-weight W] [--minimal-surface-weight W] [--eikonal-img-size S] [--eikonal-every K]

One step = forward (batch 2: image + mirrored view) + backward + three Adam steps over {azim, elev}, the NeRF W+ style and
(with lr 0 in this phase, as projector_v10.py:1074-1075 sets it) the decoder W+ / parameters.  Surrogate loss
(SURVEY 8d): MSE(rgb) + 50 MSE(thumb) against fixed random targets.  Random-init weights.
--loss vgg16_conv_random: the reference's VGG16 conv perceptual loss (projector.perceptual_loss) on a randomly initialised
VGG16 instead, against the features of the same random target images and of their bicubic thumbnails; --vgg-precision picks
the arithmetic of its convolutions (perceptual.VGG16ConvLoss(precision=...)).
--optim-noise-bufs: the noise buffers are optimised (random start) and the noise regulariser is part of the loss;
--mask-background: the image is mask-blended before the loss in every step (N_steps_pose = 0: the steps are appearance steps);
--mse-weight W: W x MSE against the target images is added.  CIPS3D_FUSED_NOISE_REG=0 / CIPS3D_FUSED_MASK_BLEND=0 run the torch
expressions of the first two instead of the HIP nodes (A/B).  With none of the three the run is what it was without them.
--metrics-every K: PSNR / SSIM of the image against the target are logged on the device every K steps (project_wplus's
`metrics_every`, metrics.MetricsLog); the JSON line gains the final re-render's "psnr" / "ssim" and the number of logged steps.
--lpips random: LPIPS against the target is reported too (project_wplus's `lpips_metric`: a perceptual.LPIPS('vgg_random') of
--vgg-precision; logged beside PSNR / SSIM with --metrics-every); the JSON line gains the final re-render's "lpips".
--ssim-weight W: W x mean (1 - SSIM) against the target images is added (project_wplus's `ssim_weight`: the Gaussian-window
SSIM node of csrc/ssim_loss.hip; CIPS3D_FUSED_SSIM=0 runs its torch expression instead, A/B).  0: the run is what it was.
--silhouette-weight W: W x mean (mask - (1 - target_masks))^2 of the render's mask map is added (project_wplus's
`silhouette_weight`); the target is the same generator's foreground (1 - mask) rendered once at another pose (azimuth +-0.35,
mean latent).  Its gradient goes through the mask map into the NeRF backward.  0: the run is what it was.
--camera axis_angle: the free camera (project_wplus's `camera`: an axis-angle rotation and a position on the unit sphere per
view, csrc/camera_free.hip, instead of (azim, elev)); --optim-fov also optimises the field of view through the render's focal
gradient (the camera chain's second instantiation).  The JSON line's config gains "camera" (and "optim_fov") in that mode;
look_at (default): the run is what it was.
--eikonal-weight W / --minimal-surface-weight W: the SDF regularisers of the point network are added (project_wplus's
`eikonal_weight`, `minimal_surface_weight`: csrc/nerf_eikonal.hip, one node on --eikonal-img-size^2 rays (default: the render's
64) every --eikonal-every steps; CIPS3D_FUSED_EIKONAL=0 runs the torch double backward instead, A/B).  Both 0: the run is what
it was."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs
from cips_3dplusplus_amd.projector import FlipProjector, perceptual_loss, surrogate_loss

ap = argparse.ArgumentParser()
ap.add_argument("--depth", type=int, default=6)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--n-samples", type=int, default=24)
ap.add_argument("--app-steps", type=int, default=0)
ap.add_argument("--loss", choices=("surrogate", "vgg16_conv_random"), default="surrogate")
ap.add_argument("--vgg-precision", choices=("fp32_exact", "split_fp16"), default="fp32_exact")
ap.add_argument("--optim-noise-bufs", action="store_true")
ap.add_argument("--mask-background", action="store_true")
ap.add_argument("--mse-weight", type=float, default=0.0)
ap.add_argument("--metrics-every", type=int, default=0)
ap.add_argument("--lpips", choices=("random",), default=None)
ap.add_argument("--ssim-weight", type=float, default=0.0)
ap.add_argument("--silhouette-weight", type=float, default=0.0)
ap.add_argument("--camera", choices=("look_at", "axis_angle"), default="look_at")
ap.add_argument("--optim-fov", action="store_true")
ap.add_argument("--eikonal-weight", type=float, default=0.0)
ap.add_argument("--minimal-surface-weight", type=float, default=0.0)
ap.add_argument("--eikonal-img-size", type=int, default=None)
ap.add_argument("--eikonal-every", type=int, default=1)
a = ap.parse_args()
dev = "cuda"
cfg = configs.ffhq_G_cfg(a.res, a.depth)
G = pkg.build_generator(cfg, dev, seed=0)
cam_cfg = {"img_size": 64, "fov_ang": configs.COMPCARS_CAM_CFG["fov_ang"], "dist_radius": configs.COMPCARS_CAM_CFG["dist_radius"]}
ncfg = {"N_samples": a.n_samples, "perturb": False, "static_viewdirs": True}
g = torch.Generator(device=dev).manual_seed(1)
t_rgb = torch.randn(2, 3, a.res, a.res, device=dev, generator=g).clamp(-1, 1)
t_thumb = torch.randn(2, 3, 64, 64, device=dev, generator=g).clamp(-1, 1)
if a.loss == "surrogate":
    loss_fn = surrogate_loss(t_rgb, t_thumb)
else:
    from cips_3dplusplus_amd.perceptual import VGG16ConvLoss
    net = VGG16ConvLoss(a.loss, generator=torch.Generator().manual_seed(2), precision=a.vgg_precision)
    assert net.precision == a.vgg_precision
    loss_fn = perceptual_loss(net, t_rgb, img_size=a.res)
proj = FlipProjector(G, dev)
marks = {}

def on_step(step, loss, azim, elev):
    if step == 4:                       # first steps: allocator warm-up, plan builds
        torch.cuda.synchronize(); marks["t0"] = time.perf_counter(); marks["s0"] = step
    marks["last"] = float(loss.detach()) if step % 50 == 0 else marks.get("last")

extra, knobs = {}, {}
if a.optim_noise_bufs:
    extra.update(optim_noise_bufs=True, zero_noise_bufs=False)
    knobs["optim_noise_bufs"] = True
if a.mse_weight > 0:
    extra.update(mse_weight=a.mse_weight, target_images=t_rgb)
    knobs["mse_weight"] = a.mse_weight
if a.ssim_weight > 0:
    from cips_3dplusplus_amd import projector as _P
    extra.update(ssim_weight=a.ssim_weight, target_images=t_rgb)
    knobs["ssim_weight"], knobs["fused_ssim"] = a.ssim_weight, _P.FUSED_SSIM
if a.silhouette_weight > 0:
    from cips_3dplusplus_amd.camera import Camera
    with torch.no_grad():
        mr, md = G.get_mean_latent(2000, dev)
        e, f, n, fa, _ = Camera.generate_camera_params(64, dev, locations=torch.tensor([[0.35, 0.0], [-0.35, 0.0]], device=dev),
                                                       fov_ang=cam_cfg["fov_ang"], dist_radius=cam_cfg["dist_radius"])
        t = G(zs=[None, None], style_render=mr.reshape(1, 1, -1).repeat(2, G.N_layers_renderer + 1, 1),
              style_decoder=md.reshape(1, 1, -1).repeat(2, G.decoder.n_latent, 1), cam_poses=e, focals=f, img_size=64, near=n,
              far=fa, nerf_cfg=ncfg)
        t_masks = (1 - t["mask"]).clone()
    extra.update(silhouette_weight=a.silhouette_weight, target_masks=t_masks)
    knobs["silhouette_weight"] = a.silhouette_weight
if a.metrics_every > 0:
    extra.update(metrics_every=a.metrics_every, target_images=t_rgb)
    knobs["metrics_every"] = a.metrics_every
if a.lpips:
    from cips_3dplusplus_amd.perceptual import LPIPS
    extra.update(lpips_metric=LPIPS("vgg_random", generator=torch.Generator().manual_seed(3), precision=a.vgg_precision),
                 target_images=t_rgb)
    knobs["lpips"] = a.lpips
if a.camera != "look_at" or a.optim_fov:
    extra.update(camera=a.camera, optim_fov=a.optim_fov)
    knobs["camera"] = a.camera
    if a.optim_fov:
        knobs["optim_fov"] = True
if a.eikonal_weight > 0 or a.minimal_surface_weight > 0:
    extra.update(eikonal_weight=a.eikonal_weight, minimal_surface_weight=a.minimal_surface_weight,
                 eikonal_img_size=a.eikonal_img_size, eikonal_every=a.eikonal_every)
    knobs.update(eikonal_weight=a.eikonal_weight, minimal_surface_weight=a.minimal_surface_weight,
                 eikonal_img_size=a.eikonal_img_size or 64, eikonal_every=a.eikonal_every,
                 fused_eikonal=os.environ.get("CIPS3D_FUSED_EIKONAL", "1") != "0")
n_pose, n_app = a.steps, a.app_steps
if a.mask_background:                   # the blend runs from the appearance phase on: time appearance steps
    extra.update(mask_background=True)
    knobs["mask_background"] = True
    n_pose, n_app = 0, a.steps + a.app_steps
if set(knobs) - {"metrics_every", "lpips", "ssim_weight", "fused_ssim", "silhouette_weight", "camera", "optim_fov", "eikonal_weight",
                   "minimal_surface_weight", "eikonal_img_size", "eikonal_every", "fused_eikonal"}:
    from cips_3dplusplus_amd import projector as _P
    knobs["fused_noise_reg"], knobs["fused_mask_blend"] = _P.FUSED_NOISE_REG, _P.FUSED_MASK_BLEND
out = proj.project_wplus(cam_cfg, ncfg, loss_fn, N_steps_pose=n_pose, N_steps_app=n_app,
                         w_avg_samples=2000, on_step=on_step, azim_init=(-1.0, 3.0), **extra)
torch.cuda.synchronize()
dt = time.perf_counter() - marks["t0"]
n = a.steps + a.app_steps - 1 - marks["s0"]
print(json.dumps({"metric": "flip-inversion steps/s (fwd + bwd + Adam, batch 2)", "value": n / dt, "unit": "steps/s",
                  "ms_per_step": dt / n * 1e3, "config": {"workload": f"compcars_r{a.res}_D{a.depth}_N{a.n_samples}_B2_pose_phase",
                  "steps": a.steps, "app_steps": a.app_steps, **knobs, **({} if a.loss == "surrogate" else {"loss": a.loss, "vgg_precision": a.vgg_precision})}, "dtype": "f32", "data": "synthetic",
                  **({"psnr": out["psnr"], "ssim": out["ssim"], "metrics_logged": len(out["metrics_history"]["steps"])} if a.metrics_every > 0 else {}),
                  **({"lpips": out["lpips"]} if a.lpips else {}),
                  "peak_mem_GB": torch.cuda.max_memory_allocated() / 2 ** 30}))
