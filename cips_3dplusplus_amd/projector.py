"""Flip-inversion optimisation loop over the HIP forward + backward (BASELINE config 5).

Follows `StyleGAN2Projector_Flip.project_wplus` of /root/reference/exp/cips3d/models/projector_v10.py:915-1280:
three Adam optimisers (camera angles; NeRF W+ styles; decoder W+ styles + decoder parameters [+ noise buffers]), the
cosine ramp-down / linear ramp-up learning-rate multiplier (:174-186), a pose phase with the decoder frozen (lr 0),
an appearance phase that starts from the truncated NeRF style and flips the decoder styles of the (image, mirrored
image) pair every `flip_w_decoder_every` steps, and the noise regulariser (:1179-1192).  The batch is the image and its
horizontal flip rendered from mirrored azimuths.

The loss is a callable `loss_fn(rgb, thumb)`.  `perceptual_loss` is the reference's (:980-982, 1170-1174): the VGG16 conv
features of the image batch and of the 64^2 thumbnail against fixed target features, on the HIP kernels of csrc/vgg.hip
(perceptual.VGG16ConvLoss; `vgg16_conv_random`, or the pretrained network when the user has its weights).  `surrogate_loss`
(MSE on `rgb` + `thumb_weight` x MSE on `thumb_rgb` against fixed targets) stays the default of the
benchmarks.  The other terms of the step loss (:1164-1200) are knobs of `project_wplus` with the reference's names and off
defaults: `mask_background` (`mask_blend`, :1164-1167), `mse_weight` + `target_images` (:1176-1181) and `optim_noise_bufs` +
`regularize_noise_weight` (`noise_regulariser`, :1183-1195); on the GPU the blend and the regulariser are one autograd node
each (csrc/inversion_loss.hip).  `ssim_weight` + `target_images` is not the reference's: ssim_weight x mean (1 - SSIM), the
Gaussian-window SSIM on continuous values as one more autograd node (`ssim_loss`, csrc/ssim_loss.hip).  `silhouette_weight` +
`target_masks` is not the reference's either: silhouette_weight x mean (mask - (1 - target_masks))^2 on the render's own mask map,
whose gradient the NeRF backward takes in its compositing kernel (`silhouette_loss`; autograd.NerfRenderFn).  `metrics_every` > 0 logs the PSNR and SSIM the reference charts (:1125-1139) and returns those of
the final re-render (:1229-1242, 1266-1279), computed on the device (metrics.MetricsLog, csrc/metrics.hip) and read once after the
loop.  What is NOT here: `use_stat_loss` / `vgg16_relu`; LPIPS; Streamlit charts and videos.

The three Adam optimisers of the reference run as `optim.HipAdam` (csrc/optim.hip: torch.optim.Adam's update rule, one
bandwidth-bound launch per 48 tensors; CIPS3D_HIP_ADAM=0: torch.optim.Adam, fused where torch offers it).
"""
import copy
import math
import os

import torch
from torch import nn

from .camera import Camera


def _adam(groups):
    """Adam over the given parameter groups: the HIP kernel (optim.HipAdam: torch.optim.Adam's update rule, one launch per 48
    tensors) for CUDA parameters; CIPS3D_HIP_ADAM=0: torch.optim.Adam (fused=True where torch offers it, CIPS3D_FUSED_ADAM=0:
    its default form)."""
    on_gpu = all(p.is_cuda and p.dtype == torch.float32 for g in groups for p in g["params"])
    if os.environ.get("CIPS3D_HIP_ADAM", "1") != "0" and on_gpu:
        from .optim import HipAdam
        return HipAdam(groups)
    if os.environ.get("CIPS3D_FUSED_ADAM", "1") != "0" and all(p.is_cuda for g in groups for p in g["params"]):
        try:
            return torch.optim.Adam(groups, fused=True)
        except (RuntimeError, TypeError):
            pass
    return torch.optim.Adam(groups)


def _all_hip_adam(opts):
    from .optim import HipAdam
    return len(opts) > 0 and all(isinstance(o, HipAdam) for o in opts)


def cur_lr(step, num_steps, initial_learning_rate=1.0, lr_rampdown_length=0.25, lr_rampup_length=0.05):
    """projector_v10.py:174-186."""
    t = step / num_steps
    ramp = min(1.0, (1.0 - t) / lr_rampdown_length)
    ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
    ramp = ramp * min(1.0, t / lr_rampup_length)
    return initial_learning_rate * ramp


def _scale_lr(opt, mul):
    for g in opt.param_groups:          # tl2 mul_optimizer_lr: lr = initial_lr * mul
        g["lr"] = g["initial_lr"] * mul


def _set_lr(opt, lr):
    for g in opt.param_groups:
        g["lr"] = lr


FUSED_NOISE_REG = os.environ.get("CIPS3D_FUSED_NOISE_REG", "1") != "0"      # 0: the torch expression (A/B knob)
FUSED_MASK_BLEND = os.environ.get("CIPS3D_FUSED_MASK_BLEND", "1") != "0"    # 0: the torch expression (A/B knob)


def _noise_regulariser_torch(noise_bufs):
    reg = 0
    for v in noise_bufs:
        noise = v
        while True:
            reg = reg + (noise * torch.roll(noise, shifts=1, dims=3)).mean() ** 2
            reg = reg + (noise * torch.roll(noise, shifts=1, dims=2)).mean() ** 2
            if noise.shape[2] <= 8:
                break
            noise = torch.nn.functional.avg_pool2d(noise, kernel_size=2)
    return reg


def noise_regulariser(noise_bufs, weight=1.0):
    """weight x projector_v10.py:1183-1195 (StyleGAN2's multi-scale autocorrelation penalty).  fp32 HIP buffers [B,1,S,S] whose
    pooled levels have even sides go through ONE autograd node for the whole list (autograd.NoiseRegFn, csrc/inversion_loss.hip:
    at most four launches forward, one backward, the weight folded in); anything else -- CPU tensors, other dtypes, odd sides,
    nothing that requires a gradient, CIPS3D_FUSED_NOISE_REG=0 -- is the torch expression."""
    noise_bufs = list(noise_bufs)
    if FUSED_NOISE_REG and len(noise_bufs) > 0 and any(b.requires_grad for b in noise_bufs):
        from . import hip
        if hip.noise_reg_supported(noise_bufs):
            from . import autograd as AG
            return AG.NoiseRegFn.apply(float(weight), *noise_bufs)
    reg = _noise_regulariser_torch(noise_bufs)
    return reg if weight == 1.0 else weight * reg


def _mask_blend_torch(rgb, mask):
    m = (1 - mask.detach()).expand(-1, rgb.shape[1], -1, -1)
    m = torch.nn.functional.interpolate(m, scale_factor=rgb.shape[-1] / m.shape[-1], recompute_scale_factor=False, mode="bicubic")
    return rgb * m + rgb.detach() * (1 - m)


def mask_blend(rgb, mask):
    """projector_v10.py:1164-1167 with the mask of `_G_forward` (:268-273): `rgb * m + rgb.detach() * (1 - m)` with m the bicubic
    up-sampling of 1 - mask (the render's foreground mask [B,1,h,w], detached) to rgb's resolution -- the image itself up to
    rounding, with the gradient g * m.  fp32 HIP tensors with an integer factor are one autograd node (autograd.MaskBlendFn: one
    launch each way, m evaluated per pixel and never written out); CPU tensors, other factors and CIPS3D_FUSED_MASK_BLEND=0 are
    the torch expression."""
    if FUSED_MASK_BLEND and rgb.is_cuda:
        from . import hip
        if hip.mask_blend_factor(rgb, mask) >= 1:
            from . import autograd as AG
            return AG.MaskBlendFn.apply(rgb, mask)
    return _mask_blend_torch(rgb, mask)


FUSED_LOSS = os.environ.get("CIPS3D_FUSED_LOSS", "1") != "0"      # 0: the torch expression (A/B knob)


def surrogate_loss(target_rgb, target_thumb, rgb_weight=1.0, thumb_weight=50.0):
    """rgb_weight mse(rgb, target) + thumb_weight mse(thumb, target_thumb): the structure of the reference's loss
    (projector_v10.py:1173-1178) on the images themselves.  On the GPU it is one autograd node (autograd.SqDiffPairFn)."""
    def loss(rgb, thumb):
        if (FUSED_LOSS and rgb.is_cuda and rgb.dtype == torch.float32 and thumb.dtype == torch.float32
                and rgb.shape == target_rgb.shape and thumb.shape == target_thumb.shape
                and not target_rgb.requires_grad and not target_thumb.requires_grad):
            from . import autograd as AG
            return AG.weighted_mse_pair(rgb, target_rgb.to(rgb.device, torch.float32), rgb_weight,
                                        thumb, target_thumb.to(thumb.device, torch.float32), thumb_weight)
        return rgb_weight * ((rgb - target_rgb) ** 2).mean() + thumb_weight * ((thumb - target_thumb) ** 2).mean()
    return loss


def _weighted_mse(rgb, target, weight):
    """weight x F.mse_loss(rgb, target) (projector_v10.py:1176-1179); on the GPU the squared-difference node with one tensor."""
    if FUSED_LOSS and rgb.is_cuda and rgb.dtype == torch.float32 and target.dtype == torch.float32 and rgb.shape == target.shape:
        from . import autograd as AG
        return AG.SqDiffPairFn.apply(rgb, target, weight / rgb.numel(), None, None, 0.0)
    return weight * torch.nn.functional.mse_loss(rgb, target)


FUSED_SSIM = os.environ.get("CIPS3D_FUSED_SSIM", "1") != "0"      # 0: the torch expression (A/B knob)


def ssim_loss(rgb, target, weight, data_range=2.0):
    """weight x mean_i (1 - ssim_i) with ssim the Gaussian-window SSIM of metrics.ssim_gaussian (Wang et al. 2004: 11 taps, sigma
    1.5, continuous values, data range 2 for images in [-1, 1]): the structural term people add to an inversion loss to get back
    the local contrast MSE blurs away.  Differentiable with respect to `rgb`.  fp32 HIP tensors with a target that needs no
    gradient are one autograd node (autograd.SsimLossFn, csrc/ssim_loss.hip: two launches forward, one backward); anything else
    -- CPU tensors, other dtypes, CIPS3D_FUSED_SSIM=0 -- is the torch expression."""
    from .metrics import _check_pair_gaussian, _ssim_gaussian_torch
    rgb, target = _check_pair_gaussian(rgb, target, data_range)
    if FUSED_SSIM and not target.requires_grad:
        from . import hip
        if hip.ssim_loss_supported(rgb, target):
            from . import autograd as AG
            return AG.SsimLossFn.apply(rgb, target, float(weight), float(data_range))
    return weight * (1 - _ssim_gaussian_torch(rgb, target, data_range)[0]).mean()


def silhouette_loss(mask, target_masks, weight):
    """weight x mean (mask - (1 - target_masks))^2: fits the render's silhouette to a segmentation.  `mask` is the generator's
    `ret["mask"]` [B,1,S,S] -- the weight of the last sample of every ray, i.e. the probability of the BACKGROUND
    (nerf_utils.py:333-336) -- and `target_masks` the FOREGROUND segmentation in [0, 1] at the same resolution, a constant.
    Differentiable with respect to `mask`, whose gradient the NeRF backward carries to the pose and the styles.  fp32 HIP tensors
    go through the squared-difference node (autograd.SqDiffPairFn); a loop forms 1 - target_masks once and calls `_weighted_mse`
    itself (project_wplus)."""
    return _weighted_mse(mask, 1 - target_masks.detach(), weight)


def eikonal_regulariser(renderer, cams, styles, eikonal_weight, minimal_surface_weight, img_size, N_samples, beta=100):
    """eikonal_weight x mean((|d sdf / d pts| - 1)^2) + minimal_surface_weight x mean(exp(-beta |sdf|)) of the renderer's SDF at the
    sample points of the cameras `cams` = (cam_poses [B,3,4], focals, near, far [B,1,1]; constants: detached here) on img_size^2
    rays x N_samples un-jittered samples: the reference's two geometry regularisers (exp/stylesdf/losses.py:13-24), which keep
    the SDF head a distance field while the image losses move `styles` ([1 | B, D+1, style_dim], the W+ styles of the point
    network).  One autograd node with one kernel call (VolumeFeatureRenderer.eikonal_loss with `weights`); differentiable with
    respect to `styles` only -- the renderer's own weights are constants of the node."""
    extr, focal, near, far = (t.detach() for t in cams[:4])
    return renderer.eikonal_loss(extr, focal, near, far, styles, img_size, N_samples, beta=beta,
                                 weights=(float(eikonal_weight), float(minimal_surface_weight)))[0]


def perceptual_loss(net, target_images, rgb_weight=1.0, thumb_weight=1.0, img_size=1024):
    """rgb_weight sum (fea(rgb) - fea(target))^2 + thumb_weight sum (fea(thumb) - fea(target_thumb))^2 with `net` a
    perceptual.VGG16ConvLoss (projector_v10.py:1170-1174).  The target features -- of `target_images` [B,3,S,S] in [-1, 1] and of
    their bicubic 64^2 thumbnails (`get_perceptual_fea`, :131-151, scale 64 / img_size) -- are computed once (:980-982).  Each of
    the two terms is one autograd node that never builds the concatenated feature vector."""
    taps_rgb, taps_thumb = net.get_perceptual_taps(target_images, img_size=img_size)

    def loss(rgb, thumb):
        return rgb_weight * net.loss(rgb, taps_rgb) + thumb_weight * net.loss(thumb, taps_thumb)
    return loss


class FlipProjector:
    def __init__(self, G, device="cuda"):
        self.G, self.device = G, device

    # ---- optimisers (projector_v10.py:279-390)
    def _cam_optimizer(self, optim_cam, lr_cam, azim_init, bs):
        """-> (locations [bs, 2] = (azim, elev) per view, optimiser).  The reference keeps azim and elev as two [bs, 1] parameters of
        one Adam group and concatenates them every step (projector_v10.py:279-300, 240-241); Adam is element-wise, so ONE [bs, 2]
        parameter takes exactly the same steps -- without the cat launch of every forward and the two slice copies its backward is.
        `azim` / `elev` of the returned dict and of `on_step` are its two columns."""
        loc = torch.zeros(bs, 2, device=self.device)
        loc[:, 0] = torch.tensor(azim_init[:bs], dtype=torch.float32)
        groups = []
        if optim_cam:
            loc = nn.Parameter(loc)
            groups.append({"params": [loc], "lr": lr_cam, "initial_lr": lr_cam, "betas": (0.9, 0.999)})
        return loc, _adam(groups) if groups else None

    def _free_cam_optimizer(self, optim_cam, lr_cam, bs, rot_init, trans_init, optim_fov, lr_fov, fov_init):
        """-> (pose [bs, 6] = (rot | trans) per view, fov [bs] | None, optimiser).  The reference keeps rot and trans as two [bs, 3]
        parameters of one Adam group (projector_axis_angle.py:260-278); as for (azim, elev) above, ONE [bs, 6] parameter takes
        the same element-wise steps.  Starts at rot = 0, trans = (0, 0, 1): the frontal look-at camera.  `fov` (optim_fov: a
        parameter in its own group at lr_fov) is the field of view in degrees per view."""
        pose = torch.zeros(bs, 6, device=self.device)
        pose[:, 5] = 1
        if rot_init is not None:
            pose[:, :3] = torch.as_tensor(rot_init, dtype=torch.float32).reshape(-1, 3).to(self.device)
        if trans_init is not None:
            pose[:, 3:] = torch.as_tensor(trans_init, dtype=torch.float32).reshape(-1, 3).to(self.device)
        groups, fov = [], None
        if optim_cam:
            pose = nn.Parameter(pose)
            groups.append({"params": [pose], "lr": lr_cam, "initial_lr": lr_cam, "betas": (0.9, 0.999)})
        if optim_fov:
            fov = nn.Parameter(torch.full((bs,), float(fov_init), device=self.device))
            groups.append({"params": [fov], "lr": lr_fov, "initial_lr": lr_fov, "betas": (0.9, 0.999)})
        return pose, fov, _adam(groups) if groups else None

    def _render_optimizer(self, G, mean_r, optim_render_w, lr_render_w, bs, optim_render_params=False):
        w = mean_r.detach().reshape(1, 1, -1).repeat(bs, G.N_layers_renderer + 1, 1).contiguous()
        groups = []
        if optim_render_w:
            w = nn.Parameter(w)
            groups.append({"params": [w], "lr": lr_render_w, "initial_lr": lr_render_w, "betas": (0.9, 0.999)})
        if optim_render_params:                          # projector_v10.py:866-872 (lr fixed at 1e-4 there)
            groups.append({"params": list(G.renderer.parameters()), "lr": 0.0001, "initial_lr": 0.0001, "betas": (0.9, 0.999)})
        return w, _adam(groups) if groups else None

    def _decoder_optimizer(self, G, mean_d, optim_decoder_w, optim_decoder_params, optim_noise_bufs, zero_noise_bufs,
                           lr_decoder_w, lr_decoder_params, lr_noise, bs, start_size):
        w = mean_d.detach().reshape(1, 1, -1).repeat(bs, G.decoder.n_latent, 1).contiguous()
        groups = []
        if optim_decoder_w:
            w = nn.Parameter(w)
            groups.append({"params": [w], "lr": lr_decoder_w, "initial_lr": lr_decoder_w, "betas": (0.9, 0.999)})
        if optim_decoder_params:
            groups.append({"params": list(G.decoder.parameters()), "lr": lr_decoder_params,
                           "initial_lr": lr_decoder_params, "betas": (0.9, 0.999)})
        noise_bufs = G.create_noise_bufs(start_size, self.device)
        if zero_noise_bufs:
            noise_bufs = [torch.zeros_like(b) for b in noise_bufs]
        if optim_noise_bufs:
            noise_bufs = [nn.Parameter(b) for b in noise_bufs]
            groups.append({"params": noise_bufs, "lr": lr_noise, "initial_lr": lr_noise, "betas": (0.9, 0.999)})
        return w, noise_bufs, _adam(groups) if groups else None

    def _cameras(self, cam_cfg, rot, trans=None, camera="look_at", fov=None, img_size=None):
        """(cam_poses, focals, near, far) of g_forward's camera arguments, at cam_cfg's img_size or at `img_size`."""
        cam_cfg = dict(cam_cfg)
        size = cam_cfg.pop("img_size")
        if img_size is not None:
            size = img_size
        cam_cfg = {k: v for k, v in cam_cfg.items() if k in ("fov_ang", "dist_radius")}
        if camera == "axis_angle":
            if fov is not None:
                cam_cfg["fov_ang"] = fov
            return Camera.free_camera_params(size, self.device, rot, trans, **cam_cfg)
        if camera == "look_at":
            return Camera.generate_camera_params(size, self.device, locations=rot if trans is None else torch.cat([rot, trans], 1),
                                                 **cam_cfg)[:4]
        raise ValueError(f"g_forward: camera must be 'look_at' or 'axis_angle', got {camera!r}")

    # ---- one generator call of the loop (projector_v10.py:211-277)
    def g_forward(self, G, style_render, style_decoder, noise_bufs, cam_cfg, nerf_cfg, rot, trans=None, flip_w_decoder=False,
                  camera="look_at", fov=None):
        """rot, trans: azimuth and elevation [B, 1] each -- or rot = the [B, 2] locations and trans = None.
        camera="axis_angle" (projector_axis_angle.py:190-203): rot [B, 3] an axis-angle vector, trans [B, 3] a position that is
        normalised onto the unit sphere, fov None (cam_cfg's) or the [B] field of view in degrees."""
        img_size = cam_cfg["img_size"]
        extr, focal, near, far = self._cameras(cam_cfg, rot, trans, camera, fov)
        if flip_w_decoder:
            style_decoder = style_decoder.detach().flip(dims=(0,))      # only the decoder parameters are updated
        r = G(zs=[None, None], style_render=style_render, style_decoder=style_decoder, cam_poses=extr, focals=focal,
              img_size=img_size, near=near, far=far, noise_bufs=noise_bufs, nerf_cfg=nerf_cfg, renderer_detach=False)
        return r["rgb"], r["thumb_rgb"], r["mask"]

    def project_wplus(self, cam_cfg, nerf_cfg, loss_fn, N_steps_pose=200, N_steps_app=0, optim_cam=True, optim_render_w=True,
                      optim_render_params=False, optim_decoder_w=True, optim_decoder_params=True, optim_noise_bufs=False, zero_noise_bufs=True,
                      bs_cam=2, bs_render=1, bs_decoder=2, lr_cam=0.02, lr_render_w=0.001, lr_decoder_w=0.01,
                      lr_decoder_params=0.005, lr_noise=0.001, truncation_psi=1.0, flip_w_decoder_every=10,
                      azim_init=(0.0, 0.0), w_avg_samples=10000, regularize_noise_weight=1e5, on_step=None,
                      mask_background=False, mse_weight=0.0, target_images=None, metrics_every=0, lpips_metric=None,
                      ssim_weight=0.0, silhouette_weight=0.0, target_masks=None, camera="look_at", optim_fov=False, lr_fov=0.05,
                      rot_init=None, trans_init=None, eikonal_weight=0.0, minimal_surface_weight=0.0, eikonal_img_size=None,
                      eikonal_every=1):
        """Returns the dict `checkpoint.save_inversion` writes (azim, elev, W+ styles, state dicts, noise).
        `camera`: "look_at" (the default: (azim, elev) of a look-at camera with a fixed up vector and field of view) or
        "axis_angle", the free camera of the reference's projector_axis_angle.py: per view an axis-angle rotation `rot` (start
        0, or rot_init [bs_cam, 3]) and a position `trans` (start (0, 0, 1), or trans_init; normalised onto the unit sphere in
        every forward, never in place), one Adam group at lr_cam -- it can follow an in-plane roll, which the look-at camera
        cannot.  `optim_fov` (free camera only) also optimises the field of view in degrees per view, in its own group at
        lr_fov, through the render's focal gradient.  In that mode the dict gains "rot", "trans" [bs_cam, 3], "fov" [bs_cam] and
        "cam_poses" [bs_cam, 3, 4] (the final poses), "azim" / "elev" are None, and `on_step` receives (step, loss, rot, trans).
        `mask_background`: from the appearance phase on, the image's gradient only flows where the render's foreground mask says
        so (mask_blend; the thumbnail is not blended, as in the reference).  `mse_weight` > 0 adds mse_weight x
        F.mse_loss(image, target_images) (projector_v10.py:1176-1181).  `ssim_weight` > 0 (needs `target_images`) adds
        ssim_weight x mean (1 - SSIM) of the same image -- after the mask blending -- against target_images (`ssim_loss`:
        Gaussian window, continuous values), between the MSE term and the regulariser; 0: nothing new runs.
        `silhouette_weight` > 0 (needs `target_masks`, the foreground segmentation [bs_cam, 1, S, S] in [0, 1] at the render's
        resolution S = cam_cfg["img_size"]; resizing is the caller's preprocessing, as for target_images) adds
        silhouette_weight x mean (mask - (1 - target_masks))^2 of the render's mask map (`silhouette_loss`) in both phases, after
        the SSIM term and before the regulariser: the term that moves the pose where the perceptual loss is flat in azimuth.  Its
        gradient enters the NeRF backward's compositing kernel (no further launch there).  0: nothing new runs.
        `metrics_every` > 0 (needs `target_images`): PSNR and SSIM (metrics.py: scikit-image's defaults on 8-bit images) of view 0
        of the generator's image, before the mask blending, against target_images[0], at the steps with step % metrics_every == 0
        and at the last one (the reference's logging condition, :1125-1139) -- two launches per logged step, no copy and no
        synchronisation inside the loop.  After the loop the image is rendered once more under no_grad at the optimised pose and
        styles (:1229-1242); the dict gains "psnr" and "ssim" of that image (floats, :1266-1279) and "metrics_history"
        ({"steps", "psnr", "ssim"} of the logged steps), all from one read.  0: nothing new runs and the dict has no new keys.
        `lpips_metric` (the reference's argument, :694-707, 1267-1280; needs `target_images`): a perceptual.LPIPS instance.  The
        final re-render's LPIPS of view 0 against target_images[0] becomes "lpips" (a float); with `metrics_every` > 0 the logged
        steps' values go to metrics_history["lpips"], enqueued beside the PSNR / SSIM launches (perceptual.LPIPSLog) and read
        once.  None: no network is built (the reference's default downloads one) and nothing changes.
        `eikonal_weight` / `minimal_surface_weight` > 0 add eikonal_weight x mean((|d sdf / d pts| - 1)^2) + minimal_surface_weight
        x mean(exp(-100 |sdf|)) of the point network's SDF (`eikonal_regulariser`, the reference's two geometry regularisers,
        exp/stylesdf/losses.py:13-24) in both phases, after the silhouette term and before the noise regulariser: the image
        losses alone do not keep the SDF head a distance field, which marching cubes, the normal maps and the texture atlas of
        an inverted subject assume.  The term uses the step's cameras, detached, and the step's `w_render`, on eikonal_img_size^2
        rays (default: cam_cfg["img_size"]; the focal follows the size, so a smaller value samples the same frustum more
        coarsely) x nerf_cfg["N_samples"] un-jittered samples, at the steps with step % eikonal_every == 0.  One autograd node,
        one kernel call; its gradient reaches `w_render` only, so it cannot be combined with `optim_render_params` (the
        renderer's own weights are constants of the node): ValueError.  Both 0: nothing new runs and the dict is unchanged."""
        if eikonal_weight < 0 or minimal_surface_weight < 0:
            raise ValueError(f"project_wplus: eikonal_weight and minimal_surface_weight must be non-negative, got {eikonal_weight}, "
                             f"{minimal_surface_weight}")
        if eikonal_every < 1 or int(eikonal_every) != eikonal_every:
            raise ValueError(f"project_wplus: eikonal_every must be a positive integer, got {eikonal_every}")
        eikonal_on = eikonal_weight > 0 or minimal_surface_weight > 0
        if eikonal_on and optim_render_params:
            raise ValueError("project_wplus: eikonal_weight / minimal_surface_weight > 0 cannot be combined with optim_render_params: "
                             "the renderer's own weights are constants of the eikonal node (it differentiates the styles only)")
        if eikonal_on and (eikonal_img_size is not None and (eikonal_img_size < 1 or int(eikonal_img_size) != eikonal_img_size)):
            raise ValueError(f"project_wplus: eikonal_img_size must be a positive integer, got {eikonal_img_size}")
        if camera not in ("look_at", "axis_angle"):
            raise ValueError(f"project_wplus: camera must be 'look_at' or 'axis_angle', got {camera!r}")
        if optim_fov and camera != "axis_angle":
            raise ValueError("project_wplus: optim_fov needs camera='axis_angle' (the look-at camera's field of view is fixed)")
        free = camera == "axis_angle"
        if mse_weight > 0 and target_images is None:
            raise ValueError("project_wplus: mse_weight > 0 needs target_images")
        if ssim_weight > 0 and target_images is None:
            raise ValueError("project_wplus: ssim_weight > 0 needs target_images")
        bg_target = None
        if silhouette_weight > 0:
            if target_masks is None:
                raise ValueError("project_wplus: silhouette_weight > 0 needs target_masks")
            want = (bs_cam, 1, cam_cfg["img_size"], cam_cfg["img_size"])
            if not torch.is_tensor(target_masks) or tuple(target_masks.shape) != want:
                raise ValueError(f"project_wplus: target_masks must be a tensor of shape {list(want)} (the render's resolution), got "
                                 f"{list(target_masks.shape) if torch.is_tensor(target_masks) else type(target_masks).__name__}")
            bg_target = (1 - target_masks.detach().to(self.device, torch.float32)).contiguous()      # formed once
        metrics_log = None
        if metrics_every < 0 or int(metrics_every) != metrics_every:
            raise ValueError(f"project_wplus: metrics_every must be a non-negative integer, got {metrics_every}")
        if metrics_every > 0:
            if target_images is None:
                raise ValueError("project_wplus: metrics_every > 0 needs target_images")
            from .metrics import MetricsLog
            n_logged = len([s for s in range(N_steps_pose + N_steps_app) if s % metrics_every == 0 or s == N_steps_pose + N_steps_app - 1])
            metrics_log = MetricsLog(target_images[0:1].detach().to(self.device), n_logged + 1)      # (+ 1: the final re-render)
        lpips_log = None
        if lpips_metric is not None:
            if target_images is None:
                raise ValueError("project_wplus: lpips_metric needs target_images")
            from .perceptual import LPIPS, LPIPSLog
            if not isinstance(lpips_metric, LPIPS):
                raise ValueError(f"project_wplus: lpips_metric must be a perceptual.LPIPS instance, got {type(lpips_metric).__name__}")
            n_logged = len([s for s in range(N_steps_pose + N_steps_app) if s % metrics_every == 0 or s == N_steps_pose + N_steps_app - 1]) \
                if metrics_every > 0 else 0
            lpips_log = LPIPSLog(lpips_metric, target_images[0:1].detach().to(self.device), n_logged + 1)
        if mse_weight > 0 or ssim_weight > 0:
            target_images = target_images.detach().to(self.device, torch.float32).contiguous()
        G = copy.deepcopy(self.G).eval().requires_grad_(False).to(self.device)
        if optim_render_params:                              # projector_v10.py:967-968
            G.renderer.requires_grad_(True)
        G.decoder.requires_grad_(True)
        with torch.no_grad():
            mean_r, mean_d = G.get_mean_latent(w_avg_samples, self.device)
        if free:
            loc, fov, opt_cam = self._free_cam_optimizer(optim_cam, lr_cam, bs_cam, rot_init, trans_init, optim_fov, lr_fov,
                                                         cam_cfg.get("fov_ang", 6))
            azim, elev = loc.detach()[:, :3], loc.detach()[:, 3:]        # (rot, trans: what on_step receives in this mode)
            cam_kw = lambda: dict(rot=loc[:, :3], trans=loc[:, 3:], camera="axis_angle", fov=fov)
        else:
            loc, opt_cam = self._cam_optimizer(optim_cam, lr_cam, list(azim_init), bs_cam)
            azim, elev = loc.detach()[:, 0:1], loc.detach()[:, 1:2]      # (views: they follow the optimiser's in-place updates)
            cam_kw = lambda: dict(rot=loc)
        one = torch.ones((), device=self.device)                         # d loss / d loss, allocated once (backward() would fill one per step)
        w_render, opt_render = self._render_optimizer(G, mean_r, optim_render_w, lr_render_w, bs_render, optim_render_params)
        w_decoder, noise_bufs, opt_dec = self._decoder_optimizer(
            G, mean_d, optim_decoder_w, optim_decoder_params, optim_noise_bufs, zero_noise_bufs, lr_decoder_w,
            lr_decoder_params, lr_noise, bs_decoder, cam_cfg["img_size"])
        opts = [o for o in (opt_cam, opt_render, opt_dec) if o is not None]
        N_steps = N_steps_pose + N_steps_app
        history = []
        for step in range(N_steps):
            if step < N_steps_pose:
                lr_mul = cur_lr(step, N_steps_pose)
            else:
                lr_mul = cur_lr(step - N_steps_pose, N_steps_app, lr_rampup_length=0.25)
            for o in opts:
                _scale_lr(o, lr_mul)
            flip_w_decoder = False
            if step < N_steps_pose:                      # camera + NeRF style; decoder frozen
                if opt_dec is not None:
                    _set_lr(opt_dec, 0)
            else:                                        # camera + decoder
                if step == N_steps_pose:
                    with torch.no_grad():
                        w_render.copy_(torch.lerp(mean_r.reshape(1, 1, -1).expand_as(w_render), w_render, truncation_psi))
                if (step + flip_w_decoder_every - 1) % flip_w_decoder_every == 0 and step != N_steps - 1:
                    flip_w_decoder = True
            # (one NeRF latent for both views, bs_render = 1: the generator broadcasts it inside the FiLM table's launch)
            rgb, thumb, mask = self.g_forward(
                G, w_render, w_decoder if w_decoder.shape[0] == 2 else w_decoder.repeat(2, 1, 1), noise_bufs, cam_cfg, nerf_cfg,
                flip_w_decoder=flip_w_decoder, **cam_kw())
            if metrics_log is not None and (step % metrics_every == 0 or step == N_steps - 1):
                metrics_log.update(step, rgb[0:1])
                if lpips_log is not None:
                    lpips_log.update(step, rgb[0:1])
            if mask_background and step >= N_steps_pose:
                rgb = mask_blend(rgb, mask)
            loss = loss_fn(rgb, thumb)                   # (term order of projector_v10.py:1200: perceptual + mse + regulariser)
            if mse_weight > 0:
                loss = loss + _weighted_mse(rgb, target_images, mse_weight)
            if ssim_weight > 0:
                loss = loss + ssim_loss(rgb, target_images, ssim_weight)
            if silhouette_weight > 0:
                loss = loss + _weighted_mse(mask, bg_target, silhouette_weight)
            if eikonal_on and step % eikonal_every == 0:
                with torch.no_grad():
                    cams = self._cameras(cam_cfg, img_size=eikonal_img_size, **cam_kw())
                loss = loss + eikonal_regulariser(G.renderer, cams, w_render, eikonal_weight, minimal_surface_weight,
                                                  int(eikonal_img_size or cam_cfg["img_size"]), int(nerf_cfg["N_samples"]))
            if optim_noise_bufs and regularize_noise_weight > 0:
                loss = loss + noise_regulariser(noise_bufs, regularize_noise_weight)
            for o in opts:
                o.zero_grad(set_to_none=True)
            loss.backward(one if loss.dim() == 0 and loss.dtype == one.dtype else None)
            if _all_hip_adam(opts):
                from .optim import step_many
                step_many(opts)                          # the three optimisers' tensors share launches
            else:
                for o in opts:
                    o.step()
            if on_step is not None:
                on_step(step, loss, azim, elev)
            else:
                history.append(loss.detach())
        out = {"azim": azim.clone(), "elev": elev.clone(), "w_render_opt": w_render.detach(),
               "w_decoder_opt": w_decoder.detach(), "render_state_dict": G.renderer.state_dict(),
               "decoder_state_dict": G.decoder.state_dict(), "noise_bufs": [b.detach() for b in noise_bufs], "padding": 0,
               "loss_history": torch.stack(history).cpu() if history else None, "G": G}
        if free:
            with torch.no_grad():
                cs = int(cam_cfg["img_size"])
                fov_out = fov.detach().clone() if fov is not None else torch.full((bs_cam,), float(cam_cfg.get("fov_ang", 6)),
                                                                                  device=self.device)
                poses = Camera.free_camera_params(cs, self.device, loc.detach()[:, :3], loc.detach()[:, 3:], fov_ang=fov_out,
                                                  dist_radius=cam_cfg.get("dist_radius", 0.12))[0]
            out.update({"azim": None, "elev": None, "rot": azim.clone(), "trans": elev.clone(), "fov": fov_out,
                        "cam_poses": poses})
        if metrics_log is not None or lpips_log is not None:
            with torch.no_grad():                        # projector_v10.py:1229-1242: the clean re-render at the optimised state
                proj_rgb, _, _ = self.g_forward(
                    G, w_render, w_decoder if w_decoder.shape[0] == 2 else w_decoder.repeat(2, 1, 1), noise_bufs, cam_cfg, nerf_cfg,
                    **cam_kw())
                if metrics_log is not None:
                    metrics_log.update(N_steps, proj_rgb[0:1])
                if lpips_log is not None:
                    lpips_log.update(N_steps, proj_rgb[0:1])
        if metrics_log is not None:
            res = metrics_log.result()                   # the single device-to-host read
            out["psnr"], out["ssim"] = float(res["psnr"][-1]), float(res["ssim"][-1])
            out["metrics_history"] = {"steps": res["steps"][:-1], "psnr": res["psnr"][:-1], "ssim": res["ssim"][:-1]}
        if lpips_log is not None:
            res = lpips_log.result()
            out["lpips"] = float(res["lpips"][-1])
            if metrics_log is not None:
                out["metrics_history"]["lpips"] = res["lpips"][:-1]
        return out
