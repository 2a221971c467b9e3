"""PSNR and SSIM of images on the GPU (csrc/metrics.hip), without leaving the stream.

The reference's `project_wplus` logs tl2's `sk_psnr` / `sk_ssim` of the projected image against the target every
`st_log_every` steps and once more after the last one (/root/reference/exp/cips3d/models/projector_v10.py:1125-1139,
1266-1279).  Those are thin wrappers over scikit-image; this module computes what scikit-image documents as the defaults of
`peak_signal_noise_ratio` and `structural_similarity` on 8-bit images:

* images are `[B, C, H, W]` (or `[C, H, W]`), C in {1, 3}, uint8 with data range R = 255; an fp32 image in [-1, 1] is
  quantised inside the kernel exactly as `hip.rgb_to_uint8` does (clamp, (c + 1) * 127.5, round to nearest even);
* PSNR = 10 log10(R^2 C H W / SSE) per image, SSE the integer sum of squared differences (SSE = 0: +inf);
* SSIM: win_size 7, uniform window, K1 = 0.01, K2 = 0.03, sample covariance (n - 1 = 48), the mean over the C (H - 6) (W - 6)
  windows that lie wholly inside the image (scikit-image crops the 3-pixel border, so its padding never matters); H or
  W < 7 raises ValueError, as scikit-image does.  The multi-scale variant is not built.

`ssim_gaussian` is the other published form (Wang et al. 2004; scikit-image's `gaussian_weights=True, sigma=1.5,
use_sample_covariance=False`) on CONTINUOUS fp32 images -- nothing quantised, nothing clamped, 11-tap Gaussian window, data range
2 for images in [-1, 1] -- from csrc/ssim_loss.hip, whose other face is the differentiable loss `projector.ssim_loss`.

SSE is exact; SSIM is within (12 + d) 2^-24 of the float64 evaluation (d = 16, the depth of a tile's fp32 sum), and both are
bit-identical run to run and independent of the batch (tests/test_gpu_image_metrics.py).

`image_metrics` makes one device-to-host read.  `MetricsLog` makes none until `result()`: `update` enqueues two launches on
the current stream that write one row of a device-side record.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

WIN = 7
_DTYPES = (torch.float32, torch.uint8)


def psnr_from_sse(sse, numel):
    """10 log10(255^2 numel / sse) in float64, elementwise: `sse` an integer (or a tensor / array of them) over `numel` values
    per image; sse = 0 -> +inf."""
    s = np.asarray(sse.cpu() if isinstance(sse, torch.Tensor) else sse, dtype=np.float64)
    with np.errstate(divide="ignore"):
        out = 10.0 * np.log10(np.float64(65025.0 * numel) / s)
    return float(out) if s.ndim == 0 else torch.from_numpy(out)


def _as_batch(x, name):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(x).__name__}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4:
        raise ValueError(f"{name} must be [B, C, H, W] or [C, H, W], got {tuple(x.shape)}")
    if x.dtype not in _DTYPES:
        raise ValueError(f"{name} must be float32 (in [-1, 1]) or uint8, got {x.dtype}")
    return x


def _check_pair(a, b):
    """The argument errors of every entry point, raised before the library is touched. -> (a, b) as [B, C, H, W]."""
    a, b = _as_batch(a, "a"), _as_batch(b, "b")
    if a.shape != b.shape:
        raise ValueError(f"the images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    B, Cc, H, W = a.shape
    if B < 1:
        raise ValueError("an empty batch has no metrics")
    if Cc not in (1, 3):
        raise ValueError(f"images have 1 or 3 channels, got {Cc}")
    if H < WIN or W < WIN:
        raise ValueError(f"win_size {WIN} exceeds the image extent {H} x {W}")
    if a.device != b.device:
        raise ValueError(f"the images are on different devices: {a.device} and {b.device}")
    return a, b


def _require_hip(x):
    if not x.is_cuda:
        raise RuntimeError("image metrics run on HIP tensors (the cips3d HIP path has no CPU fallback)")


def tile():
    """(tile_h, tile_w, threads): the sides of a workgroup's tile of window origins and its thread count."""
    th, tw = C.c_int(0), C.c_int(0)
    threads = _lib.load().cips3d_image_metrics_tile(C.byref(th), C.byref(tw))
    return th.value, tw.value, threads


def _workspace(B, Cc, H, W, device):
    n = _lib.load().cips3d_image_metrics_workspace_bytes(B, Cc, H, W)
    if n < 0:
        raise RuntimeError(f"cips3d_image_metrics_workspace_bytes({B}, {Cc}, {H}, {W}) failed ({n})")
    return torch.empty(n // 8, dtype=torch.int64, device=device)


def _launch(a, b, workspace, record, row):
    """Two launches on the current stream: the metrics of a[i] against b[i] into record[row + i].  No copy, no synchronisation."""
    lib = _lib.load()
    a, b = a.contiguous(), b.contiguous()
    B, Cc, H, W = a.shape
    _lib.check(lib.cips3d_image_metrics(_lib.dev_ptr(a, "a", dtype=a.dtype), int(a.dtype == torch.uint8),
                                        _lib.dev_ptr(b, "b", dtype=b.dtype), int(b.dtype == torch.uint8), B, Cc, H, W,
                                        _lib.dev_ptr(workspace, "workspace", dtype=torch.int64),
                                        _lib.dev_ptr(record, "record", dtype=torch.int64), row, _lib.stream_ptr()),
                "cips3d_image_metrics")


def _read(record, numel):
    """The single device-to-host read: record [n, 2] int64 -> (sse int64 [n], psnr float64 [n], ssim float64 [n]) on the CPU."""
    rec = record.cpu()
    sse = rec[:, 0].contiguous()
    ssim = rec[:, 1].contiguous().view(torch.float64)
    return sse, psnr_from_sse(sse, numel), ssim


def image_sse_ssim(a, b):
    """-> (sse int64 [B], ssim float64 [B]) on the CPU: the two numbers the kernel writes per image."""
    a, b = _check_pair(a, b)
    _require_hip(a)
    B, Cc, H, W = a.shape
    record = torch.empty(B, 2, dtype=torch.int64, device=a.device)
    _launch(a, b, _workspace(B, Cc, H, W, a.device), record, 0)
    sse, _, ssim = _read(record, Cc * H * W)
    return sse, ssim


def image_metrics(a, b):
    """-> (psnr [B], ssim [B]) as float64 CPU tensors, image by image, at scikit-image's defaults for 8-bit images (module
    docstring).  a, b: [B, C, H, W] or [C, H, W] HIP tensors, each float32 in [-1, 1] or uint8."""
    sse, ssim_ = image_sse_ssim(a, b)
    return psnr_from_sse(sse, int(np.prod(a.shape[-3:]))), ssim_


def psnr(a, b):
    return image_metrics(a, b)[0]


def ssim(a, b):
    return image_metrics(a, b)[1]


class MetricsLog:
    """PSNR / SSIM of a sequence of images against one target, kept on the device until `result()`.

    `target`: [1, C, H, W] or [C, H, W], float32 in [-1, 1] or uint8; `capacity`: rows of the record.  `update(step, image)`
    enqueues the two launches on the current stream and returns at once -- no device-to-host copy, no synchronisation -- so it
    can sit inside an optimisation loop; `result()` makes the single read."""

    def __init__(self, target, capacity):
        target = _as_batch(target, "target")
        if target.shape[0] != 1:
            raise ValueError(f"target must be one image, got a batch of {target.shape[0]}")
        _check_pair(target, target)
        if int(capacity) < 1:
            raise ValueError(f"capacity must be at least 1, got {capacity}")
        self.target = target.detach().contiguous()
        self.capacity = int(capacity)
        self.steps = {}                      # row -> step, in the order of the updates
        self._record = None                  # (allocated with the first update: argument errors never touch the device)
        self._workspace = None

    def _next_row(self):
        for row in range(self.capacity):
            if row not in self.steps:
                return row
        raise ValueError(f"the record is full ({self.capacity} rows)")

    def update(self, step, image, row=None):
        """Record the metrics of `image` (one image of the target's shape) under `step`, in the next free row or in `row`."""
        image = _as_batch(image, "image")
        image, _ = _check_pair(image, self.target)
        row = self._next_row() if row is None else int(row)
        if not 0 <= row < self.capacity:
            raise ValueError(f"row {row} is outside the record ({self.capacity} rows)")
        _require_hip(image)
        if self._record is None:
            _, Cc, H, W = self.target.shape
            self._record = torch.zeros(self.capacity, 2, dtype=torch.int64, device=self.target.device)
            self._workspace = _workspace(1, Cc, H, W, self.target.device)
        _launch(image.detach(), self.target, self._workspace, self._record, row)
        self.steps.pop(row, None)            # (a row written again moves to the end of the order)
        self.steps[row] = int(step)
        return row

    def result(self):
        """-> {"steps": [..], "psnr": float64 [n], "ssim": float64 [n]} of the rows written, in the order of the updates."""
        rows = list(self.steps)
        if not rows:
            return {"steps": [], "psnr": torch.empty(0, dtype=torch.float64), "ssim": torch.empty(0, dtype=torch.float64)}
        _, psnr_, ssim_ = _read(self._record, self.target[0].numel())
        idx = torch.tensor(rows)
        return {"steps": [self.steps[r] for r in rows], "psnr": psnr_[idx], "ssim": ssim_[idx]}


# ------------------------------------------------------------------------------------ Gaussian-window SSIM (csrc/ssim_loss.hip)
GAUSS_WIN, GAUSS_SIGMA = 11, 1.5


def gaussian_window(dtype=torch.float64, device="cpu"):
    """The 11 taps g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 (computed in float64)."""
    d = torch.arange(GAUSS_WIN, dtype=torch.float64) - GAUSS_WIN // 2
    g = torch.exp(-(d * d) / (2.0 * GAUSS_SIGMA ** 2))
    return (g / g.sum()).to(device=device, dtype=dtype)


def _check_pair_gaussian(a, b, data_range=2.0):
    """The argument errors of the Gaussian-window SSIM, raised before the library is touched. -> (a, b) as [B, C, H, W]."""
    for x, name in ((a, "a"), (b, "b")):
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"{name} must be a tensor, got {type(x).__name__}")
        if not x.is_floating_point():
            raise ValueError(f"{name} must be a floating-point image, got {x.dtype}")
    if a.dim() == 3:
        a = a.unsqueeze(0)
    if b.dim() == 3:
        b = b.unsqueeze(0)
    if a.dim() != 4:
        raise ValueError(f"a must be [B, C, H, W] or [C, H, W], got {tuple(a.shape)}")
    if a.shape != b.shape:
        raise ValueError(f"the images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    B, Cc, H, W = a.shape
    if B < 1:
        raise ValueError("an empty batch has no metrics")
    if Cc not in (1, 3):
        raise ValueError(f"images have 1 or 3 channels, got {Cc}")
    if H < GAUSS_WIN or W < GAUSS_WIN:
        raise ValueError(f"win_size {GAUSS_WIN} exceeds the image extent {H} x {W}")
    if a.device != b.device:
        raise ValueError(f"the images are on different devices: {a.device} and {b.device}")
    if not data_range > 0:
        raise ValueError(f"data_range must be positive, got {data_range}")
    return a, b


def _ssim_gaussian_torch(a, b, data_range=2.0):
    """The definition as a plain torch expression (F.conv2d, groups = C), on any device and in a's dtype (fp64 included), with
    autograd: -> (ssim [B], S [B, C, H - 10, W - 10]).  The fallback of `ssim_gaussian` / `projector.ssim_loss` and the A/B
    partner of the kernels."""
    import torch.nn.functional as F
    Cc = a.shape[1]
    b = b.to(a.dtype)
    g = gaussian_window(a.dtype, a.device)
    wr, wc = g.reshape(1, 1, 1, -1).repeat(Cc, 1, 1, 1), g.reshape(1, 1, -1, 1).repeat(Cc, 1, 1, 1)

    def E(x):
        return F.conv2d(F.conv2d(x, wr, groups=Cc), wc, groups=Cc)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = E(a), E(b)
    vx, vy, vxy = E(a * a) - mx * mx, E(b * b) - my * my, E(a * b) - mx * my
    S = ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return S.mean(dim=(1, 2, 3)), S


def ssim_gaussian(a, b, data_range=2.0, return_map=False):
    """Gaussian-window SSIM of a against b, image by image -> float64 [B] on the CPU (one device-to-host read); with
    `return_map` also S per window, [B, C, H - 10, W - 10] on the images' device.  a, b: [B, C, H, W] or [C, H, W], C in {1, 3},
    continuous values (no quantisation, no clamp).  fp32 HIP tensors run csrc/ssim_loss.hip; anything else is the torch
    expression."""
    a, b = _check_pair_gaussian(a, b, data_range)
    from . import hip
    if hip.ssim_loss_supported(a, b):
        _, ssim_, _, smap = hip.ssim_loss(a.detach().contiguous(), b.detach().contiguous(), 1.0, data_range, return_map=return_map)
        ssim_ = ssim_.cpu()
    else:
        with torch.no_grad():
            ssim_, smap = _ssim_gaussian_torch(a, b, data_range)
        ssim_ = ssim_.double().cpu()
    return (ssim_, smap) if return_map else ssim_
