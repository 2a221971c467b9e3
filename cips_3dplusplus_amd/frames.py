"""Frame panels on the device: Pillow's 8-bit resampling, bit for bit (csrc/frame_resample.hip), and what the demo pages build
from it -- the rgb | thumbnail | geometry panel of `_sample_multi_view_web` (render_video_web_v10.py:1825-1890:
`pil_utils.pil_resize` of the two small pictures, `merge_image_pil([...], nrow=3)`) and the inversion's target preprocessing
(`load_pil_crop_resize` with `Image.LANCZOS`, `StyleGAN2Projector_Flip._get_target_image`).

The definition is `PIL.Image.resize((ow, oh), resample)` on 8-bit images with the default `box` and `reducing_gap=None`
(Pillow's src/libImaging/Resample.c), channel by channel.  Per axis, input size I, output size O, filter support S_f
(box 0.5, bilinear 1, bicubic 2, lanczos 3):
    scale = I / O, fs = max(scale, 1), support = S_f fs, ksize = 2 ceil(support) + 1
    output xx: center = (xx + 0.5) scale, xmin = max(0, int(center - support + 0.5)),
               n = min(I, int(center + support + 0.5)) - xmin,  w_x = f((x + xmin - center + 0.5) (1 / fs)) for x < n,
               normalised by their sum in index order (all float64);  k = int(w 2^22 +- 0.5) (truncating)
    pixel = clamp((2^21 + sum_x p[xmin + x] k_x) >> 22, 0, 255) in int32; the horizontal pass first, its uint8 result is what the
    vertical pass reads; an axis whose size does not change is not filtered.
The coefficient tables are float64 work of the host (`resample_coeffs`: made once per (I, O, filter), uploaded once per device);
everything behind them is 32-bit integer arithmetic, so the device result has no tolerance: `_resize_u8_host`, the numpy
mirror that CPU tensors take, equals Pillow byte for byte (tests/test_frames_host.py) and the kernels equal the mirror
(tests/test_gpu_frames.py).  There is no eager-PyTorch route for device tensors.
"""
import math

import numpy as np
import torch

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
_SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}
PRECISION_BITS = 22               # Pillow's: 32 - 8 bits of result - 2 bits for the filters' over- and undershoot
ROUTES = ("auto", "fused", "two_launch")         # CIPS3D_RESAMPLE_*, in this order from 0


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x       # (libm's sin, as Pillow's C: not numpy's vectorised one)


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTER_FN = {"box": _box, "bilinear": _bilinear, "bicubic": _bicubic, "lanczos": _lanczos}
_HOST_TABLES, _DEV_TABLES = {}, {}


def _filter_name(resample):
    """'lanczos' / PIL.Image.LANCZOS / PIL.Image.Resampling.LANCZOS -> 'lanczos' (Pillow's numbers: 4 box, 2 bilinear, 3 bicubic,
    1 lanczos; 0 nearest and 5 hamming are not built)."""
    if isinstance(resample, str):
        name = resample.lower()
    else:
        name = {4: "box", 2: "bilinear", 3: "bicubic", 1: "lanczos"}.get(int(resample))
    if name not in FILTERS:
        raise ValueError(f"resample {resample!r}: one of {FILTERS}")
    return name


def ksize_of(in_size, out_size, resample):
    fs = max(in_size / out_size, 1.0)
    return 2 * int(math.ceil(_SUPPORT[_filter_name(resample)] * fs)) + 1


def _host_tables(in_size, out_size, name):
    key = (int(in_size), int(out_size), name)
    if key not in _HOST_TABLES:
        I, O = key[0], key[1]
        if I < 1 or O < 1:
            raise ValueError(f"resample {I} -> {O}: sizes must be positive")
        f = _FILTER_FN[name]
        scale = I / O
        fs = max(scale, 1.0)
        support = _SUPPORT[name] * fs
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / fs
        bounds = np.zeros((O, 2), np.int32)
        coeffs = np.zeros((O, ksize), np.int32)
        one = float(1 << PRECISION_BITS)
        for xx in range(O):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            n = min(int(center + support + 0.5), I) - xmin
            w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
            ww = 0.0
            for v in w:
                ww += v
            if ww != 0.0:
                w = [v / ww for v in w]
            bounds[xx] = (xmin, n)
            coeffs[xx, :n] = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w]
        _HOST_TABLES[key] = (bounds, coeffs)
    return _HOST_TABLES[key]


def resample_coeffs(in_size, out_size, resample="lanczos", device=None):
    """(bounds int32 [O, 2] = (xmin, n) per output index, coeffs int32 [O, ksize], zero behind n): Pillow's `precompute_coeffs`
    and `normalize_coeffs_8bpc`.  Host float64 work, done once per (I, O, filter); with a HIP `device` the tables are uploaded
    once per device, and the upload is complete before this returns, so any stream may read them afterwards."""
    name = _filter_name(resample)
    bounds, coeffs = _host_tables(in_size, out_size, name)
    dev = torch.device("cpu") if device is None else torch.device(device)
    if dev.type == "cpu":
        return torch.from_numpy(bounds.copy()), torch.from_numpy(coeffs.copy())
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    key = (int(in_size), int(out_size), name, dev)
    if key not in _DEV_TABLES:
        with torch.cuda.device(dev):
            t = (torch.from_numpy(bounds).to(dev), torch.from_numpy(coeffs).to(dev))
            torch.cuda.current_stream().synchronize()
        _DEV_TABLES[key] = t
    return _DEV_TABLES[key]


def _size2(size):
    if isinstance(size, (tuple, list)):
        oh, ow = int(size[0]), int(size[1])
    else:
        oh = ow = int(size)
    if oh < 1 or ow < 1:
        raise ValueError(f"size {size!r}: must be positive")
    return oh, ow


def _quantize_host(x):
    """cips3d_rgb_to_uint8's arithmetic in fp32: clamp to [-1, 1], (c + 1) 127.5, round to nearest even."""
    c = np.clip(np.asarray(x, np.float32), np.float32(-1), np.float32(1))
    return np.rint((c + np.float32(1)) * np.float32(127.5)).astype(np.uint8)


def _pass_host(a, in_size, out_size, name, axis):
    """One pass of the resampling along `axis` of a uint8 array: int32 multiply-adds, rounded, shifted, clamped."""
    bounds, coeffs = _host_tables(in_size, out_size, name)
    a = np.moveaxis(a, axis, -1)
    acc = np.full(a.shape[:-1] + (out_size,), 1 << (PRECISION_BITS - 1), np.int32)
    xmin = bounds[:, 0].astype(np.int64)
    for k in range(coeffs.shape[1]):
        idx = np.minimum(xmin + k, in_size - 1)              # (behind n the coefficient is 0)
        acc += a[..., idx].astype(np.int32) * coeffs[:, k]
    out = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis)


def _resize_u8_host(images, size, resample="lanczos"):
    """The mirror of the kernels on the host: [n, C, H, W] uint8 (or fp32 in [-1, 1], quantised first) CPU tensor or array ->
    [n, C, oh, ow] uint8 of the same kind, by the integer arithmetic of the module docstring."""
    name = _filter_name(resample)
    oh, ow = _size2(size)
    is_t = torch.is_tensor(images)
    a = images.detach().cpu().numpy() if is_t else np.asarray(images)
    if a.ndim != 4:
        raise ValueError("images: [n, C, H, W]")
    if a.dtype == np.float32:
        a = _quantize_host(a)
    elif a.dtype != np.uint8:
        raise TypeError(f"images: uint8 or float32, got {a.dtype}")
    H, W = a.shape[-2:]
    if ow != W:
        a = _pass_host(a, W, ow, name, 3)
    if oh != H:
        a = _pass_host(a, H, oh, name, 2)
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.copy()) if is_t else a


def tile():
    """(tile_h, tile_w) of the fused route's output tile and the rows it can stage (csrc/frame_resample.h)."""
    import ctypes as C
    from . import _lib
    th, tw, rows = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.load().cips3d_resample_tile(C.byref(th), C.byref(tw), C.byref(rows))
    return th.value, tw.value, rows.value


def resample_route(in_hw, out_hw, resample="lanczos"):
    """The route `resize_u8` takes for [.., H, W] -> [.., oh, ow]: 'fused' (both axes change, and the input rows and columns
    that an output tile reaches fit in LDS: one launch, the intermediate picture stays on chip) or 'two_launch' (everything
    else: horizontal, then vertical through a uint8 workspace; the pass of an axis that does not change is skipped).  Decided
    by the library (cips3d_resample_route), the one place that decides it."""
    from . import _lib
    H, W = _size2(in_hw)
    oh, ow = _size2(out_hw)
    name = _filter_name(resample)
    kx = ksize_of(W, ow, name) if ow != W else 0
    ky = ksize_of(H, oh, name) if oh != H else 0
    r = _lib.load().cips3d_resample_route(H, W, oh, ow, kx, ky)
    if r <= 0:
        raise RuntimeError(f"cips3d_resample_route({H}, {W}, {oh}, {ow}) failed ({r})")
    return ROUTES[r]


def resize_u8(images, size, resample="lanczos", out=None, route="auto"):
    """`PIL.Image.resize` of every channel of every image, on the tensor's device.  images: [n, C, H, W] uint8, or fp32 in
    [-1, 1] (quantised on load with `hip.rgb_to_uint8`'s arithmetic; the result equals resize_u8(hip.rgb_to_uint8(images))).
    size: int or (oh, ow).  Returns [n, C, oh, ow] uint8; `out` may be given: a uint8 tensor of that shape with unit stride in
    W and any other strides (a cell of a panel block, a slice of a rank's frame block) -- only its own bytes are written.
    `route`: 'auto', or 'fused' / 'two_launch' to force one where both axes change (same bytes).  CPU tensors take the numpy
    mirror."""
    name = _filter_name(resample)
    oh, ow = _size2(size)
    if images.dim() != 4:
        raise ValueError("images: [n, C, H, W]")
    if images.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"images: uint8 or float32, got {images.dtype}")
    n, C_, H, W = images.shape
    if out is not None:
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, C_, oh, ow) or out.device != images.device:
            raise ValueError(f"out: uint8 {(n, C_, oh, ow)} on {images.device}")
        if ow > 1 and out.stride(3) != 1:
            raise ValueError("out: unit stride in W")
    if not images.is_cuda:
        res = _resize_u8_host(images, (oh, ow), name)
        if out is None:
            return res
        out.copy_(res)
        return out
    import ctypes
    from . import _lib
    lib = _lib.load()
    if route not in ROUTES:
        raise ValueError(f"route {route!r}: one of {ROUTES}")
    src = images if (W <= 1 or images.stride(3) == 1) else images.contiguous()
    if out is None:
        out = torch.empty(n, C_, oh, ow, dtype=torch.uint8, device=images.device)
    if n * C_ == 0:
        return out
    dev = images.device
    bx = cx = by = cy = None
    kx = ky = 0
    if ow != W:
        bx, cx = resample_coeffs(W, ow, name, dev)
        kx = cx.shape[1]
    if oh != H:
        by, cy = resample_coeffs(H, oh, name, dev)
        ky = cy.shape[1]
    ws_bytes = lib.cips3d_resample_workspace_bytes(n, C_, H, W, oh, ow, kx, ky, ROUTES.index(route))
    if ws_bytes < 0:
        raise RuntimeError(f"resize_u8: route {route!r} cannot take {H}x{W} -> {oh}x{ow} ({name})")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(lib.cips3d_resample_u8(
            ptr(src), n, C_, H, W, src.stride(2), src.stride(1), src.stride(0),
            ptr(out), oh, ow, out.stride(2), out.stride(1), out.stride(0),
            ptr(bx), ptr(cx), kx, ptr(by), ptr(cy), ky, int(images.dtype == torch.float32),
            ptr(ws), ws_bytes, ROUTES.index(route), _lib.stream_ptr()), "cips3d_resample_u8")
    return out


def compose_panels(panels, size=None, resample="lanczos", nrow=None, out=None):
    """The demo's frame panel: every entry of `panels` ([n, 3, Hi, Wi], uint8 or fp32 in [-1, 1]; any channel count, the same
    in all) resized to `size` (int or (S_h, S_w); default: the first panel's size) and written into its cell of one uint8
    block [n, C, rows S_h, cols S_w]: left to right, `nrow` cells per row (default: all in one row), no padding between
    cells; the unused cells of a short last row are white (255).  A panel already at `size` is copied by the same kernel's
    unfiltered path; every cell is written straight into the block (`out`, if given, must be that block), no copy afterwards.
    tl2's `merge_image_pil` is not available to compare against, so its padding and its default filter could not be read:
    this is the paste of Pillow's resizes side by side with no padding, and the filter is the caller's (`pil_resize`'s
    LANCZOS by default)."""
    if not panels:
        raise ValueError("compose_panels: no panels")
    p0 = panels[0]
    n, C_ = p0.shape[0], p0.shape[1]
    if any(p.dim() != 4 or p.shape[0] != n or p.shape[1] != C_ or p.device != p0.device for p in panels):
        raise ValueError("compose_panels: panels must be [n, C, Hi, Wi] with the same n and C on one device")
    sh, sw = _size2(size) if size is not None else (p0.shape[2], p0.shape[3])
    cols = len(panels) if nrow is None else int(nrow)
    if cols < 1:
        raise ValueError("nrow must be positive")
    cols = min(cols, len(panels)) if nrow is None else cols
    rows = (len(panels) + cols - 1) // cols
    shape = (n, C_, rows * sh, cols * sw)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=p0.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != p0.device:
        raise ValueError(f"out: uint8 {shape} on {p0.device}")
    for i in range(rows * cols):
        r, c = divmod(i, cols)
        cell = out[:, :, r * sh:(r + 1) * sh, c * sw:(c + 1) * sw]
        if i < len(panels):
            resize_u8(panels[i], (sh, sw), resample, out=cell)
        else:
            cell.fill_(255)
    return out


def center_crop_resize(image_u8, out_size, resample="lanczos"):
    """`load_pil_crop_resize` without the file: the centred square crop of side s = min(H, W) (torchvision's `center_crop`:
    int(round((H - s) / 2)) from the top, the same from the left), resized to out_size^2 -- not resized at all when it already
    has that size.  image_u8: [n, C, H, W] or [C, H, W] uint8."""
    x = image_u8 if image_u8.dim() == 4 else image_u8[None]
    H, W = x.shape[-2:]
    s = min(H, W)
    top, left = int(round((H - s) / 2.0)), int(round((W - s) / 2.0))
    res = resize_u8(x[:, :, top:top + s, left:left + s], int(out_size), resample)
    return res if image_u8.dim() == 4 else res[0]


def target_images_from_u8(image_u8, out_size):
    """`StyleGAN2Projector_Flip._get_target_image` without the file reading: the picture ([3, H, W] or [1, 3, H, W] uint8),
    centre-cropped and LANCZOS-resized to out_size^2, as fp32 (v / 255 - 0.5) * 2, and its horizontal flip: [2, 3, S, S]."""
    x = image_u8 if image_u8.dim() == 4 else image_u8[None]
    if x.shape[0] != 1:
        raise ValueError("target_images_from_u8: one image")
    u8 = center_crop_resize(x, out_size, "lanczos")
    # the reference divides on the host (IEEE division); a device may divide by multiplying with a reciprocal, which differs in
    # the last bit for some of the 256 levels: the levels are computed on the host and looked up
    lut = (torch.arange(256, dtype=torch.float32) / 255 - 0.5) * 2
    img = lut.to(u8.device)[u8.long()]
    return torch.cat([img, img.flip(3)], 0)
