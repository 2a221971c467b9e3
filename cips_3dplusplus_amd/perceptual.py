"""VGG16 conv perceptual loss of flip inversion on the HIP kernels of csrc/vgg.hip and csrc/vgg_split.hip.

Follows `VGG16ConvLoss` of exp/cips3d/models/vgg_per_loss.py:203-334 (arguments, defaults, the `layers` property, the four
`loss_weight` tables, `forward` = the weighted, flattened, concatenated taps) and `get_perceptual_fea` of
models/projector_v10.py:131-151.  The network is torchvision's vgg16.features: 13 3x3 convolutions with ReLU, four max-pools,
taps at PRE-ReLU conv outputs (`features_N` = the output of `features.N`).

    net = VGG16ConvLoss('vgg16_conv_random')                 # Kaiming-normal fan_out weights, zero bias (vgg_per_loss.py:138-143)
    net = VGG16ConvLoss('vgg16_conv', weights='vgg16-397923af.pth')      # a torchvision state dict the user has
    t = net.taps(target)                                     # constants of the loss, computed once
    loss = net.loss(x, t)                                    # ONE autograd node: sum_k w_k^2 sum (f_k(x) - t_k)^2

`precision="fp32_exact"` (the default) runs every product on the fp32 matrix instruction; `precision="split_fp16"` runs convs
1 .. 12 and their data gradients on three fp16 products per fp32 product (csrc/vgg_split.hip: fp32-accurate, several times
faster, not bit-equal to the exact mode).  The mode belongs to the net: every method works in both.

`loss` never builds the concatenated vector (8.0 M floats per image at 256^2); `forward` does, for callers who want it.
There is no CPU path: tensors must live on the GPU.  `vgg16_relu` and `use_stat_loss` are not implemented.
"""
import ctypes as C

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function

from . import _lib, hip

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)       # vgg16.features.N of conv l
CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_BEFORE = (0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0)              # a 2x2/2 max-pool sits in front of conv l
TAP_CONV = {f"features_{n}": l for l, n in enumerate(CONV_INDEX)}   # tap name -> conv l
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
MODEL_NAMES = ("vgg16_relu", "vgg16_conv", "vgg16_conv_random")
PRECISIONS = ("fp32_exact", "split_fp16")


def conv_shapes(H, W, n_convs=13):
    """[(C_l, H_l, W_l)] of the outputs of convs 0 .. n_convs - 1 for an H x W input."""
    out = []
    for l in range(n_convs):
        if POOL_BEFORE[l]:
            H, W = H // 2, W // 2
        out.append((CHANNELS[l], H, W))
    return out


def feature_length(H, W, layers):
    """Length of one sample's row of `forward` (sum_k C_k H_k W_k)."""
    shapes = conv_shapes(H, W)
    return sum(shapes[TAP_CONV[k]][0] * shapes[TAP_CONV[k]][1] * shapes[TAP_CONV[k]][2] for k in layers)


def random_weights(generator=None):
    """The reference's `vgg16_conv_random` initialisation (vgg_per_loss.py:138-143): kaiming_normal_(mode='fan_out',
    nonlinearity='relu') = N(0, 2 / (9 Cout)), zero bias; drawn from `generator` (None: torch's global one)."""
    ws, cin = [], 3
    for cout in CHANNELS:
        std = (2.0 / (cout * 9)) ** 0.5
        ws.append((torch.empty(cout, cin, 3, 3).normal_(0.0, std, generator=generator), torch.zeros(cout)))
        cin = cout
    return ws


def weights_from_state_dict(sd):
    """[(weight, bias)] of the 13 convs from a state dict in the torchvision layout `features.N.weight` / `features.N.bias`
    (N in CONV_INDEX); `classifier.*` and any other key is ignored.  A missing or mis-shaped entry raises."""
    ws, cin = [], 3
    for n, cout in zip(CONV_INDEX, CHANNELS):
        for suffix, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            key = f"features.{n}.{suffix}"
            if key not in sd:
                raise KeyError(f"VGG16 state dict has no '{key}' (expected the torchvision layout features.N.weight / .bias)")
            if tuple(sd[key].shape) != shape:
                raise ValueError(f"'{key}' has shape {tuple(sd[key].shape)}, expected {shape}")
        ws.append((sd[f"features.{n}.weight"].detach().float().clone(), sd[f"features.{n}.bias"].detach().float().clone()))
        cin = cout
    return ws


def split_pack_reference(w):
    """The operands `cips3d_vgg_split_pack` makes of one conv's [Cout,Cin,3,3] fp32 weights, restated in numpy: (fwd, bwd, e).
    e puts max|w| 2^-e in [2^14, 2^15); hi = fp16(w 2^-e), lo = fp16(w 2^-e - hi).  Both arrays are fp16 in the order the lanes
    of v_mfma_f32_16x16x32_f16 read, [M/16][K/32][tap][hi | lo][q][i][j] with m = 16 mt + i and k = 32 ks + 8 q + j: the forward
    form holds w[m][k][tap] (M = Cout, K = Cin), the data-gradient form w[k][m][8 - tap] (M = Cin, K = Cout)."""
    import numpy as np
    w = np.ascontiguousarray(w, dtype=np.float32)
    cout, cin = w.shape[:2]
    e = int(np.frexp(np.abs(w).max())[1]) - 1 - 14
    s = (w * np.float32(2.0 ** -e)).reshape(cout, cin, 9)
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float32)).astype(np.float16)

    def form(a):                     # a[m][k][tap]
        M, K = a.shape[:2]
        return a.reshape(M // 16, 16, K // 32, 4, 8, 9).transpose(0, 2, 5, 3, 1, 4)       # mt, ks, tap, q, i, j

    fwd = np.stack([form(hi), form(lo)], axis=3)
    bwd = np.stack([form(hi[:, :, ::-1].transpose(1, 0, 2)), form(lo[:, :, ::-1].transpose(1, 0, 2))], axis=3)
    return np.ascontiguousarray(fwd), np.ascontiguousarray(bwd), e


class _Run:
    """The buffers of one forward call: the io struct, the pre-ReLU tensors z_l it points at, everything it must keep alive."""
    __slots__ = ("io", "arg", "z", "keep", "shape")      # arg: the struct the C calls take (io itself, or the split io around it)


class _VGGLossFn(Function):
    @staticmethod
    def forward(ctx, x, net, targets, tap_w, normalize):
        run, loss = net._loss_forward(x, targets, tap_w, normalize)
        ctx.net, ctx.run = net, run
        return loss

    @staticmethod
    def backward(ctx, g):
        dx = ctx.net._loss_backward(ctx.run, g)
        return dx, None, None, None, None


class VGG16ConvLoss(nn.Module):
    def __init__(self, model_name="vgg16_conv", downsample_size=-1, use_stat_loss=False, layers=None, loss_w_dict=None,
                 weights=None, generator=None, precision="fp32_exact", **kwargs):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        self.precision = precision
        if model_name not in MODEL_NAMES:
            raise ValueError(f"model_name must be one of {MODEL_NAMES}, got {model_name!r}")
        if model_name == "vgg16_relu":
            raise NotImplementedError("vgg16_relu (taps behind the ReLUs) is not implemented; use vgg16_conv or vgg16_conv_random")
        if use_stat_loss:
            raise NotImplementedError("use_stat_loss=True is not implemented")
        self.model_name, self.downsample_size, self.use_stat_loss = model_name, downsample_size, False
        self._layers = list(self.layers if layers is None else layers)
        for k in self._layers:
            if k not in TAP_CONV:
                raise ValueError(f"unknown tap {k!r}: taps are the conv outputs {sorted(TAP_CONV, key=TAP_CONV.get)}")
        if sorted(set(self._layers), key=TAP_CONV.get) != self._layers:
            raise ValueError("layers must be distinct and in network order")
        self.n_convs = max(TAP_CONV[k] for k in self._layers) + 1       # only the layers up to the deepest tap run
        if model_name == "vgg16_conv_random":
            ws = random_weights(generator)
        else:
            if weights is None:
                raise RuntimeError(
                    "VGG16ConvLoss('vgg16_conv') needs the pretrained VGG16: pass weights= (a path to, or the state dict of, "
                    "torchvision's vgg16 checkpoint with features.N.weight / features.N.bias), or use "
                    "model_name='vgg16_conv_random' for the reference's randomly initialised network")
            sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") \
                else weights
            ws = weights_from_state_dict(sd)
        for n, (w, b) in zip(CONV_INDEX, ws):
            self.register_buffer(f"weight_{n}", w.contiguous())
            self.register_buffer(f"bias_{n}", b.contiguous())
        self.loss_w_dict = dict(self.loss_weight("vgg16_conv_1024") if loss_w_dict is None else loss_w_dict)
        self._packed = {}                # device -> (cips3d_vgg_ctx, the tensors it points at)

    # ---- the reference's tables (vgg_per_loss.py:248-295)
    @property
    def layers(self):
        if getattr(self, "_layers", None) is not None:
            return list(self._layers)
        return ["features_2", "features_7", "features_14", "features_21", "features_28"]

    def loss_weight(self, name):
        tables = {
            "vgg16_conv_1024": (0.0002, 0.0001, 0.0001, 0.0002, 0.0005),
            "vgg16_conv_256": (0.001, 0.0006, 0.0005, 0.0005, 0.001),
            "vgg16_relu_1024": (0.0006, 0.0004, 0.0004, 0.0007, 0.007),
            "vgg16_relu_256": (0.001, 0.001, 0.001, 0.002, 0.01),
        }
        if name not in tables:
            raise ValueError(f"no loss weight table {name!r}")
        return dict(zip(("features_2", "features_7", "features_14", "features_21", "features_28"), tables[name]))

    def conv_weights(self):
        """[(weight, bias)] of the convs, as loaded (torchvision layout order)."""
        return [(getattr(self, f"weight_{n}"), getattr(self, f"bias_{n}")) for n in CONV_INDEX]

    def state_dict_torchvision(self):
        """The weights back in the torchvision layout (features.N.weight / features.N.bias)."""
        sd = {}
        for n, (w, b) in zip(CONV_INDEX, self.conv_weights()):
            sd[f"features.{n}.weight"], sd[f"features.{n}.bias"] = w, b
        return sd

    # ---- device state
    def _ctx(self, device):
        key = (device.type, device.index)
        if key not in self._packed:
            lib = _lib.load()
            split = self.precision == "split_fp16"
            ctx, keep, srcs = (_lib.VggSplitCtx() if split else _lib.VggCtx()), [], (C.c_void_p * _lib.VGG_CONVS)()
            for l in range(self.n_convs):
                w, b = (t.to(device=device, dtype=torch.float32).contiguous() for t in self.conv_weights()[l])
                n = w.numel()
                fwd = torch.empty(n, device=device)
                bwd = torch.empty(n, device=device) if l > 0 else None
                keep += [w, b, fwd, bwd]
                srcs[l] = w.data_ptr()
                ctx.w_fwd[l], ctx.w_bwd[l], ctx.bias[l] = fwd.data_ptr(), (bwd.data_ptr() if l > 0 else None), b.data_ptr()
            with torch.cuda.device(device):
                if split:       # hi / lo fp16 halves take the bytes of the fp32 weights; the layers' maxima go with them
                    w_amax = torch.zeros(_lib.VGG_CONVS, device=device, dtype=torch.int32)
                    ctx.w_amax = w_amax.data_ptr()
                    keep += [None, w_amax, None, None]
                    _lib.check(lib.cips3d_vgg_split_pack(C.byref(ctx), srcs, self.n_convs, _lib.stream_ptr()),
                               "cips3d_vgg_split_pack")
                else:
                    _lib.check(lib.cips3d_vgg_pack(C.byref(ctx), srcs, self.n_convs, _lib.stream_ptr()), "cips3d_vgg_pack")
                torch.cuda.current_stream().synchronize()       # the fp32 sources are dropped below
            self._packed[key] = (ctx, [t for i, t in enumerate(keep) if i % 4 != 0])
        return self._packed[key][0]

    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"VGG16ConvLoss expects [B,3,H,W], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("VGG16ConvLoss runs on the GPU only (the cips3d HIP path has no CPU fallback)")
        hip.vgg_check_supported(x.shape[0], x.shape[2], x.shape[3])

    def _prepare(self, x):
        """-> (network input, normalize flag).  downsample_size > 0: the normalisation and the area down-sampling are torch
        plumbing in front of the first layer (vgg_per_loss.py:312-316), which then takes its input as it is."""
        x = x.float()
        if self.downsample_size > 0:
            mean = x.new_tensor(IMAGENET_MEAN).view(1, 3, 1, 1)
            std = x.new_tensor(IMAGENET_STD).view(1, 3, 1, 1)
            x = ((x + 1) / 2.0 - mean) / std
            return F.interpolate(x, size=(self.downsample_size, self.downsample_size), mode="area").contiguous(), 0
        return x.contiguous(), 1

    def _new_run(self, x, normalize):
        B, _, H, W = x.shape
        shapes = conv_shapes(H, W, self.n_convs)
        al = lambda n: (n + 63) // 64 * 64
        zn = [al(B * c * h * w) for c, h, w in shapes]
        pn = [al(B * shapes[l - 1][0] * shapes[l][1] * shapes[l][2]) for l in range(self.n_convs) if POOL_BEFORE[l]]
        buf = torch.empty(sum(zn) + sum(pn), device=x.device)
        run = _Run()
        if self.precision == "split_fp16":
            run.arg = _lib.VggSplitIO()
            io = run.arg.io                  # (a view of the struct inside run.arg)
            rng = torch.empty(int(_lib.load().cips3d_vgg_split_range_bytes(B)) // 4, device=x.device, dtype=torch.int32)
            run.arg.range = rng.data_ptr()
        else:
            run.arg = io = _lib.VggIO()
            rng = None
        io.x, io.B, io.H, io.W, io.n_convs, io.normalize = x.data_ptr(), B, H, W, self.n_convs, normalize
        off, run.z = 0, []
        for l, (c, h, w) in enumerate(shapes):
            zl = buf[off:off + B * c * h * w].view(B, c, h, w)
            io.z[l] = zl.data_ptr()
            run.z.append(zl)
            off += zn[l]
        for k, n in enumerate(pn):
            io.pooled[k] = buf.data_ptr() + 4 * off
            off += n
        run.io, run.keep, run.shape = io, [x, buf, rng], (B, H, W)
        return run

    def _call(self, name, x, run):
        """One C call of this net's precision mode: cips3d_vgg_<name> or cips3d_vgg_split_<name>."""
        fn = ("cips3d_vgg_split_" if self.precision == "split_fp16" else "cips3d_vgg_") + name
        with torch.cuda.device(x.device):
            _lib.check(getattr(_lib.load(), fn)(C.byref(self._ctx(x.device)), C.byref(run.arg), _lib.stream_ptr()), fn)

    def _features(self, x, normalize):
        self._check_input(x)
        run = self._new_run(x, normalize)
        self._call("features", x, run)
        return run

    def _tap_weights(self, loss_w_dict):
        d = self.loss_w_dict if loss_w_dict is None else loss_w_dict
        return [float(d[k]) for k in self._layers]

    def _loss_forward(self, x, targets, tap_w, normalize):
        self._check_input(x)
        run = self._new_run(x, normalize)
        io = run.io
        for k, t, w in zip(self._layers, targets, tap_w):
            l = TAP_CONV[k]
            if tuple(t.shape) != tuple(run.z[l].shape):
                raise RuntimeError(f"target of {k} has shape {tuple(t.shape)}, the tap is {tuple(run.z[l].shape)}")
            io.target[l] = _lib.dev_ptr(t, f"target of {k}")
            io.tap_w[l] = w
        lib = _lib.load()
        partial = torch.empty(int(lib.cips3d_vgg_partial_bytes()) // 8, device=x.device, dtype=torch.float64)
        loss = torch.empty((), device=x.device)
        io.partial, io.loss = partial.data_ptr(), loss.data_ptr()
        run.keep += [partial, list(targets)]
        self._call("loss_forward", x, run)
        return run, loss

    def _loss_backward(self, run, gloss):
        B, H, W = run.shape
        x = run.keep[0]
        gloss = gloss.detach().to(device=x.device, dtype=torch.float32).reshape(1).contiguous()
        g = torch.empty(2, B * 64 * H * W, device=x.device)
        dx = torch.empty_like(x)
        io = run.io
        io.gloss, io.dx = gloss.data_ptr(), dx.data_ptr()
        io.g[0], io.g[1] = g[0].data_ptr(), g[1].data_ptr()
        self._call("loss_backward", x, run)
        return dx

    # ---- public
    def taps(self, x):
        """The raw (unweighted) taps of x in [-1, 1], [B,C_k,H_k,W_k] each, in `layers` order; no gradient (targets)."""
        with torch.no_grad():
            xin, normalize = self._prepare(x)
            run = self._features(xin, normalize)
            return [run.z[TAP_CONV[k]].clone() for k in self._layers]

    def forward(self, x, *args, loss_w_dict=None, use_stat_loss=None, **kwargs):
        """x in [-1, 1], [B,3,H,W] -> [B, sum_k C_k H_k W_k]: every tap flattened (C,H,W), times its weight, concatenated in
        `layers` order (vgg_per_loss.py:318-334).  Not differentiable: the differentiable form is `loss`."""
        if use_stat_loss:
            raise NotImplementedError("use_stat_loss=True is not implemented")
        ws = self._tap_weights(loss_w_dict)
        return torch.cat([t.flatten(1) * w for t, w in zip(self.taps(x), ws)], dim=1)

    def loss(self, x, target_taps, loss_w_dict=None):
        """sum_k w_k^2 sum (tap_k(x) - target_taps[k])^2 = ((forward(x) - forward(target)) ** 2).sum() as one autograd node;
        differentiable with respect to x only (the targets are constants, the weights are frozen)."""
        if len(target_taps) != len(self._layers):
            raise RuntimeError(f"{len(self._layers)} target taps expected ({self._layers}), got {len(target_taps)}")
        xin, normalize = self._prepare(x)
        return _VGGLossFn.apply(xin, self, [t.detach() for t in target_taps], self._tap_weights(loss_w_dict), normalize)

    def _thumb(self, image, img_size):
        return F.interpolate(image, scale_factor=64 / img_size, recompute_scale_factor=False, mode="bicubic", align_corners=False)

    def get_perceptual_fea(self, image, image_thumb=None, img_size=1024, **kwargs):
        """(features, features_thumb) of an image in [-1, 1] and its 64^2 thumbnail (bicubic from `image` when not given):
        projector_v10.py:131-151."""
        if image.dim() == 3:
            image = image.unsqueeze(0)
        if image_thumb is None:
            image_thumb = self._thumb(image, img_size)
        return self(image, **kwargs), self(image_thumb, **kwargs)

    def get_perceptual_taps(self, image, image_thumb=None, img_size=1024):
        """The same pair as raw tap lists: the targets `loss` takes."""
        if image.dim() == 3:
            image = image.unsqueeze(0)
        if image_thumb is None:
            image_thumb = self._thumb(image, img_size)
        return self.taps(image), self.taps(image_thumb)


# ---------------------------------------------------------------------------------------------------------------------------
# LPIPS v0.1, net = 'vgg' (csrc/lpips.hip): the trunk above plus a head on the taps behind five ReLUs.
#
#     net = LPIPS('vgg', weights='vgg16-397923af.pth', lin_weights='vgg.pth')      # files the user has
#     net = LPIPS('vgg_random', generator=g)                                       # Kaiming convs, random lin weights >= 0
#     d = net(a, b)                                # float64 [B] on the CPU, one read
#     t = net.prepare(target);  d = net(x, t)      # the target's taps computed once; the same bits as net(x, target)
#
# The scaling layer of LPIPS, (x - shift) / scale on images in [-1, 1], is the trunk's own normalisation: 2 mean - 1 = shift and
# 2 std = scale with the ImageNet constants.  Not built: 'alex' / 'squeeze', the up-sampled spatial map (`spatial=True` returns
# the five maps at their own sizes), LPIPS as a differentiable loss.
LPIPS_CONVS = (1, 3, 6, 9, 12)                    # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
LPIPS_CHANNELS = tuple(CHANNELS[l] for l in LPIPS_CONVS)
LPIPS_NETS = ("vgg", "vgg_random", "alex", "squeeze")
_LPIPS_ROW = _lib.LPIPS_LAYERS + 1                # a record row: {total, layer 0 .. 4} float64


def lin_weights_from_state_dict(sd):
    """[lin_k [C_k]] fp32 from the lpips package's vgg.pth layout, `lin{k}.model.1.weight` of shape [1, C_k, 1, 1]; any other
    key is ignored.  A missing key or a wrong width raises."""
    out = []
    for k, c in enumerate(LPIPS_CHANNELS):
        key = f"lin{k}.model.1.weight"
        if key not in sd:
            raise KeyError(f"LPIPS lin state dict has no '{key}' (expected the lpips package's vgg.pth layout)")
        if tuple(sd[key].shape) != (1, c, 1, 1):
            raise ValueError(f"'{key}' has shape {tuple(sd[key].shape)}, expected {(1, c, 1, 1)}")
        out.append(sd[key].detach().float().reshape(c).clone())
    return out


def random_lin_weights(generator=None):
    """Non-negative lin weights rand(C_k) * 2 / C_k (mean 1 / C_k, so a layer's value stays of the order of 1)."""
    return [torch.rand(c, generator=generator) * (2.0 / c) for c in LPIPS_CHANNELS]


def _load_sd(obj):
    return torch.load(obj, map_location="cpu") if isinstance(obj, (str, bytes)) or hasattr(obj, "__fspath__") else obj


def _lpips_check_supported(B, H, W):
    code = _lib.load().cips3d_lpips_supported(int(B), int(H), int(W))
    if code != 0:
        raise ValueError(f"LPIPS: B = {B}, H = {H}, W = {W} is outside the size contract of the VGG16 trunk (B >= 1, H and W "
                         f"multiples of 16): {_lib.load().cips3d_strerror(code).decode()}")


def _lpips_image(x, name):
    """[B,3,H,W] or [3,H,W], fp32 in [-1, 1] or uint8 (x / 127.5 - 1, the pairing of metrics.py) -> [B,3,H,W] fp32 on the GPU."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(x).__name__}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{name} must be [B,3,H,W] or [3,H,W], got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{name} must be float32 (in [-1, 1]) or uint8, got {x.dtype}")
    _lpips_check_supported(x.shape[0], x.shape[2], x.shape[3])
    if not x.is_cuda:
        raise RuntimeError("LPIPS runs on the GPU only (the cips3d HIP path has no CPU fallback)")
    x = x.detach()
    if x.dtype == torch.uint8:
        x = x.float() / 127.5 - 1.0
    return x.contiguous()


class LPIPSTarget:
    """The five pre-ReLU taps of a prepared target ([Bt,C_k,H_k,W_k] on the device) and the image size they belong to."""
    __slots__ = ("taps", "shape")

    def __init__(self, taps, shape):
        self.taps, self.shape = taps, tuple(shape)


def lpips_layer_distance(za, zb, lin):
    """One layer of the head on given maps: za, zb [B,C,H,W] fp32 PRE-ReLU (the ReLU is applied on load), lin [C], C in {64,
    128, 256, 512} -> (map [B,1,H,W] fp32, mean [B] float64), both on the device; two launches, no synchronisation."""
    if za.dim() != 4 or za.shape != zb.shape:
        raise ValueError(f"za and zb must be [B,C,H,W] of one shape, got {tuple(za.shape)} and {tuple(zb.shape)}")
    B, Cc, H, W = za.shape
    if lin.numel() != Cc:
        raise ValueError(f"lin has {lin.numel()} weights for {Cc} channels")
    lib = _lib.load()
    lin = lin.reshape(Cc)
    pa, pb, pl = _lib.dev_ptr(za, "za"), _lib.dev_ptr(zb, "zb"), _lib.dev_ptr(lin, "lin")
    dmap = torch.empty(B, 1, H, W, device=za.device)
    mean = torch.empty(B, device=za.device, dtype=torch.float64)
    nbytes = int(lib.cips3d_lpips_partial_bytes(B))
    if nbytes < 0:
        raise RuntimeError(f"cips3d_lpips_partial_bytes({B}) failed ({nbytes})")
    partial = torch.empty(nbytes // 8, device=za.device, dtype=torch.float64)
    with torch.cuda.device(za.device):
        _lib.check(lib.cips3d_lpips_head(pa, pb, pl, B, Cc, H, W, dmap.data_ptr(), partial.data_ptr(), mean.data_ptr(),
                                         _lib.stream_ptr()), "cips3d_lpips_head")
    return dmap, mean


class LPIPS(nn.Module):
    def __init__(self, net="vgg", weights=None, lin_weights=None, generator=None, precision="fp32_exact"):
        super().__init__()
        if net not in LPIPS_NETS:
            raise ValueError(f"net must be one of {LPIPS_NETS}, got {net!r}")
        if net in ("alex", "squeeze"):
            raise NotImplementedError(f"LPIPS(net={net!r}) is not implemented: only the VGG16 form is built ('vgg', 'vgg_random')")
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        self.net, self.precision = net, precision
        if net == "vgg_random":
            self.trunk = VGG16ConvLoss("vgg16_conv_random", generator=generator, precision=precision)
            lins = random_lin_weights(generator)
        else:
            if weights is None or lin_weights is None:
                raise RuntimeError(
                    "LPIPS('vgg') needs two pretrained files: pass weights= (a path to, or the state dict of, torchvision's "
                    "vgg16 checkpoint with features.N.weight / features.N.bias) and lin_weights= (a path to, or the state dict "
                    "of, the lpips package's weights/v0.1/vgg.pth with lin{k}.model.1.weight), or use net='vgg_random' for a "
                    "randomly initialised network")
            self.trunk = VGG16ConvLoss("vgg16_conv", weights=weights, precision=precision)
            lins = lin_weights_from_state_dict(_load_sd(lin_weights))
        for k, w in enumerate(lins):
            self.register_buffer(f"lin_{k}", w.contiguous())
        self._lin_dev = {}                 # device -> the five lin tensors there

    def lin_weights(self):
        return [getattr(self, f"lin_{k}") for k in range(_lib.LPIPS_LAYERS)]

    def _lins(self, device):
        """The five lin vectors on `device`.  Copies are kept per device and made again when a buffer was replaced or written
        (load_state_dict, .to(), an in-place edit): the stamp is every buffer's (data_ptr, _version)."""
        key = (device.type, device.index)
        stamp = tuple((w.data_ptr(), w._version) for w in self.lin_weights())
        if key not in self._lin_dev or self._lin_dev[key][0] != stamp:
            self._lin_dev[key] = (stamp, [w.to(device=device, dtype=torch.float32).contiguous() for w in self.lin_weights()])
        return self._lin_dev[key][1]

    def _enqueue(self, x, target, record, row, partial, maps=None, run=None, heads_only=False):
        """The trunk on x ([2B,3,H,W]: a then b; with `target`, [B,3,H,W]) and the head, rows `row` .. of `record`.  Only
        enqueues: no host copy, no synchronisation.  `run`: the trunk's buffers of an earlier `_new_run(x, 1)` on this very x
        (None: allocated here); `heads_only`: the trunk is not run, `run` holds its maps already."""
        if run is None:
            run = self.trunk._new_run(x, 1)
        lio = _lib.LpipsIO()
        lio.heads_only = int(heads_only)
        lio.trunk = C.addressof(run.arg)
        B = x.shape[0] if target is not None else x.shape[0] // 2
        for k, w in enumerate(self._lins(x.device)):
            lio.lin[k] = w.data_ptr()
            if target is not None:
                lio.target[k] = target.taps[k].data_ptr()
            if maps is not None:
                lio.map[k] = maps[k].data_ptr()
        lio.partial, lio.record, lio.row, lio.B = partial.data_ptr(), record.data_ptr(), int(row), B
        lio.target_broadcast = int(target is not None and target.taps[0].shape[0] == 1 and B > 1)
        fn = "cips3d_lpips_split" if self.precision == "split_fp16" else "cips3d_lpips"
        with torch.cuda.device(x.device):
            _lib.check(getattr(_lib.load(), fn)(C.byref(self.trunk._ctx(x.device)), C.byref(lio), _lib.stream_ptr()), fn)

    def _partial(self, B, device):
        return torch.empty(int(_lib.load().cips3d_lpips_partial_bytes(B)) // 8, device=device, dtype=torch.float64)

    def _check_target(self, a, target):
        if not isinstance(target, LPIPSTarget):
            raise ValueError("the second argument must be an image tensor or the result of LPIPS.prepare")
        Bt, H, W = target.shape
        if (H, W) != tuple(a.shape[2:]):
            raise ValueError(f"the prepared target is {H} x {W}, the image {a.shape[2]} x {a.shape[3]}")
        if Bt not in (1, a.shape[0]):
            raise ValueError(f"the prepared target holds {Bt} images, the batch {a.shape[0]}")
        if target.taps[0].device != a.device:
            raise ValueError(f"the prepared target is on {target.taps[0].device}, the image on {a.device}")

    def prepare(self, target):
        """The target's five taps, computed once: `forward(image, prepared)` then runs the trunk on `image` alone and gives the
        bits of `forward(image, target)` (the trunk does not depend on the batch).  One image serves every sample of a batch."""
        t = _lpips_image(target, "target")
        with torch.no_grad():
            run = self.trunk._features(t, 1)
            return LPIPSTarget([run.z[l].clone() for l in LPIPS_CONVS], (t.shape[0], t.shape[2], t.shape[3]))

    def forward(self, a, b, return_layers=False, spatial=False):
        """LPIPS of a against b (an image batch like a, or `prepare(b)`): float64 [B] on the CPU through one read; with
        `return_layers` also the five layers' values [B, 5]; with `spatial` also the five distance maps [B,1,H_k,W_k] on the
        device, at their own sizes."""
        a = _lpips_image(a, "a")
        B, _, H, W = a.shape
        if isinstance(b, torch.Tensor):
            b = _lpips_image(b, "b")
            if a.shape != b.shape:
                raise ValueError(f"the images differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
            if a.device != b.device:
                raise ValueError(f"the images are on different devices: {a.device} and {b.device}")
            x, target = torch.cat([a, b], dim=0), None
        else:
            self._check_target(a, b)
            x, target = a, b
        maps = [torch.empty(B, 1, h, w, device=a.device) for _, h, w in (conv_shapes(H, W)[l] for l in LPIPS_CONVS)] \
            if spatial else None
        record = torch.empty(B, _LPIPS_ROW, device=a.device, dtype=torch.float64)
        self._enqueue(x, target, record, 0, self._partial(B, a.device), maps)
        rec = record.cpu()                          # the single device-to-host read
        out = (rec[:, 0].contiguous(),)
        if return_layers:
            out += (rec[:, 1:].contiguous(),)
        if spatial:
            out += (maps,)
        return out[0] if len(out) == 1 else out


class LPIPSLog:
    """LPIPS of a sequence of images against one target, kept on the device until `result()` (metrics.MetricsLog's pattern).

    `target`: [1,3,H,W] or [3,H,W], prepared once; the record, the scratch and the trunk's buffers are allocated here.
    `update(step, image)` copies the image into the log's own input buffer and enqueues the trunk and the head on the current
    stream, then returns -- no device-to-host copy, no synchronisation, no allocation for an fp32 image; `result()` makes the
    single read.  Updates belong on one stream (they share the buffers)."""

    def __init__(self, net, target, capacity):
        if not isinstance(net, LPIPS):
            raise ValueError(f"net must be an LPIPS instance, got {type(net).__name__}")
        if int(capacity) < 1:
            raise ValueError(f"capacity must be at least 1, got {capacity}")
        if isinstance(target, torch.Tensor) and target.dim() == 4 and target.shape[0] != 1:
            raise ValueError(f"target must be one image, got a batch of {target.shape[0]}")
        self.net, self.capacity = net, int(capacity)
        self.target = net.prepare(target)
        device = self.target.taps[0].device
        self.steps = {}                      # row -> step, in the order of the updates
        self._record = torch.zeros(self.capacity, _LPIPS_ROW, dtype=torch.float64, device=device)
        self._partial = net._partial(1, device)
        # the image's staging copy and the trunk's buffers, allocated once: an update never meets the allocator's slow path
        self._x = torch.empty(1, 3, self.target.shape[1], self.target.shape[2], device=device)
        self._run = net.trunk._new_run(self._x, 1)

    def _next_row(self):
        for row in range(self.capacity):
            if row not in self.steps:
                return row
        raise ValueError(f"the record is full ({self.capacity} rows)")

    def update(self, step, image, row=None):
        """Record the LPIPS of `image` (one image of the target's size) under `step`, in the next free row or in `row`."""
        image = _lpips_image(image, "image")
        if image.shape[0] != 1:
            raise ValueError(f"image must be one image, got a batch of {image.shape[0]}")
        self.net._check_target(image, self.target)
        row = self._next_row() if row is None else int(row)
        if not 0 <= row < self.capacity:
            raise ValueError(f"row {row} is outside the record ({self.capacity} rows)")
        self._x.copy_(image)                 # (device to device, on the current stream)
        self.net._enqueue(self._x, self.target, self._record, row, self._partial, run=self._run)
        self.steps.pop(row, None)            # (a row written again moves to the end of the order)
        self.steps[row] = int(step)
        return row

    def result(self):
        """-> {"steps": [..], "lpips": float64 [n], "lpips_layers": float64 [n, 5]} of the rows written, in update order."""
        rows = list(self.steps)
        if not rows:
            return {"steps": [], "lpips": torch.empty(0, dtype=torch.float64),
                    "lpips_layers": torch.empty(0, _lib.LPIPS_LAYERS, dtype=torch.float64)}
        rec = self._record.cpu()[torch.tensor(rows)]
        return {"steps": [self.steps[r] for r in rows], "lpips": rec[:, 0].contiguous(), "lpips_layers": rec[:, 1:].contiguous()}
