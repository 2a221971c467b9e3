"""Oracle and shared cases of the VGG16 conv perceptual loss tests (test_perceptual_host.py, test_gpu_perceptual.py).

The oracle is the network written with torch.nn.functional on the CPU -- conv2d(padding=1) / relu / max_pool2d(2) in the
order of torchvision's vgg16.features, which is what the reference's nn.Conv2d stack is (exp/cips3d/models/vgg_per_loss.py:
93-110, 312-334) -- evaluated in fp64 (the truth) and in fp32 (the yardstick e_32 of the accuracy rule).  Each case is
computed once per session and shared.
"""
import functools

import torch
import torch.nn.functional as F

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CHANNELS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_BEFORE = (0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0)
DEFAULT_LAYERS = ("features_2", "features_7", "features_14", "features_21", "features_28")
W_1024 = dict(zip(DEFAULT_LAYERS, (0.0002, 0.0001, 0.0001, 0.0002, 0.0005)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# the issue's cases: (B, H, W, layers or None = the default five)
CASES = {
    "smallest_16x16": (1, 16, 16, None),                                   # last map 1x1, all halo
    "thumb_2x64x64": (2, 64, 64, None),                                    # the thumbnail's real shape, maps 64 ... 4
    "nonsquare_2x80x48": (2, 80, 48, None),                                # wider than a tile, deep maps 5x3
    "cut_short_128x128": (1, 128, 128, ("features_2", "features_7")),      # many workgroups, the network cut short
    # taps that no max-pool follows: their gradient enters through the data-gradient conv's epilogue, not the pool backward
    "inner_taps_2x32x48": (2, 32, 48, ("features_0", "features_5", "features_12")),
}
INNER_W = {"features_0": 0.002, "features_5": 0.001, "features_12": 0.003}


def case_weights(layers):
    """The loss weights of a case: the reference's 1024 table for its taps, INNER_W for the others."""
    return {k: W_1024[k] if k in W_1024 else INNER_W[k] for k in layers}

# Accuracy rule (tests/test_gpu_split_fp16.py's form): e_hip <= M * e_32 + 2e-7 * range, with e_32 the error of torch's own fp32
# CPU evaluation against the fp64 evaluation of the same inputs.  The cap for M is 8: torch's default fp32 errs 2.3-6.9e-7 of the
# tap maximum at full VGG16 widths, a second legitimate fp32 summation order (permuted channels, channels-last) 0.5-2.5e-6, i.e.
# 2-5 x the default (gradient relative L2: 1.8-2.5e-7 against 2.7-6.6e-7).  The kernels' order is a third one (fmaf chains of 144
# products, folded after every 16-channel stage); measured on the MI355X over the five cases: taps 0.20-1.44 x e_32,
# gradient 0.11-3.11 x (max-abs) and 0.13-2.57 x (relative L2).  M = 6 is twice the worst of them and stays under the cap.
M = 6.0
FLOOR = 2e-7


def within(e_hip, e_32, rng):
    return e_hip <= M * e_32 + FLOOR * rng


@functools.lru_cache(maxsize=None)
def weights(seed=0):
    """[(weight, bias)] fp32: Kaiming-normal fan_out weights and biases of about 0.1 randn, so that the bias path is live."""
    g = torch.Generator().manual_seed(seed)
    ws, cin = [], 3
    for cout in CHANNELS:
        std = (2.0 / (cout * 9)) ** 0.5
        ws.append((torch.randn(cout, cin, 3, 3, generator=g) * std, 0.1 * torch.randn(cout, generator=g)))
        cin = cout
    return ws


def state_dict(ws):
    """torchvision layout, with classifier entries that a loader must ignore."""
    sd = {}
    for n, (w, b) in zip(CONV_INDEX, ws):
        sd[f"features.{n}.weight"], sd[f"features.{n}.bias"] = w.clone(), b.clone()
    sd["classifier.0.weight"], sd["classifier.0.bias"] = torch.zeros(4, 4), torch.zeros(4)
    return sd


def oracle_taps(x, ws, layers=DEFAULT_LAYERS, dtype=torch.float64):
    """{tap name: pre-ReLU conv output} of x in [-1, 1] ([B,3,H,W]), evaluated in `dtype` on the CPU."""
    want = {f"features_{CONV_INDEX[l]}": l for l in range(13)}
    last = max(want[k] for k in layers)
    x = x.to(dtype)
    h = ((x + 1) / 2 - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    taps = {}
    for l in range(last + 1):
        if POOL_BEFORE[l]:
            h = F.max_pool2d(h, 2)
        z = F.conv2d(h, ws[l][0].to(dtype), ws[l][1].to(dtype), padding=1)
        name = f"features_{CONV_INDEX[l]}"
        if name in layers:
            taps[name] = z
        h = F.relu(z)
    return taps


def oracle_vector(taps, layers, w_dict):
    return torch.cat([taps[k].flatten(1) * w_dict[k] for k in layers], dim=1)


def oracle_loss(x, ws, targets, layers, w_dict, dtype):
    taps = oracle_taps(x, ws, layers, dtype)
    return sum((w_dict[k] ** 2) * ((taps[k] - targets[k].to(dtype)) ** 2).sum() for k in layers)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and oracle results of one case: x, the target image, fp64 / fp32 taps of both, the fp64 / fp32 loss and gradient."""
    B, H, W, layers = CASES[name]
    layers = tuple(DEFAULT_LAYERS if layers is None else layers)
    g = torch.Generator().manual_seed(100 + sum(map(ord, name)))
    x = (torch.rand(B, 3, H, W, generator=g) * 2 - 1)
    t = (torch.rand(B, 3, H, W, generator=g) * 2 - 1)
    ws = weights()
    wd = case_weights(layers)
    out = {"x": x, "t": t, "layers": layers, "ws": ws, "w": wd}
    with torch.no_grad():
        out["taps64"] = oracle_taps(x, ws, layers, torch.float64)
        out["taps32"] = oracle_taps(x, ws, layers, torch.float32)
        out["ttaps64"] = oracle_taps(t, ws, layers, torch.float64)
    # the loss against fp32 targets (what the GPU is given), in both precisions
    targets = {k: v.float() for k, v in out["ttaps64"].items()}
    out["targets"] = targets
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        xx = x.clone().to(dtype).requires_grad_(True)          # (a copy: x itself stays a plain tensor for the callers)
        loss = oracle_loss(xx, ws, targets, layers, wd, dtype)
        loss.backward()
        out["loss" + tag], out["grad" + tag] = loss.detach(), xx.grad.detach()
    return out
