"""Oracle and shared cases of the LPIPS tests (test_lpips_host.py, test_gpu_lpips.py).

The oracle is the published LPIPS v0.1 formula (net = 'vgg', spatial = False) written with torch on the CPU: the VGG16 trunk
of _perceptual_cases (F.conv2d / relu / max_pool2d), the taps behind the ReLUs of convs 1, 3, 6, 9, 12, and per layer

    f = relu(z);  n(p) = sqrt(sum_c f[c,p]^2) + 1e-10;  d_k(p) = sum_c lin_k[c] (fa[c,p] / na(p) - fb[c,p] / nb(p))^2
    lpips = sum_k mean_p d_k(p)

evaluated in fp64 (the truth) and in fp32 (the yardstick e_32 of the accuracy rule).  Each case is computed once per session
and shared; nobody writes into it.

Accuracy rule (the project's, _perceptual_cases.within's form): e_hip <= M * e_32 + 2e-7 * range, layer by layer -- with random
Kaiming weights the deep layers' distances are 10^2 .. 10^4 times smaller than layer 0's, so a wrong relu5_3 head would vanish
in the total.
  * a distance map: e = max-abs error of the map against fp64, range = the fp64 map's maximum;
  * a per-layer scalar (per sample): e_hip = |value - fp64 value|, e_32 = the MEAN OVER PIXELS of the fp32 map's absolute error
    for that sample and layer (not the fp32 scalar's own error, which is near zero by accident too often), range = the value;
  * the total: e_32 = the sum of the five layers' e_32 (the total is their sum, so its error is at most the sum of theirs),
    range = the total.
"""
import functools

import torch
import torch.nn.functional as F

import _perceptual_cases as PC

LPIPS_CONVS = (1, 3, 6, 9, 12)
CHANNELS = (64, 128, 256, 512, 512)
TAPS = PC.DEFAULT_LAYERS                  # features_2, 7, 14, 21, 28: the conv outputs whose ReLUs LPIPS taps
assert tuple(f"features_{PC.CONV_INDEX[l]}" for l in LPIPS_CONVS) == tuple(TAPS)

# whole-metric cases (B, H, W)
CASES = {
    "deepest_1x1_16x16": (1, 16, 16),         # the deepest map is 1 x 1: one live lane
    "nonsquare_2x32x48": (2, 32, 48),
    "tails_3x80x48": (3, 80, 48),             # odd batch; maps of 3840 / 960 / 240 / 60 / 15 pixels: every tail
    "many_workgroups_128x128": (1, 128, 128),  # many workgroups per layer: the order of the partial sums
}
# head-only cases (C, H, W), B = 2
HEAD_CASES = ((64, 1, 1), (512, 3, 5), (256, 7, 9), (128, 16, 20))
# one more, (C, H, W, B): 153600 pixels = 2400 tiles of 64 for the head's 2048 workgroups per sample, so some workgroups walk a
# second tile -- the path every layer-0 map above 362^2 takes (1024^2 images); the smallest width keeps it at 39 MB a map
HEAD_CASE_STRIDED = (64, 512, 300, 1)

# M: twice the worst e_hip / e_32 (the rule's floor taken off e_hip first) measured on the MI355X over CASES and HEAD_CASES in both
# precision modes, under the project's cap of 8 (_perceptual_cases.py:36-42: the spread between legitimate fp32 summation orders).
# Worst ratio per case, over maps, per-layer scalars and totals (test_gpu_lpips.py prints every one before it asserts):
#                              fp32_exact   split_fp16
#   deepest_1x1_16x16             0.78         1.11
#   nonsquare_2x32x48             1.49         1.33
#   tails_3x80x48                 1.13         1.36
#   many_workgroups_128x128       0.91         1.66
#   head alone (all five cases)   <= 0.03 (e_hip 0.9 .. 1.4 x e_32 before the floor: the head's own order costs nothing)
# 2 x 1.661 = 3.33.  A ratio that needs more than the cap is a finding about the head, not a reason to raise it.
M = 3.33
FLOOR = 2e-7


def within(e_hip, e_32, rng):
    return e_hip <= M * e_32 + FLOOR * rng


@functools.lru_cache(maxsize=None)
def lin_weights(seed=11):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.rand(c, generator=g) * (2.0 / c) for c in CHANNELS)


def lin_state_dict(lins):
    """The lpips package's vgg.pth layout, with entries a loader must ignore."""
    sd = {f"lin{k}.model.1.weight": w.clone().view(1, -1, 1, 1) for k, w in enumerate(lins)}
    sd["lins.0.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    sd["scaling_layer.shift"] = torch.zeros(1, 3, 1, 1)
    return sd


def head(za, zb, lin, dtype):
    """One layer's distance map [B,1,H,W] in `dtype` from PRE-ReLU maps."""
    fa, fb = F.relu(za.to(dtype)), F.relu(zb.to(dtype))
    na = torch.sqrt((fa * fa).sum(1, keepdim=True)) + 1e-10
    nb = torch.sqrt((fb * fb).sum(1, keepdim=True)) + 1e-10
    return (lin.to(dtype).view(1, -1, 1, 1) * (fa / na - fb / nb) ** 2).sum(1, keepdim=True)


def oracle(a, b, ws, lins, dtype):
    """-> (maps: five [B,1,H_k,W_k], layers [B,5], total [B]) in `dtype`."""
    ta, tb = PC.oracle_taps(a, ws, TAPS, dtype), PC.oracle_taps(b, ws, TAPS, dtype)
    maps = [head(ta[k], tb[k], lin, dtype) for k, lin in zip(TAPS, lins)]
    layers = torch.stack([m.mean(dim=(1, 2, 3)) for m in maps], dim=1)
    return maps, layers, layers.sum(1)


@functools.lru_cache(maxsize=None)
def case(name):
    B, H, W = CASES[name]
    g = torch.Generator().manual_seed(300 + sum(map(ord, name)))
    a = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    b = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    ws, lins = PC.weights(), lin_weights()
    out = {"a": a, "b": b}
    with torch.no_grad():
        out["maps64"], out["layers64"], out["total64"] = oracle(a, b, ws, lins, torch.float64)
        out["maps32"], out["layers32"], out["total32"] = oracle(a, b, ws, lins, torch.float32)
    # e_32 of the per-layer scalars: the mean over pixels of the fp32 map's absolute error, [B, 5]
    out["e32_layers"] = torch.stack([(m32.double() - m64).abs().mean(dim=(1, 2, 3))
                                     for m32, m64 in zip(out["maps32"], out["maps64"])], dim=1)
    return out


@functools.lru_cache(maxsize=None)
def head_case(C, H, W, B=2):
    """randn maps in which some pixels have every channel negative in za, some in zb, some in both (when there is room)."""
    g = torch.Generator().manual_seed(1000 + C + 31 * H + W)
    za, zb = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    lin = torch.rand(C, generator=g) * (2.0 / C)
    dead = {"za": [], "zb": [], "both": []}
    pix = [(y, x) for y in range(H) for x in range(W)]
    if len(pix) == 1:                     # a single pixel: sample 0 dead in za, sample 1 dead in both
        za[0, :, 0, 0] = -za[0, :, 0, 0].abs() - 0.1
        za[1, :, 0, 0] = -za[1, :, 0, 0].abs() - 0.1
        zb[1, :, 0, 0] = -zb[1, :, 0, 0].abs() - 0.1
        dead["za"].append((0, 0, 0))
        dead["both"].append((1, 0, 0))
    else:
        for bi in range(B):
            (y0, x0), (y1, x1), (y2, x2) = pix[1], pix[len(pix) // 2], pix[-1]
            za[bi, :, y0, x0] = -za[bi, :, y0, x0].abs() - 0.1
            zb[bi, :, y1, x1] = -zb[bi, :, y1, x1].abs() - 0.1
            za[bi, :, y2, x2] = -za[bi, :, y2, x2].abs() - 0.1
            zb[bi, :, y2, x2] = -zb[bi, :, y2, x2].abs() - 0.1
            dead["za"].append((bi, y0, x0))
            dead["zb"].append((bi, y1, x1))
            dead["both"].append((bi, y2, x2))
    with torch.no_grad():
        m64, m32 = head(za, zb, lin, torch.float64), head(za, zb, lin, torch.float32)
    return {"za": za, "zb": zb, "lin": lin, "dead": dead, "map64": m64, "map32": m32,
            "mean64": m64.mean(dim=(1, 2, 3)), "e32_mean": (m32.double() - m64).abs().mean(dim=(1, 2, 3))}
