"""The VGG16 conv perceptual loss of a flip-inversion step, alone: forward + backward at B = 2, 256^2 image + 64^2 thumbnail.

    python tools/bench_perceptual.py [--res 256] [--iters 30] [--precision fp32_exact|split_fp16|both]
    python tools/bench_perceptual.py --lpips [--iters 30] [--precision fp32_exact|split_fp16]

Prints one JSON line: the HIP node (perceptual.VGG16ConvLoss.loss; csrc/vgg.hip for fp32_exact, csrc/vgg_split.hip for
split_fp16: `hip_*` is the mode asked for, with `both` the exact one, next to `split_*`) and the same loss evaluated by torch's
F.conv2d / max_pool2d / relu with autograd on the device -- the only alternative there is.  HIP events around each iteration,
median after warm-up; everything in one process on one device, interleaved by rounds.

--lpips: LPIPS (perceptual.LPIPS, csrc/lpips.hip) of one image pair instead, one JSON line per size 64^2, 256^2, 1024^2 with
three times: the trunk on the pair (`trunk_ms`: cips3d_vgg_features at B = 2), the head (`head_ms`: the six launches of
cips3d_lpips with heads_only on the kept maps of one trunk run, record and scratch allocated beforehand) and the head as its
torch expression on the same maps on the device (`torch_head_ms`); `whole_ms` is the full cips3d_lpips call."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from cips_3dplusplus_amd.perceptual import CONV_INDEX, IMAGENET_MEAN, IMAGENET_STD, POOL_BEFORE, VGG16ConvLoss

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--precision", choices=("fp32_exact", "split_fp16", "both"), default="fp32_exact")
ap.add_argument("--lpips", action="store_true")
a = ap.parse_args()
dev = "cuda"


def timed(fn, iters):
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def bench_lpips():
    from cips_3dplusplus_amd.perceptual import LPIPS, LPIPS_CONVS
    net = LPIPS("vgg_random", generator=torch.Generator().manual_seed(2), precision="fp32_exact" if a.precision == "both" else a.precision)
    g = torch.Generator(device=dev).manual_seed(1)
    for res in (64, 256, 1024):
        x = torch.randn(2, 3, res, res, device=dev, generator=g).clamp(-1, 1)
        lins = net._lins(x.device)
        record = torch.empty(1, 6, device=dev, dtype=torch.float64)
        partial = net._partial(1, x.device)
        run = net.trunk._features(x, 1)
        taps = [(run.z[l][0:1].clone(), run.z[l][1:2].clone()) for l in LPIPS_CONVS]

        def torch_head():
            total = 0
            for (za, zb), lin in zip(taps, lins):
                fa, fb = F.relu(za), F.relu(zb)
                na = torch.sqrt((fa * fa).sum(1, keepdim=True)) + 1e-10
                nb = torch.sqrt((fb * fb).sum(1, keepdim=True)) + 1e-10
                total = total + (lin.view(1, -1, 1, 1) * (fa / na - fb / nb) ** 2).sum(1, keepdim=True).mean(dim=(1, 2, 3))
            return total

        fns = {"trunk": lambda: net.trunk._features(x, 1), "whole": lambda: net._enqueue(x, None, record, 0, partial),
               "head": lambda: net._enqueue(x, None, record, 0, partial, run=run, heads_only=True), "torch_head": torch_head}
        res_ms = {k: [] for k in fns}
        for fn in fns.values():
            timed(fn, 3)
        for _ in range(a.rounds):
            for k, fn in fns.items():
                res_ms[k] += timed(fn, a.iters)
        med = {k: statistics.median(v) for k, v in res_ms.items()}
        ref = float(torch_head()[0])
        print(json.dumps({"metric": "LPIPS (vgg) of one image pair", "res": res, "precision": net.precision,
                          "trunk_ms": med["trunk"], "head_ms": med["head"], "torch_head_ms": med["torch_head"],
                          "whole_ms": med["whole"], "head_over_trunk": med["head"] / med["trunk"],
                          "lpips": float(record.cpu()[0, 0]), "lpips_torch_head": ref, "device": torch.cuda.get_device_name(0)}))


if a.lpips:
    bench_lpips()
    sys.exit(0)
modes = ("fp32_exact", "split_fp16") if a.precision == "both" else (a.precision,)
nets = [VGG16ConvLoss("vgg16_conv_random", generator=torch.Generator().manual_seed(2), precision=m) for m in modes]
assert [n.precision for n in nets] == list(modes)
net = nets[0]
g = torch.Generator(device=dev).manual_seed(1)
target = torch.randn(2, 3, a.res, a.res, device=dev, generator=g).clamp(-1, 1)
rgb = torch.randn(2, 3, a.res, a.res, device=dev, generator=g).clamp(-1, 1).requires_grad_(True)
thumb = torch.randn(2, 3, 64, 64, device=dev, generator=g).clamp(-1, 1).requires_grad_(True)
taps = [n.get_perceptual_taps(target, img_size=a.res) for n in nets]       # each mode against its own targets
taps_rgb, taps_thumb = taps[0]
ws = [(w.to(dev), b.to(dev)) for w, b in net.conv_weights()]
wk = [float(net.loss_w_dict[k]) for k in net.layers]
mean = torch.tensor(IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
std = torch.tensor(IMAGENET_STD, device=dev).view(1, 3, 1, 1)


def torch_loss(x, targets):
    h = ((x + 1) / 2 - mean) / std
    total, k = 0, 0
    for l in range(13):
        if POOL_BEFORE[l]:
            h = F.max_pool2d(h, 2)
        z = F.conv2d(h, ws[l][0], ws[l][1], padding=1)
        if f"features_{CONV_INDEX[l]}" in net.layers:
            total = total + wk[k] ** 2 * ((z - targets[k]) ** 2).sum()
            k += 1
        h = F.relu(z)
    return total


def step_hip(k=0):
    rgb.grad = thumb.grad = None
    (nets[k].loss(rgb, taps[k][0]) + nets[k].loss(thumb, taps[k][1])).backward()


def step_torch():
    rgb.grad = thumb.grad = None
    (torch_loss(rgb, taps_rgb) + torch_loss(thumb, taps_thumb)).backward()


step_hip(); g_hip = rgb.grad.clone(); l_hip = float(net.loss(rgb, taps_rgb))
step_torch(); g_torch = rgb.grad.clone(); l_torch = float(torch_loss(rgb, taps_rgb))
steps = [lambda k=k: step_hip(k) for k in range(len(nets))]
if len(nets) == 2:
    step_hip(1); g_split = rgb.grad.clone(); l_split = float(nets[1].loss(rgb, taps[1][0]))
for fn in (*steps, step_torch):
    timed(fn, 5)
res = {"hip": [], "split": [], "torch": []}
for _ in range(a.rounds):
    res["hip"] += timed(steps[0], a.iters)
    if len(nets) == 2:
        res["split"] += timed(steps[1], a.iters)
    res["torch"] += timed(step_torch, a.iters)
shapes = [(2, a.res), (2, 64)]
flop = sum(2 * B * 2.0 * 9 * sum((3 if l == 0 else net.conv_weights()[l][0].shape[1]) * net.conv_weights()[l][0].shape[0]
                                 * (S >> sum(POOL_BEFORE[:l + 1])) ** 2 for l in range(13)) for B, S in shapes)
hip_ms, torch_ms = statistics.median(res["hip"]), statistics.median(res["torch"])
split = {}
if len(nets) == 2:
    split_ms = statistics.median(res["split"])
    split = {"split_ms": split_ms, "split_min_ms": min(res["split"]), "split_tflops": flop / split_ms / 1e9,
             "split_fraction_of_833_tflops": flop / split_ms / 1e9 / 833.0, "exact_over_split": hip_ms / split_ms,
             "split_over_torch": split_ms / torch_ms, "split_median_below_exact_min": split_ms < min(res["hip"]),
             "loss_split": l_split, "grad_rel_l2_split_vs_torch": float((g_split - g_torch).norm() / g_torch.norm())}
print(json.dumps({"metric": "VGG16 conv perceptual loss, forward + backward, B=2 image + 64^2 thumbnail", "res": a.res,
                  "precision": a.precision,
                  "hip_ms": hip_ms, "torch_conv2d_ms": torch_ms, "hip_min_ms": min(res["hip"]), "torch_min_ms": min(res["torch"]),
                  "flop_fwd_plus_data_grad": flop, "hip_tflops": flop / hip_ms / 1e9,
                  "loss_hip": l_hip, "loss_torch": l_torch,
                  "grad_rel_l2_hip_vs_torch": float((g_hip - g_torch).norm() / g_torch.norm()), "device": torch.cuda.get_device_name(0), **split}))
