"""The split-fp16 mode of the VGG16 conv perceptual loss on the GPU (csrc/vgg_split.hip, perceptual.VGG16ConvLoss(...,
precision="split_fp16")) against the fp64 CPU oracle of tests/_perceptual_cases.py.

Accuracy rule of every numeric check, unchanged from the exact mode's tests: e_hip <= M * e_32 + 2e-7 * range with e_32 the
error of torch's own fp32 CPU evaluation against fp64 (PC.within, M = 6).  The mode's own claims come on top: its kernels
really ran (taps differ in bits from the exact mode's), a sample's bits do not depend on the batch, and every scale follows
the data's exponent (inputs scaled by a power of two give outputs scaled by it bit for bit).

Measured on the MI355X (worst ratio e_hip / e_32 per case; taps, gradient max-abs, gradient relative L2): see DESIGN 9.5.
"""
import numpy as np
import pytest
import torch

import _perceptual_cases as PC
import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, perceptual
from cips_3dplusplus_amd.perceptual import TAP_CONV, VGG16ConvLoss

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NETS = {}


def net_for(layers, precision="split_fp16"):
    """One network per (tap set, mode), shared by the tests (the packed weights live on the device once)."""
    key = (tuple(layers), precision)
    if key not in _NETS:
        _NETS[key] = VGG16ConvLoss("vgg16_conv", weights=PC.state_dict(PC.weights()), layers=list(layers),
                                   loss_w_dict=PC.case_weights(layers), precision=precision)
    assert _NETS[key].precision == precision
    return _NETS[key]


def maxabs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def rel_l2(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("name", list(PC.CASES))
def test_features_and_loss_against_fp64(name):
    c = PC.case(name)
    net = net_for(c["layers"])
    assert net.precision == "split_fp16"
    x = c["x"].to(DEV)
    taps = net.taps(x)
    assert len(taps) == len(c["layers"])
    for k, z in zip(c["layers"], taps):
        ref64, ref32 = c["taps64"][k], c["taps32"][k]
        assert tuple(z.shape) == tuple(ref64.shape), k
        e_hip, e_32, rng = maxabs(z, ref64), maxabs(ref32, ref64), float(ref64.abs().max())
        print(f"{name} {k} {tuple(z.shape)}: |split - fp64| {e_hip:.3e}  |fp32 cpu - fp64| {e_32:.3e}  ratio {e_hip / e_32:.2f}  max {rng:.3f}")
        assert PC.within(e_hip, e_32, rng), (k, e_hip, e_32, rng)
    # the concatenated vector: order, layout (C, H, W) and weights
    vec = net(x)
    ref_vec = PC.oracle_vector(c["taps64"], c["layers"], c["w"])
    assert tuple(vec.shape) == tuple(ref_vec.shape)
    off = 0
    for k in c["layers"]:
        n = c["taps64"][k][0].numel()
        e_32 = maxabs(c["taps32"][k], c["taps64"][k]) * c["w"][k]
        assert PC.within(maxabs(vec[:, off:off + n], ref_vec[:, off:off + n]), e_32, float(ref_vec[:, off:off + n].abs().max())), k
        off += n
    assert off == vec.shape[1]
    # the scalar loss
    targets = [c["targets"][k].to(DEV) for k in c["layers"]]
    loss = net.loss(x, targets)
    assert loss.dim() == 0
    e_hip, e_32 = abs(float(loss) - float(c["loss64"])), abs(float(c["loss32"]) - float(c["loss64"]))
    print(f"{name} loss {float(loss):.9e}: |split - fp64| {e_hip:.3e}  |fp32 cpu - fp64| {e_32:.3e}")
    assert PC.within(e_hip, e_32, abs(float(c["loss64"])))


@pytest.mark.parametrize("name", list(PC.CASES))
def test_gradient_against_fp64_autograd(name):
    c = PC.case(name)
    net = net_for(c["layers"])
    assert net.precision == "split_fp16"
    x = c["x"].to(DEV).requires_grad_(True)
    loss = net.loss(x, [c["targets"][k].to(DEV) for k in c["layers"]])
    loss.backward()
    g, g64, g32 = x.grad, c["grad64"], c["grad32"]
    assert tuple(g.shape) == tuple(g64.shape) and bool(torch.isfinite(g).all())
    e_hip, e_32, rng = maxabs(g, g64), maxabs(g32, g64), float(g64.abs().max())
    r_hip, r_32 = rel_l2(g, g64), rel_l2(g32, g64)
    print(f"{name} d loss / d x: max-abs |split - fp64| {e_hip:.3e} |fp32 cpu - fp64| {e_32:.3e} ratio {e_hip / e_32:.2f} (max |g| {rng:.3e});  "
          f"rel L2 split {r_hip:.3e} fp32 cpu {r_32:.3e} ratio {r_hip / r_32:.2f}")
    assert PC.within(e_hip, e_32, rng)
    assert PC.within(r_hip, r_32, 1.0)


def test_the_split_kernels_really_ran():
    """The two modes agree within the accuracy rule and differ in bits: `precision=` reached other kernels."""
    c = PC.case("thumb_2x64x64")
    split, exact = net_for(c["layers"]), net_for(c["layers"], "fp32_exact")
    assert split.precision == "split_fp16" and exact.precision == "fp32_exact"
    x = c["x"].to(DEV)
    ts, te = split.taps(x), exact.taps(x)
    differ = 0
    for k, a, b in zip(c["layers"], ts, te):
        e_32, rng = maxabs(c["taps32"][k], c["taps64"][k]), float(c["taps64"][k].abs().max())
        assert PC.within(maxabs(a, b), e_32, rng), k
        differ += not torch.equal(a, b)
    assert differ >= 1


def test_packed_weights_are_the_documented_order():
    """The device's hi / lo operands and exponent of convs 1 and 2 equal the numpy restatement bit for bit."""
    net = net_for(("features_5",))
    assert net.precision == "split_fp16" and net.n_convs == 3
    net._ctx(torch.device(DEV, torch.cuda.current_device()))
    kept = next(iter(net._packed.values()))[1]              # per conv: bias, forward form, data-gradient form; then the maxima
    w_amax = kept[3 * net.n_convs]
    for l in (1, 2):
        w = PC.weights()[l][0]
        fwd, bwd, e = perceptual.split_pack_reference(w.numpy())
        assert float(w_amax[l:l + 1].view(torch.float32)) == float(w.abs().max())
        for got, ref in ((kept[3 * l + 1], fwd), (kept[3 * l + 2], bwd)):
            assert np.array_equal(got.cpu().numpy().view(np.uint16), ref.reshape(-1).view(np.uint16)), l


def test_batch_independence_and_determinism():
    c = PC.case("thumb_2x64x64")
    net = net_for(c["layers"])
    assert net.precision == "split_fp16"
    x = c["x"].to(DEV)
    both = net.taps(x)
    for b in range(2):
        one = net.taps(x[b:b + 1].contiguous())
        for k, z2, z1 in zip(c["layers"], both, one):
            assert torch.equal(z2[b:b + 1], z1), (k, b)
    targets = [c["targets"][k].to(DEV) for k in c["layers"]]
    runs = []
    for _ in range(2):
        xx = x.clone().requires_grad_(True)
        loss = net.loss(xx, targets)
        loss.backward()
        runs.append((loss.detach().clone(), xx.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][1].abs().max()) > 0
    # the gradient of a sample does not depend on the batch either
    for b in range(2):
        xx = x[b:b + 1].clone().requires_grad_(True)
        net.loss(xx, [t[b:b + 1].contiguous() for t in targets]).backward()
        assert torch.equal(xx.grad, runs[0][1][b:b + 1]), b


def test_both_tile_shapes_give_the_same_bits():
    """The launcher takes 16 x 16 pixel tiles once they alone give 256 workgroups and 4 x 16 tiles below that; both walk K in the
    same order.  Conv 1 of a B = 4, 128^2 call is the smallest launch of the big tile (4 * 64 workgroups); the B = 1 calls take
    the small one, which the five cases pin to fp64.  Taps and gradients of the two must agree bit for bit."""
    layers = ("features_2",)
    net = net_for(layers)
    assert net.precision == "split_fp16" and net.n_convs == 2
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(4, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
    t = (torch.rand(4, 3, 128, 128, generator=g) * 2 - 1).to(DEV)
    taps, targets = net.taps(x)[0], net.taps(t)
    xx = x.clone().requires_grad_(True)
    net.loss(xx, targets).backward()
    assert float(xx.grad.abs().max()) > 0
    for b in range(4):
        xb = x[b:b + 1].clone().requires_grad_(True)
        assert torch.equal(net.taps(xb)[0], taps[b:b + 1]), b
        net.loss(xb, [targets[0][b:b + 1].contiguous()]).backward()
        assert torch.equal(xb.grad, xx.grad[b:b + 1]), b


@pytest.mark.parametrize("k", [17, -14])
def test_scales_follow_the_exponent(k):
    """Conv 1's weight and bias and the biases of convs 2 .. 12 times 2^k: in exact arithmetic every pre-ReLU tensor from conv 1
    on is 2^k times the base's.  With one power of two per (tensor, sample) taken from the data, the split operands are the same
    fp16 bits in both nets, so the taps, the loss (/ 4^k) and the gradient (/ 4^k) agree bit for bit.  Unscaled, k = 17 overflows
    fp16 and the gradients (1e-8 and below) underflow it."""
    c = PC.case("thumb_2x64x64")
    base = net_for(c["layers"])
    ws = [(w.clone(), b.clone()) for w, b in PC.weights()]
    ws[1] = (ws[1][0] * 2.0 ** k, ws[1][1] * 2.0 ** k)
    for l in range(2, 13):
        ws[l] = (ws[l][0], ws[l][1] * 2.0 ** k)
    scaled = VGG16ConvLoss("vgg16_conv", weights=PC.state_dict(ws), layers=list(c["layers"]),
                           loss_w_dict=PC.case_weights(c["layers"]), precision="split_fp16")
    assert base.precision == scaled.precision == "split_fp16"
    x = c["x"].to(DEV)
    for name, tb, ts in zip(c["layers"], base.taps(x), scaled.taps(x)):
        assert bool(torch.isfinite(ts).all()), name
        assert torch.equal(ts, tb * 2.0 ** k), name
    targets = [c["targets"][name].to(DEV) for name in c["layers"]]
    out = []
    for net, tt in ((base, targets), (scaled, [t * 2.0 ** k for t in targets])):
        xx = x.clone().requires_grad_(True)
        loss = net.loss(xx, tt)
        loss.backward()
        out.append((loss.detach(), xx.grad))
    assert float(out[0][1].abs().max()) > 0
    assert torch.equal(out[1][0], out[0][0] * 4.0 ** k)
    assert torch.equal(out[1][1], out[0][1] * 4.0 ** k)


def test_options_and_contract():
    c = PC.case("thumb_2x64x64")
    layers = c["layers"]
    net = net_for(layers)
    assert net.precision == "split_fp16"
    x, t = c["x"].to(DEV), c["t"].to(DEV)
    targets = net.taps(t)
    # per-tap terms from the fp64 oracle (the targets here are the GPU's own taps of t)
    term64 = {k: float(((c["taps64"][k] - tt.double().cpu()) ** 2).sum()) for k, tt in zip(layers, targets)}
    term32 = {k: float(((c["taps32"][k] - tt.cpu()) ** 2).sum()) for k, tt in zip(layers, targets)}

    def expect(wd, ls, terms):
        return sum(wd[k] ** 2 * terms[k] for k in ls)

    base = float(net.loss(x, targets))
    override = dict(PC.W_1024, features_14=0.003)
    over = float(net.loss(x, targets, loss_w_dict=override))
    for got, wd in ((base, PC.W_1024), (over, override)):
        ref = expect(wd, layers, term64)
        assert PC.within(abs(got - ref), abs(expect(wd, layers, term32) - ref), abs(ref)), (got, ref)
    # only the named term moved: the difference is (w'^2 - w^2) * that tap's sum
    d_ref = (override["features_14"] ** 2 - PC.W_1024["features_14"] ** 2) * term64["features_14"]
    assert abs((over - base) - d_ref) <= 1e-5 * abs(d_ref)
    # the override reaches forward() too, and only there
    v0, v1 = net(x), net(x, loss_w_dict=override)
    changed = (v0 != v1).any(dim=0).nonzero().flatten()
    lo = sum(c["taps64"][k][0].numel() for k in layers[:2])
    hi = lo + c["taps64"]["features_14"][0].numel()
    assert int(changed.min()) >= lo and int(changed.max()) < hi and changed.numel() > 0.9 * (hi - lo)
    # a layers subset: the same taps bit for bit, only the layers up to the deepest one
    sub = net_for(("features_2", "features_14"))
    assert sub.precision == "split_fp16" and sub.n_convs == TAP_CONV["features_14"] + 1
    sub_taps, full_taps = sub.taps(x), net.taps(x)
    assert torch.equal(sub_taps[0], full_taps[0]) and torch.equal(sub_taps[1], full_taps[2])
    # the size contract, CPU tensors, the precision argument
    with pytest.raises(RuntimeError, match="multiples of 16"):
        net.taps(torch.zeros(1, 3, 72, 64, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        net.taps(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError, match="precision"):
        VGG16ConvLoss("vgg16_conv_random", precision="fp16")


def test_downsample_size_goes_through_area_interpolation():
    ws = PC.weights()
    net = VGG16ConvLoss("vgg16_conv", weights=PC.state_dict(ws), downsample_size=16, layers=["features_2", "features_7"],
                        precision="split_fp16")
    assert net.precision == "split_fp16"
    g = torch.Generator().manual_seed(9)
    x = torch.rand(1, 3, 32, 32, generator=g) * 2 - 1
    # area down-sampling by 2 is a 2x2 mean, and it commutes with the affine normalisation
    small = torch.nn.functional.avg_pool2d(x.double(), 2)
    ref = PC.oracle_taps(small, ws, ("features_2", "features_7"), torch.float64)
    ref32 = PC.oracle_taps(small.float(), ws, ("features_2", "features_7"), torch.float32)
    xg = x.to(DEV).requires_grad_(True)
    for k, z in zip(("features_2", "features_7"), net.taps(xg)):
        assert PC.within(maxabs(z, ref[k]), maxabs(ref32[k], ref[k]), float(ref[k].abs().max())), k
    net.loss(xg, [torch.zeros_like(z) for z in net.taps(xg)]).backward()
    assert tuple(xg.grad.shape) == (1, 3, 32, 32) and float(xg.grad.abs().max()) > 0


def test_through_the_generator():
    """FlipProjector.project_wplus with the split perceptual loss on the tiny generator: projector.perceptual_loss passes the
    net through as it is, the loss is finite, and the camera and W+ leaves receive finite, non-zero gradients."""
    from cips_3dplusplus_amd.camera import Camera
    from cips_3dplusplus_amd.projector import FlipProjector, perceptual_loss
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=2)
    g = torch.Generator(device=DEV).manual_seed(0)
    target = torch.randn(2, 3, 64, 64, device=DEV, generator=g).clamp(-1, 1)
    net = VGG16ConvLoss("vgg16_conv_random", generator=torch.Generator().manual_seed(4), precision="split_fp16")
    assert net.precision == "split_fp16"
    loss_fn = perceptual_loss(net, target, rgb_weight=1.0, thumb_weight=1.0, img_size=256)      # thumbnail: 64 * 64 / 256 = 16^2
    cam_cfg = {"img_size": 16, "fov_ang": 6, "dist_radius": 0.12}
    ncfg = {"N_samples": 6, "perturb": False, "static_viewdirs": True}
    seen = []
    out = FlipProjector(G, DEV).project_wplus(cam_cfg, ncfg, loss_fn, N_steps_pose=2, N_steps_app=0, w_avg_samples=64,
                                             on_step=lambda step, loss, azim, elev: seen.append(loss.detach().clone()))
    assert len(seen) == 2 and all(bool(torch.isfinite(v)) and float(v) > 0 for v in seen)
    assert bool(torch.isfinite(out["azim"]).all()) and bool(torch.isfinite(out["w_render_opt"]).all())
    # the same call pattern by hand, to look at the leaves' gradients
    Gc = out["G"]
    loc = torch.tensor([[0.1, 0.05], [-0.1, 0.05]], device=DEV, requires_grad=True)
    w_r = out["w_render_opt"].clone().requires_grad_(True)
    w_d = out["w_decoder_opt"].clone().requires_grad_(True)
    e, f, n, fa, _ = Camera.generate_camera_params(16, DEV, locations=loc, fov_ang=6, dist_radius=0.12)
    r = Gc(zs=[None, None], style_render=w_r, style_decoder=w_d, cam_poses=e, focals=f, img_size=16, near=n, far=fa,
           noise_bufs=out["noise_bufs"], nerf_cfg=ncfg, renderer_detach=False)
    assert tuple(r["rgb"].shape) == (2, 3, 64, 64) and tuple(r["thumb_rgb"].shape) == (2, 3, 16, 16)
    loss = loss_fn(r["rgb"], r["thumb_rgb"])
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, leaf in (("camera", loc), ("w_render", w_r), ("w_decoder", w_d)):
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0, name
