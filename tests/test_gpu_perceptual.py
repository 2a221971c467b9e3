"""VGG16 conv perceptual loss on the GPU (csrc/vgg.hip, perceptual.VGG16ConvLoss) against the fp64 CPU oracle of
tests/_perceptual_cases.py.

Accuracy rule of every numeric check: e_hip <= M * e_32 + 2e-7 * range, where e_32 is the error of torch's own fp32 CPU
evaluation against the fp64 evaluation of the same inputs (computed here, per case) -- max-abs per tap for the features,
max-abs and relative L2 for the gradient.  M and its derivation: _perceptual_cases.py.
"""
import pytest
import torch

import _perceptual_cases as PC
import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs
from cips_3dplusplus_amd.perceptual import TAP_CONV, VGG16ConvLoss

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NETS = {}


def net_for(layers):
    """One network per tap set, shared by the tests (the packed weights live on the device once)."""
    if layers not in _NETS:
        _NETS[layers] = VGG16ConvLoss("vgg16_conv", weights=PC.state_dict(PC.weights()), layers=list(layers),
                                      loss_w_dict=PC.case_weights(layers))
    return _NETS[layers]


def maxabs(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


def rel_l2(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("name", list(PC.CASES))
def test_features_and_loss_against_fp64(name):
    c = PC.case(name)
    net = net_for(c["layers"])
    x = c["x"].to(DEV)
    taps = net.taps(x)
    assert len(taps) == len(c["layers"])
    for k, z in zip(c["layers"], taps):
        ref64, ref32 = c["taps64"][k], c["taps32"][k]
        assert tuple(z.shape) == tuple(ref64.shape), k
        e_hip, e_32, rng = maxabs(z, ref64), maxabs(ref32, ref64), float(ref64.abs().max())
        print(f"{name} {k} {tuple(z.shape)}: |hip - fp64| {e_hip:.3e}  |fp32 cpu - fp64| {e_32:.3e}  ratio {e_hip / e_32:.2f}  max {rng:.3f}")
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
    print(f"{name} loss {float(loss):.9e}: |hip - fp64| {e_hip:.3e}  |fp32 cpu - fp64| {e_32:.3e}")
    assert PC.within(e_hip, e_32, abs(float(c["loss64"])))


@pytest.mark.parametrize("name", list(PC.CASES))
def test_gradient_against_fp64_autograd(name):
    c = PC.case(name)
    net = net_for(c["layers"])
    x = c["x"].to(DEV).requires_grad_(True)
    loss = net.loss(x, [c["targets"][k].to(DEV) for k in c["layers"]])
    loss.backward()
    g, g64, g32 = x.grad, c["grad64"], c["grad32"]
    assert tuple(g.shape) == tuple(g64.shape) and bool(torch.isfinite(g).all())
    e_hip, e_32, rng = maxabs(g, g64), maxabs(g32, g64), float(g64.abs().max())
    r_hip, r_32 = rel_l2(g, g64), rel_l2(g32, g64)
    print(f"{name} d loss / d x: max-abs |hip - fp64| {e_hip:.3e} |fp32 cpu - fp64| {e_32:.3e} ratio {e_hip / e_32:.2f} (max |g| {rng:.3e});  "
          f"rel L2 hip {r_hip:.3e} fp32 cpu {r_32:.3e} ratio {r_hip / r_32:.2f}")
    assert PC.within(e_hip, e_32, rng)
    assert PC.within(r_hip, r_32, 1.0)


def test_batch_independence_and_determinism():
    c = PC.case("thumb_2x64x64")
    net = net_for(c["layers"])
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


def test_options_change_exactly_the_terms_they_name():
    c = PC.case("thumb_2x64x64")
    layers = c["layers"]
    net = net_for(layers)
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
    # a layers subset: the same taps, only its terms, only the layers up to the deepest one
    sub_layers = ("features_2", "features_14")
    sub = net_for(sub_layers)
    assert sub.n_convs == TAP_CONV["features_14"] + 1
    sub_taps = sub.taps(x)
    assert torch.equal(sub_taps[0], net.taps(x)[0]) and torch.equal(sub_taps[1], net.taps(x)[2])
    got = float(sub.loss(x, [targets[0], targets[2]]))
    ref = expect(PC.W_1024, sub_layers, term64)
    assert PC.within(abs(got - ref), abs(expect(PC.W_1024, sub_layers, term32) - ref), abs(ref))
    # loss == ((forward(x) - forward(t)) ** 2).sum()
    vec_loss64 = float(((PC.oracle_vector(c["taps64"], layers, PC.W_1024)
                         - PC.oracle_vector(c["ttaps64"], layers, PC.W_1024)) ** 2).sum())
    vec_loss32 = float(((PC.oracle_vector(c["taps32"], layers, PC.W_1024)
                         - PC.oracle_vector({k: v.float() for k, v in c["ttaps64"].items()}, layers, PC.W_1024)) ** 2).sum())
    via_forward = float(((net(x).double() - net(t).double()) ** 2).sum())
    for got in (base, via_forward):
        assert PC.within(abs(got - vec_loss64), abs(vec_loss32 - vec_loss64), abs(vec_loss64)), (got, vec_loss64)


def test_size_contract_and_cpu_tensors_raise():
    net = net_for(PC.DEFAULT_LAYERS)
    with pytest.raises(RuntimeError, match="multiples of 16"):
        net.taps(torch.zeros(1, 3, 72, 64, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        net.taps(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="shape"):
        net.loss(torch.zeros(1, 3, 32, 32, device=DEV), net.taps(torch.zeros(1, 3, 16, 16, device=DEV)))


def test_downsample_size_goes_through_area_interpolation():
    ws = PC.weights()
    net = VGG16ConvLoss("vgg16_conv", weights=PC.state_dict(ws), downsample_size=16, layers=["features_2", "features_7"])
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
    """FlipProjector.project_wplus with the perceptual loss on the tiny generator: it runs, the loss is finite, and the camera
    and W+ leaves receive finite, non-zero gradients."""
    from cips_3dplusplus_amd.camera import Camera
    from cips_3dplusplus_amd.projector import FlipProjector, perceptual_loss
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=2)
    g = torch.Generator(device=DEV).manual_seed(0)
    target = torch.randn(2, 3, 64, 64, device=DEV, generator=g).clamp(-1, 1)
    net = VGG16ConvLoss("vgg16_conv_random", generator=torch.Generator().manual_seed(4))
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
