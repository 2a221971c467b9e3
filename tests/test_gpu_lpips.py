"""LPIPS on the GPU (csrc/lpips.hip, perceptual.LPIPS / LPIPSLog / lpips_layer_distance) against the published formula in
fp64 (_lpips_cases), layer by layer, in both precision modes of the trunk; exact zeros, symmetry, determinism, batch
independence, the prepared form, the uint8 pairing, the device-side log and `project_wplus(lpips_metric=...)`."""
import math

import pytest
import torch

import _lpips_cases as LC
import _perceptual_cases as PC
import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs
from cips_3dplusplus_amd import projector as P
from cips_3dplusplus_amd.perceptual import LPIPS, LPIPSLog, lpips_layer_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ("fp32_exact", "split_fp16")


@pytest.fixture(scope="module")
def nets():
    ws, lins = PC.weights(), LC.lin_weights()
    return {p: LPIPS("vgg", weights=PC.state_dict(ws), lin_weights=LC.lin_state_dict(lins), precision=p) for p in PRECISIONS}


def _ratio(e_hip, e_32, rng):
    """e_hip / e_32 once the rule's floor is taken off (what M has to cover)."""
    over = e_hip - LC.FLOOR * rng
    return 0.0 if over <= 0 else (over / e_32 if e_32 > 0 else math.inf)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(LC.CASES))
def test_maps_layers_and_totals_against_fp64(nets, name, precision):
    c = LC.case(name)
    total, layers, maps = nets[precision](c["a"].to(DEV), c["b"].to(DEV), return_layers=True, spatial=True)
    B = c["a"].shape[0]
    assert total.dtype == torch.float64 and tuple(total.shape) == (B,) and tuple(layers.shape) == (B, 5)
    assert bool(torch.isfinite(total).all()) and bool(torch.isfinite(layers).all())
    worst, checks = 0.0, []
    for k in range(5):
        m64, m32 = c["maps64"][k], c["maps32"][k]
        assert tuple(maps[k].shape) == tuple(m64.shape) and maps[k].dtype == torch.float32
        e_hip = float((maps[k].cpu().double() - m64).abs().max())
        e_32 = float((m32.double() - m64).abs().max())
        checks.append((f"map {k}", e_hip, e_32, float(m64.max())))
        for i in range(B):
            checks.append((f"layer {k} sample {i}", abs(float(layers[i, k]) - float(c["layers64"][i, k])),
                           float(c["e32_layers"][i, k]), float(c["layers64"][i, k])))
    for i in range(B):
        checks.append((f"total sample {i}", abs(float(total[i]) - float(c["total64"][i])), float(c["e32_layers"][i].sum()),
                       float(c["total64"][i])))
    for what, e_hip, e_32, rng in checks:
        r = _ratio(e_hip, e_32, rng)
        worst = max(worst, r)
        print(f"{name} {precision} {what}: e_hip {e_hip:.3e} e_32 {e_32:.3e} range {rng:.3e} ratio {r:.3f}")
    print(f"{name} {precision} WORST ratio {worst:.3f}")
    for what, e_hip, e_32, rng in checks:
        assert LC.within(e_hip, e_32, rng), (name, precision, what, e_hip, e_32, rng)


@pytest.mark.parametrize("shape", LC.HEAD_CASES + (LC.HEAD_CASE_STRIDED,))
def test_head_alone_against_fp64(shape):
    c = LC.head_case(*shape)
    B = c["za"].shape[0]
    dmap, mean = lpips_layer_distance(c["za"].to(DEV), c["zb"].to(DEV), c["lin"].to(DEV))
    assert tuple(dmap.shape) == tuple(c["map64"].shape) and mean.dtype == torch.float64 and tuple(mean.shape) == (B,)
    dmap, mean = dmap.cpu(), mean.cpu()
    assert bool(torch.isfinite(dmap).all()) and bool(torch.isfinite(mean).all())
    for bi, y, x in c["dead"]["both"]:                      # no live channel on either side: exactly 0, never a NaN
        assert float(dmap[bi, 0, y, x]) == 0.0
    for bi, y, x in c["dead"]["za"] + c["dead"]["zb"]:      # one side dead: that side adds exactly 0, the other its weights
        assert float(dmap[bi, 0, y, x]) > 0.0
    e_hip, e_32 = float((dmap.double() - c["map64"]).abs().max()), float((c["map32"].double() - c["map64"]).abs().max())
    print(f"head {shape} map: e_hip {e_hip:.3e} e_32 {e_32:.3e} ratio {_ratio(e_hip, e_32, float(c['map64'].max())):.3f}")
    assert LC.within(e_hip, e_32, float(c["map64"].max()))
    for i in range(B):
        e_hip, e_32, rng = abs(float(mean[i]) - float(c["mean64"][i])), float(c["e32_mean"][i]), float(c["mean64"][i])
        print(f"head {shape} mean {i}: e_hip {e_hip:.3e} e_32 {e_32:.3e} ratio {_ratio(e_hip, e_32, rng):.3f}")
        assert LC.within(e_hip, e_32, rng)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_identical_images_give_exactly_zero(nets, precision):
    a = LC.case("tails_3x80x48")["a"].to(DEV)
    total, layers, maps = nets[precision](a, a.clone(), return_layers=True, spatial=True)
    assert bool((total == 0.0).all()) and bool((layers == 0.0).all())
    assert all(bool((m == 0.0).all()) for m in maps)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_symmetric_bit_for_bit(nets, precision):
    c = LC.case("tails_3x80x48")
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    t_ab, l_ab = nets[precision](a, b, return_layers=True)
    t_ba, l_ba = nets[precision](b, a, return_layers=True)
    assert torch.equal(t_ab, t_ba) and torch.equal(l_ab, l_ba) and float(t_ab.min()) > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_deterministic_batch_independent_and_prepared(nets, precision):
    net = nets[precision]
    c = LC.case("tails_3x80x48")
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    t0, l0, m0 = net(a, b, return_layers=True, spatial=True)
    t1, l1, m1 = net(a, b, return_layers=True, spatial=True)
    assert torch.equal(t0, t1) and torch.equal(l0, l1) and all(torch.equal(x, y) for x, y in zip(m0, m1))
    for i in range(3):                                      # a B = 3 call equals three B = 1 calls
        ti, li = net(a[i:i + 1], b[i:i + 1], return_layers=True)
        assert torch.equal(ti, t0[i:i + 1]) and torch.equal(li, l0[i:i + 1])
    tp, lp = net(a, net.prepare(b), return_layers=True)     # the trunk on a alone, b's taps from an earlier call
    assert torch.equal(tp, t0) and torch.equal(lp, l0)
    one = net.prepare(b[1])                                 # one prepared image serves every sample of a batch
    tb, lb = net(a, one, return_layers=True)
    tr, lr = net(a, b[1:2].expand(3, -1, -1, -1).contiguous(), return_layers=True)
    assert torch.equal(tb, tr) and torch.equal(lb, lr)


def test_uint8_is_its_fp32_form(nets):
    g = torch.Generator().manual_seed(5)
    ua = torch.randint(0, 256, (2, 3, 32, 48), generator=g, dtype=torch.uint8).to(DEV)
    ub = torch.randint(0, 256, (2, 3, 32, 48), generator=g, dtype=torch.uint8).to(DEV)
    fa, fb = ua.float() / 127.5 - 1, ub.float() / 127.5 - 1
    net = nets["fp32_exact"]
    t_u, l_u = net(ua, ub, return_layers=True)
    t_f, l_f = net(fa, fb, return_layers=True)
    t_m, l_m = net(ua, fb, return_layers=True)
    assert torch.equal(t_u, t_f) and torch.equal(l_u, l_f) and torch.equal(t_m, t_f) and torch.equal(l_m, l_f)
    assert torch.equal(net(ua[0], ub[0]), t_u[0:1])         # [3,H,W] is one image


def test_one_layer_of_lin_weights_is_that_layer(nets):
    c = LC.case("nonsquare_2x32x48")
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    _, full = nets["fp32_exact"](a, b, return_layers=True)
    ws, lins = PC.weights(), LC.lin_weights()
    for k in range(5):
        only = [w if j == k else torch.zeros_like(w) for j, w in enumerate(lins)]
        net = LPIPS("vgg", weights=PC.state_dict(ws), lin_weights=LC.lin_state_dict(only))
        total, layers = net(a, b, return_layers=True)
        assert torch.equal(total, full[:, k]) and torch.equal(layers[:, k], full[:, k])
        assert bool((layers[:, [j for j in range(5) if j != k]] == 0.0).all())


def test_lin_weights_follow_the_buffers(nets):
    """The device copies of the lin vectors are made again when the registered buffers change (load_state_dict, in place)."""
    c = LC.case("deepest_1x1_16x16")
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    ws, lins = PC.weights(), LC.lin_weights()
    net = LPIPS("vgg", weights=PC.state_dict(ws), lin_weights=LC.lin_state_dict(lins))
    _, l0 = net(a, b, return_layers=True)
    assert torch.equal(l0, nets["fp32_exact"](a, b, return_layers=True)[1])
    sd = net.state_dict()
    sd["lin_0"] = torch.zeros_like(sd["lin_0"])
    net.load_state_dict(sd)
    _, l1 = net(a, b, return_layers=True)
    assert float(l1[0, 0]) == 0.0 and torch.equal(l1[:, 1:], l0[:, 1:])
    net.lin_1.mul_(2.0)
    _, l2 = net(a, b, return_layers=True)
    assert float(l2[0, 1]) == 2.0 * float(l0[0, 1]) and torch.equal(l2[:, 2:], l0[:, 2:])


def test_random_net_is_seeded():
    a = LC.case("deepest_1x1_16x16")["a"].to(DEV)
    b = LC.case("deepest_1x1_16x16")["b"].to(DEV)
    n0 = LPIPS("vgg_random", generator=torch.Generator().manual_seed(4))
    n1 = LPIPS("vgg_random", generator=torch.Generator().manual_seed(4))
    assert all(bool((w >= 0).all()) for w in n0.lin_weights())
    assert torch.equal(n0(a, b), n1(a, b)) and float(n0(a, b)[0]) > 0


def test_lpips_log(nets):
    net = nets["fp32_exact"]
    c = LC.case("tails_3x80x48")
    imgs, target = c["a"].to(DEV), c["b"][0:1].to(DEV)
    direct_t, direct_l = net(imgs, target.expand(3, -1, -1, -1).contiguous(), return_layers=True)
    log = LPIPSLog(net, target, 3)
    assert log.result()["steps"] == [] and tuple(log.result()["lpips_layers"].shape) == (0, 5)
    for i, step in enumerate((0, 5, 9)):
        assert log.update(step, imgs[i:i + 1]) == i
    res = log.result()
    assert res["steps"] == [0, 5, 9] and res["lpips"].dtype == torch.float64
    assert torch.equal(res["lpips"], direct_t) and torch.equal(res["lpips_layers"], direct_l)
    with pytest.raises(ValueError, match="full"):
        log.update(11, imgs[0:1])
    assert log.update(12, imgs[2], row=0) == 0              # row= overwrites; the row moves to the end of the order
    res = log.result()
    assert res["steps"] == [5, 9, 12]
    assert torch.equal(res["lpips"], direct_t[[1, 2, 2]]) and torch.equal(res["lpips_layers"], direct_l[[1, 2, 2]])
    with pytest.raises(ValueError, match="outside the record"):
        log.update(13, imgs[0:1], row=3)


class CapturingProjector(P.FlipProjector):
    """Keeps view 0 of every image the generator returns (the loop's, then the final re-render's)."""
    def __init__(self, G, device):
        super().__init__(G, device)
        self.captured = []

    def g_forward(self, *a, **k):
        rgb, thumb, mask = super().g_forward(*a, **k)
        self.captured.append(rgb[0:1].detach().clone())
        return rgb, thumb, mask


def test_project_wplus_lpips_metric():
    """The smallest generator config of test_gpu_perceptual.py::test_through_the_generator: 64^2 images, three steps."""
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=2)
    g = torch.Generator(device=DEV).manual_seed(0)
    target = torch.randn(2, 3, 64, 64, device=DEV, generator=g).clamp(-1, 1)
    t_thumb = torch.randn(2, 3, 16, 16, device=DEV, generator=g).clamp(-1, 1)
    net = LPIPS("vgg_random", generator=torch.Generator().manual_seed(4))
    cam_cfg = {"img_size": 16, "fov_ang": 6, "dist_radius": 0.12}
    ncfg = {"N_samples": 6, "perturb": False, "static_viewdirs": True}

    def run(proj, **kw):
        torch.manual_seed(3)
        return proj.project_wplus(cam_cfg, ncfg, P.surrogate_loss(target, t_thumb), N_steps_pose=3, N_steps_app=0,
                                  w_avg_samples=64, target_images=target, **kw)

    cap = CapturingProjector(G, DEV)
    out = run(cap, lpips_metric=net, metrics_every=2)
    assert len(cap.captured) == 4
    assert isinstance(out["lpips"], float) and math.isfinite(out["lpips"]) and out["lpips"] > 0
    assert out["lpips"] == float(net(cap.captured[3], target[0:1])[0])
    hist = out["metrics_history"]
    assert hist["steps"] == [0, 2] and tuple(hist["lpips"].shape) == (2,) and len(hist["psnr"]) == 2
    for j, step in enumerate(hist["steps"]):
        assert float(hist["lpips"][j]) == float(net(cap.captured[step], target[0:1])[0])
    # without lpips_metric there is no "lpips" anywhere; with it alone, the final value and nothing of the PSNR / SSIM log.
    # (Separate runs of the loop are not compared: its backward adds with float atomics, so two runs may differ in the last bits.)
    plain = P.FlipProjector(G, DEV)
    off = run(plain, metrics_every=2)
    assert "lpips" not in off and "lpips" not in off["metrics_history"]
    assert set(out) - set(off) == {"lpips"} and off["metrics_history"]["steps"] == hist["steps"]
    cap2 = CapturingProjector(G, DEV)
    only = run(cap2, lpips_metric=net)
    assert len(cap2.captured) == 4 and "metrics_history" not in only and "psnr" not in only
    assert isinstance(only["lpips"], float) and only["lpips"] == float(net(cap2.captured[3], target[0:1])[0])
