"""PSNR and SSIM on the GPU (cips_3dplusplus_amd/metrics.py, csrc/metrics.hip) against scikit-image's documented defaults for
8-bit images, written out here in float64 with numpy and scipy.ndimage.uniform_filter (win_size 7, uniform window, K1 = 0.01,
K2 = 0.03, sample covariance, the 3-pixel border cropped, data range 255), and `project_wplus(metrics_every=...)`.

Bounds.  The squared error is an integer: exact.  PSNR is one float64 expression of it: equal to the last bit.  A window of the
kernel is evaluated in fp32 from exact integers in at most 12 roundings (csrc/metrics.hip counts 9), each at most u = 2^-24
relative, on factors whose quotients are at most 1 in magnitude: 12 u absolute per window.  The windows of a tile are added in
fp32 through a tree of depth d -- a thread's tile_h * tile_w / threads windows in sequence, the log2(64) butterfly stages of the
wave, the log2(threads / 64) stages over the waves -- so the tile's sum carries at most d u relative to the sum of |S| <= the
window count; the tiles are added in fp64.  Hence |SSIM - oracle| <= (12 + d) u, with d = 8 + 6 + 2 = 16 for the 32 x 64 tile
of 256 threads; the test computes d from what the library reports."""
import functools
import math

import numpy as np
import pytest
import torch
from scipy.ndimage import uniform_filter

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, hip, metrics as M, projector as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


@functools.lru_cache(maxsize=None)
def tile():
    return M.tile()


def ssim_bound():
    th, tw, threads = tile()
    # depth of the fp32 summation tree: windows per thread (sequential) + wave butterfly + stages over the waves (8 + 6 + 2 = 16)
    d = th * tw // threads + int(math.log2(64)) + int(math.ceil(math.log2(threads // 64)))
    return (12 + d) * U


def sizes():
    th, tw, _ = tile()
    return {"7x7": (7, 7), "8x9": (8, 9), "70x133": (70, 133), "tile": (th, tw), "tile+1": (th + 1, tw + 1),
            "tile+6,+7": (th + 6, tw + 7), "2tile+3,tile-1": (2 * th + 3, tw - 1)}


SIZE_NAMES = ["7x7", "8x9", "70x133", "tile", "tile+1", "tile+6,+7", "2tile+3,tile-1"]
KINDS = ["random", "near", "equal", "constant", "flat_noise"]


def make_pair(kind, B, C, H, W, seed):
    """-> (a, b) uint8 [B,C,H,W] numpy."""
    rng = np.random.default_rng(seed)
    shape = (B, C, H, W)
    if kind == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "near":                      # +-3 grey levels
        a = rng.integers(0, 256, shape).astype(np.int64)
        return a.astype(np.uint8), np.clip(a + rng.integers(-3, 4, shape), 0, 255).astype(np.uint8)
    if kind == "equal":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        return a, a.copy()
    if kind == "constant":
        return np.full(shape, 200, np.uint8), np.full(shape, 17, np.uint8)
    assert kind == "flat_noise"             # flat 128 plus +-1 noise
    return (128 + rng.integers(-1, 2, shape)).astype(np.uint8), (128 + rng.integers(-1, 2, shape)).astype(np.uint8)


def oracle_ssim(a, b):
    """structural_similarity's defaults on one 8-bit image pair [C,H,W], in float64."""
    out = []
    for x, y in zip(a.astype(np.float64), b.astype(np.float64)):
        H, W = x.shape
        f = lambda v: uniform_filter(v, size=7)[3:H - 3, 3:W - 3]           # noqa: E731  (windows wholly inside the image)
        ux, uy = f(x), f(y)
        cov = 49.0 / 48.0
        vx, vy, vxy = cov * (f(x * x) - ux * ux), cov * (f(y * y) - uy * uy), cov * (f(x * y) - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        assert S.shape == (H - 6, W - 6)
        out.append(S.mean())
    return float(np.mean(out))


def oracle(a, b):
    """-> (sse int64 [B], psnr float64 [B], ssim float64 [B]) of uint8 numpy batches."""
    sse = ((a.astype(np.int64) - b.astype(np.int64)) ** 2).reshape(a.shape[0], -1).sum(1)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(np.float64(65025.0 * a[0].size) / sse.astype(np.float64))
    return sse, psnr, np.array([oracle_ssim(x, y) for x, y in zip(a, b)])


def check_against_oracle(a, b, tag):
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    sse, ssim = M.image_sse_ssim(ta, tb)
    psnr, ssim2 = M.image_metrics(ta, tb)
    o_sse, o_psnr, o_ssim = oracle(a, b)
    err = np.abs(ssim.numpy() - o_ssim)
    print(f"\n{tag}: sse {sse.tolist()} | ssim {ssim.tolist()} | |ssim - oracle| / 2^-24 = {(err / U).tolist()} "
          f"(bound {ssim_bound() / U:.0f})")
    assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and psnr.dtype == torch.float64
    assert np.array_equal(sse.numpy(), o_sse)                                          # exact
    assert np.array_equal(psnr.numpy().view(np.int64), o_psnr.view(np.int64))          # to the last bit
    assert torch.equal(ssim, ssim2)                                                    # two calls: identical bits
    assert bool((err <= ssim_bound()).all()), (tag, err / U)
    assert torch.equal(M.psnr(ta, tb), psnr) and torch.equal(M.ssim(ta, tb), ssim)
    return sse, psnr, ssim


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,C", [(1, 1), (1, 3), (3, 1), (3, 3)])
@pytest.mark.parametrize("size", SIZE_NAMES)
def test_metrics_match_the_float64_definition(size, B, C, kind):
    H, W = sizes()[size]
    a, b = make_pair(kind, B, C, H, W, seed=sum(map(ord, size + kind)) + 7 * B + C)
    sse, psnr, ssim = check_against_oracle(a, b, f"{size} {H}x{W} B{B} C{C} {kind}")
    if kind == "equal":
        assert bool((sse == 0).all()) and bool(torch.isinf(psnr).all()) and bool((psnr > 0).all())
        assert bool((ssim == 1.0).all())                                               # exactly
    if kind == "constant":
        want = (2 * 200 * 17 + C1) / (200 ** 2 + 17 ** 2 + C1)
        assert bool(((ssim - want).abs() <= ssim_bound()).all())
        assert bool((sse == (200 - 17) ** 2 * C * H * W).all())


def test_squared_error_accumulates_in_64_bits():
    """1024 x 1024 RGB, all 0 against all 255: SSE = 65025 * 3 * 2^20 > 2^37."""
    a = torch.zeros(1, 3, 1024, 1024, dtype=torch.uint8, device=DEV)
    b = torch.full_like(a, 255)
    sse, ssim = M.image_sse_ssim(a, b)
    assert int(sse[0]) == 65025 * 3 * 2 ** 20
    assert abs(float(ssim[0]) - C1 / (255.0 ** 2 + C1)) <= ssim_bound()
    psnr, _ = M.image_metrics(a, b)
    assert float(psnr[0]) == 0.0


def float_images(B, C, H, W, seed):
    """fp32 images with values beyond +-1, infinities, and exact rounding ties (c + 1) * 127.5 == k + 1/2 in fp32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g) * 0.8
    k = torch.arange(0, 255, dtype=torch.float64)
    c = ((k + 0.5) / 127.5 - 1.0).float()
    ties = c[((c + 1.0) * 127.5 == (k + 0.5).float())]
    assert ties.numel() >= 8 and bool((ties == 0).any())                               # (0 -> 127.5 is one of them)
    flat = x.reshape(-1)
    flat[:ties.numel()] = ties
    flat[ties.numel():ties.numel() + 6] = torch.tensor([-3.0, 2.5, 1.0, -1.0, float("inf"), float("-inf")])
    idx = torch.randperm(flat.numel(), generator=g)
    return flat[idx].reshape(B, C, H, W).contiguous(), ties.numel()


def test_fp32_operands_are_quantised_like_rgb_to_uint8():
    th, tw, _ = tile()
    H, W = th + 6, tw + 7
    fa, n_ties = float_images(2, 3, H, W, 1)
    fb, _ = float_images(2, 3, H, W, 2)
    fa, fb = fa.to(DEV), fb.to(DEV)
    assert float(fa.abs().max()) > 1 and n_ties >= 8
    ua, ub = hip.rgb_to_uint8(fa), hip.rgb_to_uint8(fb)
    ref = M.image_sse_ssim(ua, ub)
    check_against_oracle(ua.cpu().numpy(), ub.cpu().numpy(), "quantised fp32 pair")
    for a, b in ((fa, fb), (fa, ub), (ua, fb)):
        got = M.image_sse_ssim(a, b)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(M.image_metrics(fa, ub)[0], M.image_metrics(ua, ub)[0])
    # an image against its own quantisation: no error at all
    sse, ssim = M.image_sse_ssim(fa, ua)
    assert bool((sse == 0).all()) and bool((ssim == 1.0).all())
    # [C, H, W] is one image
    one = M.image_sse_ssim(fa[1], ub[1])
    assert one[0].shape == (1,) and int(one[0][0]) == int(ref[0][1]) and float(one[1][0]) == float(ref[1][1])


@pytest.mark.parametrize("C", [1, 3])
def test_an_image_does_not_depend_on_its_batch(C):
    th, tw, _ = tile()
    a, b = make_pair("near", 3, C, 2 * th + 3, tw + 7, seed=5)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    sse, ssim = M.image_sse_ssim(ta, tb)
    for i in range(3):
        s1, m1 = M.image_sse_ssim(ta[i:i + 1], tb[i:i + 1])
        assert int(s1[0]) == int(sse[i]) and float(m1[0]) == float(ssim[i])
    fsse, fssim = M.image_sse_ssim(ta.flip(0), tb.flip(0))
    assert torch.equal(fsse, sse.flip(0)) and torch.equal(fssim, ssim.flip(0))


def test_metrics_log_rows_and_single_read():
    a, b = make_pair("near", 4, 3, 40, 75, seed=9)
    imgs, target = torch.from_numpy(a).to(DEV), torch.from_numpy(b[:1]).to(DEV)
    each = [M.image_metrics(imgs[i:i + 1], target) for i in range(4)]
    log = M.MetricsLog(target, 6)
    assert log.update(30, imgs[3:4], row=4) == 4                       # out of order, rows 1, 3 and 5 never written
    assert log.update(10, imgs[1:2], row=2) == 2
    assert log.update(0, imgs[0:1]) == 0                               # the next free row
    assert log._record.shape == (6, 2) and log._record.is_cuda
    rec = log._record.cpu()
    assert bool((rec[[1, 3, 5]] == 0).all()) and bool((rec[[0, 2, 4], 0] > 0).all())
    res = log.result()
    assert res["steps"] == [30, 10, 0] and res["psnr"].shape == (3,) and res["ssim"].dtype == torch.float64
    for j, i in enumerate((3, 1, 0)):
        assert float(res["psnr"][j]) == float(each[i][0][0]) and float(res["ssim"][j]) == float(each[i][1][0])
    log.update(11, imgs[2], row=2)                                     # a row written again holds the new image ([C,H,W] accepted)
    res = log.result()
    assert res["steps"] == [30, 0, 11] and float(res["ssim"][2]) == float(each[2][1][0])
    log.update(1, imgs[0:1]); log.update(2, imgs[0:1]); log.update(3, imgs[0:1])
    with pytest.raises(ValueError, match="full"):
        log.update(4, imgs[0:1])
    # an fp32 target and fp32 images: the same rows as their quantisations
    ft = torch.from_numpy(b[:1]).to(DEV).float() / 127.5 - 1.0
    flog = M.MetricsLog(ft, 1)
    flog.update(0, imgs[0:1])
    assert float(flog.result()["ssim"][0]) == float(M.image_metrics(imgs[0:1], hip.rgb_to_uint8(ft))[1][0])


class CapturingProjector(P.FlipProjector):
    """Keeps view 0 of every image the generator returns (the loop's, then the final re-render's)."""
    def __init__(self, G, device):
        super().__init__(G, device)
        self.captured = []

    def g_forward(self, *a, **k):
        rgb, thumb, mask = super().g_forward(*a, **k)
        self.captured.append(rgb[0:1].detach().clone())
        return rgb, thumb, mask


def test_project_wplus_metrics_every():
    cam_cfg = {"img_size": 8, "fov_ang": 6, "dist_radius": 0.12}
    nerf_cfg = {"N_samples": 6, "perturb": False, "static_viewdirs": True}
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=2)
    g = torch.Generator(device=DEV).manual_seed(0)
    t_rgb = torch.randn(2, 3, 32, 32, device=DEV, generator=g).clamp(-1, 1)
    t_thumb = torch.randn(2, 3, 8, 8, device=DEV, generator=g).clamp(-1, 1)

    def run(proj, **kw):
        torch.manual_seed(3)
        return proj.project_wplus(cam_cfg, nerf_cfg, P.surrogate_loss(t_rgb, t_thumb), N_steps_pose=3, N_steps_app=2,
                                  w_avg_samples=64, mask_background=True, **kw)

    cap = CapturingProjector(G, DEV)
    out = run(cap, metrics_every=2, target_images=t_rgb)
    hist = out["metrics_history"]
    assert hist["steps"] == [0, 2, 4] and len(cap.captured) == 6
    for j, step in enumerate(hist["steps"]):
        psnr, ssim = M.image_metrics(cap.captured[step], t_rgb[0:1])
        assert float(hist["psnr"][j]) == float(psnr[0]) and float(hist["ssim"][j]) == float(ssim[0])
        assert math.isfinite(float(psnr[0])) and -1.0 <= float(ssim[0]) <= 1.0
    psnr, ssim = M.image_metrics(cap.captured[5], t_rgb[0:1])
    assert isinstance(out["psnr"], float) and out["psnr"] == float(psnr[0]) and out["ssim"] == float(ssim[0])

    # metrics_every = 0: no new keys, the same loop (run twice: equal bits), and its final state re-rendered here gives the
    # metrics the logging run returned
    plain = P.FlipProjector(G, DEV)
    off, off2 = run(plain), run(plain, target_images=t_rgb)
    assert not {"psnr", "ssim", "metrics_history"} & set(off) and not {"psnr", "ssim", "metrics_history"} & set(off2)
    assert set(out) - set(off) == {"psnr", "ssim", "metrics_history"}
    assert torch.equal(off["loss_history"], off2["loss_history"]) and torch.equal(off["loss_history"], out["loss_history"])
    with torch.no_grad():
        rgb, _, _ = plain.g_forward(off["G"], off["w_render_opt"], off["w_decoder_opt"], off["noise_bufs"], cam_cfg, nerf_cfg,
                                    rot=torch.cat([off["azim"], off["elev"]], 1))
    psnr, ssim = M.image_metrics(rgb[0:1], t_rgb[0:1])
    assert out["psnr"] == float(psnr[0]) and out["ssim"] == float(ssim[0])
