"""The Gaussian-window SSIM loss on the GPU (csrc/ssim_loss.hip; metrics.ssim_gaussian, autograd.SsimLossFn,
projector.ssim_loss, project_wplus(ssim_weight=...)) against the definition evaluated in fp64: Wang et al. 2004 with the 11-tap
window g (x) g, g[i] ~ exp(-(i - 5)^2 / 4.5), the windows wholly inside the image, C1 = (0.01 R)^2, C2 = (0.03 R)^2,
    S = (2 mux muy + C1) (2 vxy + C2) / ((mux^2 + muy^2 + C1) (vx + vy + C2)) = (A1 A2) / (B1 B2),
ssim_i = mean of S over image i, loss = weight * mean_i (1 - ssim_i), gradient by fp64 autograd of that expression.

Bounds.  u = 2^-24; first order in u; evaluated in fp64 from the oracle's own intermediates; E is the window's weighted mean.
The kernel takes its moments of A = a - ca, B = b - cb with ca, cb the first pixel of the tile that holds the window's origin
(the tile sides come from the library).  On the way to a first moment a pixel passes K1 = 25 roundings (the shift 1, the two
rounded weights 2, the 11 fmas of the row pass, the 11 of the column pass), a product of two pixels K2 = 27 (two shifts, the
product, 2, 22):
    e(ma) = K1 u E|A|,  e(maa) = K2 u E[A^2],  e(mab) = K2 u E|A B|                                   (likewise for b)
    vx = fma(-ma, ma, maa):      e(vx)  = u (K2 E[A^2] + 2 K1 E|A| |ma| + |vx|)
    vxy = fma(-ma, mb, mab):     e(vxy) = u (K2 E|A B| + K1 (E|A| |mb| + E|B| |ma|) + |vxy|)
    mux = ma + ca:               e(mux) = e(ma) + u |mux|
    A1 = 2 (mux muy) + C1:       e(A1) = 2 (|muy| e(mux) + |mux| e(muy)) + u (2 |mux muy| + |A1| + C1)
    B1 = (mux^2 + muy^2) + C1:   e(B1) = 2 (|mux| e(mux) + |muy| e(muy)) + u (2 (mux^2 + muy^2) + B1 + C1)
    A2 = 2 vxy + C2:             e(A2) = 2 e(vxy) + u (|A2| + C2)
    B2 = (vx + vy) + C2:         e(B2) = e(vx) + e(vy) + u (|vx + vy| + B2 + C2)
(the + C: the constant itself is rounded to fp32).  B1 >= C1 and B2 >= C2, so a moment error of k u E[A^2] is a relative factor
error of at most k u E[A^2] / C2.  With N = A1 A2, D = B1 B2, S = N / D (three more roundings):
    e(S) = (|A2| e(A1) + |A1| e(A2) + u |N|) / D + |S| (B2 e(B1) + B1 e(B2) + u D) / D + u |S|        per window.
The windows of a tile are added in fp32 through a tree of depth d = (tile_h tile_w / threads) + 6 + log2(threads / 64) and the
tiles in fp64: |ssim_i - oracle| <= mean e(S) + d u mean |S|; the loss is one fp32 rounding of weight x the fp64 mean.

Gradient.  The forward stores D2 = Svx = -S / B2, D3 = Svxy = (2 A1) / D and, with ka, kb the first pixel of the plane,
sa = ma + (ca - ka), sb likewise, D1 = fma(-2 sa, Svx, fma(-sb, Svxy, Smu)), Smu = (2 / B1) fma(muy, A2 / B2, -(mux S)):
    e(Svx) = e(S) / B2 + |S| e(B2) / B2^2 + u |Svx|,   e(Svxy) = 2 e(A1) / D + 2 |A1| e(D) / D^2 + u |Svxy|
    q = A2 / B2: e(q) = e(A2) / B2 + |q| e(B2) / B2 + u |q|;   r = 2 / B1: e(r) = 2 e(B1) / B1^2 + u r
    t = muy q - mux S:  e(t) = |q| e(muy) + |muy| e(q) + |S| e(mux) + |mux| e(S) + u (|mux S| + |t|)
    e(Smu) = |t| e(r) + r e(t) + u |Smu|;   e(sa) = e(ma) + u (|ca - ka| + |sa|)
    e(D1) = e(Smu) + 2 (|Svx| e(sa) + |sa| e(Svx)) + |Svxy| e(sb) + |sb| e(Svxy) + u (|Smu - sb Svxy| + |D1|).
The backward is the transposed convolution T_k = G^T D_k (two rounded weights, 22 fmas: e(T_k) = G^T e(D_k) + 24 u G^T |D_k|),
then with pa = a(p) - ka, pb = b(p) - kb (one rounding each), inner = fma(pb, T3, fma(2 pa, T2, T1)) and da = cg inner with
cg = fl(fl(coef) gloss):
    e(inner) = e(T1) + 2 |pa| (e(T2) + u |T2|) + |pb| (e(T3) + u |T3|) + u (|T1 + 2 pa T2| + |inner|)
    e(da) = |cg| e(inner) + 3 u |da|.
The same expression is dS/da for every constant ka, kb, so fp64 autograd of the plain definition is its oracle.

Two conditions keep the bounds honest: (a) the torch fp32 expression (metrics._ssim_gaussian_torch), evaluated on the CPU in the
same test, must meet the same bound, per window and per pixel of the gradient, on every kind except `bright` and `const`; (b) on
`bright` and `const` -- where E[x^2] - mux^2 cancels in plain fp32 and the shifted moments do not -- the kernel's worst per-window
error must not exceed torch fp32's own worst per-window error on the same input.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import autograd as AG, configs, hip, metrics as M, projector as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
K1, K2 = 25, 27
R = 2.0
C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
WEIGHT, GLOSS = 3.5, 0.25
KINDS = ["random", "near", "smooth", "bright", "const", "out", "equal"]
CANCELLING = ("bright", "const")
BC = [(1, 1), (3, 3), (1, 3), (3, 1)]


@functools.lru_cache(maxsize=None)
def tile():
    return hip.ssim_loss_tile()


def sizes():
    th, tw, _ = tile()
    return {"11x11": (11, 11), "12x75": (12, tw + 11), "th-1,tw+1": (th - 1, tw + 1), "th,tw": (th, tw), "th+1,tw-1": (th + 1, tw - 1),
            "th+10,12": (th + 10, 12), "th+11,tw+10": (th + 11, tw + 10), "11,tw+11": (11, tw + 11), "th+10,tw+11": (th + 10, tw + 11),
            "2th+3,2tw+3": (2 * th + 3, 2 * tw + 3)}


SIZE_NAMES = ["11x11", "12x75", "th-1,tw+1", "th,tw", "th+1,tw-1", "th+10,12", "th+11,tw+10", "11,tw+11", "th+10,tw+11", "2th+3,2tw+3"]


def make_pair(kind, B, C, H, W, seed):
    """-> (a, b) fp32 [B,C,H,W] on the CPU."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, C, H, W)
    uni = lambda *s: torch.rand(*s, generator=g) * 2 - 1              # noqa: E731
    nrm = lambda: torch.randn(shape, generator=g)                     # noqa: E731
    if kind == "random":
        return uni(shape), uni(shape)
    if kind == "near":
        a = uni(shape)
        return a, a + 0.02 * nrm()
    if kind == "smooth":
        a = F.avg_pool2d(uni(B, C, H + 8, W + 8), 9, stride=1).contiguous()
        return a, a + 0.05 * nrm()
    if kind == "bright":
        return 0.98 + 0.004 * nrm(), 0.97 + 0.004 * nrm()
    if kind == "const":
        return torch.full(shape, 0.75), torch.full(shape, -0.5)
    if kind == "out":                                                  # values outside [-1, 1]: there is no clamp
        a = 3 * uni(shape)
        return a, a + 0.06 * nrm()
    assert kind == "equal"
    a = uni(shape)
    return a, a.clone()


def gauss(x, transpose=False):
    """E over the windows inside the image (or its transpose, the full convolution), fp64, separable, groups = C."""
    Cc = x.shape[1]
    g = M.gaussian_window(torch.float64)
    wr, wc = g.reshape(1, 1, 1, -1).repeat(Cc, 1, 1, 1), g.reshape(1, 1, -1, 1).repeat(Cc, 1, 1, 1)
    if transpose:
        return F.conv_transpose2d(F.conv_transpose2d(x, wc, groups=Cc), wr, groups=Cc)
    return F.conv2d(F.conv2d(x, wr, groups=Cc), wc, groups=Cc)


def definition(a, b):
    """The definition in fp64 -> dict of the window's terms ([B,C,H-10,W-10])."""
    mux, muy = gauss(a), gauss(b)
    vx, vy, vxy = gauss(a * a) - mux * mux, gauss(b * b) - muy * muy, gauss(a * b) - mux * muy
    A1, A2, B1, B2 = 2 * mux * muy + C1, 2 * vxy + C2, mux * mux + muy * muy + C1, vx + vy + C2
    return dict(mux=mux, muy=muy, vx=vx, vy=vy, vxy=vxy, A1=A1, A2=A2, B1=B1, B2=B2, S=(A1 * A2) / (B1 * B2))


def tile_moments(a, b):
    """Per window: the tile constants ca, cb and the weighted means of |A|, |B|, A^2, B^2, |A B| of the shifted images."""
    th, tw, _ = tile()
    Bn, Cc, H, W = a.shape
    Ho, Wo = H - 10, W - 10
    out = {k: torch.zeros(Bn, Cc, Ho, Wo, dtype=torch.float64) for k in ("ca", "cb", "EA", "EB", "EAA", "EBB", "EAB")}
    for y0 in range(0, Ho, th):
        for x0 in range(0, Wo, tw):
            y1, x1 = min(Ho, y0 + th), min(Wo, x0 + tw)
            ca, cb = a[:, :, y0:y0 + 1, x0:x0 + 1], b[:, :, y0:y0 + 1, x0:x0 + 1]
            A, Bs = (a[:, :, y0:y1 + 10, x0:x1 + 10] - ca).abs(), (b[:, :, y0:y1 + 10, x0:x1 + 10] - cb).abs()
            for k, v in (("EA", A), ("EB", Bs), ("EAA", A * A), ("EBB", Bs * Bs), ("EAB", A * Bs)):
                out[k][:, :, y0:y1, x0:x1] = gauss(v)
            out["ca"][:, :, y0:y1, x0:x1] = ca
            out["cb"][:, :, y0:y1, x0:x1] = cb
    return out


def bounds(a, b, weight, gloss):
    """a, b fp64 -> dict: the oracle's S, ssim, loss and gradient with the bounds of the module docstring."""
    th, tw, threads = tile()
    Bn, Cc, H, W = a.shape
    n_win = Cc * (H - 10) * (W - 10)
    a = a.clone().requires_grad_(True)
    d = definition(a, b)
    ssim = d["S"].mean(dim=(1, 2, 3))
    loss = weight * (1 - ssim).mean()
    (grad,) = torch.autograd.grad(loss, a, torch.tensor(gloss, dtype=torch.float64))
    a = a.detach()
    d = {k: v.detach() for k, v in d.items()}
    t = tile_moments(a, b)
    mux, muy, vx, vy, vxy, A1, A2, B1, B2, S = (d[k] for k in ("mux", "muy", "vx", "vy", "vxy", "A1", "A2", "B1", "B2", "S"))
    ma, mb = mux - t["ca"], muy - t["cb"]
    e_ma, e_mb = K1 * U * t["EA"], K1 * U * t["EB"]
    e_vx = U * (K2 * t["EAA"] + 2 * K1 * t["EA"] * ma.abs() + vx.abs())
    e_vy = U * (K2 * t["EBB"] + 2 * K1 * t["EB"] * mb.abs() + vy.abs())
    e_vxy = U * (K2 * t["EAB"] + K1 * (t["EA"] * mb.abs() + t["EB"] * ma.abs()) + vxy.abs())
    e_mux, e_muy = e_ma + U * mux.abs(), e_mb + U * muy.abs()
    e_A1 = 2 * (muy.abs() * e_mux + mux.abs() * e_muy) + U * (2 * (mux * muy).abs() + A1.abs() + C1)
    e_B1 = 2 * (mux.abs() * e_mux + muy.abs() * e_muy) + U * (2 * (mux * mux + muy * muy) + B1 + C1)
    e_A2 = 2 * e_vxy + U * (A2.abs() + C2)
    e_B2 = e_vx + e_vy + U * ((vx + vy).abs() + B2 + C2)
    N, D = A1 * A2, B1 * B2
    e_D = B2 * e_B1 + B1 * e_B2 + U * D
    e_S = (A2.abs() * e_A1 + A1.abs() * e_A2 + U * N.abs()) / D + S.abs() * e_D / D + U * S.abs()
    depth = th * tw // threads + 6 + int(math.ceil(math.log2(threads // 64)))
    e_ssim = e_S.mean(dim=(1, 2, 3)) + depth * U * S.abs().mean(dim=(1, 2, 3)) + 2.0 ** -50
    e_loss = weight * e_ssim.mean() + U * loss.detach().abs()
    # the derivative maps
    ka, kb = a[:, :, 0:1, 0:1], b[:, :, 0:1, 0:1]
    Svx, Svxy = -S / B2, 2 * A1 / D
    e_Svx = e_S / B2 + S.abs() * e_B2 / B2 ** 2 + U * Svx.abs()
    e_Svxy = 2 * e_A1 / D + 2 * A1.abs() * e_D / D ** 2 + U * Svxy.abs()
    q, r = A2 / B2, 2 / B1
    e_q = e_A2 / B2 + q.abs() * e_B2 / B2 + U * q.abs()
    e_r = 2 * e_B1 / B1 ** 2 + U * r
    tt = muy * q - mux * S
    e_t = q.abs() * e_muy + muy.abs() * e_q + S.abs() * e_mux + mux.abs() * e_S + U * ((mux * S).abs() + tt.abs())
    Smu = r * tt
    e_Smu = tt.abs() * e_r + r * e_t + U * Smu.abs()
    sa, sb = mux - ka, muy - kb
    e_sa, e_sb = e_ma + U * ((t["ca"] - ka).abs() + sa.abs()), e_mb + U * ((t["cb"] - kb).abs() + sb.abs())
    D1 = Smu - 2 * sa * Svx - sb * Svxy
    e_D1 = (e_Smu + 2 * (Svx.abs() * e_sa + sa.abs() * e_Svx) + Svxy.abs() * e_sb + sb.abs() * e_Svxy
            + U * ((Smu - sb * Svxy).abs() + D1.abs()))
    T1, T2, T3 = gauss(D1, True), gauss(Svx, True), gauss(Svxy, True)
    e_T1 = gauss(e_D1, True) + 24 * U * gauss(D1.abs(), True)
    e_T2 = gauss(e_Svx, True) + 24 * U * gauss(Svx.abs(), True)
    e_T3 = gauss(e_Svxy, True) + 24 * U * gauss(Svxy.abs(), True)
    pa, pb = a - ka, b - kb
    inner = T1 + 2 * pa * T2 + pb * T3
    e_inner = (e_T1 + 2 * pa.abs() * (e_T2 + U * T2.abs()) + pb.abs() * (e_T3 + U * T3.abs())
               + U * ((T1 + 2 * pa * T2).abs() + inner.abs()))
    cg = -weight / (Bn * n_win) * gloss
    da = cg * inner
    assert float((da - grad).abs().max()) <= 1e-9 * max(1.0, float(grad.abs().max()))        # the two forms of the oracle agree
    e_da = abs(cg) * e_inner + 3 * U * da.abs()
    return dict(S=S, e_S=e_S, ssim=ssim.detach(), e_ssim=e_ssim, loss=loss.detach(), e_loss=e_loss, grad=grad, e_grad=e_da,
                n_win=n_win)


def torch32(a, b, weight, gloss):
    """The torch fp32 expression on the CPU -> (S, ssim, loss, gradient), as fp64 tensors."""
    a = a.clone().requires_grad_(True)
    ssim, S = M._ssim_gaussian_torch(a, b, R)
    loss = weight * (1 - ssim).mean()
    (g,) = torch.autograd.grad(loss, a, torch.tensor(gloss))
    return S.detach().double(), ssim.detach().double(), loss.detach().double(), g.double()


@functools.lru_cache(maxsize=None)
def case(size, kind):
    """(a, b) fp32 on the CPU, the fp64 oracle with its bounds and the torch fp32 results, computed once per (size, kind)."""
    H, W = sizes()[size]
    B, C = BC[(SIZE_NAMES.index(size) + KINDS.index(kind)) % len(BC)]
    a, b = make_pair(kind, B, C, H, W, seed=sum(map(ord, size + kind)))
    return a, b, bounds(a.double(), b.double(), WEIGHT, GLOSS), torch32(a, b, WEIGHT, GLOSS)


def worst(x):
    return float(x.abs().max())


def ratio(err, bound):
    """max of err / bound where the bound is positive; an error where the bound is zero counts as infinite."""
    err, bound = err.abs().reshape(-1), bound.reshape(-1)
    if bool(((bound == 0) & (err > 0)).any()):
        return math.inf
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZE_NAMES)
def test_value_and_map_match_the_float64_definition(size, kind):
    a, b, o, (S32, ssim32, _, _) = case(size, kind)
    ssim, smap = M.ssim_gaussian(a.to(DEV), b.to(DEV), R, return_map=True)
    assert ssim.dtype == torch.float64 and ssim.device.type == "cpu" and smap.is_cuda and smap.shape == o["S"].shape
    smap = smap.double().cpu()
    e_hip, e_32 = worst(smap - o["S"]), worst(S32 - o["S"])
    print(f"\n{size} {tuple(a.shape)} {kind}: per window |hip - f64| {e_hip:.3g} ({ratio(smap - o['S'], o['e_S']):.3g} of the bound), "
          f"|torch32 - f64| {e_32:.3g} ({ratio(S32 - o['S'], o['e_S']):.3g} of the bound), e_hip / e_32 = {e_hip / e_32 if e_32 else math.nan:.3g}; "
          f"per image |hip - f64| {worst(ssim - o['ssim']):.3g} ({ratio(ssim - o['ssim'], o['e_ssim']):.3g} of the bound)")
    assert bool(((smap - o["S"]).abs() <= o["e_S"]).all())
    assert bool(((ssim - o["ssim"]).abs() <= o["e_ssim"]).all())
    assert torch.equal(M.ssim_gaussian(a.to(DEV), b.to(DEV), R), ssim)
    if kind in CANCELLING:
        assert e_hip <= e_32                                                            # (b)
    else:
        assert bool(((S32 - o["S"]).abs() <= o["e_S"]).all())                           # (a)
        assert bool(((ssim32 - o["ssim"]).abs() <= o["e_ssim"]).all())
    if kind == "equal":
        assert bool((ssim == 1.0).all()) and bool((smap == 1.0).all())                  # exactly
    if kind == "const":
        want = (2 * 0.75 * -0.5 + C1) / (0.75 ** 2 + 0.5 ** 2 + C1)
        assert bool(((smap - want).abs() <= o["e_S"]).all())


def hip_loss_and_grad(a, b, weight=WEIGHT, gloss=GLOSS):
    a = a.to(DEV).requires_grad_(True)
    loss = AG.SsimLossFn.apply(a, b.to(DEV), weight, R)
    loss.backward(torch.tensor(gloss, device=DEV))                   # the upstream gradient: a device scalar
    return loss.detach(), a.grad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZE_NAMES)
def test_gradient_matches_float64_autograd(size, kind):
    a, b, o, (_, _, loss32, g32) = case(size, kind)
    loss, grad = hip_loss_and_grad(a, b)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.shape == a.shape and grad.dtype == torch.float32
    loss, grad = loss.double().cpu(), grad.double().cpu()
    n = a.shape[0] * o["n_win"]
    print(f"\n{size} {tuple(a.shape)} {kind}: loss |hip - f64| {abs(float(loss - o['loss'])):.3g} (bound {float(o['e_loss']):.3g}); "
          f"gradient x windows |hip - f64| {worst(grad - o['grad']) * n:.3g} ({ratio(grad - o['grad'], o['e_grad']):.3g} of the bound), "
          f"|torch32 - f64| {worst(g32 - o['grad']) * n:.3g} ({ratio(g32 - o['grad'], o['e_grad']):.3g} of the bound)")
    assert abs(float(loss - o["loss"])) <= float(o["e_loss"])
    assert bool(((grad - o["grad"]).abs() <= o["e_grad"]).all())
    if kind not in CANCELLING:
        assert abs(float(loss32 - o["loss"])) <= float(o["e_loss"])                     # (a)
        assert bool(((g32 - o["grad"]).abs() <= o["e_grad"]).all())
    if kind == "equal":
        assert float(loss) == 0.0                                                       # exactly


@pytest.mark.parametrize("kind", ["random", "near", "bright"])
def test_one_window_gradient_is_the_closed_form(kind):
    """11 x 11: one window per channel, every pixel in exactly that one; the derivatives written out with numpy."""
    a, b, o, _ = case("11x11", kind)
    _, grad = hip_loss_and_grad(a, b)
    g = M.gaussian_window().numpy()
    w2 = np.outer(g, g)
    x, y = a.double().numpy(), b.double().numpy()
    Bn, Cc = x.shape[:2]
    want = np.zeros_like(x)
    for i in range(Bn):
        for c in range(Cc):
            mx, my = (w2 * x[i, c]).sum(), (w2 * y[i, c]).sum()
            vx, vy = (w2 * (x[i, c] - mx) ** 2).sum(), (w2 * (y[i, c] - my) ** 2).sum()
            vxy = (w2 * (x[i, c] - mx) * (y[i, c] - my)).sum()
            A1, A2, B1, B2 = 2 * mx * my + C1, 2 * vxy + C2, mx * mx + my * my + C1, vx + vy + C2
            S = A1 * A2 / (B1 * B2)
            Smu, Svx, Svxy = 2 * my * A2 / (B1 * B2) - 2 * mx * S / B1, -S / B2, 2 * A1 / (B1 * B2)
            want[i, c] = -WEIGHT * GLOSS / (Bn * Cc) * w2 * (Smu + 2 * (x[i, c] - mx) * Svx + (y[i, c] - my) * Svxy)
    assert bool(((grad.double().cpu() - torch.from_numpy(want)).abs() <= o["e_grad"]).all())


def test_constant_images_have_exactly_zero_variance():
    """0.75 against -0.5 at a size with several tiles: the shifted moments are exactly 0, so S is (2 mux muy + C1) / (mux^2 +
    muy^2 + C1) up to the roundings of the two factors and the quotient (no moment error at all)."""
    th, tw, _ = tile()
    a, b = make_pair("const", 2, 3, 2 * th + 3, tw + 12, 0)
    ssim, smap = M.ssim_gaussian(a.to(DEV), b.to(DEV), R, return_map=True)
    want = (2 * 0.75 * -0.5 + C1) / (0.75 ** 2 + 0.5 ** 2 + C1)
    assert worst(smap.double().cpu() - want) <= 12 * U * abs(want)
    assert bool((smap == smap.reshape(-1)[0]).all())                  # every window: the same bits
    assert worst(ssim - want) <= 12 * U * abs(want)


def test_results_are_bit_identical_and_batch_independent():
    th, tw, _ = tile()
    H, W = 2 * th + 3, tw + 12
    a, b = make_pair("near", 4, 3, H, W, 11)
    a, b = a.to(DEV), b.to(DEV)
    runs = [(M.ssim_gaussian(a[:3], b[:3], R, return_map=True), hip_loss_and_grad(a[:3], b[:3])) for _ in range(3)]
    for (ssim, smap), (loss, grad) in runs[1:]:
        assert torch.equal(ssim, runs[0][0][0]) and torch.equal(smap, runs[0][0][1])
        assert torch.equal(loss, runs[0][1][0]) and torch.equal(grad, runs[0][1][1])
    ssim3 = runs[0][0][0]
    for i in range(3):
        assert float(M.ssim_gaussian(a[i:i + 1], b[i:i + 1], R)[0]) == float(ssim3[i])
    # the coefficient -weight / (B windows) halves exactly with B: image 0's gradient in a batch of 2 (4) is half (a quarter)
    g1 = hip_loss_and_grad(a[:1], b[:1])[1]
    assert float(g1.abs().max()) > 0
    assert torch.equal(hip_loss_and_grad(a[:2], b[:2])[1][0], 0.5 * g1[0])
    assert torch.equal(hip_loss_and_grad(a[:4], b[:4])[1][0], 0.25 * g1[0])


def test_routing_between_the_fused_node_and_the_torch_expression(monkeypatch):
    a, b, o, _ = case("th+11,tw+10", "near")
    da, db = a.to(DEV), b.to(DEV)

    def run():
        x = da.clone().requires_grad_(True)
        loss = P.ssim_loss(x, db, WEIGHT)
        loss.backward(torch.tensor(GLOSS, device=DEV))
        return loss, x.grad

    fused, fused_grad = run()
    assert type(fused.grad_fn).__name__ == "SsimLossFnBackward"
    monkeypatch.setattr(P, "FUSED_SSIM", False)
    plain, plain_grad = run()
    assert plain.is_cuda and type(plain.grad_fn).__name__ != "SsimLossFnBackward"
    assert abs(float(fused.detach()) - float(plain.detach())) <= 2 * float(o["e_loss"])
    assert bool(((fused_grad - plain_grad).double().cpu().abs() <= 2 * o["e_grad"]).all())
    monkeypatch.setattr(P, "FUSED_SSIM", True)
    # a target that requires a gradient, fp64 tensors: the torch expression
    assert type(P.ssim_loss(da, db.clone().requires_grad_(True), 1.0).grad_fn).__name__ != "SsimLossFnBackward"
    assert P.ssim_loss(da.double().requires_grad_(True), db.double(), 1.0).dtype == torch.float64


class CapturingProjector(P.FlipProjector):
    """Keeps every (image, thumbnail) pair the generator returns."""
    def __init__(self, G, device):
        super().__init__(G, device)
        self.captured = []

    def g_forward(self, *a, **k):
        rgb, thumb, mask = super().g_forward(*a, **k)
        self.captured.append((rgb.detach().clone(), thumb.detach().clone()))
        return rgb, thumb, mask


def test_project_wplus_ssim_weight():
    cam_cfg = {"img_size": 8, "fov_ang": 6, "dist_radius": 0.12}
    nerf_cfg = {"N_samples": 6, "perturb": False, "static_viewdirs": True}
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=2)
    g = torch.Generator(device=DEV).manual_seed(0)
    t_rgb = torch.randn(2, 3, 32, 32, device=DEV, generator=g).clamp(-1, 1)
    t_thumb = torch.randn(2, 3, 8, 8, device=DEV, generator=g).clamp(-1, 1)
    loss_fn = P.surrogate_loss(t_rgb, t_thumb)

    def run(proj, **kw):
        torch.manual_seed(3)
        return proj.project_wplus(cam_cfg, nerf_cfg, loss_fn, N_steps_pose=3, N_steps_app=2, w_avg_samples=64,
                                  mask_background=True, **kw)

    plain = P.FlipProjector(G, DEV)
    absent, zero = run(plain), run(plain, ssim_weight=0.0, target_images=t_rgb)
    assert torch.equal(absent["loss_history"], zero["loss_history"]) and set(absent) == set(zero)
    cap = CapturingProjector(G, DEV)
    on = run(cap, ssim_weight=2.0, target_images=t_rgb)
    assert set(on) == set(absent) and on["loss_history"].shape == absent["loss_history"].shape
    assert not torch.equal(on["loss_history"], absent["loss_history"])
    assert torch.equal(run(plain, ssim_weight=2.0, target_images=t_rgb)["loss_history"], on["loss_history"])
    rgb, thumb = cap.captured[0]                                      # step 0: the pose phase, no mask blending
    with torch.no_grad():
        base, term = loss_fn(rgb, thumb), P.ssim_loss(rgb, t_rgb, 2.0)
    assert float(on["loss_history"][0]) == float(base + term)         # the same kernels on the same image: the same bits
    assert float(absent["loss_history"][0]) == float(base)
    o = bounds(rgb.double().cpu(), t_rgb.double().cpu(), 2.0, 1.0)
    got, want = float(on["loss_history"][0]), float(base) + float(o["loss"])
    assert abs(got - want) <= float(o["e_loss"]) + U * abs(want)
