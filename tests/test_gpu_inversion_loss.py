"""The fused inversion-loss terms of csrc/inversion_loss.hip -- the noise regulariser over a list of buffers and the mask
blending -- and the knobs of `FlipProjector.project_wplus` that use them, against the reference's torch expressions
(/root/reference/exp/cips3d/models/projector_v10.py:1164-1200, mask of :268-273) evaluated in fp64 on the CPU with autograd.

Every bound below is derived from the arithmetic that is being checked (u = 2^-24, the unit roundoff of fp32; first order in u;
the bounds are evaluated in fp64 from the reference's own intermediates), and every test also evaluates the torch fp32
expression on the CPU and requires it to meet the same bound: a bound the reference's own fp32 cannot meet would be wrong.

Regulariser.  Level l of a buffer is l pooling steps; one step is three additions in two stages and an exact scaling, so
|n_l - exact| <= 2 l u a_l with a_l the same pyramid of |v| (a_l >= |n_l|).  A product of two level-l values then carries
(4 l + 1) u a_l a_l' (the + 1: torch rounds the product; the kernel's fma does not).  The kernel sums count_l products as: 16
sequential fmas per thread, the 6-stage wave butterfly, 2 stages over the workgroup's waves (nr_partial_kernel), then per level
ceil(blocks_l / 64) sequential additions per lane and another 6-stage butterfly (nr_finish_kernel): every product passes through
at most D_l = 16 + 6 + 2 + ceil(blocks_l / 64) + 6 roundings.  The division by count_l is correctly rounded (+ 1).  So
    |mean - exact| <= E_l = u (4 l + 2 + D_l) mean(a_l roll(a_l))                                       per mean.
Value: w sum m^2 with every square and every addition rounded; the kernel adds at most 2 ceil(levels / 16) + 16 terms in a
chain, torch 2 levels, the weight is one more: |value - exact| <= w sum (2 |m| E + E^2) + u (2 levels + 19) w sum (|m| + E)^2.
Gradient: d/dv = w sum_l 4^-l (2 / count_l) up_l(m_w (left + right) + m_h (upper + lower)).  Per level the coefficient is at most
4 roundings, the neighbour sum 1, the product 1, the sum of the two directions 1 (8 with one spare for autograd's separate
accumulation of the two roll directions), the neighbours carry 2 l u a_l, the means E_l, and the levels are accumulated in a
chain (L additions in the kernel, 2 per level in autograd):
    |grad - exact| <= w sum_l 4^-l (2 / count_l) up_l( (E_w + |m_w| (2 l + 8 + 2 L) u) (a_left + a_right) + (same for h) ).

Mask blending.  m = sum_i cy_i sum_j cx_j t_ij with t = 1 - mask (one rounding) and torch's cubic coefficients (A = -0.75).  For
the factors tested (powers of two) the source coordinate and its fraction are exact; a coefficient is a Horner form of six
operations on intermediates of magnitude <= 6 whose errors are amplified by at most two more multiplications by x <= 2:
|c - exact| <= EPS_C = 40 u (the outer pair: 6 + 12 + 9 + 6 + 3.1 + 0.1 + 1.5 u for x = t + 1; the inner pair <= 9 u).  With one
rounding each for t, the product with cx, the three additions of a row, the product with cy and the three additions of the
column (9 u):
    |m - exact| <= E_m = sum_ij |t_ij| (EPS_C (|cy_i| + |cx_j|) + EPS_C^2) + 9 u sum_ij |cy_i| |cx_j| |t_ij|.
Forward x m + x (1 - m): an error of m cancels between the two products, what remains is one rounding of x m, two of x (1 - m)
and one of the sum: |out - x| <= 3 u |x| (|m| + |1 - m| + 2 E_m).  Gradient g m: |dx - g m| <= |g| (E_m + u (|m| + E_m)).
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, hip, projector as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
EPS_C = 40 * U


# ----------------------------------------------------------------------------------------------------------- regulariser
def reference_regulariser(bufs):
    """projector_v10.py:1185-1194 -> (reg, [means per buffer and level, (w, h)])."""
    reg, means = 0, []
    for v in bufs:
        noise = v
        while True:
            mw, mh = (noise * torch.roll(noise, shifts=1, dims=3)).mean(), (noise * torch.roll(noise, shifts=1, dims=2)).mean()
            reg = reg + mw ** 2
            reg = reg + mh ** 2
            means.append((mw, mh))
            if noise.shape[2] <= 8:
                break
            noise = F.avg_pool2d(noise, kernel_size=2)
    return reg, means


def make_bufs(sizes, kind, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for b, s in sizes:
        v = torch.randn(b, 1, s, s, generator=g)
        if kind == "smooth":                    # 3 x 3 circular box filter: means far from zero
            v = sum(torch.roll(v, (dy, dx), (2, 3)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9
        elif kind == "zero":
            v = torch.zeros_like(v)
        out.append(v.contiguous())
    return out


def regulariser_bounds(bufs64, weight, means64):
    """-> (E per mean [(Ew, Eh)], value bound, [gradient bound per buffer]) as derived in the module docstring."""
    E, grad_bounds, k = [], [], 0
    levels_total = len(means64)
    for v in bufs64:
        a, l, s = v.abs(), 0, v.shape[2]
        L = 1 + max(0, math.ceil(math.log2(s / 8)))
        gb = torch.zeros_like(v)
        while True:
            cnt = a.numel()
            D = 16 + 6 + 2 + math.ceil(math.ceil(cnt / 4096) / 64) + 6
            Ew = U * (4 * l + 2 + D) * float((a * torch.roll(a, 1, 3)).mean())
            Eh = U * (4 * l + 2 + D) * float((a * torch.roll(a, 1, 2)).mean())
            E.append((Ew, Eh))
            mw, mh = (abs(float(m)) for m in means64[k])
            r = (2 * l + 8 + 2 * L) * U
            t = (Ew + mw * r) * (torch.roll(a, 1, 3) + torch.roll(a, -1, 3)) + (Eh + mh * r) * (torch.roll(a, 1, 2) + torch.roll(a, -1, 2))
            t = t * (weight * 2 / cnt * 0.25 ** l)
            gb += F.interpolate(t, scale_factor=2 ** l, mode="nearest") if l else t
            k += 1
            if a.shape[2] <= 8:
                break
            a, l = F.avg_pool2d(a, 2), l + 1
        assert l + 1 == L
        grad_bounds.append(gb)
    assert k == levels_total
    vb = 0.0
    sq = 0.0
    for (Ew, Eh), (mw, mh) in zip(E, means64):
        for e, m in ((Ew, abs(float(mw))), (Eh, abs(float(mh)))):
            vb += 2 * m * e + e * e
            sq += (m + e) ** 2
    return E, weight * (vb + U * (2 * levels_total + 19) * sq), grad_bounds


TINY_DECODER = [(1, 8), (1, 16), (1, 16), (1, 32), (1, 32)]      # create_noise_bufs of the tiny generator (8^2 start, 32^2 image)
REG_SHAPES = {"4": [(1, 4)], "8": [(1, 8)], "16": [(1, 16)], "B2_32": [(2, 32)], "tiny_decoder": TINY_DECODER, "128": [(1, 128)],
              "1024": [(1, 1024)]}


@functools.lru_cache(maxsize=None)
def regulariser_case(name, kind, weight):
    """Inputs and every CPU result of one case, computed once: fp64 reference with autograd, the torch fp32 expression, bounds."""
    bufs = make_bufs(REG_SHAPES[name], kind, seed=sum(map(ord, name + kind)))
    b64 = [b.double().requires_grad_(True) for b in bufs]
    reg64, means64 = reference_regulariser(b64)
    val64 = weight * reg64
    g64 = torch.autograd.grad(val64, b64)
    b32 = [b.clone().requires_grad_(True) for b in bufs]
    reg32, means32 = reference_regulariser(b32)
    val32 = reg32 * weight
    g32 = torch.autograd.grad(val32, b32)
    E, vb, gb = regulariser_bounds([b.detach() for b in b64], weight, means64)
    return {"bufs": bufs, "val64": float(val64), "g64": [g.detach() for g in g64], "means64": [(float(a), float(b)) for a, b in means64],
            "val32": float(val32), "g32": [g.detach() for g in g32], "means32": [(float(a), float(b)) for a, b in means32],
            "E": E, "vb": vb, "gb": gb}


def check_regulariser(tag, case, value, grads, means):
    """value / grads / means of one implementation against the case's fp64 reference and bounds -> (value error, gradient error),
    both relative to the reference's size (max-norm)."""
    for i, ((mw, mh), (rw, rh), (Ew, Eh)) in enumerate(zip(means, case["means64"], case["E"])):
        assert abs(mw - rw) <= Ew and abs(mh - rh) <= Eh, (tag, "mean", i, mw - rw, Ew, mh - rh, Eh)
    assert abs(value - case["val64"]) <= case["vb"], (tag, "value", value - case["val64"], case["vb"])
    worst = 0.0
    for i, (g, r, b) in enumerate(zip(grads, case["g64"], case["gb"])):
        err = (g.double() - r).abs()
        assert bool((err <= b).all()), (tag, "gradient", i, float((err - b).max()), float(b.max()))
        worst = max(worst, float(err.max()) / max(float(r.abs().max()), 1e-300))
    return abs(value - case["val64"]) / max(abs(case["val64"]), 1e-300), worst


@pytest.mark.parametrize("kind", ["white", "smooth"])
@pytest.mark.parametrize("name", list(REG_SHAPES))
def test_noise_regulariser_value_and_gradients(name, kind):
    """cips3d_noise_reg / _bwd on the shapes that reach each branch (one level with the wrap as the whole row; the exit condition;
    two levels; the batch in the mean; several sizes in one launch; more than one tile; the production size, whose coarsest
    levels need the second pyramid pass) against fp64 autograd, per mean, for the value and for every buffer's gradient, with the
    bounds of the module docstring; the torch fp32 expression must meet the same bounds; two calls give identical bits."""
    weight = 1e5
    case = regulariser_case(name, kind, weight)
    bufs = [b.to(DEV) for b in case["bufs"]]
    gloss = torch.ones((), device=DEV)
    loss, ws = hip.noise_reg(bufs, weight)
    grads = hip.noise_reg_bwd(bufs, weight, ws, gloss)
    n_levels = len(case["means64"])
    means = ws[-2 * n_levels:].cpu().reshape(n_levels, 2).tolist()
    loss2, ws2 = hip.noise_reg(bufs, weight)
    grads2 = hip.noise_reg_bwd(bufs, weight, ws2, gloss)
    assert torch.equal(loss, loss2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    ev_t, eg_t = check_regulariser("torch fp32", case, case["val32"], case["g32"], case["means32"])
    ev_h, eg_h = check_regulariser("hip", case, float(loss), [g.cpu() for g in grads], means)
    print(f"\nnoise_reg {name} {kind}: value rel err hip {ev_h:.2e} torch-fp32 {ev_t:.2e} ratio {ev_h / max(ev_t, 1e-300):.2f} | "
          f"gradient rel err hip {eg_h:.2e} torch-fp32 {eg_t:.2e} ratio {eg_h / max(eg_t, 1e-300):.2f}")
    # a gradient scaled by the incoming one (a device scalar), and the node: same bits as the raw calls
    half = hip.noise_reg_bwd(bufs, weight, ws, torch.full((), 0.5, device=DEV))
    assert all(torch.equal(h, 0.5 * g) for h, g in zip(half, grads))
    leaves = [b.clone().requires_grad_(True) for b in bufs]
    out = P.noise_regulariser(leaves, weight)
    assert type(out.grad_fn).__name__.startswith("NoiseRegFn")
    out.backward()
    assert torch.equal(out.detach(), loss) and all(torch.equal(a.grad, g) for a, g in zip(leaves, grads))


@pytest.mark.parametrize("name", list(REG_SHAPES))
def test_noise_regulariser_of_zero_buffers_is_exactly_zero(name):
    bufs = [b.to(DEV) for b in make_bufs(REG_SHAPES[name], "zero", 0)]
    loss, ws = hip.noise_reg(bufs, 1e5)
    grads = hip.noise_reg_bwd(bufs, 1e5, ws, torch.ones((), device=DEV))
    assert float(loss) == 0.0
    for g in grads:
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0


def test_noise_regulariser_dispatch():
    """Odd pooled sides, CPU tensors, nothing that requires a gradient and other dtypes keep the torch expression; a list longer
    than one launch's 32 buffers is still one node with the same value as the sum of its parts' references."""
    g = torch.Generator().manual_seed(5)
    odd = [torch.randn(1, 1, 18, 18, generator=g).to(DEV).requires_grad_(True)]
    assert not hip.noise_reg_supported(odd)
    assert "NoiseRegFn" not in type(P.noise_regulariser(odd, 2.0).grad_fn).__name__
    ok = [torch.randn(1, 1, 16, 16, generator=g).to(DEV)]
    assert P.noise_regulariser(ok, 2.0).grad_fn is None                                     # no leaf requires a gradient
    assert "NoiseRegFn" not in type(P.noise_regulariser([ok[0].double().requires_grad_(True)], 2.0).grad_fn).__name__
    many = [torch.randn(1, 1, 8 if i % 2 else 16, 8 if i % 2 else 16, generator=g) for i in range(35)]
    ref, _ = reference_regulariser([b.double() for b in many])
    leaves = [b.to(DEV).requires_grad_(i != 3) for i, b in enumerate(many)]
    out = P.noise_regulariser(leaves, 3.0)
    assert "NoiseRegFn" in type(out.grad_fn).__name__
    assert abs(float(out) - 3.0 * float(ref)) <= 1e-5 * 3.0 * float(ref)                    # (dispatch check; bounds: the test above)
    out.backward()
    assert leaves[3].grad is None and all(b.grad is not None and bool(b.grad.abs().max() > 0) for i, b in enumerate(leaves) if i != 3)


# ----------------------------------------------------------------------------------------------------------- mask blending
def bicubic_taps64(n_out, n_in, f):
    """torch's bicubic taps in fp64: -> (|weights| accumulated per clamped source index [n_out, n_in], tap counts [n_out, n_in],
    signed weights [n_out, n_in])."""
    A = -0.75
    Wabs, Cnt, Wsgn = np.zeros((n_out, n_in)), np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    for d in range(n_out):
        src = (d + 0.5) / f - 0.5
        i0 = math.floor(src)
        t = src - i0
        c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1                   # noqa: E731
        c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A             # noqa: E731
        for j, c in enumerate((c2(t + 1), c1(t), c1(1 - t), c2(2 - t))):
            i = min(max(i0 - 1 + j, 0), n_in - 1)
            Wabs[d, i] += abs(c); Cnt[d, i] += 1; Wsgn[d, i] += c
    return torch.from_numpy(Wabs), torch.from_numpy(Cnt), torch.from_numpy(Wsgn)


def reference_mask(mask, channels, size):
    """`_G_forward`, :269-273."""
    mt = 1 - mask.detach().expand(-1, channels, -1, -1)
    return F.interpolate(mt, scale_factor=size / mt.shape[-1], recompute_scale_factor=False, mode="bicubic")


def mask_bound(mask64, H, W, f):
    """E_m of the module docstring, [B,1,H,W]."""
    t = (1 - mask64).abs()
    Wy, Cy, Sy = bicubic_taps64(H, mask64.shape[2], f)
    Wx, Cx, Sx = bicubic_taps64(W, mask64.shape[3], f)
    mm = lambda L, M, R: torch.einsum("yi,bcij,xj->bcyx", L, M, R)          # noqa: E731
    Em = EPS_C * (mm(Wy, t, Cx) + mm(Cy, t, Wx)) + EPS_C ** 2 * mm(Cy, t, Cx) + 9 * U * mm(Wy, t, Wx)
    return Em, mm(Sy, 1 - mask64, Sx)


BLEND_SHAPES = {"f1": ((1, 8, 8), 1), "f4": ((2, 8, 8), 4), "f16": ((2, 16, 16), 16), "f2": ((1, 6, 7), 2)}


@functools.lru_cache(maxsize=None)
def blend_case(name, kind):
    (B, h, w), f = BLEND_SHAPES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name + kind)))
    if kind == "random":
        mask = torch.rand(B, 1, h, w, generator=g)
    elif kind == "exact01":                     # random with exact zeros and ones (the render's mask saturates)
        mask = (torch.rand(B, 1, h, w, generator=g) * 1.5 - 0.25).clamp(0, 1)
        mask[:, :, 0, 0], mask[:, :, -1, -1] = 0.0, 1.0
    else:                                       # checkerboard: the bicubic mask leaves [0, 1]
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        mask = ((yy + xx) % 2).float().reshape(1, 1, h, w).repeat(B, 1, 1, 1)
    H, W = h * f, w * f
    x = torch.randn(B, 3, H, W, generator=g)
    gout = torch.randn(B, 3, H, W, generator=g)
    m64 = reference_mask(mask.double(), 3, W)
    Em, m_own = mask_bound(mask.double(), H, W, f)
    assert float((m_own - m64[:, :1]).abs().max()) < 1e-13          # the bound's taps are the reference's
    x64 = x.double().requires_grad_(True)
    out64 = x64 * m64 + x64.detach() * (1 - m64)
    (gx64,) = torch.autograd.grad(out64, x64, gout.double())
    x32 = x.clone().requires_grad_(True)
    m32 = reference_mask(mask, 3, W)
    out32 = x32 * m32 + x32.detach() * (1 - m32)
    (gx32,) = torch.autograd.grad(out32, x32, gout)
    fwd_b = 3 * U * x.double().abs() * (m64.abs() + (1 - m64).abs() + 2 * Em)
    bwd_b = gout.double().abs() * (Em + U * (m64.abs() + Em))
    border = torch.zeros(H, W, dtype=torch.bool)
    k = 2 * f
    border[:k], border[-k:], border[:, :k], border[:, -k:] = True, True, True, True
    return {"mask": mask, "x": x, "gout": gout, "m64": m64, "out64": out64.detach(), "gx64": gx64, "out32": out32.detach(),
            "gx32": gx32, "fwd_b": fwd_b, "bwd_b": bwd_b, "border": border, "Em": Em}


def check_blend(tag, case, out, gx):
    """-> worst error / bound over (forward border, forward interior, gradient border, gradient interior)."""
    ratios = []
    for what, got, ref, bound in (("forward", out, case["out64"], case["fwd_b"]), ("gradient", gx, case["gx64"], case["bwd_b"])):
        err = (got.double() - ref).abs()
        for region, sel in (("border", case["border"]), ("interior", ~case["border"])):
            if not bool(sel.any()):
                ratios.append(0.0)
                continue
            e, b = err[..., sel], bound[..., sel]
            assert bool((e <= b).all()), (tag, what, region, float((e - b).max()), float(b.max()))
            ratios.append(float((e / b.clamp_min(1e-300)).max()))
    return ratios


@pytest.mark.parametrize("kind", ["random", "exact01", "checkerboard"])
@pytest.mark.parametrize("name", list(BLEND_SHAPES))
def test_mask_blend_forward_and_gradient(name, kind):
    """cips3d_mask_blend / _bwd for the factors 1, 2 (an image width that is no multiple of four), 4 and 16 against the reference's
    expression in fp64, element by element with the bounds of the module docstring, border rows and columns apart from the
    interior; the torch fp32 expression must meet the same bounds; the overshoot of the checkerboard's bicubic mask is kept; two
    calls give identical bits."""
    case = blend_case(name, kind)
    x, mask, gout = case["x"].to(DEV), case["mask"].to(DEV), case["gout"].to(DEV)
    out, gx = hip.mask_blend(x, mask), hip.mask_blend(gout, mask, backward=True)
    assert torch.equal(out, hip.mask_blend(x, mask)) and torch.equal(gx, hip.mask_blend(gout, mask, backward=True))
    r_t = check_blend("torch fp32", case, case["out32"], case["gx32"])
    r_h = check_blend("hip", case, out.cpu(), gx.cpu())
    print(f"\nmask_blend {name} {kind}: error / bound (fwd border, fwd interior, grad border, grad interior) hip "
          + " ".join(f"{r:.3f}" for r in r_h) + " | torch-fp32 " + " ".join(f"{r:.3f}" for r in r_t))
    m_hip = hip.mask_blend(torch.ones_like(x), mask, backward=True).cpu()          # g = 1: the kernel's own m
    if kind == "checkerboard" and BLEND_SHAPES[name][1] > 1:
        lo, hi = float(case["m64"].min()), float(case["m64"].max())
        assert lo < -0.05 and hi > 1.05                                            # the reference leaves [0, 1] ...
        assert abs(float(m_hip.min()) - lo) <= float(case["Em"].max()) and abs(float(m_hip.max()) - hi) <= float(case["Em"].max())
        assert float(m_hip.min()) < -0.05 and float(m_hip.max()) > 1.05            # ... and the kernel follows it, unclamped
    if BLEND_SHAPES[name][1] == 1:
        assert torch.equal(m_hip, (1 - case["mask"]).expand_as(m_hip))             # factor 1: m is 1 - mask itself
    # the node: same bits, and no gradient for the mask
    leaf, mleaf = x.clone().requires_grad_(True), mask.clone().requires_grad_(True)
    y = P.mask_blend(leaf, mleaf)
    assert type(y.grad_fn).__name__.startswith("MaskBlendFn")
    y.backward(gout)
    assert torch.equal(y.detach(), out) and torch.equal(leaf.grad, gx) and mleaf.grad is None


def test_mask_blend_dispatch():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 3, 12, 12, generator=g).to(DEV).requires_grad_(True)
    y = P.mask_blend(x, torch.rand(1, 1, 8, 8, generator=g).to(DEV))              # factor 1.5: the torch expression
    assert "MaskBlendFn" not in type(y.grad_fn).__name__ and y.shape == x.shape
    assert hip.mask_blend_factor(x, torch.rand(1, 1, 4, 4, device=DEV)) == 3
    assert hip.mask_blend_factor(x, torch.rand(1, 1, 4, 6, device=DEV)) == 0


# ------------------------------------------------------------------------------------------------------------------ the loop
class RecordingProjector(P.FlipProjector):
    def _decoder_optimizer(self, *a, **k):
        w, noise_bufs, opt = super()._decoder_optimizer(*a, **k)
        self.initial_noise = [b.detach().clone() for b in noise_bufs]
        return w, noise_bufs, opt


def test_project_wplus_with_every_loss_knob():
    """The loop with the noise buffers optimised, the regulariser, the mask blending and the MSE term on the tiny generator of the
    other inversion tests: it finishes, the loss history is finite and has one entry per step, and the appearance phase moved
    the noise buffers."""
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2, 1), DEV, seed=2)
    g = torch.Generator(device=DEV).manual_seed(0)
    t_rgb = torch.randn(2, 3, 32, 32, device=DEV, generator=g).clamp(-1, 1)
    t_thumb = torch.randn(2, 3, 8, 8, device=DEV, generator=g).clamp(-1, 1)
    proj = RecordingProjector(G, DEV)
    out = proj.project_wplus({"img_size": 8, "fov_ang": 6, "dist_radius": 0.12},
                             {"N_samples": 6, "perturb": False, "static_viewdirs": True}, P.surrogate_loss(t_rgb, t_thumb),
                             N_steps_pose=2, N_steps_app=3, w_avg_samples=64, optim_noise_bufs=True, zero_noise_bufs=False,
                             regularize_noise_weight=1e5, mask_background=True, mse_weight=1.0, target_images=t_rgb)
    hist = out["loss_history"]
    assert hist.shape == (5,) and bool(torch.isfinite(hist).all())
    assert [tuple(b.shape) for b in out["noise_bufs"]] == [(b, 1, s, s) for b, s in TINY_DECODER]
    for now, before in zip(out["noise_bufs"], proj.initial_noise):
        assert bool(torch.isfinite(now).all()) and not torch.equal(now, before)


def test_composite_step_loss_against_fp64():
    """One step's loss through the fused nodes -- surrogate(blend(rgb), thumb) + mse_weight mse(blend(rgb), target) +
    regulariser -- for fixed tensors against the torch expressions in fp64 on the CPU: the value and the gradients with respect
    to rgb, thumb and every noise buffer (the mask takes none).  Bounds: the regulariser's and the blend's of the module
    docstring; a squared-difference term c sum (a - b)^2 of the existing node is (3 roundings per term, 16 fmas per thread, 6 + 2
    stages, <= 2 + 6 + 2 in the total, the weight and the sum of the terms: 39 u) relative; its gradient 2 c g (a - b) is 4 u
    relative (c, the product with the incoming gradient, the difference, the product; torch's weighted thumbnail term has one
    multiplication more: 5 u) plus 2 c times the error of a; the blend's gradient multiplies the sum of the two incoming ones
    (+ 1 u) by m."""
    mse_weight, reg_weight, thumb_weight = 1.0, 1e5, 50.0
    g = torch.Generator().manual_seed(11)
    rgb, thumb = torch.randn(2, 3, 32, 32, generator=g), torch.randn(2, 3, 8, 8, generator=g)
    t_rgb, t_thumb = torch.randn(2, 3, 32, 32, generator=g).clamp(-1, 1), torch.randn(2, 3, 8, 8, generator=g).clamp(-1, 1)
    mask = (torch.rand(2, 1, 8, 8, generator=g) * 1.5 - 0.25).clamp(0, 1)
    bufs = make_bufs(TINY_DECODER, "smooth", 12)

    def run(dt, dev, blend, reg, loss_fn, mse):
        r, t = rgb.to(dev, dt).requires_grad_(True), thumb.to(dev, dt).requires_grad_(True)
        mk = mask.to(dev, dt).requires_grad_(True)
        nb = [b.to(dev, dt).requires_grad_(True) for b in bufs]
        rb = blend(r, mk)
        loss = loss_fn(rb, t) + mse(rb) + reg(nb)
        *grads, g_mask = torch.autograd.grad(loss, [r, t] + nb + [mk], allow_unused=True)
        assert g_mask is None
        return loss.detach(), [x.detach().cpu() for x in grads], rb.detach().cpu()

    def torch_terms(dt):
        tr, tt = t_rgb.to(dt), t_thumb.to(dt)
        return (lambda r, mk: r * reference_mask(mk, 3, 32) + r.detach() * (1 - reference_mask(mk, 3, 32)),
                lambda nb: reg_weight * reference_regulariser(nb)[0],
                lambda r, t: ((r - tr) ** 2).mean() + thumb_weight * ((t - tt) ** 2).mean(),
                lambda r: mse_weight * F.mse_loss(r, tr))

    l64, g64, rb64 = run(torch.float64, "cpu", *torch_terms(torch.float64))
    l32, g32, _ = run(torch.float32, "cpu", *torch_terms(torch.float32))
    d_rgb, d_thumb = t_rgb.to(DEV), t_thumb.to(DEV)
    lh, gh, _ = run(torch.float32, DEV, P.mask_blend, lambda nb: P.noise_regulariser(nb, reg_weight),
                    P.surrogate_loss(d_rgb, d_thumb, thumb_weight=thumb_weight), lambda r: P._weighted_mse(r, d_rgb, mse_weight))
    # bounds
    b64 = [b.double() for b in bufs]
    _, means64 = reference_regulariser(b64)
    _, reg_vb, reg_gb = regulariser_bounds(b64, reg_weight, means64)
    m64 = reference_mask(mask.double(), 3, 32)
    Em, _ = mask_bound(mask.double(), 32, 32, 4)
    fwd_b = 3 * U * rgb.double().abs() * (m64.abs() + (1 - m64).abs() + 2 * Em)
    d = rb64 - t_rgb.double()
    c = 1.0 / rgb.numel()
    sq_rgb = float((d ** 2).sum()) * c
    sq_thumb = float(((thumb.double() - t_thumb.double()) ** 2).sum()) / thumb.numel()
    value_b = reg_vb + 39 * U * ((1 + mse_weight) * sq_rgb + thumb_weight * sq_thumb) \
        + (1 + mse_weight) * c * float((2 * d.abs() * fwd_b).sum()) + 3 * U * abs(float(l64))
    gin = 2 * c * (1 + mse_weight) * d                                     # d loss / d blended image
    gin_b = 2 * c * (1 + mse_weight) * fwd_b + (4 + 1) * U * gin.abs()
    rgb_b = gin_b * (m64.abs() + Em) + gin.abs() * (Em + U * (m64.abs() + Em))
    thumb_b = 5 * U * g64[1].abs()
    bounds = [rgb_b, thumb_b] + reg_gb
    for tag, lv, gv in (("torch fp32", l32, g32), ("hip", lh, gh)):
        ev = abs(float(lv) - float(l64))
        assert ev <= value_b, (tag, "value", ev, value_b)
        line = [f"value {ev / abs(float(l64)):.2e}"]
        for name, a, r, b in zip(["rgb", "thumb"] + [f"noise{i}" for i in range(len(bufs))], gv, g64, bounds):
            err = (a.double() - r).abs()
            assert bool((err <= b).all()), (tag, name, float((err - b).max()), float(b.max()))
            line.append(f"{name} {float(err.max()) / float(r.abs().max()):.2e}")
        print(f"\ncomposite step loss, {tag} against fp64 (relative, max-norm): " + ", ".join(line))
