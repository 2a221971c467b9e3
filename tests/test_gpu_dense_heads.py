"""The small dense kernels against fp64, element by element, at their edge shapes: cips3d_linear, cips3d_pixel_norm,
cips3d_linear_table (csrc/linear.hip), linear_bwd_* and table_bwd_* (csrc/backward.hip), the broadcast table of
autograd.film_table, and the style phase against the oracle's mapping networks in fp64.
Reference: models/model_v3.py:32-65,183-210,1299-1418 (PixelNorm, MappingLinear, EqualLinear, the mapping networks),
:254,268 (modulation heads); cips3d/volume_renderer.py:15-35,66-67 (FiLM heads).

Cases, references and the per-element bounds (with their derivation) are in tests/_dense_cases.py; test_dense_cases_host.py
shows on the CPU that every bound admits torch fp32 and rejects a subtly wrong reference.  No tolerance of a single-layer test
here is a constant.  The style phase (eight chained 512-wide layers) has no useful closed-form bound: see
test_style_phase_against_the_oracle_in_fp64."""
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import autograd as AG
from cips_3dplusplus_amd import _lib, configs, hip
from oracle import path as O

import _dense_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SENTINEL = -77.25


def cu(t):
    return t.to(DEV).contiguous() if t is not None else None


def within(got, ref, bound, what):
    got = got.detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got - ref).abs()
    ratio, at = DC.worst(err, bound)
    print(f"{what}: worst |hip - fp64| / bound = {ratio:.3f}")
    assert bool((err <= bound).all()), (f"{what}: |hip - fp64| is {ratio:.3g} x its bound at flat element {at} "
                                        f"(hip {float(got.reshape(-1)[at])!r}, fp64 {float(ref.reshape(-1)[at])!r})")


def raw_linear(x, W, b, out, s, mean=None, B=None):
    """cips3d_linear on views: x and out may have any row stride (hip.linear takes contiguous tensors only)"""
    assert x.stride(1) == 1 and out.stride(1) == 1 and W.is_contiguous() and x.is_cuda and out.is_cuda
    hip.check(_lib.load().cips3d_linear(x.data_ptr(), x.stride(0), W.data_ptr(), b.data_ptr() if b is not None else None,
                                        out.data_ptr(), out.stride(0), x.shape[0] if B is None else B, x.shape[1], W.shape[0],
                                        s["w_scale"], s["b_scale"], int(s["pixelnorm"]), int(s["lrelu"]), s["act_gain"],
                                        s["out_scale"], s["out_shift"], mean.data_ptr() if mean is not None else None,
                                        s["trunc_psi"], 1, 0, hip.stream_ptr()), "cips3d_linear")


def run_linear(case, t=None, **kw):
    t = case.tensors() if t is None else t
    return hip.linear(cu(t["x"]), cu(t["W"]), cu(t["b"]), trunc_mean=cu(t["mean"]), **case.scalars(), **kw)


# ------------------------------------------------------------------------------------------------------------ 1. hip.linear
FORWARD = DC.SHAPE_CASES + DC.EPILOGUE_CASES + DC.ZERO_ROW_CASES


@pytest.mark.parametrize("case", FORWARD, ids=[c.id for c in FORWARD])
def test_linear_against_fp64(case):
    t, s = case.tensors(), case.scalars()
    y = run_linear(case, t)
    assert y.shape == (case.B, case.out_dim)
    within(y, DC.linear_ref(t, s, F64), DC.linear_bound(t, s), case.id)


def offset_view(t):
    """a contiguous copy of t that starts one float into its storage (4 bytes off every 16-byte boundary)"""
    base = torch.empty(t.numel() + 1, device=DEV)
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("how", ["x_offset", "W_offset", "x_stride"])
@pytest.mark.parametrize("case", DC.FALLBACK_CASES, ids=[c.id for c in DC.FALLBACK_CASES])
def test_linear_scalar_fallbacks_of_dot_rows(case, how):
    """in % 4 == 0, but x or W starts off a 16-byte boundary or x's row stride is no multiple of 4: dot_rows takes its scalar
    path by its own test.  The result is the layer's (scalar-path bound) and the aligned call's within both bounds."""
    t, s = case.tensors(), case.scalars()
    x, W, b = cu(t["x"]), cu(t["W"]), cu(t["b"])
    aligned = hip.linear(x, W, b, **s)
    if how == "x_offset":
        got = hip.linear(offset_view(x), W, b, **s)
    elif how == "W_offset":
        got = hip.linear(x, offset_view(W), b, **s)
    else:
        wide = torch.full((case.B, case.in_dim + 1), SENTINEL, device=DEV)
        wide[:, :case.in_dim] = x
        xv = wide[:, :case.in_dim]
        assert xv.stride(0) % 4 != 0 and xv.data_ptr() % 16 == 0
        got = torch.empty(case.B, case.out_dim, device=DEV)
        raw_linear(xv, W, b, got, s)
    ref, e_s, e_v = DC.linear_ref(t, s, F64), DC.linear_bound(t, s, vec=False), DC.linear_bound(t, s, vec=True)
    within(aligned, ref, e_v, f"{case.id} aligned")
    within(got, ref, e_s, f"{case.id} {how}")
    within(got, aligned.cpu().double(), e_s + e_v, f"{case.id} {how} against the aligned call")


def test_linear_out_repeat_writes_three_copies_and_nothing_else():
    case = DC.LinearCase(5, 260, 5, lrelu=True, trunc=True, seed=4)
    t, s = case.tensors(), case.scalars()
    B, o, guard = case.B, case.out_dim, 64
    buf = torch.full((guard + B * 3 * o + guard,), SENTINEL, device=DEV)
    out = buf[guard:guard + B * 3 * o].view(B, 3, o)
    run_linear(case, t, out=out, out_repeat=3, out_repeat_stride=o)
    ref, e = DC.linear_ref(t, s, F64), DC.linear_bound(t, s)
    for r in range(3):
        within(out[:, r], ref, e, f"copy {r}")
        assert torch.equal(out[:, r], out[:, 0])
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + B * 3 * o:] == SENTINEL).all())


def test_linear_out_row_stride_larger_than_out_dim_keeps_the_gap():
    case = DC.LinearCase(9, 63, 5, affine=True, seed=4)
    t, s = case.tensors(), case.scalars()
    wide = torch.full((case.B, case.out_dim + 3), SENTINEL, device=DEV)
    raw_linear(cu(t["x"]), cu(t["W"]), cu(t["b"]), wide[:, :case.out_dim], s)
    within(wide[:, :case.out_dim], DC.linear_ref(t, s, F64), DC.linear_bound(t, s), "strided out")
    assert bool((wide[:, case.out_dim:] == SENTINEL).all())


def test_linear_of_an_empty_batch_launches_nothing():
    case = DC.LinearCase(4, 64, 5)
    t, s = case.tensors(), case.scalars()
    y = hip.linear(torch.empty(0, case.in_dim, device=DEV), cu(t["W"]), cu(t["b"]), **s)
    assert y.shape == (0, case.out_dim)
    out = torch.full((case.B, case.out_dim), SENTINEL, device=DEV)      # B = 0 over buffers that could take four rows
    raw_linear(cu(t["x"]), cu(t["W"]), cu(t["b"]), out, s, B=0)
    assert bool((out == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------- 2. cips3d_pixel_norm
@pytest.mark.parametrize("B,C", DC.PIXEL_NORM_SHAPES)
def test_pixel_norm_against_fp64(B, C):
    from cips_3dplusplus_amd.decoder import PixelNorm
    x = DC.pixel_norm_input(B, C)
    within(PixelNorm()(cu(x)), DC.pixel_norm_ref(x, F64), DC.pixel_norm_bound(x), f"pixel_norm {B}x{C}")


# ------------------------------------------------------------------------------------------------------ 3. LinearTable.run
def device_table(tab):
    """hip.LinearTable of a DC.Table -> (table, x on the device, output buffer pre-filled with the sentinel)"""
    xd = cu(tab.xflat)
    out = torch.full((tab.out_len,), SENTINEL, device=DEV)
    t = hip.LinearTable(DEV)
    for h in tab.heads:
        t.add(cu(h.W), cu(h.b), xd, h.x_stride, out, h.out_stride, w_scale=h.ws, b_scale=h.bs, out_scale=h.os, out_shift=h.oh,
              x_offset=h.x_off, out_offset=h.out_off)
    return t, xd, out


def table_forward_within(tab, out):
    ref, e = DC.table_ref(tab, F64), DC.table_bounds(tab)
    flat = out.detach().cpu()
    for i, h in enumerate(tab.heads):
        within(flat[h.out_index(tab.B)], ref[i], e[i], f"{tab.name} head {i}")
    assert bool((flat[~tab.written()] == SENTINEL).all()), "an element no head owns was written"


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n_desc", DC.TABLE_SIZES)
def test_linear_table_against_fp64(n_desc, B):
    tab = DC.forward_table(n_desc, B)
    t, _, out = device_table(tab)
    t.run(B)
    table_forward_within(tab, out)


# ------------------------------------------------------------------------------------------ 4. hip.linear_bwd / AG.linear
@pytest.mark.parametrize("case", DC.BWD_CASES, ids=[c.id for c in DC.BWD_CASES])
def test_linear_bwd_against_fp64_autograd(case):
    t, s = case.tensors(), case.s
    x, W, b = (cu(t[k]).requires_grad_(True) for k in ("x", "W", "b"))
    AG.linear(x, W, b, **s).backward(cu(t["dy"]))
    ref, e = DC.linear_grads(t, s, F64), DC.linear_bwd_bounds(t, s)
    for name, got, r, eb in zip(("dx", "dW", "db"), (x.grad, W.grad, b.grad), ref, e):
        within(got, r, eb, f"{case.id} {name}")


@pytest.mark.parametrize("case", [DC.LinearBwdCase(5, 65, 17, True), DC.LinearBwdCase(5, 260, 130, False)], ids=lambda c: c.id)
def test_linear_bwd_outputs_that_are_not_needed(case):
    t, s = case.tensors(), case.s
    x, W, dy = cu(t["x"]), cu(t["W"]), cu(t["dy"])
    kw = dict(w_scale=s["w_scale"], b_scale=s["b_scale"], lrelu=s["lrelu"], act_gain=s["act_gain"], out_scale=s["out_scale"])
    y = hip.linear(x, W, cu(t["b"]), **s)
    full = hip.linear_bwd(x, W, dy, out=y, **kw)
    for k, off in enumerate(("need_dx", "need_dW", "need_db")):
        got = hip.linear_bwd(x, W, dy, out=y, **kw, **{off: False})
        assert got[k] is None
        assert all(torch.equal(got[j], full[j]) for j in range(3) if j != k)


def test_linear_bwd_takes_a_sliced_gradient():
    """autograd hands over the caller's own tensor: a slice of a wider one, row stride != out_dim"""
    case = DC.LinearBwdCase(5, 63, 17, True)
    t, s = case.tensors(), case.s
    x, W, b = (cu(t[k]).requires_grad_(True) for k in ("x", "W", "b"))
    wide = torch.full((case.B, case.out_dim + 5), SENTINEL, device=DEV)
    wide[:, 2:2 + case.out_dim] = cu(t["dy"])
    dy = wide[:, 2:2 + case.out_dim]
    assert not dy.is_contiguous()
    AG.linear(x, W, b, **s).backward(dy)
    ref, e = DC.linear_grads(t, s, F64), DC.linear_bwd_bounds(t, s)
    for name, got, r, eb in zip(("dx", "dW", "db"), (x.grad, W.grad, b.grad), ref, e):
        within(got, r, eb, f"sliced dy {name}")


def test_autograd_linear_refuses_an_activation_whose_slope_the_backward_cannot_read():
    """linear_bwd_* take the slope from the sign of the forward's output: with lrelu, an output shift or a negative output
    scale would silently give the gradient of another function"""
    x, W = torch.zeros(2, 4, device=DEV, requires_grad=True), torch.zeros(3, 4, device=DEV)
    for kw in (dict(out_shift=30.0), dict(out_scale=-1.0)):
        with pytest.raises(ValueError, match="lrelu"):
            AG.linear(x, W, None, lrelu=True, **kw)


# ------------------------------------------------------------------------------------------------ 5. LinearTable.backward
def table_backward_within(tab, t, xd, out, dx_like=None):
    B = tab.B
    dy = torch.zeros(tab.out_len, device=DEV)
    for h, d in zip(tab.heads, tab.dys):
        dy[h.out_index(B).to(DEV)] = cu(d)
    dx = torch.zeros_like(xd)
    dW, woffs, db = t.backward(B, out, dy, xd, dx)
    (rx, rW, rb), (ex, eW, eb) = DC.table_grads(tab, F64), DC.table_bwd_bounds(tab)
    within(dx, rx, ex, f"{tab.name} dx")
    row = 0
    for i, h in enumerate(tab.heads):
        within(dW[woffs[i]:woffs[i] + h.out_dim * h.in_dim], rW[i], eW[i], f"{tab.name} dW{i}")
        if h.b is not None:
            within(db[row:row + h.out_dim], rb[i], eb[i], f"{tab.name} db{i}")
        row += h.out_dim


@pytest.mark.parametrize("kind", DC.BACKWARD_TABLES, ids=lambda k: "-".join(map(str, k)))
def test_linear_table_bwd_against_fp64_autograd(kind):
    """("own",): heads of in_dim 36, 512, 64 in that order.  With the grid of the columns kernel sized from head 0's in_dim
    (LinearTable.backward before this test existed) the 512-wide head's dx stayed zero beyond column 63; measured on an MI355X:
        AssertionError: own-in36,512,64-B3 dx: |hip - fp64| is 1.51e+06 x its bound at flat element 879 (hip 0.0,
        fp64 11.78037655556243)
    (element 879 = sample 1, column 259 of that head)."""
    tab = DC.backward_table(kind)
    t, xd, out = device_table(tab)
    t.run(tab.B)
    table_forward_within(tab, out)
    table_backward_within(tab, t, xd, out)


def _refused(t, B, out, x, match):
    dx = torch.zeros_like(x)
    with pytest.raises(RuntimeError, match=match):
        t.backward(B, out, torch.zeros_like(out), x, dx)
    assert float(dx.abs().max()) == 0.0


def test_linear_table_bwd_refuses_what_its_kernels_cannot_take():
    """in_dim or x_stride no multiple of 4, x off a 16-byte boundary, more than 64 heads: refused in Python, naming the head,
    before any launch (the kernels read x and write dW in 16-byte pieces and find the head of a row with one 64-lane ballot)"""
    B = 2
    x, out = torch.zeros(B * 64, device=DEV), torch.zeros(B * 16, device=DEV)
    good, W6 = torch.zeros(4, 8, device=DEV), torch.zeros(4, 6, device=DEV)

    def table(*second):
        t = hip.LinearTable(DEV)
        t.add(good, None, x, 32, out, 8)
        if second:
            W, stride, off = second
            t.add(W, None, x, stride, out, 8, x_offset=off, out_offset=4)
        return t

    _refused(table(W6, 32, 8), B, out, x, r"head 1 \(in_dim 6")
    _refused(table(good, 30, 8), B, out, x, r"head 1 \(in_dim 8, x_stride 30")
    _refused(table(good, 32, 9), B, out, x, r"head 1 .*x at byte 4")
    many = hip.LinearTable(DEV)
    one = torch.zeros(1, 8, device=DEV)
    big_out = torch.zeros(B * 65, device=DEV)
    for i in range(65):
        many.add(one, None, x, 32, big_out, 65, out_offset=i)
    _refused(many, B, big_out, x, "65 heads")
    # and the table all of whose heads qualify is taken
    t = table(good, 32, 8)
    t.backward(B, out, torch.zeros_like(out), x, torch.zeros_like(x))


# --------------------------------------------------------------------------------- 6. the broadcast table, AG.film_table
def test_film_table_broadcast_of_one_latent():
    """One latent for B views: the second call with the same tensor reads it in place with row stride 0 (LinearTable.repointed),
    and the table backward's atomics sum the views' gradients into the one row."""
    B = 3
    G = pkg.build_generator(configs.tiny_G_cfg(32, 2), DEV, seed=7)
    r = G.renderer
    D, H, S = r.N_layers_renderer, r.hidden_dim, r.style_dim
    g = torch.Generator().manual_seed(11)
    styles_cpu = torch.randn(1, D + 1, S, generator=g)
    dfilm = torch.randn(B, D + 1, 2, H, generator=g)
    styles = cu(styles_cpu).requires_grad_(True)
    layers = list(r.network.pts_linears) + [r.network.views_linears]
    mods = [head for layer in layers for head in (layer.gamma, layer.beta)]
    for m in mods:
        m.weight.requires_grad_(True).grad, m.bias.requires_grad_(True).grad = None, None
    first = AG.film_table(r, styles, batch=B).detach().clone()             # stages (an address seen for the first time)
    dev_tab = r._film_table(B, torch.device(DEV))[2]
    assert not dev_tab.__dict__.get("_repointed")
    film = AG.film_table(r, styles, batch=B)
    assert dev_tab._repointed and all(d.x_stride == 0 for ent in dev_tab._repointed.values() for d in ent._descs)
    assert film.shape == (B, D + 1, 2, H) and torch.equal(first, film.detach())

    heads = [DC.Head(m.weight.detach().cpu(), m.bias.detach().cpu(), (i // 2) * S, 0, i * H, (D + 1) * 2 * H,
                     os=float(m.std_init), oh=float(m.bias_init)) for i, m in enumerate(mods)]
    tab = DC.Table(heads, styles_cpu.reshape(-1), B, B * (D + 1) * 2 * H, "film-broadcast")
    tab.dys = [dfilm[:, i // 2, i % 2] for i in range(len(mods))]
    ref, e = DC.table_ref(tab, F64), DC.table_bounds(tab)
    for i in range(len(mods)):
        within(film[:, i // 2, i % 2], ref[i], e[i], f"film head {i}")

    film.backward(cu(dfilm))
    assert styles.grad.shape == (1, D + 1, S)
    (rx, rW, rb), (ex, eW, eb) = DC.table_grads(tab, F64), DC.table_bwd_bounds(tab)
    within(styles.grad, rx, ex, "d styles")
    for i, m in enumerate(mods):
        within(m.weight.grad, rW[i], eW[i], f"film dW{i}")
        within(m.bias.grad, rb[i], eb[i], f"film db{i}")


# ------------------------------------------------------------------------------- 7. the style phase against the oracle
# max |hip - fp64| over max |oracle in fp32 on the CPU - fp64|, per output tensor: the bar (see the test's docstring)
STYLE_PHASE_BAR = {"styles_r": 1.02, "styles_d": 1.47, "film": 1.29, "s_buf": 1.27}


@pytest.fixture(scope="module")
def planned():
    from test_gpu_style_phase import _plan
    G, _ = _plan(256, 1)
    cfg = configs.ffhq_G_cfg(256, 2)
    sd32 = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd32.items()}
    return G, cfg, {torch.float32: sd32, F64: sd64}


def oracle_style_phase(G, cfg, sd, z_r, z_d, trunc, mean_r, mean_d, dtype):
    """styles_r, styles_d, film, s_buf as the plan lays them out, from the oracle's mapping networks in `dtype` and the affine
    heads (renderer._film_table, decoder._style_table) applied to those latents"""
    c = lambda t: None if t is None else t.to(dtype)      # noqa: E731
    w_r = O.mapping_renderer(sd, cfg, c(z_r), trunc, c(mean_r))
    w_d = O.mapping_decoder(sd, cfg, c(z_d), trunc, c(mean_d))
    net = G.renderer.network
    film = []
    for l, layer in enumerate(list(net.pts_linears) + [net.views_linears]):
        gb = [(w_r[:, l] @ c(h.weight.detach().cpu()).t() + c(h.bias.detach().cpu())) * float(h.std_init) + float(h.bias_init)
              for h in (layer.gamma, layer.beta)]
        film.append(torch.stack(gb, 1))
    s = []
    for m, li in G.decoder._mod_layers():
        mod = m.conv.modulation
        s.append(w_d[:, li] @ (c(mod.weight.detach().cpu()) * mod.scale).t() + c(mod.bias.detach().cpu()) * mod.lr_mul)
    return dict(styles_r=w_r, styles_d=w_d, film=torch.stack(film, 1), s_buf=torch.cat(s, 1))


@pytest.mark.parametrize("trunc", [1.0, 0.6])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B", [1, 5, 8])
def test_style_phase_against_the_oracle_in_fp64(planned, B, mode, trunc):
    """plan.style_phase (mode 0: the chain of launches, mode 1: the one launch) of the planned ffhq_G_cfg(256, 2) generator
    against oracle.path.mapping_renderer / mapping_decoder and the affine heads, all evaluated in float64.

    The error of eight chained 512-wide layers is measured against the error the same oracle functions make in fp32 on the CPU:
    ratio = max |hip - fp64| / max |fp32 oracle - fp64| per output tensor.  Measured on an MI355X over B in {1, 5, 8},
    mode in {0, 1}, truncation in {1.0, 0.6} (the modes are bit-identical, the kernels deterministic):
        styles_r  0.33 .. 0.51   (e_hip <= 1.0e-6, e_32 <= 2.0e-6)
        styles_d  0.43 .. 0.73   (e_hip <= 2.3e-6, e_32 <= 3.9e-6)
        film      0.43 .. 0.64   (e_hip <= 4.6e-6, e_32 <= 1.1e-5)
        s_buf     0.38 .. 0.63   (e_hip <= 2.0e-6, e_32 <= 4.4e-6)
    -- the kernels' wave-wide trees are more accurate than the CPU's fp32 sums.  The bar of a tensor is twice its worst ratio
    (room for a compiler's reassociation): 1.02, 1.47, 1.29, 1.27; a bar above 8 would be a finding, not a tolerance."""
    G, cfg, sds = planned
    plan = G._forward_plan(B, 64, 12, False)
    assert plan is not None
    g = torch.Generator().manual_seed(100 * B + int(10 * trunc))
    z_r, z_d = torch.randn(B, G.z_dim, generator=g), torch.randn(B, G.z_dim, generator=g)
    mean_r = torch.randn(plan.plan.style_dim_r, generator=g) if trunc < 1 else None
    mean_d = torch.randn(plan.plan.style_dim_d, generator=g) if trunc < 1 else None
    for o in (plan.styles_r, plan.styles_d, plan.film, plan.s_buf):
        o.fill_(float("nan"))
    plan.style_phase(cu(z_r), cu(z_d), mode=mode, trunc_psi=trunc, mean_r=cu(mean_r), mean_d=cu(mean_d))
    got = dict(styles_r=plan.styles_r, styles_d=plan.styles_d, film=plan.film, s_buf=plan.s_buf)
    got = {k: v.detach().cpu().double() for k, v in got.items()}
    if mode == 1:
        assert int(plan.style_sync[1]) == 0
    ref = oracle_style_phase(G, cfg, sds[F64], z_r, z_d, trunc, mean_r, mean_d, F64)
    cpu = oracle_style_phase(G, cfg, sds[torch.float32], z_r, z_d, trunc, mean_r, mean_d, torch.float32)
    ratios = {}
    for k in STYLE_PHASE_BAR:
        assert got[k].numel() == ref[k].numel() and bool(torch.isfinite(got[k]).all()), k
        e_hip = float((got[k].reshape(ref[k].shape) - ref[k]).abs().max())
        e_32 = float((cpu[k].double() - ref[k]).abs().max())
        ratios[k] = e_hip / e_32
        print(f"style phase B={B} mode={mode} trunc={trunc} {k}: e_hip {e_hip:.3e} e_32 {e_32:.3e} ratio {ratios[k]:.3f}")
    for k, bar in STYLE_PHASE_BAR.items():
        assert ratios[k] <= bar, f"{k}: the kernel's error is {ratios[k]:.2f} x the fp32 oracle's (bar {bar})"
