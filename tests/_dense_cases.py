"""Cases, fp64 references and rounding-error bounds of the small dense kernels (csrc/linear.hip: cips3d_linear,
cips3d_linear_table, cips3d_pixel_norm; csrc/backward.hip: linear_bwd_*, table_bwd_*).  Shared by test_dense_cases_host.py (CPU:
every bound admits torch fp32 and rejects every mutant) and test_gpu_dense_heads.py (the kernels).  Imports no GPU code.

Every reference is a plain torch expression, generic in its dtype: evaluated in float64 it is the oracle, in float32 (on the
CPU) it is "a correct fp32 implementation", with a `mutant` it is a subtly wrong one.  Scalars (w_scale, ...) are fp32 numbers,
so the kernel and the reference see the same values.

Bounds.  u = 2^-24, gamma_k = k u / (1 - k u); first order in u behind the dot product; evaluated in fp64 from the reference's
own intermediates; per element.

One dense layer (dot_rows, linear_rows / table_rows).  Lane l accumulates its products with one fma each: n = ceil(in / 64)
terms on the scalar path, n = 4 ceil(in / 256) on the vector path; the 64 lane sums meet in six butterfly additions.  Every
product passes at most k = n + 6 roundings, so with S = sum_i w_i x_i and A = sum_i |w_i x_i|
    e(acc) = gamma_k A.
The epilogue, in the kernel's order (each line: the value p in fp64, its error e):
    PixelNorm   r = rsqrt(ss / in + 1e-8), ss = sum x^2 through its own chain of ns = ceil(in / 64) + 6 roundings, one division,
                one addition, the constant 1e-8 rounded to fp32 (three more), halved by the square root, and rsqrtf itself
                (the device's v_rsq_f32: 1 ulp; 2 ulp = 4 u allowed):  rel(r) = ((ns + 3) / 2 + 4) u
                p = S r:             e = |r| e(acc) + |p| (rel(r) + u)
    bias        bb = bias b_scale:   e(bb) = u |bb|
    affine      p1 = fma(p, w_scale, bb):          e1 = |w_scale| e + e(bb) + u |p1|
    lrelu       p2 = max(p1, 0.2f p1) act_gain:    e2 = act_gain s e1 + 3 u |p2|   (0.2f against 0.2, two products; s = 0.2 where
                                                   p1 < -e1, else 1: the function is continuous, so a sign decided the other way
                                                   within e1 of zero costs no more)
    output map  p3 = fma(p2, out_scale, out_shift):  e3 = |out_scale| e2 + u |p3|
    truncation  t = p3 - m, p4 = fma(psi, t, m):     e4 = |psi| (e3 + u |t|) + u |p4|
i.e. u (k A |scales| + c |intermediates|) with k = n + 6 and c = 1 per affine step, 3 for the activation, (ns + 3) / 2 + 5 for
the norm.  cips3d_pixel_norm alone: y = x r, e = |y| (rel(r) + u).

Backward of one layer (linear_bwd_*).  g = d(pre-activation) = dout out_scale [act_gain slope]: one rounding, with lrelu three
more (0.2f, act_gain * slope, the product): rel(g) = cg u, cg = 1 or 4.  (The slope is decided by the sign of the forward's
output; a case keeps every pre-activation far from zero, see `bwd_margin`.)
    dW[o][i] = w_scale sum_b g x:    B fmas, the scale:                e = u |w_scale| (B + cg + 1) sum_b |g x|
    db[o]    = b_scale sum_b g:      B additions, the scale:           e = u |b_scale| (B + cg + 1) sum_b |g|
    dx[b][i] = w_scale sum_o g W:    ceil(out / 16) fmas per row group, 16 additions of the partial sums, the scale:
                                                                       e = u |w_scale| (ceil(out / 16) + 16 + cg + 1) sum_o |g W|
Backward of a table (table_bwd_*): dy is used as it is, the scale sc = w_scale out_scale is one rounding.
    dW, db:  B fmas / additions, sc, the product:                      e = u |sc| (B + 2) sum_b |dy x|   (db: |b_scale out_scale|, |dy|)
    dx:      per head and row group (4 of them) ceil(out / 16) fmas, two additions of the partial-sum tree, sc, the product,
             then float atomics in any order: an address takes m = 4 x (heads on the slot) x (B when one row is broadcast)
             of them, each term passing at most m additions:
                                                                       e = u sum_heads |sc| (ceil(out / 16) + 4 + m) sum_o |dy W|
"""
import math

import torch

U = 2.0 ** -24


def f32(v):
    """the fp32 number a C float argument becomes"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def gamma(k):
    return k * U / (1.0 - k * U)


def chain_terms(in_dim, vec):
    return 4 * math.ceil(in_dim / 256) if vec else math.ceil(in_dim / 64)


def worst(err, bound):
    """(largest err / bound, its flat index); 0 / 0 counts as 0"""
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).reshape(-1)
    i = int(ratio.argmax()) if ratio.numel() else 0
    return (float(ratio[i]) if ratio.numel() else 0.0), i


def inside(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------------------------- one layer
WS, BS, GAIN, OS, OH, PSI = f32(0.37), f32(0.5), f32(2 ** 0.5), 15.0, 30.0, f32(0.7)


class LinearCase:
    def __init__(self, B, in_dim, out_dim, bias=True, pixelnorm=False, lrelu=False, affine=False, trunc=False, zero_row=None,
                 seed=0):
        self.B, self.in_dim, self.out_dim = B, in_dim, out_dim
        self.bias, self.pixelnorm, self.lrelu, self.affine, self.trunc, self.zero_row = bias, pixelnorm, lrelu, affine, trunc, zero_row
        self.seed = seed

    @property
    def id(self):
        sw = "".join(c for c, on in zip("bnlat", (self.bias, self.pixelnorm, self.lrelu, self.affine, self.trunc)) if on) or "-"
        return f"B{self.B}-in{self.in_dim}-out{self.out_dim}-{sw}" + ("-zero" if self.zero_row is not None else "")

    def tensors(self):
        """fp32 CPU inputs: x [B,in], W [out,in], b [out] | None, mean [out] | None"""
        g = torch.Generator().manual_seed(1000 * self.in_dim + 10 * self.out_dim + self.B + 7919 * self.seed)
        x = torch.randn(self.B, self.in_dim, generator=g)
        W = torch.randn(self.out_dim, self.in_dim, generator=g)
        b = torch.randn(self.out_dim, generator=g)
        mean = torch.randn(self.out_dim, generator=g)
        if self.zero_row is not None:
            x[self.zero_row] = 0.0
        return dict(x=x, W=W, b=b if self.bias else None, mean=mean if self.trunc else None)

    def scalars(self):
        """keyword arguments of hip.linear"""
        return dict(w_scale=WS, b_scale=BS, pixelnorm=self.pixelnorm, lrelu=self.lrelu, act_gain=GAIN if self.lrelu else 1.0,
                    out_scale=OS if self.affine else 1.0, out_shift=OH if self.affine else 0.0,
                    trunc_psi=PSI if self.trunc else 1.0)

    def mutants(self):
        return ["drop_col"] + (["slope"] if self.lrelu else []) + (["norm_short"] if self.pixelnorm else []) + \
            (["lerp_reversed"] if self.trunc else [])


def _lrelu(pre, gain, mutant=None):
    if mutant == "slope":
        return pre * 0.2 * gain
    return torch.nn.functional.leaky_relu(pre, 0.2) * gain


def pixel_norm_ref(x, dtype, mutant=None):
    x = x.to(dtype)
    ss = (x[:, :-1] ** 2).sum(1, keepdim=True) if mutant == "norm_short" else (x ** 2).sum(1, keepdim=True)
    return x * torch.rsqrt(ss / x.shape[1] + 1e-8)


def linear_ref(t, s, dtype, mutant=None):
    """the layer as a torch expression in `dtype`; t = LinearCase.tensors(), s = LinearCase.scalars()"""
    x, W = t["x"].to(dtype), t["W"].to(dtype)
    h = pixel_norm_ref(x, dtype, mutant) if s["pixelnorm"] else x
    if mutant == "drop_col":
        h, W = h[:, :-1], W[:, :-1]
    y = h @ (W * s["w_scale"]).t()
    if t["b"] is not None:
        y = y + t["b"].to(dtype) * s["b_scale"]
    if s["lrelu"]:
        y = _lrelu(y, s["act_gain"], mutant)
    y = y * s["out_scale"] + s["out_shift"]
    if t["mean"] is not None:
        m, psi = t["mean"].to(dtype), s["trunc_psi"]
        y = (m + (1 - psi) * (y - m)) if mutant == "lerp_reversed" else (m + psi * (y - m))
    return y


def norm_rel(in_dim):
    return ((math.ceil(in_dim / 64) + 6 + 3) / 2 + 4) * U


def pixel_norm_bound(x):
    return pixel_norm_ref(x, torch.float64).abs() * (norm_rel(x.shape[1]) + U)


def dense_bound(x, W, b, w_scale=1.0, b_scale=1.0, pixelnorm=False, lrelu=False, act_gain=1.0, out_scale=1.0, out_shift=0.0,
                mean=None, trunc_psi=1.0, vec=None):
    """per-element bound [B,out] of |kernel - fp64| for one dense layer (module docstring).  vec: which path dot_rows takes;
    None = the aligned call's (in % 4 == 0)."""
    x, W = x.double(), W.double()
    in_dim = x.shape[1]
    vec = (in_dim % 4 == 0) if vec is None else vec
    S, A = x @ W.t(), x.abs() @ W.abs().t()
    e = gamma(chain_terms(in_dim, vec) + 6) * A
    p = S
    if pixelnorm:
        r = torch.rsqrt((x ** 2).sum(1, keepdim=True) / in_dim + 1e-8)
        p = S * r
        e = r * e + p.abs() * (norm_rel(in_dim) + U)
    bb = b.double() * b_scale if b is not None else torch.zeros(W.shape[0], dtype=torch.float64)
    p = p * w_scale + bb
    e = abs(w_scale) * e + U * bb.abs() + U * p.abs()
    if lrelu:
        slope = torch.where(p < -e, torch.full_like(p, 0.2), torch.ones_like(p))
        p = torch.nn.functional.leaky_relu(p, 0.2) * act_gain
        e = act_gain * slope * e + 3 * U * p.abs()
    p = p * out_scale + out_shift
    e = abs(out_scale) * e + U * p.abs()
    if mean is not None:
        m = mean.double()
        t = p - m
        p = m + trunc_psi * t
        e = abs(trunc_psi) * (e + U * t.abs()) + U * p.abs()
    return e


def linear_bound(t, s, vec=None):
    return dense_bound(t["x"], t["W"], t["b"], mean=t["mean"], vec=vec, **s)


IN_DIMS = (1, 3, 4, 63, 64, 252, 256, 258, 260, 516)
OUT_DIMS = (1, 3, 4, 5, 130)
BATCHES = (1, 4, 5, 9)
# every (in, out) pair; B walks its axis along both, so every (in, B) and (out, B) pair occurs too
SHAPE_CASES = [LinearCase(BATCHES[(i + j) % 4], n, o) for i, n in enumerate(IN_DIMS) for j, o in enumerate(OUT_DIMS)]
_SWITCHES = [dict(bias=False), dict(), dict(pixelnorm=True), dict(lrelu=True), dict(affine=True), dict(trunc=True),
             dict(bias=False, pixelnorm=True, lrelu=True, affine=True, trunc=True),
             dict(pixelnorm=True, lrelu=True, affine=True, trunc=True)]
# the epilogue switches alone and together, on the scalar and on the vector path (ragged batch pass, more than one workgroup)
EPILOGUE_CASES = [LinearCase(B, n, o, seed=1, **sw) for (B, n, o) in ((5, 63, 5), (9, 260, 130)) for sw in _SWITCHES]
ZERO_ROW_CASES = [LinearCase(5, n, 5, pixelnorm=True, zero_row=2, seed=2, **sw) for n in (63, 260) for sw in (dict(), dict(lrelu=True, trunc=True))]
# the aligned form of the three fall-backs (in % 4 == 0: the vector path unless a pointer or a stride forbids it)
FALLBACK_CASES = [LinearCase(5, n, 5, pixelnorm=True, lrelu=True, seed=3) for n in (4, 260)]
PIXEL_NORM_SHAPES = ((1, 1), (3, 63), (5, 64), (4, 65), (9, 512))


def pixel_norm_input(B, C):
    return torch.randn(B, C, generator=torch.Generator().manual_seed(100 * C + B))


# ---------------------------------------------------------------------------------------------------- backward of one layer
class LinearBwdCase:
    def __init__(self, B, in_dim, out_dim, lrelu):
        self.B, self.in_dim, self.out_dim, self.lrelu = B, in_dim, out_dim, lrelu
        # (the kernel takes the slope from the sign of the forward's OUTPUT: with lrelu the output map is the identity)
        self.s = dict(w_scale=WS, b_scale=f32(0.01), lrelu=lrelu, act_gain=GAIN if lrelu else 1.0,
                      out_scale=1.0 if lrelu else OS, out_shift=0.0 if lrelu else OH)

    @property
    def id(self):
        return f"B{self.B}-in{self.in_dim}-out{self.out_dim}" + ("-lrelu" if self.lrelu else "")

    def tensors(self):
        g = torch.Generator().manual_seed(1000 * self.in_dim + 10 * self.out_dim + self.B + 31)
        return dict(x=torch.randn(self.B, self.in_dim, generator=g), W=torch.randn(self.out_dim, self.in_dim, generator=g),
                    b=torch.randn(self.out_dim, generator=g), dy=torch.randn(self.B, self.out_dim, generator=g))

    def mutants(self):
        # (slope 0.2 everywhere is the truth where no pre-activation is positive: the 1 x 1 layers)
        some_positive = self.lrelu and bool((_pre(self.tensors(), self.s, torch.float64) > 0).any())
        return ["drop_batch_row", "drop_out_row"] + (["slope"] if some_positive else [])


def _pre(t, s, dtype):
    return t["x"].to(dtype) @ (t["W"].to(dtype) * s["w_scale"]).t() + t["b"].to(dtype) * s["b_scale"]


def linear_grads(t, s, dtype, mutant=None):
    """(dx, dW, db) by autograd of the expression in `dtype`"""
    x, W, b = (t[k].to(dtype).clone().requires_grad_(True) for k in ("x", "W", "b"))
    pre = x @ (W * s["w_scale"]).t() + b * s["b_scale"]
    y = (_lrelu(pre, s["act_gain"], mutant) if s["lrelu"] else pre) * s["out_scale"] + s["out_shift"]
    dy = t["dy"].to(dtype)
    if mutant == "drop_out_row":          # the last output row never reaches dx
        (y[:, :-1] * dy[:, :-1]).sum().backward()
        dx = x.grad.clone()
        x.grad, W.grad, b.grad = None, None, None
        pre = x @ (W * s["w_scale"]).t() + b * s["b_scale"]
        y = (_lrelu(pre, s["act_gain"]) if s["lrelu"] else pre) * s["out_scale"] + s["out_shift"]
        (y * dy).sum().backward()
        return dx, W.grad, b.grad
    if mutant == "drop_batch_row":        # the last sample never reaches dW / db
        (y * dy).sum().backward()
        dx = x.grad.clone()
        x.grad, W.grad, b.grad = None, None, None
        pre = x @ (W * s["w_scale"]).t() + b * s["b_scale"]
        y = (_lrelu(pre, s["act_gain"]) if s["lrelu"] else pre) * s["out_scale"] + s["out_shift"]
        (y[:-1] * dy[:-1]).sum().backward()
        dW = W.grad if W.grad is not None else torch.zeros_like(W)
        db = b.grad if b.grad is not None else torch.zeros_like(b)
        return dx, dW, db
    (y * dy).sum().backward()
    return x.grad, W.grad, b.grad


def linear_bwd_bounds(t, s):
    """(e_dx, e_dW, e_db), module docstring"""
    x, W, dy = t["x"].double(), t["W"].double(), t["dy"].double()
    B, out_dim = x.shape[0], W.shape[0]
    g = dy * s["out_scale"]
    cg = 1
    if s["lrelu"]:
        pre = _pre(t, s, torch.float64)
        g = g * s["act_gain"] * torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, 0.2))
        cg = 4
    G = g.abs()
    e_dW = U * abs(s["w_scale"]) * (B + cg + 1) * (G.t() @ x.abs())
    e_db = U * abs(s["b_scale"]) * (B + cg + 1) * G.sum(0)
    e_dx = U * abs(s["w_scale"]) * (math.ceil(out_dim / 16) + 16 + cg + 1) * (G @ W.abs())
    return e_dx, e_dW, e_db


def bwd_margin(t, s):
    """smallest |pre-activation| over the forward's own error bound there: the kernel and fp64 must agree on every slope"""
    pre = _pre(t, s, torch.float64)
    e = dense_bound(t["x"], t["W"], t["b"], w_scale=s["w_scale"], b_scale=s["b_scale"])
    return float((pre.abs() / e).min())


BWD_CASES = [LinearBwdCase(B, n, o, lrelu) for n in (1, 63, 65, 260) for o in (1, 15, 16, 17, 130) for B in (1, 5)
             for lrelu in (False, True)]


# --------------------------------------------------------------------------------------------------------- tables of heads
class Head:
    """one head of a table over flat buffers, as cips3d_linear_desc has it: x[b] = xflat[x_off + b x_stride : + in_dim],
    out[b][row] = oflat[out_off + b out_stride + row]"""

    def __init__(self, W, b, x_off, x_stride, out_off, out_stride, ws=1.0, bs=1.0, os=1.0, oh=0.0):
        self.W, self.b = W, b
        self.out_dim, self.in_dim = W.shape
        self.x_off, self.x_stride, self.out_off, self.out_stride = x_off, x_stride, out_off, out_stride
        self.ws, self.bs, self.os, self.oh = f32(ws), f32(bs), f32(os), f32(oh)

    def x_index(self, B):
        return (self.x_off + torch.arange(B)[:, None] * self.x_stride + torch.arange(self.in_dim)[None, :])

    def out_index(self, B):
        return (self.out_off + torch.arange(B)[:, None] * self.out_stride + torch.arange(self.out_dim)[None, :])


class Table:
    def __init__(self, heads, xflat, B, out_len, name):
        self.heads, self.xflat, self.B, self.out_len, self.name = heads, xflat, B, out_len, name
        g = torch.Generator().manual_seed(len(heads) * 17 + B)
        self.dys = [torch.randn(B, h.out_dim, generator=g) for h in heads]

    def written(self):
        """mask over the flat output buffer of the elements some head writes"""
        m = torch.zeros(self.out_len, dtype=torch.bool)
        for h in self.heads:
            m[h.out_index(self.B).reshape(-1)] = True
        return m


def table_ref(tab, dtype, mutant=None, xflat=None):
    """[B,out] of every head, a torch expression in `dtype`"""
    xf = tab.xflat.to(dtype) if xflat is None else xflat
    outs = []
    for h in tab.heads:
        X, W = xf[h.x_index(tab.B)], h.W.to(dtype)
        if mutant == "drop_col":
            X, W = X[:, :-1], W[:, :-1]
        y = X @ (W * h.ws).t()
        if h.b is not None:
            y = y + h.b.to(dtype) * h.bs
        outs.append(y * h.os + h.oh)
    return outs


def table_bounds(tab):
    xf = tab.xflat
    return [dense_bound(xf[h.x_index(tab.B)], h.W, h.b, w_scale=h.ws, b_scale=h.bs, out_scale=h.os, out_shift=h.oh,
                        vec=(h.in_dim % 4 == 0 and h.x_stride % 4 == 0 and h.x_off % 4 == 0)) for h in tab.heads]


def table_grads(tab, dtype, mutant=None):
    """(dxflat, [dW], [db | None]) by autograd in `dtype` of sum_heads <out, dy>"""
    xf = tab.xflat.to(dtype).clone().requires_grad_(True)
    Ws = [h.W.to(dtype).clone().requires_grad_(True) for h in tab.heads]
    bs = [h.b.to(dtype).clone().requires_grad_(True) if h.b is not None else None for h in tab.heads]

    def total(rows=None, cols=None):
        tot = 0
        for h, W, b, dy in zip(tab.heads, Ws, bs, tab.dys):
            y = (xf[h.x_index(tab.B)] @ (W * h.ws).t() + (b * h.bs if b is not None else 0)) * h.os + h.oh
            tot = tot + (y * dy.to(dtype))[:rows, :cols].sum()
        return tot

    def grads(of, **kw):
        got = torch.autograd.grad(total(**kw), of, allow_unused=True)
        return [g if g is not None else torch.zeros_like(p) for g, p in zip(got, of)]

    params = Ws + [b for b in bs if b is not None]
    dx = grads([xf], cols=-1 if mutant == "drop_out_row" else None)[0]
    dp = grads(params, rows=-1 if mutant == "drop_batch_row" else None)
    dW, rest = dp[:len(Ws)], list(dp[len(Ws):])
    db = [rest.pop(0) if b is not None else None for b in bs]
    return dx, dW, db


def table_bwd_bounds(tab):
    """(e_dxflat, [e_dW], [e_db]) of table_bwd_*, module docstring (e_db also for heads without a bias: the kernel writes db)"""
    B = tab.B
    xf = tab.xflat.double()
    e_dW, e_db = [], []
    count = torch.zeros_like(xf)                     # atomics an address takes
    for h in tab.heads:
        count.index_put_((h.x_index(B).reshape(-1),), torch.full((B * h.in_dim,), 4.0, dtype=torch.float64), accumulate=True)
    e_dx = torch.zeros_like(xf)
    for h, dy in zip(tab.heads, tab.dys):
        dy = dy.double().abs()
        idx = h.x_index(B)
        e_dW.append(U * abs(h.ws * h.os) * (B + 2) * (dy.t() @ xf[idx].abs()))
        e_db.append(U * abs(h.bs * h.os) * (B + 2) * dy.sum(0))
        term = abs(h.ws * h.os) * (dy @ h.W.double().abs())                    # [B,in]
        k = math.ceil(h.out_dim / 16) + 4 + count[idx]
        e_dx.index_put_((idx.reshape(-1),), (U * k * term).reshape(-1), accumulate=True)
    return e_dx, e_dW, e_db


TABLE_SIZES = (1, 63, 64, 65, 130)
_HEIGHTS, _WIDTHS, _SLOTS, _SLOT_W = (1, 2, 3, 5), (8, 36, 7), 4, 36


def forward_table(n_desc, B):
    """n_desc heads of heights 1, 2, 3, 5, ... and input widths 8, 36, 7, ... over four shared input slots; every scalar its
    own; every fourth head without a bias; the output rows [B, total] with 16 unused floats behind them"""
    g = torch.Generator().manual_seed(n_desc * 10 + B)
    xflat = torch.randn(B * _SLOTS * _SLOT_W, generator=g)
    total = sum(_HEIGHTS[i % 4] for i in range(n_desc))
    heads, row = [], 0
    for i in range(n_desc):
        o, n = _HEIGHTS[i % 4], _WIDTHS[i % 3]
        heads.append(Head(torch.randn(o, n, generator=g), None if i % 4 == 3 else torch.randn(o, generator=g),
                          ((5 * i) % _SLOTS) * _SLOT_W, _SLOTS * _SLOT_W, row, total,
                          ws=0.1 + 0.01 * i, bs=0.5 + 0.003 * i, os=1.0 + 0.25 * (i % 7), oh=-2.0 + 0.1 * i))
        row += o
    return Table(heads, xflat, B, B * total + 16, f"n{n_desc}-B{B}")


def backward_table(kind):
    """"shared": the heads of test_gpu_backward.test_linear_table_bwd ((in, B) = kind[1:]) -- heights 48, 3, 130, 64, 7 over four
    slots, two pairs sharing one; "own": heads of widths 36, 512, 64 in that order, each over its own input rows, B = 3"""
    if kind[0] == "shared":
        _, n, B = kind
        g = torch.Generator().manual_seed(n + B)
        outs, slots, n_slots = (48, 3, 130, 64, 7), (0, 1, 1, 3, 0), 4
        xflat = torch.randn(B * n_slots * n, generator=g)
        heads, off = [], 0
        for o, sl in zip(outs, slots):
            heads.append(Head(torch.randn(o, n, generator=g), torch.randn(o, generator=g), sl * n, n_slots * n, off, o,
                              ws=0.21, bs=0.5, os=3.0, oh=1.5))
            off += B * o
        return Table(heads, xflat, B, off, f"shared-in{n}-B{B}")
    B, widths, outs = 3, (36, 512, 64), (5, 20, 33)
    g = torch.Generator().manual_seed(99)
    xflat = torch.randn(B * sum(widths), generator=g)
    heads, xo, oo = [], 0, 0
    for i, (n, o) in enumerate(zip(widths, outs)):
        heads.append(Head(torch.randn(o, n, generator=g), torch.randn(o, generator=g) if i != 2 else None, xo, n, oo, o,
                          ws=0.2 + 0.1 * i, bs=0.5, os=2.0 + i, oh=0.5 * i))
        xo += B * n
        oo += B * o
    return Table(heads, xflat, B, oo, "own-in36,512,64-B3")


BACKWARD_TABLES = [("shared", 512, 2), ("shared", 36, 3), ("shared", 256, 1), ("own",)]
