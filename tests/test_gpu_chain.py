"""The chain GEMM on planes (csrc/chain.hip: chain_gemm_kernel <1,4,2,64,2>, the half-chip <2,4,2,64,2> and the bf16 <1,4,2,64,3,1>)
and the converters to_planes / from_planes / to_planes16 / from_planes16 against fp64, element by element, called directly through
hip.modconv1x1_planes, hip.modconv1x1_planes16 and the four converters: ragged last pixel blocks of every kind, contractions of
1, 2, 3, 4, 8 and 9 stages against the 2- and 3-slot rings, hand-built input planes whose every sample and pixel block has an
exponent of its own, with exact, loose and no patch maxima, unranged planes, an all-zero sample beside a spike, every exit, the
fold and the riding fold, the half-chip window and its neighbours.
Reference: models/model_v3.py:218-341 (modulation, convolution, noise, activation), :418-482 (ToRGB).

Cases, references, the per-element bounds (with their derivation) and every check that needs the reference are in
tests/_chain_cases.py (check_outputs); test_chain_cases_host.py shows on the CPU that the checks admit an fp32 emulation and reject
every mutant.  No tolerance here is a constant.  Every call is made twice, the first call's outputs overwritten and freed in
between, and the second call's outputs equal the first's bit for bit.  EVERY output is handed in by the test, as a view into a
larger buffer of sentinels: the elements in front of and behind it stay untouched; exponents start as an int sentinel, patch
maxima and fold slots as NaN, and every entry must have been written.

Largest |hip - fp64| / bound per kernel form, exit and check, measured on an MI355X over all cases, scales and both calls (the scales
agree to the digits printed: the bounds scale with the data), and the case it was seen at, as (B, Cin, Cout, HW):
    split 64x128    planes exit   0.999  (2, 64, 64, 129) rng e, no epilogue: under the spike the block's other values sit at the
                                         pair's floor, and half a subnormal step of lo (2^-25 2^e') IS the bound there; 0.30 without
                                         a spike, at per-sample noise (the epilogue's three roundings); 0.0011 at (1, 576, 64, 129)
                    fp32 exit     0.50   (2, 64, 64, 200) rng e;  about 0.3 else, at per-sample noise;  down to 0.0014 at (1, 512, 64, 128) without noise
                    bf16 exit     the fp32 exit of the same inputs, rounded, bit for bit (its fp32 twin: 0.24 to 0.0037)
                    fold slot, against the fp64 output   0.033 (2, 64, 128, 65);  down to 0.0004 at 256 rows, no epilogue
                    fold slot, against the stored output (the fold alone)   0.34 (2, 64, 128, 129) unranged planes;  nothing below 0.085
                    the slots' sum against ToRGB of the stored output   0.24, the same case;  nothing below 0.027
                    three layers from to_planes   0.0087 / 0.0072 / 0.0085
    split 128x128   planes exit   0.30   (3, 64, 128, 4261);  0.0090 at (1, 128, 256, 6337);  fp32 exit 0.0090 there
                    fold slot 0.0006 / alone 0.15 / sum 0.047;  riding fold 0.45 (5 slots, 2 biases, skip)
                    planes, exponents, slots and pmax.amax(-1) equal the 64-row form's bit for bit
    planes16        fp32 exit     0.30   (2, 64, 128, 250);  down to 0.0023 at (1, 512, 192, 128) without an epilogue
                    planes16 / bf16 exits: the rounded fp32 exit, bit for bit
                    fold slot 0.032 / alone 0.17 / sum 0.075;  nothing of the fold alone below 0.081
No ratio exceeds 1.  The small ones, 0.001 to 0.01, are all contractions without noise: the bound charges gamma_(3 K + 8) on K terms
of one sign (it has to hold for any order of the additions), a matrix instruction's own tree errs as sqrt(K) terms of mixed signs,
so the ratio falls as 1 / K^(3/2) -- 0.02 at one stage, 0.001 at nine.  The fold against the fp64 output is lower still for the
reason test_gpu_gemm1x1.py gives (every row's worst case charged with one sign through a sum of mixed signs); hence the check of
the fold alone.  What this costs is stated in test_chain_cases_host.py: a lost lo product is caught up to three stages, not at
eight; every other mutant is caught at every case it applies to.
Deviations from the issue's text, each derived in _chain_cases.py: a pair is canonical if fp16(hi + lo) == hi OR |lo| is exactly
half hi's spacing (the header's own split produces such ties); the patch maximum's lower limit subtracts the pair's floor;
HW = 200 is a two-half block (HW = 180 added for the ragged single half); tiles64 = 258 stands in for the prime 257.
This file: 85 tests, 2.2 s on an MI355X; the slowest test 0.29 s (the first: library load), the largest case 0.11 s.
"""
import ctypes as C

import pytest
import torch

from cips_3dplusplus_amd import _lib, hip

import _chain_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SENTINEL = -77.5                                  # (an fp16 and a bf16 number too)
INT_SENTINEL = -12345
GUARD = 256                                       # elements in front of and behind a guarded tensor (16-byte aligned)
CASES = CC.CHAIN_CASES
ids = [c.id for c in CASES]
NAN = float("nan")


def cu(t):
    return t.to(DEV).contiguous() if t is not None else None


def bits(v):
    if v.dtype in (torch.bfloat16, torch.float16):
        return v.contiguous().view(torch.int16)
    return v.contiguous().view(torch.int32) if v.dtype == F32 else v


class Guarded:
    """a tensor inside a buffer of sentinels"""

    def __init__(self, *shape, dtype=F32, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.sentinel = INT_SENTINEL if dtype == torch.int32 else SENTINEL
        self.buf = torch.full((n + 2 * GUARD,), self.sentinel, device=DEV, dtype=dtype)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if fill is not None:
            self.t.fill_(fill)
        self.n = n

    def intact(self):
        return bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.n:] == self.sentinel).all())


def twice(call):
    """[outputs of the first call, outputs of the second] on the CPU; call() returns ({name: tensor}, guards); the first call's
    device outputs are overwritten and freed before the second call allocates its own; every guard band is checked; the second
    call's outputs equal the first's bit for bit"""
    results = []
    for _ in range(2):
        out, guards = call()
        torch.cuda.synchronize()
        for g in guards:
            assert g.intact(), "a write outside the output tensor"
        results.append({k: (None if o is None else o.detach().cpu().clone()) for k, o in out.items()})
        for g in guards:
            g.buf.fill_(1)
        torch.cuda.synchronize()
        del out, guards
    for k, a in results[0].items():
        if a is not None:
            assert torch.equal(bits(a), bits(results[1][k])), f"{k}: the second call differs from the first"
    return results


def record(case, ratios, form):
    for k, v in ratios.items():
        print(f"RATIO | {case.kernel + (' ' + form if case.split else '')} | {case.exit} | {k} | {v:.3g} | {case.id}")


class Launch:
    """the operands of one case at one scale on the device, the stored operands back on the CPU, and the launches"""

    def __init__(self, case, gs):
        self.case, self.t = case, case.tensors(gs)
        c, t = case, self.t
        W, s = cu(t["W"]).view(1, c.Cout, c.Cin, 1, 1), cu(t["s"])
        if c.split:
            self.wm = hip.modulate_weights(W, s, c.Cin, c.B, c.Cout, c.Cin, 1, t["scale"], True, True, split=True)
            wh, wl = CC.unpack_split_halves(self.wm.cpu(), c.B, c.Cout, c.Cin)
            assert torch.equal((wh + wl) / 256.0, CC.unpack_split(self.wm.cpu(), c.B, c.Cout, c.Cin, False))
            self.ops = c.operands(t, wh=wh, wl=wl)
        else:
            self.wm = hip.modulate_weights(W, s, c.Cin, c.B, c.Cout, c.Cin, 1, t["scale"], True, True, bf16=True)
            self.ops = c.operands(t, w16=CC.unpack_bf16(self.wm.cpu(), c.B, c.Cout, c.Cin))
        # the modulation itself is test_gpu_gemm1x1.py's; here it only has to be the layer the torch expression describes
        w_st = (self.ops["wh"] + self.ops["wl"]) / 256.0 if c.split else self.ops["w"]
        assert float((w_st - t["w"]).abs().max()) < (2.0 ** -7 if not c.split else 2.0 ** -16)
        self.xp = cu(self.ops["p"])
        if c.ranged:
            self.xp.cips3d_exp, self.xp.cips3d_pmax = cu(self.ops["exps"]), cu(self.ops["pmax"])
        ep = c.epilogue == 1
        self.noise = cu(t["noise"]) if (ep and t["noise"] is not None) else None
        self.nw = torch.tensor([CC.NOISE_W], device=DEV) if self.noise is not None else None
        self.bias = cu(t["bias"]) if ep else None
        self.w_rgb = cu(t["w_rgb"]) if c.fold else None
        self.lconst = cu(self.ops["lconst"]) if c.tracked else None
        self.ride = {k: cu(v) for k, v in t["ride"].items()} if c.ride else None

    def run(self, exit=None, hint=None):
        c = self.case
        exit = c.exit if exit is None else exit
        hint = c.hint if hint is None else hint
        slots = c.Cout // 64
        planes = exit in ("planes", "planes16")
        if exit == "planes":
            g_out = Guarded(c.B, c.Cout // 8, 2, c.HW, 8, dtype=torch.float16)
        elif exit == "planes16":
            g_out = Guarded(c.B, c.Cout // 8, c.HW, 8, dtype=torch.bfloat16)
        else:
            g_out = Guarded(c.B, c.Cout, c.HW, dtype=torch.bfloat16 if exit == "bf16" else F32)
        guards, out = [g_out], dict(out=g_out.t)
        g_part = Guarded(slots + 1, c.B, 3, c.HW, fill=NAN) if c.fold else None
        if c.fold:
            guards.append(g_part)
        kw = dict(epilogue=c.epilogue, noise=self.noise, noise_w=self.nw, bias=self.bias, rgb_w=self.w_rgb,
                  rgb_part=g_part.t if c.fold else None, out=g_out.t)
        if not c.split:
            y, nblk = hip.modconv1x1_planes16(self.xp, self.wm, c.Cout, c.HW, exit, **kw)
            assert nblk == slots and y.data_ptr() == g_out.t.data_ptr()
        else:
            tracked = c.ranged and exit == "planes"
            if tracked:
                g_exp, g_pm = Guarded(c.B, c.nblk, dtype=torch.int32), Guarded(c.B, c.nhalf, c.Cout // 16, fill=NAN)
                guards += [g_exp, g_pm]
                kw.update(out_exp=g_exp.t, out_pmax=g_pm.t, lconst=self.lconst)
                out.update(exp=g_exp.t, pmax=g_pm.t)
            if c.ranged and not planes:
                g_am = Guarded(c.B, hip.amax_floats(), fill=0.0)
                guards.append(g_am)
                kw.update(out_amax=g_am.t)
            if c.ride:
                g_ride = Guarded(1, 3, 260)
                guards.append(g_ride)
                kw.update(ride=dict(part=self.ride["part"], biases=[self.ride["biases"][0], self.ride["biases"][1]],
                                    skip=self.ride["skip"], out=g_ride.t))
                out.update(ride=g_ride.t)
            y = hip.modconv1x1_planes(self.xp, self.wm, c.Cout, c.HW, exit, half_chip=hint, **kw)
            assert y.data_ptr() == g_out.t.data_ptr()
            assert _lib.load().cips3d_planes_torgb_blocks(c.Cout) == slots
            if tracked:
                assert y.cips3d_exp.data_ptr() == g_exp.t.data_ptr() and y.cips3d_pmax.data_ptr() == g_pm.t.data_ptr()
                assert not bool((g_exp.t == INT_SENTINEL).any()), "out_exp: an entry was not written"
            if c.ranged and not planes:
                out.update(amax=hip.amax_value(g_am.t))
        if c.fold:
            assert bool(torch.isnan(g_part.t[slots]).all()), "a write behind the last ToRGB slot"
            out.update(slots=g_part.t[:slots])
        return out, guards

    def got(self, res, exit, out32=None):
        """the form check_outputs takes"""
        g = dict(slots=res.get("slots"), amax=res.get("amax") if exit == "fp32" else None)
        if exit == "planes":
            g["hi"], g["lo"] = CC.planes_halves(res["out"])
            g["exp"], g["pmax"] = res.get("exp"), res.get("pmax")
        else:
            g["out32"] = res["out"] if exit == "fp32" else out32
        return g


def rounded_exit_equals(case, res, exit, r32):
    """bf16 / planes16: the RNE rounding of the fp32 exit of the same launch inputs, bit for bit (amax and slots: the same bits)"""
    want = r32["out"].to(torch.bfloat16)
    if exit == "planes16":
        want = CC.planes16_of(r32["out"])
    assert res["out"].dtype == torch.bfloat16 and torch.equal(bits(res["out"]), bits(want)), f"{exit} exit is not the rounded fp32 exit"
    for k in ("amax", "slots"):
        if r32.get(k) is not None:
            assert torch.equal(bits(res[k]), bits(r32[k])), f"{exit} exit: {k} differs from the fp32 exit's"


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_chain_gemm_against_fp64(case):
    form = case.regime()["form"]
    for gs in case.scales:
        L = Launch(case, gs)
        ref = CC.reference(case, L.t, L.ops)
        r32 = None
        if case.exit in ("bf16", "planes16"):
            out, guards = L.run("fp32")
            torch.cuda.synchronize()
            assert all(g.intact() for g in guards)
            r32 = {k: v.detach().cpu().clone() for k, v in out.items()}
        for i, res in enumerate(twice(L.run)):
            if r32 is not None:
                rounded_exit_equals(case, res, case.exit, r32)
            ratios = CC.check_outputs(case, L.t, L.ops, ref, L.got(res, case.exit, None if r32 is None else r32["out"]))
            if i == 0:
                record(case, ratios, form)
            if case.ride:
                tr = L.t["ride"]
                rr, rb = CC.reference_ride(tr)
                err = (res["ride"].double() - rr).abs()
                assert bool((err <= rb).all()), "riding fold outside reduce_bound"
                print(f"RATIO | split {form} | ride | riding fold | {CC.worst(err, rb)[0]:.3g} | {case.id}")
                assert torch.equal(bits(res["ride"]), bits(torgb_reduce(L.ride).cpu())), "riding fold differs from cips3d_torgb_reduce"
        if not case.hint:
            continue
        # the hint: the 128-row form inside the window, the 64-row form at its neighbours -- the same bits either way
        plain = twice(lambda: L.run(hint=False))[0]
        for k in ("out", "exp", "slots", "amax", "ride"):
            if res.get(k) is not None:
                assert torch.equal(bits(res[k]), bits(plain[k])), f"{k}: the hinted launch differs from the plain one"
        if res.get("pmax") is not None:
            ph, pp = res["pmax"], plain["pmax"]
            assert torch.equal(ph.amax(-1), pp.amax(-1))
            assert not torch.equal(pp[..., 0::2], pp[..., 1::2]), "the 64-row form's patch maxima come in equal pairs"
            if form == "128x128":
                assert torch.equal(ph[..., 0::2], ph[..., 1::2]), "the 128-row form leaves one maximum per pair of 16-row tiles"
                assert torch.equal(ph[..., 0::2], torch.maximum(pp[..., 0::2], pp[..., 1::2]))
            else:
                assert torch.equal(bits(ph), bits(pp)), "outside the window the hint changed the form"


def torgb_reduce(ride):
    lib = _lib.load()
    part = ride["part"]
    n_slots, Br, _, HWr = part.shape
    out = torch.empty(Br, 3, HWr, device=DEV)
    biases = (C.c_void_p * 2)(ride["biases"][0].data_ptr(), ride["biases"][1].data_ptr())
    _lib.check(lib.cips3d_torgb_reduce(part.data_ptr(), n_slots, biases, 2, ride["skip"].data_ptr(), out.data_ptr(), Br, HWr,
                                       hip.stream_ptr()), "cips3d_torgb_reduce")
    return out


# --------------------------------------------------------------------------------------------------------------- refusals
def _raw(lib, x, w, o, fmt, B, Cin, Cout, HW, ep=0, bias=None, rgb_w=None, rgb_part=None, rg=None, nblk=None):
    p = lambda v: v.data_ptr() if v is not None else None      # noqa: E731
    return lib.cips3d_modconv1x1_planes(p(x), p(w), p(o), fmt, B, Cin, Cout, HW, ep, None, 0, None, p(bias), p(rgb_w), p(rgb_part),
                                        C.byref(nblk) if nblk is not None else None, C.byref(rg) if rg is not None else None,
                                        hip.stream_ptr())


def test_planes_entry_point_refusals():
    lib = _lib.load()
    x = torch.zeros(1, 72, 2, 64, 8, device=DEV, dtype=torch.float16)           # room for Cin = 576
    w = torch.zeros(576 * 64, device=DEV)
    g = Guarded(1, 64, 64)
    bias, rgb_w, part = torch.zeros(64, device=DEV), torch.zeros(1, 3, 64, device=DEV), torch.zeros(1, 1, 3, 64, device=DEV)
    exps, pmax = torch.zeros(1, 1, device=DEV, dtype=torch.int32), torch.ones(1, 1, 36, device=DEV)
    lconst, oexp = torch.ones(1, 4, device=DEV), torch.zeros(1, 1, device=DEV, dtype=torch.int32)
    nblk = C.c_int(-1)
    assert _raw(lib, x, w, g.t, 0, 1, 64, 64, 64, nblk=nblk) == 0 and nblk.value == 1                        # the call that works
    for fmt in (3, -1):
        assert _raw(lib, x, w, g.t, fmt, 1, 64, 64, 64) != 0
    g.t.fill_(SENTINEL)
    assert _raw(lib, x, w, g.t, 0, 1, 64, 64, 64, ep=1) != 0                                                # epilogue without bias
    assert _raw(lib, x, w, g.t, 0, 1, 64, 64, 64, rgb_w=rgb_w) != 0 and _raw(lib, x, w, g.t, 0, 1, 64, 64, 64, rgb_part=part) != 0
    rg, _k = hip._range(x_exp=exps)
    assert _raw(lib, x, w, g.t, 1, 1, 64, 64, 64, rg=rg) != 0                                               # planes, rg, no lconst
    rg, _k = hip._range(x_exp=exps, lconst=lconst)
    assert _raw(lib, x, w, g.t, 1, 1, 64, 64, 64, rg=rg) != 0                                               # ... no out_exp
    rg, _k = hip._range(x_exp=exps, out_exp=oexp)
    assert _raw(lib, x, w, g.t, 1, 1, 64, 64, 64, rg=rg) != 0
    assert _raw(lib, x, w, g.t, 0, 1, 32, 64, 64) != 0 and _raw(lib, x, w, g.t, 0, 1, 64, 96, 64) != 0      # Cin % 64, Cout % 64
    assert _raw(lib, x, w, g.t, 0, 1, 64, 64, 15) != 0                                                      # HW = 15
    rg, _k = hip._range(x_exp=exps, x_pmax=pmax, lconst=lconst, out_exp=oexp)
    assert _raw(lib, x, w, g.t, 1, 1, 576, 64, 64, rg=rg) != 0                                              # patch maxima, Cin = 576
    # (the loop over the entries past the first 64 in finish_ops is what this refusal keeps unreachable)
    assert _raw(lib, x, w, g.t, 0, 0, 64, 64, 64, ep=1, bias=bias) == 0                                     # B = 0: nothing happens
    torch.cuda.synchronize()
    assert bool((g.t == SENTINEL).all()) and g.intact() and int(oexp[0, 0]) == 0


def test_riding_fold_position_limit():
    """ride.n4 at exactly ceil(HW / 128) B 128 positions is accepted, one float4 more is refused"""
    lib = _lib.load()
    B, HW = 3, 128
    x = torch.zeros(B, 8, 2, HW, 8, device=DEV, dtype=torch.float16)
    w = torch.zeros(B * 64 * 64, device=DEV)
    o = torch.zeros(B, 64, HW, device=DEV)
    exps = torch.zeros(B, 1, device=DEV, dtype=torch.int32)
    limit = B * 128
    part = torch.randn((limit + 1) * 4, device=DEV)
    g = Guarded((limit + 1) * 4)
    job = _lib.ReduceJob()
    job.part, job.out, job.skip = part.data_ptr(), g.t.data_ptr(), None
    job.HW4, job.slot_stride, job.n_slots, job.n_bias = limit // 3, (limit + 1) * 4, 1, 0
    rg, _k = hip._range(x_exp=exps)
    rg.ride = C.addressof(job)
    job.n4 = limit + 1
    assert _raw(lib, x, w, o, 0, B, 64, 64, HW, rg=rg) != 0
    torch.cuda.synchronize()
    assert bool((g.t == SENTINEL).all())
    job.n4 = limit
    assert _raw(lib, x, w, o, 0, B, 64, 64, HW, rg=rg) == 0
    torch.cuda.synchronize()
    assert torch.equal(g.t[:limit * 4], part[:limit * 4]) and bool((g.t[limit * 4:] == SENTINEL).all()) and g.intact()


# -------------------------------------------------------------------------------------------------------------- converters
@pytest.mark.parametrize("B,Cc,HW", CC.CONVERTER_CASES, ids=[f"B{b}-C{c}-HW{h}" for b, c, h in CC.CONVERTER_CASES])
def test_converters(B, Cc, HW):
    g = CC._gen(31, B, Cc, HW)
    x = torch.randn(B, Cc, HW, generator=g) * torch.pow(2.0, 7.0 * torch.arange(B)).reshape(B, 1, 1)
    x[:, :, ::5] *= 2.0 ** -16                                # (values far below the sample's maximum: subnormal lo halves)
    nblk, nhalf = CC.ceil_div(HW, 128), CC.ceil_div(HW, 64)
    xd = cu(x).view(B, Cc, 1, HW)
    e_want = torch.tensor([[CC.split_exp(float(x[b].abs().max()))] * nblk for b in range(B)], dtype=torch.int32)

    def ranged():
        gp, ge = Guarded(B, Cc // 8, 2, HW, 8, dtype=torch.float16), Guarded(B, nblk, dtype=torch.int32)
        gm = Guarded(B, nhalf, Cc // 16, fill=NAN) if Cc % 16 == 0 else None
        p = hip.to_planes(xd, out=gp.t, out_exp=ge.t, out_pmax=gm.t if gm else None)
        assert p.data_ptr() == gp.t.data_ptr() and (p.cips3d_pmax is None) == (Cc % 16 != 0)
        return dict(p=gp.t, e=ge.t, pmax=gm.t if gm else None), [gp, ge] + ([gm] if gm else [])

    for r in twice(ranged):
        assert torch.equal(r["e"], e_want), "one exponent per sample, in every block"
        assert torch.equal(bits(r["p"]), bits(CC.planes_of(x, e_want))), "hi / lo are not the fp16 castings of x 2^-e and its remainder"
        if r["pmax"] is not None:
            assert torch.equal(r["pmax"], x.abs().amax((1, 2)).reshape(B, 1, 1).expand(B, nhalf, Cc // 16)), "every patch holds the sample's maximum"

    def raw():
        gp = Guarded(B, Cc // 8, 2, HW, 8, dtype=torch.float16)
        p = hip.to_planes(xd * 2.0 ** -7 if B > 1 else xd, ranged=False, out=gp.t)
        assert p.cips3d_exp is None
        return dict(p=gp.t), [gp]

    for r in twice(raw):
        assert torch.equal(bits(r["p"]), bits(CC.planes_of(x * 2.0 ** -7 if B > 1 else x, None)))
    # from_planes on hand-built planes with an exponent per sample and block
    e_own = (e_want + 13 * (torch.arange(nblk) % 3)[None, :] - 5 * torch.arange(B)[:, None]).to(torch.int32)
    xs = x * CC.per_pixel(e_own - e_want, HW, F32)
    p_own = CC.planes_of(xs, e_own)
    hi, lo = CC.planes_halves(p_own)
    want = (hi + lo) * CC.per_pixel(e_own, HW, F32)

    def back():
        pd = cu(p_own)
        pd.cips3d_exp = cu(e_own)
        gx = Guarded(B, Cc, 1, HW)
        hip.from_planes(pd, 1, HW, out=gx.t)
        return dict(x=gx.t), [gx]

    for r in twice(back):
        assert torch.equal(bits(r["x"].reshape(B, Cc, HW)), bits(want)), "from_planes is not (hi + lo) 2^e of the pixel's block"

    def p16():
        gp, gx = Guarded(B, Cc // 8, HW, 8, dtype=torch.bfloat16), Guarded(B, Cc, 1, HW)
        p = hip.to_planes16(xd, out=gp.t)
        hip.from_planes16(p, 1, HW, out=gx.t)
        return dict(p=gp.t, x=gx.t), [gp, gx]

    for r in twice(p16):
        assert torch.equal(bits(r["p"]), bits(CC.planes16_of(x)))
        assert torch.equal(bits(r["x"].reshape(B, Cc, HW)), bits(CC.bf16_round(x)))


# ---------------------------------------------------------------------------------------------- one producer-to-consumer run
def test_three_layers_from_to_planes():
    """to_planes writes one exponent per sample; the layers behind it choose their own per pixel block: with the input multiplied
    by 2^(3 blk) the exponents differ between the blocks from the second layer's output on.  Each layer against fp64 of its own
    stored input, with the lconst the library derives (cips3d_range_consts) and the patch maxima the layer before left."""
    B, Cin, Cout, HW = CC.RUN_CASE
    case = CC.ChainCase("split", B, Cin, Cout, HW, "planes", noise="per_sample")
    g = CC._gen(41, B, Cin, HW)
    x = torch.randn(B, Cin, HW, generator=g) * torch.pow(2.0, 3.0 * CC.px_block(HW)).reshape(1, 1, HW)
    cur = hip.to_planes(cu(x).view(B, Cin, 1, HW))
    nw = torch.tensor([CC.NOISE_W], device=DEV)
    for layer in range(3):
        W = torch.randn(Cout, Cin, generator=g)
        s = 1.0 + 0.4 * (2.0 * torch.rand(B, Cin, generator=g) - 1.0)
        t = dict(noise=torch.randn(B, 1, HW, generator=g), bias=torch.randn(Cout, generator=g) * 0.5, w_rgb=None)
        wm = hip.modulate_weights(cu(W).view(1, Cout, Cin, 1, 1), cu(s), Cin, B, Cout, Cin, 1, CC.f32(Cin ** -0.5), True, True, split=True)
        wh, wl = CC.unpack_split_halves(wm.cpu(), B, Cout, Cin)
        noise, bias = cu(t["noise"]), cu(t["bias"])
        lconst = hip.range_consts(B, bias, nw, Cin ** 0.5, noise=noise)
        xh, xl = CC.planes_halves(cur.cpu())
        ops = dict(xh=xh, xl=xl, wh=wh, wl=wl, exps=cur.cips3d_exp.cpu(), pmax=cur.cips3d_pmax.cpu(), lconst=lconst.cpu())
        ref = CC.reference(case, t, ops)

        def run():
            go, ge, gm = Guarded(B, Cout // 8, 2, HW, 8, dtype=torch.float16), Guarded(B, case.nblk, dtype=torch.int32), \
                Guarded(B, case.nhalf, Cout // 16, fill=NAN)
            hip.modconv1x1_planes(cur, wm, Cout, HW, "planes", epilogue=1, noise=noise, noise_w=nw, bias=bias, lconst=lconst,
                                  out=go.t, out_exp=ge.t, out_pmax=gm.t)
            return dict(out=go.t, exp=ge.t, pmax=gm.t), [go, ge, gm]

        res = twice(run)[1]
        hi, lo = CC.planes_halves(res["out"])
        ratios = CC.check_outputs(case, t, ops, ref, dict(hi=hi, lo=lo, exp=res["exp"], pmax=res["pmax"]))
        print(f"RATIO | split 64x128 | planes | run layer {layer} | {ratios['planes exit']:.3g} | three layers {CC.RUN_CASE}")
        if layer >= 1:
            assert bool((res["exp"][:, 0] != res["exp"][:, 1]).all()), f"layer {layer}: the blocks' exponents do not differ"
        cur = cu(res["out"])
        cur.cips3d_exp, cur.cips3d_pmax = cu(res["exp"]), cu(res["pmax"])

