"""The bounds and cases of tests/_decoder_bwd_cases.py, checked without a GPU on every case test_gpu_decoder_bwd.py runs and
at both gradient scales: (a) the same expression evaluated by torch in fp32 on the CPU stays inside the bound against fp64 -- a
correct fp32 implementation passes; (b) every subtly wrong reference (a float4 of pixels dropped or counted twice, a chunk's
last step counted in the next chunk too, a transposed output, the slope of zero, a dropped block, a stride-0 noise read, ...)
leaves it on at least one element -- the GPU test has teeth; (c) every case is in the regime it is listed for, and its
sentinels sit on the edges the replayed launch arithmetic gives."""
import pytest
import torch

import _decoder_bwd_cases as BC

F32, F64 = torch.float32, torch.float64
ids = lambda cases: [c.id for c in cases]      # noqa: E731


def admits_and_rejects(what, ref, bound, fp32, mutants):
    """mutants: {name: tensor}"""
    assert ref.shape == bound.shape == fp32.shape, what
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), what
    ratio, at = BC.worst((fp32.double() - ref).abs(), bound)
    assert BC.inside(fp32, ref, bound), f"{what}: torch fp32 is {ratio:.2f} x the bound at element {at}"
    for name, m in mutants.items():
        assert m.shape == ref.shape, (what, name)
        assert not BC.inside(m, ref, bound), f"{what}: the mutant `{name}` stays inside the bound"
    return ratio


def in_its_regime(case):
    got = case.regime()
    for k, v in case.expect.items():
        assert got[k] == v, f"{case.id}: {k} is {got[k]}, the case is listed for {v}"


def sentinels_on(t, positions, P):
    """the planted magnitude on every row at exactly these pixels (gradient scale 1)"""
    big = (t.abs() == BC.SENT)
    assert bool(big[..., positions].all())
    rest = torch.ones(P, dtype=torch.bool)
    rest[positions] = False
    assert not bool(big[..., rest].any())


# ------------------------------------------------------------------------------------------------------------- gemm_wgrad
@pytest.mark.parametrize("gs", BC.SCALES)
@pytest.mark.parametrize("case", BC.WGRAD_CASES, ids=ids(BC.WGRAD_CASES))
def test_gemm_wgrad_bound(case, gs):
    t = case.tensors(gs)
    chunk = case.launch()[3]
    ref = BC.wgrad_ref(t, F64)
    muts = {m: BC.wgrad_ref(t, F64, m, chunk) for m in case.mutants()}
    admits_and_rejects(case.id, ref, BC.wgrad_bound(t["dy"], t["x"]), BC.wgrad_ref(t, F32), muts)


@pytest.mark.parametrize("case", BC.WGRAD_CASES, ids=ids(BC.WGRAD_CASES))
def test_gemm_wgrad_case_regime_and_sentinels(case):
    in_its_regime(case)
    mb, kb, n, chunk = case.launch()
    assert chunk % 16 == 0 and (n - 1) * chunk < case.P <= n * chunk
    edges = BC.chunk_edges(case.P, chunk)
    assert len(edges) == n and edges[0][0] == 0 and edges[-1][1] == case.P
    assert all(a[1] == b[0] for a, b in zip(edges, edges[1:]))
    pos = case.sentinels()
    assert set(pos) == {p for a, b in edges for p in (a, b - 1)} | {case.P - 4, case.P - 1}
    t = case.tensors()
    sentinels_on(t["dy"], pos, case.P)
    sentinels_on(t["x"], pos, case.P)


def test_gemm_wgrad_cases_are_the_regimes_the_kernel_has():
    r = [c.regime() for c in BC.WGRAD_CASES]
    assert {x["n_chunks"] for x in r} >= {1, 2, 5, 9, 17}
    assert any(x["last_step"] == 4 and x["n_chunks"] > 1 for x in r) and any(x["last_step"] == 16 for x in r)
    assert any(x["idle_wave_row"] for x in r) and any(x["idle_wave_col"] for x in r)
    assert any(x["mb"] > 1 and x["kb"] > 1 for x in r)
    assert any(c.B > 1 for c in BC.WGRAD_CASES) and max(c.P for c in BC.WGRAD_CASES) <= 4112
    assert all(c.M % 32 == 0 and c.K % 32 == 0 and c.P % 4 == 0 for c in BC.WGRAD_CASES)


# ----------------------------------------------------------------------------------------------------- noise + bias + lrelu
@pytest.mark.parametrize("gs", BC.SCALES)
@pytest.mark.parametrize("case", BC.ACT_CASES, ids=ids(BC.ACT_CASES))
def test_noise_bias_act_bwd_bounds(case, gs):
    t = case.tensors(gs)
    ps = case.per_sample
    ref, fp32, bounds = BC.act_ref(t, F64, ps), BC.act_ref(t, F32, ps), BC.act_bounds(t, ps)
    muts = {m: BC.act_ref(t, F64, ps, m) for m in case.mutants()}
    for k, name in enumerate(("dx", "dnoise", "dnw", "db")):
        admits_and_rejects(f"{case.id} {name}", ref[k], bounds[k], fp32[k], {m: g[k] for m, g in muts.items() if k in BC.ACT_HITS[m]})
    assert ref[1].shape == t["noise"].shape


@pytest.mark.parametrize("case", BC.ACT_CASES + BC.RGB_CASES, ids=ids(BC.ACT_CASES + BC.RGB_CASES))
def test_block_case_regime_and_sentinels(case):
    in_its_regime(case)
    nblk, live = BC.pixel_blocks(case.HW)
    assert case.HW % 4 == 0 and (nblk - 1) * 1024 + 4 * live == case.HW and 1 <= live <= 256
    pos = case.sentinels()
    assert set(pos) == {p for b in range(nblk) for p in (1024 * b, min(1024 * (b + 1), case.HW) - 1)} | {case.HW - 4, case.HW - 1}
    t = case.tensors()
    for k in (("dy", "noise") if "dy" in t else ("drgb", "x")):
        sentinels_on(t[k], pos, case.HW)
    if "y" in t:          # both zeros are there, and on pixels that carry a sentinel gradient
        y = t["y"]
        assert bool((y[..., :2] == 0).all()) and not bool(torch.signbit(y[..., :2]).any()) and 0 in pos
        assert bool((y[..., -2:] == 0).all()) and bool(torch.signbit(y[..., -2:]).all()) and case.HW - 1 in pos
        assert int((y == 0).sum()) == 4 * case.B * case.C


def test_noise_cases_are_the_regimes_the_kernels_have():
    r = [c.regime() for c in BC.ACT_CASES]
    assert any(x["blocks"] > 1 and x["live_last"] == 1 for x in r) and any(x["live_last"] == 256 for x in r)
    assert any(x["channel_chunks"] > 1 and x["last_chunk"] == 1 for x in r)
    assert any(c.per_sample for c in BC.ACT_CASES) and any(not c.per_sample and c.B > 1 for c in BC.ACT_CASES)
    # block_sum_256 over a partly filled block: nothing to add for one live thread, the full tree for 256
    assert [BC.tree_adds(n) for n in (1, 2, 3, 64, 65, 256)] == [0, 1, 2, 6, 7, 9]
    assert BC.live_threads(4) == 1 and BC.live_threads(1028) == 256
    # the wrappers' rule: per-sample noise only if B > 1
    assert BC.noise_stride(1, 1, 1024) == 0 and BC.noise_stride(3, 3, 8) == 8 and BC.noise_stride(3, 1, 8) == 0
    assert any(c.B == 1 and c.noise_batch == 1 for c in BC.ACT_CASES)
    # the flag combinations: both accumulators (one memset), the bias alone without noise, the noise weight without the
    # bias (separate memsets), the noise map without the noise weight
    flags = {name: (kw, has_noise) for name, kw, has_noise in BC.ACT_FLAGS}
    assert all(flags["all"][0].values()) and flags["all"][1]
    assert flags["db_only"] == (dict(need_dnoise=False, need_dnw=False, need_db=True), False)
    assert flags["dnw_no_db"][0]["need_dnw"] and not flags["dnw_no_db"][0]["need_db"]
    assert flags["dnoise_no_dnw"][0]["need_dnoise"] and not flags["dnoise_no_dnw"][0]["need_dnw"]


# --------------------------------------------------------------------------------------------------------------------- ToRGB
@pytest.mark.parametrize("gs", BC.SCALES)
@pytest.mark.parametrize("case", BC.RGB_CASES, ids=ids(BC.RGB_CASES))
def test_torgb_bwd_bounds(case, gs):
    t = case.tensors(gs)
    ref, fp32, bounds = BC.rgb_ref(t, F64), BC.rgb_ref(t, F32), BC.rgb_bounds(t)
    muts = {m: BC.rgb_ref(t, F64, m) for m in case.mutants()}
    for k, name in enumerate(("dx", "dwm", "db")):
        admits_and_rejects(f"{case.id} {name}", ref[k], bounds[k], fp32[k], {m: g[k] for m, g in muts.items() if k in BC.RGB_HITS[m]})


def test_torgb_cases_are_the_regimes_the_kernel_has():
    assert {c.regime()["blocks"] for c in BC.RGB_CASES} == {1, 2, 3}
    assert any(c.C % 2 == 1 and c.C > 1 for c in BC.RGB_CASES) and any(c.C == 1 for c in BC.RGB_CASES)
    # every mutant is applied somewhere
    assert {m for c in BC.RGB_CASES for m in c.mutants()} == set(BC.RGB_HITS)
    assert {m for c in BC.ACT_CASES for m in c.mutants()} == set(BC.ACT_HITS)


# ---------------------------------------------------------------------------------------------------------------- modulation
@pytest.mark.parametrize("gs", BC.SCALES)
@pytest.mark.parametrize("case", BC.MOD_CASES, ids=ids(BC.MOD_CASES))
def test_modulate_bwd_bounds(case, gs):
    t = case.tensors(gs)
    ref, fp32, bounds = BC.mod_grads(t, case, F64), BC.mod_grads(t, case, F32), BC.mod_bounds(t, case)
    closed = BC.mod_closed(t, case, F64)
    muts = {m: BC.mod_closed(t, case, F64, m) for m in case.mutants()}
    for k, name in enumerate(("dW", "ds")):
        # the closed form the bound and the mutants are built from is the derivative of the forward formula
        assert float((closed[k] - ref[k]).abs().max()) <= 1e-12 * float(ref[k].abs().max()), name
        admits_and_rejects(f"{case.id} {name}", ref[k], bounds[k], fp32[k],
                           {m: g[k] for m, g in muts.items() if k in BC.mod_hits(m, case.demod)})


def test_modulate_cases_are_the_regimes_the_kernels_have():
    for c in BC.MOD_CASES:
        in_its_regime(c)
    assert any(not c.demod for c in BC.MOD_CASES) and any(c.regime()["idle_lanes"] for c in BC.MOD_CASES)
    assert any(c.regime()["rows"] % 4 for c in BC.MOD_CASES) and any(c.regime()["row_len"] > 256 for c in BC.MOD_CASES)
    assert {m for c in BC.MOD_CASES for m in c.mutants()} == {"tap_index", "no_projection", "eps_missing"}
    small = [c for c in BC.MOD_CASES if c.s_scale != 1.0]
    assert len(small) == 1
    t = small[0].tensors()
    u = BC._mod_parts(t, small[0], F64)[3]
    ss = (u * u).sum(-1)
    assert float(ss.min()) < 1e-5 and float(ss.max()) > 1e-8       # the 1e-8 is between 1e-3 and 1 of the sum it is added to


# ------------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("B,M,K", BC.PACK_CASES)
def test_unpack_inverts_the_kernel_index_map(B, M, K, transpose):
    wm = BC.pack_input(B, M, K)
    idx = BC.pack_index(B, M, K, transpose)
    assert sorted(idx.tolist()) == list(range(B * M * K))           # a bijection: every float of the buffer is written once
    packed = torch.empty(B * M * K)
    packed[idx] = wm.reshape(-1)
    want = wm.transpose(1, 2) if transpose else wm
    assert torch.equal(BC.unpack(packed, B, M, K, transpose), want)


@pytest.mark.parametrize("B,M,K,transpose", BC.PACK_SPLIT_CASES)
def test_unpack_split_inverts_the_kernel_index_map(B, M, K, transpose):
    """the split form built here element by element with pack_kernel's index arithmetic (hi = fp16(v), lo = fp16(v - hi))"""
    wm = BC.pack_input(B, M, K)
    OM, OK = (K, M) if transpose else (M, K)
    assert OK % 32 == 0 and OM % 16 == 0
    e = torch.arange(B * M * K)
    b, r, c = e // (M * K), (e // K) % M, e % K
    o, i = (c, r) if transpose else (r, c)
    blk = ((b * (OM // 16) + o // 16) * (OK // 32) + i // 32) * 1024
    at = blk + (((i // 8) % 4) * 16 + o % 16) * 8 + i % 8
    v = wm.reshape(-1) * 256.0
    hi = v.half()
    lo = (v - hi.float()).half()
    halves = torch.zeros(2 * B * M * K, dtype=torch.float16)
    halves[at], halves[at + 512] = hi, lo
    got = BC.unpack_split(halves.view(torch.float32), B, M, K, transpose)
    want = wm.transpose(1, 2) if transpose else wm
    assert float((got - want).abs().max()) <= 2.0 ** -21 * float(wm.abs().max())
