"""The bounds of tests/_dense_cases.py, checked without a GPU on every case test_gpu_dense_heads.py runs: (a) the same
expression evaluated by torch in fp32 on the CPU stays inside the bound against fp64 -- a correct fp32 implementation passes;
(b) a subtly wrong reference (a dropped input column, a dropped sample or output row of a gradient sum, slope 0.2 everywhere,
a norm over one element less, the truncation lerp the other way round) leaves it on at least one element -- the test has teeth."""
import pytest
import torch

import _dense_cases as DC

F32, F64 = torch.float32, torch.float64


def admits_and_rejects(what, ref, bound, fp32, mutants):
    """mutants: {name: tensor}"""
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), what
    ratio, at = DC.worst((fp32.double() - ref).abs(), bound)
    assert DC.inside(fp32, ref, bound), f"{what}: torch fp32 is {ratio:.2f} x the bound at element {at}"
    for name, m in mutants.items():
        assert not DC.inside(m, ref, bound), f"{what}: the mutant `{name}` stays inside the bound"


FORWARD = DC.SHAPE_CASES + DC.EPILOGUE_CASES + DC.ZERO_ROW_CASES + DC.FALLBACK_CASES


@pytest.mark.parametrize("case", FORWARD, ids=[c.id for c in FORWARD])
def test_linear_bound(case):
    t, s = case.tensors(), case.scalars()
    ref = DC.linear_ref(t, s, F64)
    muts = {m: DC.linear_ref(t, s, F64, m) for m in case.mutants()}
    for vec in ((False, True) if case.in_dim % 4 == 0 else (False,)):      # (the fall-backs run the scalar path at in % 4 == 0)
        admits_and_rejects(f"{case.id} vec={vec}", ref, DC.linear_bound(t, s, vec=vec), DC.linear_ref(t, s, F32), muts)
    if case.zero_row is not None:                                          # a row of zeros: the bias path, exactly
        row = ref[case.zero_row]
        bias_only = DC.linear_ref(dict(t, x=torch.zeros_like(t["x"]), W=torch.zeros_like(t["W"])), dict(s, pixelnorm=False), F64)
        assert torch.equal(row, bias_only[case.zero_row]) and bool(torch.isfinite(row).all())


@pytest.mark.parametrize("B,C", DC.PIXEL_NORM_SHAPES)
def test_pixel_norm_bound(B, C):
    x = DC.pixel_norm_input(B, C)
    admits_and_rejects(f"pixel_norm {B}x{C}", DC.pixel_norm_ref(x, F64), DC.pixel_norm_bound(x), DC.pixel_norm_ref(x, F32),
                       {"norm_short": DC.pixel_norm_ref(x, F64, "norm_short")})


@pytest.mark.parametrize("case", DC.BWD_CASES, ids=[c.id for c in DC.BWD_CASES])
def test_linear_bwd_bounds(case):
    t, s = case.tensors(), case.s
    if case.lrelu:
        assert DC.bwd_margin(t, s) > 4, "a pre-activation within four error bounds of zero: the slope may be decided differently"
    ref, fp32, bounds = DC.linear_grads(t, s, F64), DC.linear_grads(t, s, F32), DC.linear_bwd_bounds(t, s)
    muts = {m: DC.linear_grads(t, s, F64, m) for m in case.mutants()}
    hits = {"drop_out_row": (0,), "drop_batch_row": (1, 2), "slope": (0, 1, 2)}      # which gradients a mutant changes
    for k, name in enumerate(("dx", "dW", "db")):
        admits_and_rejects(f"{case.id} {name}", ref[k], bounds[k], fp32[k], {m: g[k] for m, g in muts.items() if k in hits[m]})


def _tables():
    return [DC.forward_table(n, B) for n in DC.TABLE_SIZES for B in (1, 5)] + [DC.backward_table(k) for k in DC.BACKWARD_TABLES]


@pytest.mark.parametrize("tab", _tables(), ids=lambda t: t.name)
def test_table_bounds(tab):
    ref, fp32, bounds, mut = DC.table_ref(tab, F64), DC.table_ref(tab, F32), DC.table_bounds(tab), DC.table_ref(tab, F64, "drop_col")
    for i in range(len(tab.heads)):
        admits_and_rejects(f"{tab.name} head {i}", ref[i], bounds[i], fp32[i], {"drop_col": mut[i]})
    # the heads tile the output buffer's used part without overlap
    n = sum(h.out_dim for h in tab.heads) * tab.B
    assert int(tab.written().sum()) == n


@pytest.mark.parametrize("kind", DC.BACKWARD_TABLES, ids=lambda k: "-".join(map(str, k)))
def test_table_bwd_bounds(kind):
    tab = DC.backward_table(kind)
    (dx, dW, db), (fx, fW, fb), (ex, eW, eb) = DC.table_grads(tab, F64), DC.table_grads(tab, F32), DC.table_bwd_bounds(tab)
    mx = DC.table_grads(tab, F64, "drop_out_row")[0]
    _, mW, mb = DC.table_grads(tab, F64, "drop_batch_row")
    admits_and_rejects(f"{tab.name} dx", dx, ex, fx, {"drop_out_row": mx})
    for i, h in enumerate(tab.heads):
        admits_and_rejects(f"{tab.name} dW{i}", dW[i], eW[i], fW[i], {"drop_batch_row": mW[i]})
        if h.b is not None:
            admits_and_rejects(f"{tab.name} db{i}", db[i], eb[i], fb[i], {"drop_batch_row": mb[i]})


def test_the_case_matrix_keeps_every_value_of_every_axis():
    assert {c.in_dim for c in DC.SHAPE_CASES} == set(DC.IN_DIMS) and {c.out_dim for c in DC.SHAPE_CASES} == set(DC.OUT_DIMS)
    for n in DC.IN_DIMS:
        assert {c.B for c in DC.SHAPE_CASES if c.in_dim == n} == set(DC.BATCHES)
    for o in DC.OUT_DIMS:
        assert {c.B for c in DC.SHAPE_CASES if c.out_dim == o} == set(DC.BATCHES)
