"""The NeRF backward against fp64 autograd where a wave of the fused kernels owns SEVERAL samples (csrc/nerf_bwd_fused.hip; the
stash csrc/nerf.hip writes), and the materialised sequence (csrc/nerf_bwd.hip) at its dispatch edges.

cips3d_nerf_suggest_chunks gives every small shape n_chunks == N: one sample per wave, a sample loop that runs once.  Here the
chunk count is set by hand, so that the loop's three gates run with a wrong answer possible: `live = task_ok && sg < N` (a short
last chunk, a chunk wholly beyond N), the clamp sk = min(sg, N - 1) behind it, and the tasks of a view padded to whole
workgroups beside live chunks of several samples.  Cases, reference (the render with the FiLM table as a leaf, float64) and
bound are those of tests/_nerf_bwd_cases.py; test_nerf_bwd_cases_host.py shows on the CPU that the reference is the oracle's
render and that the bound rejects a sample, or one 16-ray group of a sample, that does not reach d film or reaches it twice: the
mildest of these mutants moves a slice by 4.7e3 units of max(e32, 1e-5), the bound allows 8.

Every case runs on both stash routes: the backward recomputes the forward (`fwd=None`, n_chunks given), or the differentiable
forward filled the stash for the same n_chunks.  On the second route stash, sdf and crgb are NaN before the forward runs: a row
the forward leaves unwritten and the backward reads is a non-finite gradient.  The materialised sequence runs on the same
inputs under the same bound -- its first direct fp64 pin at hidden widths 64 .. 256.

Bound per slice (one (layer, gamma | beta) of d film; d cam_poses): K * max(e32, 1e-5) of the slice's fp64 max-abs, e32 = the
error of the same expression in fp32 on the CPU, K = 8 (split-fp16 products: 4 x; summation order and float atomics: 2 x).

Measured err / max(e32, 1e-5), largest slice of each case, on an MI355X (K = 8 admits all of them; no case needs its own K;
the float atomics move the last digit from run to run):

    case                      recompute            forward-filled       materialised
    h32-d2-b2-s8-n7-c1        0.75 (cam)           0.75 (cam)           0.94 (cam)
    h32-d2-b2-s8-n7-c2        0.53 (film.0.beta)   0.52 (film.0.beta)   0.50 (film.0.gamma)
    h64-d3-b3-s12-n7-c3       0.99 (film.0.gamma)  0.99 (film.0.gamma)  1.00 (cam)
    h64-d2-b1-s8-n7-c5        0.91 (film.0.gamma)  0.91 (film.0.gamma)  0.93 (film.0.gamma)
    h128-d2-b1-s16-n10-c4     0.70 (film.0.gamma)  0.71 (film.0.gamma)  0.70 (film.0.gamma)
    h256-d2-b2-s16-n9-c2      0.76 (cam)           0.76 (cam)           0.82 (cam)
    h256-d8-b1-s8-n5-c2       1.11 (film.5.beta)   1.11 (film.5.beta)   1.14 (film.5.beta)
    h32-d1-b1-s8-n5-c2        0.27 (film.0.gamma)  0.27 (film.0.gamma)  0.27 (film.1.beta)
    h64-d2-b2-s8-n7-c3-geo    0.77 (cam)           0.77 (cam)           0.80 (cam)
    h32-d2-b1-s6-n2           -                    -                    0.64 (cam)
    h32-d2-b1-s6-n32          -                    -                    0.43 (film.0.beta)
    h32-d2-b1-s6-n33          -                    -                    0.88 (film.0.gamma)
    h32-d2-b2-s10-n17         -                    -                    0.70 (film.0.gamma)
"""
import functools

import pytest
import torch

import _nerf_bwd_cases as NC
import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
K_OF = {}          # case id -> its own K (<= NC.K_CAP), with the analysis that allows it; none needed


@functools.lru_cache(maxsize=None)
def _setup(case):
    G = pkg.build_generator(case.cfg(), DEV, seed=case.seed)
    r = G.renderer
    t = NC.inputs(case)
    assert torch.equal(r.network.views_linears.weight.cpu(), t["sd"]["renderer.network.views_linears.weight"])
    cu = lambda v: None if v is None else v.to(DEV).contiguous()
    dF, dT, dM, dX = (cu(v) for v in NC.upstreams(case, t))
    d = {k: cu(t[k]) for k in ("cam", "focal", "near", "far", "u", "film")}
    packed, layer_bias = r._derived_buffers()
    args = (r.network, r.sigmoid_beta.detach(), d["cam"], d["focal"], d["near"], d["far"], d["u"], d["film"], layer_bias)
    return r, d, args, packed, (dF, dT), (dM, dX)


def _render(case, r, d, **kw):
    return r.render(d["cam"], d["focal"], d["near"], d["far"], None, case.S, case.N, perturb_u=d["u"], static_viewdirs=case.static,
                    film=d["film"], **kw)


def _geo(case, geo, xyz):
    return dict(d_mask=geo[0], d_xyz=geo[1], xyz=xyz) if case.geo else {}


def _check(case, route, got):
    assert all(bool(torch.isfinite(g).all()) for g in got), f"{case.id} {route}: non-finite gradient"
    ratios = NC.ratios(case, got)
    worst = max(ratios, key=ratios.get)
    print(f"RATIO {case.id} {route}: worst {ratios[worst]:.2f} at {worst}; " + " ".join(f"{k}={v:.2f}" for k, v in ratios.items()))
    k = K_OF.get(case.id, NC.K)
    assert k <= NC.K_CAP
    for name, v in ratios.items():
        assert v <= k, f"{case.id} {route} {name}: {v:.2f} x max(e32, 1e-5), bound {k}"


@pytest.mark.parametrize("route", ["recompute", "forward"])
@pytest.mark.parametrize("case", NC.CHUNK_CASES, ids=[c.id for c in NC.CHUNK_CASES])
def test_fused_backward_of_chunks_of_several_samples_vs_fp64(case, route):
    assert hip.nerf_backward_fused_supported(case.hidden, case.depth, case.S, case.N)
    r, d, args, packed, (dF, dT), geo = _setup(case)
    plain = _render(case, r, d, n_chunks=case.n_chunks)
    fwd = None
    if route == "forward":
        fwd = hip.nerf_forward_stash(case.B, case.S, case.N, case.hidden, case.depth, DEV, n_chunks=case.n_chunks)
        assert fwd["n_chunks"] == case.n_chunks and fwd["stash"].numel() == NC.stash_floats(case)
        for k in ("stash", "sdf", "crgb"):
            fwd[k].fill_(float("nan"))
        kept = _render(case, r, d, stash=fwd)
        for a, b in zip(plain, kept):
            if a is not None:
                assert torch.equal(a, b)
    got = hip.nerf_backward_fused(*args, packed, r._packed_transposed(), case.S, case.N, case.static, dF, dT, fwd=fwd,
                                  n_chunks=None if fwd is not None else case.n_chunks, **_geo(case, geo, plain[4]))
    _check(case, route, got)


@pytest.mark.parametrize("case", NC.ALL_CASES, ids=[c.id for c in NC.ALL_CASES])
def test_materialised_backward_vs_fp64(case):
    r, d, args, packed, (dF, dT), geo = _setup(case)
    xyz = _render(case, r, d)[4] if case.geo else None
    got = hip.nerf_backward(*args, case.S, case.N, case.static, dF, dT, **_geo(case, geo, xyz))
    _check(case, "materialised", got)


def test_chunk_count_outside_the_ray_is_refused():
    case = NC.CHUNK_CASES[0]
    r, d, args, packed, (dF, dT), _ = _setup(case)
    for bad in (0, case.N + 1):
        with pytest.raises(ValueError, match="n_chunks"):
            hip.nerf_backward_fused(*args, packed, r._packed_transposed(), case.S, case.N, case.static, dF, dT, n_chunks=bad)
    fwd = hip.nerf_forward_stash(case.B, case.S, case.N, case.hidden, case.depth, DEV, n_chunks=2)
    with pytest.raises(ValueError, match="n_chunks"):
        hip.nerf_backward_fused(*args, packed, r._packed_transposed(), case.S, case.N, case.static, dF, dT, fwd=fwd, n_chunks=1)
