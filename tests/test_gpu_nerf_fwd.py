"""The NeRF forward against fp64 in every instantiation cips3d_nerf_render can launch (csrc/nerf.hip: nerf_render_kernel at hidden
32 / 64 / 128 / 256, camera and explicit geometry, split-fp16 and exact fp32, four- and two-tile slabs, the fused finish and both
stand-alone finish kernels), through the public surface: VolumeFeatureRenderer.render / forward / set_precision.  Cases, reference
(the oracle's render with the FiLM table as a leaf, float64) and bound are those of tests/_nerf_fwd_cases.py;
test_nerf_fwd_cases_host.py shows on the CPU that the reference is the oracle's render, that every case is well conditioned, that
the bound rejects a lost fp16 low half of one o-tile, a sample composited twice and the naive softplus, and that the planners put
every case on the route its row names.

Bound per map (features, thumb, mask, depth, xyz, sdf), over the whole map: RMS error <= 2 x max(e32_rms, floor), max error <=
4 x max(e32_max, floor); e32 = the error of the same expression in fp32 on the CPU, floor = 2^-23 x the map's fp64 max-abs.

    row  hidden, D   B  rays     N  chunks  what it reaches
    a    32, 1       2  5 x 5    5  2       no hidden MFMA layer; finish not fused (table < 1024 floats); ragged group, scalar finish
    b    32, 2       1  4 x 4    1  1       N = 1: the only sample is the last one (delta = 1e10)
    c    32, 10      2  5 x 5    7  4       first depth at which NT = 2 fuses the finish; two ray groups per workgroup
    d    64, 1       1  6 x 6    6  2       hidden 64, table still too small to fuse; vector finish, ragged group
    e    64, 2       3  7 x 7    7  3       3 does not divide 8: `part` route; 12 tasks padded to 16
    f    64, 3       2  5 x 5    9  8       fused, the unrolled NC = 8 form; chunks 5 .. 7 wholly beyond N
    g    64, 4       1  4 x 4    8  1       fused with one chunk: one live wave of eight; odd hidden layer plus a pair
    h    128, 2      1  6 x 6    10 4       static viewdirs; NC = 4, second half of the second workgroup idle
    i    128, 5      2  4 x 4    3  2       no perturbation
    j    256, 2      2  5 x 5    9  2       four-tile slabs, fused, four groups per workgroup
    k    256, 3      1  4 x 4    5  5       odd depth at NT = 16 (pairs only); `part` route
    l    256, 9      1  4 x 4    4  4       fused finish with the LDS exactly full (calm table)
    m    256, 10     1  5 x 5    4  2       fuse refused by LDS size, four-tile unfused exactly full (calm)
    n    256, 11     1  5 x 5    4  2       launch_render<16, 2>, first depth (calm)
    o    256, 16     1  4 x 4    3  1       the two-tile form with a larger table (calm)
    p    256, 2 | 11 1  5 x 5    5  2       set_precision("fp32_exact"): the F32 instantiation and its two-tile fallback
    q    32 | 256, 2 2  37       5  2       explicit geometry (XG); R odd and ragged; z and points from the caller
    r    64, 2       1  1        3  1       one ray
    s    64, 2       2  5 x 5    7  3 | 4   sigmoid_beta = 0.01, 0.001: a hard surface, T collapses inside a chunk
    t    64 | 256, 2 2  5 x 5    7  3 | 4   with_sdf=False, sigma_linear.bias in {-20, 0, +25}; -8, -11, -14 at hidden 64

The STASH instantiation is not repeated here: test_gpu_nerf_bwd_chunks.py shows its maps equal the plain render's bit for bit.

Measured on an MI355X, error / max(e32, floor), the largest map of each case (the forward has no atomics: the figures repeat).
Every case passes with the plain factors 2 x / 4 x except the `mask` of s-...-c3-beta0.001, which has the capped factors 4 x / 8 x of
_nerf_fwd_cases.K_OF with the analysis written there (one ray 5.5 beta in front of a hard surface; e32 a lucky draw).  On the parent
of the commit that added this file the four `t` cases at bias -20 failed (features 4.6e4 x, thumb 3.3e6 x, mask 8.4e6 x: the
kernel's softplus was log(1 + exp(x)), 0 below -16.6, and the last sample lost the ray's transmittance).

    case                                       route               max                rms
    a-h32-d1-b2-s5-n5-c2                       render              1.03 (sdf)         1.14 (mask)
    b-h32-d2-b1-s4-n1-c1                       render              1.27 (sdf)         1.12 (sdf)
    c-h32-d10-b2-s5-n7-c4                      render              1.02 (xyz)         1.02 (depth)
    d-h64-d1-b1-s6-n6-c2                       render              1.26 (thumb)       1.01 (mask)
    e-h64-d2-b3-s7-n7-c3                       render              1.10 (depth)       1.05 (mask)
    f-h64-d3-b2-s5-n9-c8                       render              1.00 (mask)        1.01 (features)
    g-h64-d4-b1-s4-n8-c1                       render              1.26 (thumb)       1.22 (thumb)
    h-h128-d2-b1-s6-n10-c4-static              render              1.05 (features)    1.11 (mask)
    i-h128-d5-b2-s4-n3-c2-nou                  render              1.22 (mask)        1.05 (features)
    j-h256-d2-b2-s5-n9-c2                      render              1.25 (thumb)       1.13 (thumb)
    k-h256-d3-b1-s4-n5-c5                      render              1.11 (mask)        1.16 (mask)
    l-h256-d9-b1-s4-n4-c4-calm                 render              1.24 (mask)        1.35 (features)
    m-h256-d10-b1-s5-n4-c2-calm                render              1.46 (features)    1.27 (features)
    n-h256-d11-b1-s5-n4-c2-calm                render              1.59 (features)    1.37 (features)
    o-h256-d16-b1-s4-n3-c1-calm                render              1.25 (features)    1.35 (features)
    p-h256-d2-b1-s5-n5-c2-f32                  render              1.00 (thumb)       1.01 (thumb)
    p-h256-d11-b1-s5-n5-c2-calm-f32            render              1.47 (sdf)         1.61 (features)
    q-h32-d2-b2-r37x-n5-c2                     render              1.75 (features)    1.25 (features)
    q-h256-d2-b2-r37x-n5-c2                    render              1.40 (sdf)         1.14 (sdf)
    r-h64-d2-b1-r1x-n3-c1                      render              0.98 (features)    0.96 (features)
    s-h64-d2-b2-s5-n7-c3-beta0.01              render              1.14 (features)    1.03 (mask)
    s-h64-d2-b2-s5-n7-c4-beta0.01              render              1.14 (mask)        1.05 (xyz)
    s-h64-d2-b2-s5-n7-c3-beta0.001             render              3.27 (mask)        2.61 (mask)
    s-h64-d2-b2-s5-n7-c4-beta0.001             render              1.08 (mask)        1.09 (mask)
    t-h64-d2-b2-s5-n7-c3-raw-bias-20           render              1.00 (thumb)       1.02 (thumb)
    t-h64-d2-b2-s5-n7-c3-raw-bias0             render              1.92 (mask)        1.01 (depth)
    t-h64-d2-b2-s5-n7-c3-raw-bias25            render              1.22 (thumb)       1.04 (depth)
    t-h64-d2-b2-s5-n7-c4-raw-bias-20           render              1.00 (depth)       1.00 (depth)
    t-h64-d2-b2-s5-n7-c4-raw-bias0             render              1.07 (mask)        1.01 (thumb)
    t-h64-d2-b2-s5-n7-c4-raw-bias25            render              1.05 (features)    1.04 (features)
    t-h256-d2-b2-s5-n7-c3-raw-bias-20          render              1.00 (thumb)       1.03 (thumb)
    t-h256-d2-b2-s5-n7-c3-raw-bias0            render              1.56 (mask)        1.04 (depth)
    t-h256-d2-b2-s5-n7-c3-raw-bias25           render              1.01 (thumb)       1.08 (depth)
    t-h256-d2-b2-s5-n7-c4-raw-bias-20          render              1.04 (features)    1.00 (depth)
    t-h256-d2-b2-s5-n7-c4-raw-bias0            render              1.72 (mask)        1.01 (sdf)
    t-h256-d2-b2-s5-n7-c4-raw-bias25           render              1.02 (features)    1.02 (features)
    t-h64-d2-b2-s5-n7-c4-raw-bias-8            render              1.09 (mask)        0.99 (features)
    t-h64-d2-b2-s5-n7-c4-raw-bias-11           render              1.10 (mask)        0.99 (features)
    t-h64-d2-b2-s5-n7-c4-raw-bias-14           render              1.01 (mask)        1.18 (mask)
    t-h64-d2-b2-s5-n7-c3-raw-bias-20           forward             1.00 (thumb)       1.02 (thumb)
    t-h64-d2-b2-s5-n7-c3-raw-bias-20           volume_integration  1.00 (features)    1.04 (thumb)
    t-h64-d2-b2-s5-n7-c4-raw-bias-20           forward             1.00 (depth)       1.00 (depth)
    t-h64-d2-b2-s5-n7-c4-raw-bias-20           volume_integration  1.00 (features)    1.01 (thumb)
"""
import ctypes
import functools

import pytest
import torch

import _nerf_fwd_cases as FC
from cips_3dplusplus_amd import _lib, hip
from cips_3dplusplus_amd.renderer import VolumeFeatureRenderer

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, SENTINEL = 64, -12345.5
IDS = [c.id for c in FC.CASES]


def cu(t):
    return None if t is None else t.to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _module(hidden, depth, with_sdf, style_dim):
    return VolumeFeatureRenderer(N_layers_renderer=depth, input_dim=3, hidden_dim=hidden, style_dim=style_dim, view_dim=3,
                                 with_sdf=with_sdf, output_features=True).eval().requires_grad_(False).to(DEV)


def renderer(case):
    """the module with the case's state_dict (weights of the generator's renderer, the case's sigmoid_beta and sigma bias)"""
    sd = FC.inputs(case)["sd"]
    r = _module(case.hidden, case.depth, case.with_sdf, sd["renderer.network.pts_linears.0.gamma.weight"].shape[1])
    r.load_state_dict({k[len("renderer."):]: v for k, v in sd.items()}, strict=True)
    return r.set_precision("fp32_exact" if case.exact else "fp32")


def explicit_maps(case, r, pts, rays_d, viewdirs, z):
    t = FC.inputs(case)
    rgb, feat, sdf, mask, xyz, _ = r(cu(pts), cu(rays_d), cu(viewdirs), cu(z), cu(t["near"]), cu(t["far"]), film=cu(t["film"]),
                                     n_chunks=case.n_chunks)
    return {"features": feat.transpose(1, 2), "thumb": rgb.transpose(1, 2), "mask": mask[..., 0], "depth": mask[..., 1],
            "xyz": xyz.transpose(1, 2), "sdf": sdf[..., 0]}


def kernel_maps(case):
    B, N, R, H = case.B, case.N, case.R, case.hidden
    t, r = FC.inputs(case), renderer(case)
    if case.explicit:
        return explicit_maps(case, r, t["pts"], t["rays_d"], t["viewdirs"], t["z"])
    thumb, features, sdf, mask, xyz = r.render(cu(t["cam"]), cu(t["focal"]), cu(t["near"]), cu(t["far"]), None, case.S, N,
                                               perturb_u=cu(t["u"]), static_viewdirs=case.static, return_sdf=True,
                                               n_chunks=case.n_chunks, film=cu(t["film"]))
    return {"features": features.reshape(B, H, R), "thumb": thumb.reshape(B, 3, R), "mask": mask[:, 0].reshape(B, R),
            "depth": mask[:, 1].reshape(B, R), "xyz": xyz.reshape(B, 3, R), "sdf": sdf.reshape(B, R, N)}


def check(case, route, got):
    print(f"RATIO {case.id} {route}: max/rms " + FC.ratio_line(case, got))
    for name, v in got.items():
        assert bool(torch.isfinite(v).all()), f"{case.id} {route} {name}: non-finite"
    bad = FC.violations(case, got)
    assert not bad, f"{case.id} {route}: " + "; ".join(f"{n} {s} error {r:.2f} x the fp32 reference's, bound {k:g}" for n, s, r, k in bad)


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_render_maps_vs_fp64(case):
    check(case, "render", kernel_maps(case))


# ------------------------------------------------------------------------------------------------------------ store discipline
def _padded(n):
    buf = torch.full((PAD + n + PAD,), SENTINEL, device=DEV)
    return buf, buf[PAD:PAD + n]


def _spy_params(case, monkeypatch):
    """the keyword arguments the public call hands to hip.nerf_render_maps, its maps, and the cips3d_nerf_params of that launch"""
    seen, real = {}, hip.nerf_render_maps

    def spy(**kw):
        seen.update(kw)
        return real(**kw)

    monkeypatch.setattr(hip, "nerf_render_maps", spy)
    maps = kernel_maps(case)
    monkeypatch.setattr(hip, "nerf_render_maps", real)
    return seen, maps, hip._nerf_params(seen)


@pytest.mark.parametrize("case", FC.STORE_CASES, ids=[c.id for c in FC.STORE_CASES])
def test_every_output_element_is_written_and_nothing_else(case, monkeypatch):
    """o_*, `part` and `sdf` point into buffers padded by 64 sentinel floats on both sides: the lanes of a ragged ray group beyond
    R, the samples of a short or empty chunk and the padded tasks of a view must store nothing, and every element of the outputs
    (in `part`: every row of every live ray) must be stored"""
    B, N, R, H = case.B, case.N, case.R, case.hidden
    lib = _lib.load()
    seen, maps, p = _spy_params(case, monkeypatch)
    sizes = {"o_features": B * H * R, "o_thumb": B * 3 * R, "o_xyz": B * 3 * R, "o_mask": B * 2 * R, "sdf": B * R * N}
    if not case.fused:
        sizes["part"] = FC.part_floats(case)
    bufs = {k: _padded(n) for k, n in sizes.items()}
    for k, (_, inner) in bufs.items():
        setattr(p, k, inner.data_ptr())
    assert bool(lib.cips3d_nerf_fuses_finish(ctypes.byref(p))) == case.fused
    _lib.check(lib.cips3d_nerf_render(ctypes.byref(p), hip.stream_ptr()), "cips3d_nerf_render")
    if not case.fused:
        _lib.check(lib.cips3d_nerf_finish_rays(p.part, case.n_chunks, B, R, H, p.o_features, p.o_thumb, p.o_xyz, p.o_mask,
                                               hip.stream_ptr()), "cips3d_nerf_finish_rays")
    torch.cuda.synchronize()
    for k, (buf, inner) in bufs.items():
        n = inner.numel()
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + n:] == SENTINEL).all()), f"{k}: store outside the buffer"
        assert not bool((inner == SENTINEL).any()), f"{k}: {int((inner == SENTINEL).sum())} of {n} elements not written"
        assert bool(torch.isfinite(inner).all()), k
    mask = bufs["o_mask"][1].view(B, 2, R)
    again = {"features": bufs["o_features"][1].view(B, H, R), "thumb": bufs["o_thumb"][1].view(B, 3, R), "mask": mask[:, 0],
             "depth": mask[:, 1], "xyz": bufs["o_xyz"][1].view(B, 3, R), "sdf": bufs["sdf"][1].view(B, R, N)}
    for k in FC.MAPS:
        assert torch.equal(again[k], maps[k].reshape(again[k].shape)), k


# ------------------------------------------------------------------------------------------------------------ depth limits
def _deep(D, n_chunks):
    torch.manual_seed(11)
    r = _module(256, D, True, 256)
    g = torch.Generator().manual_seed(D)
    styles = cu(0.5 * torch.randn(1, D + 1, 256, generator=g))
    t = FC.inputs(FC.BY_ID["l-h256-d9-b1-s4-n4-c4-calm"])
    return r.render(cu(t["cam"]), cu(t["focal"]), cu(t["near"]), cu(t["far"]), styles, 4, 4, perturb_u=cu(t["u"]),
                    return_sdf=True, n_chunks=n_chunks)


def test_depth_42_renders_on_the_two_tile_form():
    """the deepest network the LDS holds (the two-tile form exactly full).  No fp64 comparison: the fp32 reference's own error is
    2.4e-2 there; the bound of test_nerf_chunk_count_does_not_change_result instead."""
    assert FC.plan(256, 42, 1) == (False, 2) and FC.plan(256, 42, 2) == (False, 2)
    one, two = _deep(42, 1), _deep(42, 2)
    for a, b in zip(one, two):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
        assert float((a - b).abs().max()) < 3e-6
    assert float(one[1].abs().max()) > 1e-3           # features: not a map of zeros


def test_depth_43_is_refused_before_any_launch(monkeypatch):
    assert FC.plan(256, 43, 2) == (False, None)
    seen, real = {}, hip.nerf_render_maps

    def spy(**kw):
        seen.update(kw)
        return real(**kw)

    monkeypatch.setattr(hip, "nerf_render_maps", spy)
    with pytest.raises(RuntimeError, match="cips3d_nerf_render"):
        _deep(43, 2)
    monkeypatch.setattr(hip, "nerf_render_maps", real)
    p = hip._nerf_params(seen)
    B, R, N, H = 1, 16, 4, 256
    sizes = {"o_features": B * H * R, "o_thumb": B * 3 * R, "o_xyz": B * 3 * R, "o_mask": B * 2 * R, "sdf": B * R * N,
             "part": 2 * B * (H + 8) * R}
    bufs = {k: _padded(n) for k, n in sizes.items()}
    for k, (_, inner) in bufs.items():
        setattr(p, k, inner.data_ptr())
    lib = _lib.load()
    assert lib.cips3d_nerf_render(ctypes.byref(p), hip.stream_ptr()) != 0
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert bool((buf == SENTINEL).all()), f"{k}: written by a refused call"


# ------------------------------------------------------------------------------------------------------------ raw density
RAW_EMPTY = [c for c in FC.CASES if c.key == "t" and c.bias == -20.0 and c.hidden == 64]


@pytest.mark.parametrize("case", RAW_EMPTY, ids=[c.id for c in RAW_EMPTY])
def test_raw_density_of_empty_space_on_every_surface(case):
    """exp(-20) of density along the whole ray: the last sample (delta = 1e10) carries the ray.  The explicit form of the render
    kernel and the stand-alone Render.volume_integration op (csrc/render_ops.hip) against the same fp64 maps, under the same
    bound, on the fp32 geometry of the camera case."""
    t, r = FC.inputs(case), renderer(case)
    pts, rays_d, viewdirs, z = FC.geometry(case, t, FC.F32)
    check(case, "forward", explicit_maps(case, r, pts, rays_d, viewdirs, z))
    sd = t["sd"]
    pts_n = FC.O.normalize_points(pts, t["near"], t["far"])
    rgb, raw, feat = FC.point_network(sd, pts_n, viewdirs, t["film"], case.depth)
    n = case.B * case.R
    rgb_map, fmap, xyz, mask = hip.volume_integration(cu(rgb.reshape(n, case.N, 3)), cu(raw.reshape(n, case.N)),
                                                      cu(feat.reshape(n, case.N, case.hidden)), cu(z.reshape(n, case.N)),
                                                      cu(rays_d.reshape(n, 3)), cu(pts.reshape(n, case.N, 3)), None, raw_density=True)
    v = lambda x: x.view(case.B, case.R, -1)
    check(case, "volume_integration", {"features": v(fmap).transpose(1, 2), "thumb": v(rgb_map).transpose(1, 2), "mask": v(mask)[..., 0],
                                       "depth": v(mask)[..., 1], "xyz": v(xyz).transpose(1, 2), "sdf": raw[..., 0]})
