"""The reference and the bound of tests/_nerf_fwd_cases.py, checked without a GPU on every case test_gpu_nerf_fwd.py runs: (a) the
film-leaf expression in fp64 IS the oracle's render -- camera and explicit form, raw density, the sigmoid_beta and sigma-bias
overrides; (b) every case is well conditioned: the fp32 reference's own error stays below 1e-4 of every map's range (a case that
broke this would be redesigned, never given a wider bound); (c) every mutant that applies to a case leaves the bound on at least
one map even at the largest factors a case may ever be given -- the test has teeth; (d) the host-callable planners put every case
on the route its row claims, and the LDS arithmetic behind the depth routes at hidden 256 is restated here, so that a change of
nerf_ring_floats / nerf_table_floats that moves a case off its regime fails here and not silently.

What this pin cannot see is stated in _nerf_fwd_cases.py: a subtle error in an early layer of a deep network under the calm table
(pinned by the shallow cases instead)."""
import ctypes

import pytest
import torch

import _nerf_fwd_cases as FC
from cips_3dplusplus_amd import _lib
from oracle import path as O

F32, F64 = torch.float32, torch.float64
IDS = [c.id for c in FC.CASES]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_film_leaf_render_is_the_oracle_render(case):
    t = FC.inputs(case)
    D = case.depth
    sd = {k: v.double() for k, v in t["sd"].items()}
    pts, rays_d, viewdirs, z = FC.geometry(case, t, F64)
    near, far, styles = t["near"].double(), t["far"].double(), t["styles"].double()
    # the table of the case is the oracle's FiLM expression in fp32 (hidden gammas halved where the case is calm)
    film32 = FC.NC.film_of_styles(t["sd"], t["styles"], D)
    if case.calm:
        film32[:, 1:D, 0] *= 0.5
    assert torch.equal(t["film"], film32)
    if case.calm:       # no styles give the calm table: the plain point network on the case's table, the ORACLE's integration
        film = t["film"].double()
        rgb_p, sdf_p, feat_p = FC.NC.point_network(sd, O.normalize_points(pts, near, far), viewdirs, film, D)
        rgb_map, feature_map, xyz, mask = O.volume_integration(rgb_p, sdf_p, feat_p, z, rays_d, pts, sd["renderer.sigmoid_beta"],
                                                               with_sdf=case.with_sdf)
    else:               # the oracle's entry point, from the styles; the leaf is then the fp64 table of the styles
        film = FC.NC.film_of_styles(sd, styles, D)
        rgb_map, feature_map, sdf_p, mask, xyz = O.renderer_forward(sd, "renderer", pts, rays_d, viewdirs, z, near, far, styles, D,
                                                                    with_sdf=case.with_sdf)
    want = {"features": feature_map.transpose(1, 2), "thumb": rgb_map.transpose(1, 2), "mask": mask[..., 0], "depth": mask[..., 1],
            "xyz": xyz.transpose(1, 2), "sdf": sdf_p[..., 0]}
    got = FC.render_maps(case, F64, film=film)
    for k in FC.MAPS:
        assert got[k].shape == want[k].shape and rel(got[k], want[k]) < 1e-12, k
    # the overrides are in the state_dict the GPU module loads
    if case.beta is not None:
        assert float(t["sd"]["renderer.sigmoid_beta"]) == torch.tensor(case.beta).item()
    if case.bias is not None:
        assert float(t["sd"]["renderer.network.sigma_linear.bias"]) == case.bias


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_cases_are_well_conditioned(case):
    ref, e32, floor = FC.reference(case)
    line = []
    for k in FC.MAPS:
        rng = float(ref[k].max() - ref[k].min()) if ref[k].numel() > 1 else float(ref[k].abs().max())
        rng = max(rng, float(ref[k].abs().max()))
        line.append(f"{k} max {e32[k][0]:.1e} rms {e32[k][1]:.1e} floor {floor[k]:.1e} range {rng:.2g}")
        assert e32[k][0] <= 1e-4 * rng, f"{case.id} {k}: e32_max {e32[k][0]:.2e} of a range {rng:.3g}"
    print(f"E32 {case.id}: " + "; ".join(line))
    # the fp32 reference itself is inside the bound by construction (ratios <= 1)
    assert not FC.violations(case, FC.render_maps(case, F32))


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_the_bound_rejects_every_mutant(case):
    for m in case.mutants():
        got = FC.render_maps(case, F32, m)
        bad = FC.violations(case, got, FC.K_CAP)
        print(f"MUTANT {case.id} {m}: max/rms ratios {FC.ratio_line(case, got)}")
        assert bad, f"{case.id}: the mutant `{m}` stays inside the bound at the caps {FC.K_CAP}"
    if not case.with_sdf and case.bias is not None and case.bias >= 0.0:
        # log(1 + exp(x)) is F.softplus to the last digit here: why random weights never showed the difference
        plain, naive = FC.render_maps(case, F32), FC.render_maps(case, F32, "softplus")
        ref, e32, floor = FC.reference(case)
        for k in FC.MAPS:
            assert FC.err_stats(naive[k], plain[k].double())[0] <= max(e32[k][0], floor[k]), k
        assert not FC.violations(case, naive)


def test_per_case_factors_carry_their_analysis():
    """A case may have factors of its own only for a map whose e32 is a lucky draw of ONE ill-conditioned ray: the sensitivity
    of that ray's value to the sdf (fp64 autograd) times the fp32 reference's RMS sdf error -- what a typical correct fp32
    implementation makes of it -- is beyond the plain bound.  Only `mask` entries exist; the sdf map keeps the plain factors."""
    assert set(FC.K_OF) <= set(FC.BY_ID)
    for cid, per_map in FC.K_OF.items():
        case = FC.BY_ID[cid]
        assert set(per_map) == {"mask"} and case.with_sdf
        assert all(FC.K[i] <= per_map["mask"][i] <= FC.K_CAP[i] for i in (0, 1))
        t = FC.inputs(case)
        ref, e32, _ = FC.reference(case)
        sd = {k: v.double() for k, v in t["sd"].items()}
        pts, rays_d, viewdirs, z = FC.geometry(case, t, F64)
        pts_n = O.normalize_points(pts, t["near"].double(), t["far"].double())
        rgb, sdf, feat = FC.point_network(sd, pts_n, viewdirs, t["film"].double(), case.depth)
        sdf = sdf.requires_grad_(True)
        mask = FC.integrate(rgb, sdf, feat, z, rays_d, pts, sd["renderer.sigmoid_beta"])[3][..., 0]
        d = (FC.render_maps(case, F32)["mask"].double() - ref["mask"]).abs()
        b, r = (int(i) for i in torch.unravel_index(d.argmax(), d.shape))
        g = torch.autograd.grad(mask[b, r], sdf)[0][b, r, :, 0]
        typical = float(g.square().sum().sqrt()) * e32["sdf"][1]
        print(f"K_OF {cid}: ray {(b, r)} holds {float(d[b, r] ** 2 / d.square().sum()):.2f} of e32^2(mask); |d mask / d sdf| = "
              f"{float(g.abs().max()):.1f}; typical error {typical:.2e} = {typical / e32['mask'][0]:.1f} x e32_max")
        assert float(d[b, r] ** 2 / d.square().sum()) > 0.9
        assert typical > FC.K[1] * e32["mask"][0] and typical / d.numel() ** 0.5 > FC.K[0] * e32["mask"][1]


def test_mutants_apply_where_the_table_says():
    by = lambda key: [c for c in FC.CASES if c.key == key]
    assert [c.dead_samples for c in by("a") + by("c")] == [1, 1]
    f, = by("f")
    assert f.chunk == 2 and f.dead_samples == 7 and f.N <= 5 * f.chunk      # chunks 5 .. 7 hold no live sample
    assert all("dead" in c.mutants() for c in by("a") + by("c") + by("e") + by("f") + by("s"))
    assert all(("softplus" in c.mutants()) == (c.bias == -20.0) for c in by("t"))
    assert {c.bias for c in by("t")} >= {-20.0, 0.0, 25.0, -8.0, -11.0, -14.0}
    assert by("b")[0].N == 1 and by("r")[0].R == 1 and all(c.explicit and c.R == 37 for c in by("q"))
    assert sorted(c.key for c in FC.STORE_CASES) == list("acefqq")


def _params(case):
    p = _lib.NerfParams()
    p.hidden, p.depth, p.n_chunks, p.B, p.img_size, p.n_samples = case.hidden, case.depth, case.n_chunks, case.B, case.S or 1, case.N
    p.n_rays = case.R if case.explicit else 0
    p.o_features = p.o_thumb = p.o_xyz = p.o_mask = 64        # non-null dummies: the planner launches nothing
    return p


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_planners_put_the_case_on_its_route(case):
    lib = _lib.load()
    assert bool(lib.cips3d_nerf_fuses_finish(ctypes.byref(_params(case)))) == case.fused
    assert FC.plan(case.hidden, case.depth, case.n_chunks) == (case.fused, case.tps)
    if not case.explicit:
        assert lib.cips3d_nerf_part_floats(case.B, case.S, case.hidden, case.n_chunks) == FC.part_floats(case)
    # regimes the rows claim
    groups = -(-case.R // FC.RAYS)
    if case.key == "c":
        assert FC.table_floats(32, 10) < 1024 <= FC.table_floats(32, 11) and groups * case.n_chunks == FC.WAVES
    if case.key in "ad":
        assert FC.table_floats(case.hidden, case.depth + 1) < 1024
    if case.key == "e":
        assert groups * case.n_chunks == 12 and case.R % 4 != 0
    if case.key == "a":
        assert case.R % 4 != 0 and case.R % FC.RAYS != 0
    if case.key == "d":
        assert case.R % 4 == 0 and case.R % FC.RAYS != 0


def test_depth_routes_at_hidden_256():
    """<= 9 fused (full at 9), 10 unfused four-tile (full), 11 .. 42 two-tile (full at 42), 43 refused"""
    full = FC.LDS_BYTES
    assert FC.lds_bytes(256, 9, 4, True) == full and FC.lds_bytes(256, 10, 4, False) == full and FC.lds_bytes(256, 42, 2, False) == full
    assert FC.lds_bytes(256, 10, 4, False) == 131072 + 10240 + 2048 * 11 and FC.lds_bytes(256, 9, 4, True) == 133120 + 10240 + 2048 * 10
    for D in range(1, 45):
        want = (True, 4) if D <= 9 else (False, 4) if D == 10 else (False, 2) if D <= 42 else (False, None)
        assert FC.plan(256, D, 2) == want, D
    lib = _lib.load()
    for D in (9, 10):
        p = _params(FC.Case("x", 256, D, 1, 4, 2, D == 9, S=4))
        assert bool(lib.cips3d_nerf_fuses_finish(ctypes.byref(p))) == (D == 9)
    # narrower widths: where the fused finish starts
    assert [min(D for D in range(1, 20) if FC.plan(H, D, 2)[0]) for H in (32, 64, 128)] == [10, 2, 1]
