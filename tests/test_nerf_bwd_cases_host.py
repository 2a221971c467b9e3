"""The reference and the bound of tests/_nerf_bwd_cases.py, checked without a GPU on every case test_gpu_nerf_bwd_chunks.py runs:
(a) the film-leaf expression IS the oracle's render, and its d film chained through the gamma / beta heads is the oracle's own
d styles; (b) autograd agrees with central finite differences; (c) every mutant (a sample, a chunk's first sample or a ray group
that does not reach d film, a sample counted twice) leaves the bound on at least one slice, even at the largest factor a case may
ever be given -- the test has teeth; (d) the stash size the C ABI reports is the one the cases assume."""
import pytest
import torch

import _nerf_bwd_cases as NC
from cips_3dplusplus_amd import _lib
from oracle import path as O

F64 = torch.float64
IDS = [c.id for c in NC.ALL_CASES]


def rel(a, b):
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max())


@pytest.mark.parametrize("case", NC.ALL_CASES, ids=IDS)
def test_film_leaf_render_is_the_oracle_render(case):
    t = NC.inputs(case)
    B, S, N, D, R = case.B, case.S, case.N, case.depth, case.S * case.S
    sd = {k: v.double() for k, v in t["sd"].items()}
    cam, styles = t["cam"].double().requires_grad_(True), t["styles"].double().requires_grad_(True)
    near, far = t["near"].double(), t["far"].double()
    rays_o, rays_d, viewdirs = O.rays_in_world(t["focal"].double(), S, cam, case.static)
    z = O.z_vals(near, far, B, S, S, N, None if t["u"] is None else t["u"].double())
    pts = O.ray_points(rays_o, rays_d, z)
    thumb, feat, _, mask, xyz = O.renderer_forward(sd, "renderer", pts.reshape(B, R, N, 3), rays_d.reshape(B, R, 3),
                                                   viewdirs.reshape(B, R, 3), z.reshape(B, R, N), near, far, styles, D)
    to_img = lambda v: v.transpose(1, 2).reshape(B, v.shape[-1], S, S)
    want = {"features": to_img(feat), "thumb": to_img(thumb), "mask": to_img(mask)[:, 0], "depth": to_img(mask)[:, 1],
            "xyz": to_img(xyz)}
    ds_ref, dc_ref = torch.autograd.grad(NC.loss(case, t, want), [styles, cam])

    film = NC.film_of_styles(sd, t["styles"].double(), D).requires_grad_(True)
    cam2 = t["cam"].double().requires_grad_(True)
    got = NC.render(case, t, F64, film, cam2)
    for k in want:
        assert rel(got[k], want[k].detach()) < 1e-12, k
    dfilm, dcam = torch.autograd.grad(NC.loss(case, t, got), [film, cam2])
    styles2 = t["styles"].double().requires_grad_(True)
    ds, = torch.autograd.grad(NC.film_of_styles(sd, styles2, D), styles2, grad_outputs=dfilm)
    assert rel(ds, ds_ref) < 1e-12 and rel(dcam, dc_ref) < 1e-12
    # the table of the case is that expression in fp32
    assert torch.equal(t["film"], NC.film_of_styles(t["sd"], t["styles"], D))


@pytest.mark.parametrize("case", NC.ALL_CASES, ids=IDS)
def test_autograd_agrees_with_central_differences(case):
    """three table entries (the largest gradient of the first layer's gamma, the last hidden layer's beta and the view layer's
    gamma) and two pose entries (the largest of the rotation and of the translation column)"""
    t = NC.inputs(case)
    (df, dc), _ = NC.reference(case)
    D = case.depth
    film0, cam0 = t["film"].double(), t["cam"].double()
    f = lambda film, cam: float(NC.loss_of(case, t, F64, film, cam))

    def central(x0, idx, other_first):
        vals = []
        for h in (1e-5, 2e-5):                      # Richardson: the h^2 term of the sine's third derivative cancels
            xp, xm = x0.clone(), x0.clone()
            xp[idx] += h
            xm[idx] -= h
            vals.append(((f(xp, cam0) - f(xm, cam0)) if other_first else (f(film0, xp) - f(film0, xm))) / (2 * h))
        return (4 * vals[0] - vals[1]) / 3

    def argmax(x):
        return tuple(int(i) for i in torch.unravel_index(x.abs().argmax(), x.shape))

    for l, k in ((0, 0), (D - 1, 1), (D, 0)):
        b, c = argmax(df[:, l, k])
        g = float(df[b, l, k, c])
        assert abs(central(film0, (b, l, k, c), True) - g) < 1e-6 * abs(g), (l, k)
    for cols in (slice(0, 3), slice(3, 4)):
        b, i, j = argmax(dc[:, :, cols])
        j += cols.start
        g = float(dc[b, i, j])
        assert abs(central(cam0, (b, i, j), False) - g) < 1e-6 * abs(g), (i, j)


@pytest.mark.parametrize("case", NC.ALL_CASES, ids=IDS)
def test_the_bound_rejects_every_mutant(case):
    _, unit = NC.reference(case)
    print(f"{case.id}: e32 floor-clamped {min(unit.values()):.2e} .. {max(unit.values()):.2e}")
    assert max(unit.values()) < 1e-4                      # a well-conditioned case: fp32 autograd itself is fp32-accurate
    for m in case.mutants():
        got = NC.grads(case, F64, m)
        w, at = NC.worst(case, got)
        print(f"  mutant {m}: {w:.3g} x the unit at {at}")
        assert w > NC.K_CAP, f"{case.id}: the mutant `{m}` stays inside the bound at K = {NC.K_CAP}"
        assert NC.ratios(case, got)["cam"] < 1e-6             # the mutants change the table's gradient alone


def test_the_chunk_cases_reach_their_regimes():
    live_last = lambda c: c.N - (c.n_chunks - 1) * c.chunk           # live samples of the last chunk (<= 0: wholly beyond N)
    by = {c.id: c for c in NC.CHUNK_CASES}
    assert all(c.n_chunks < c.N for c in NC.CHUNK_CASES)              # never the one-sample-per-wave loop of the other tests
    assert live_last(by["h32-d2-b2-s8-n7-c2"]) == 3 and by["h32-d2-b2-s8-n7-c2"].chunk == 4
    assert live_last(by["h64-d3-b3-s12-n7-c3"]) == 1 and (144 // 16 * 3) % 8 != 0
    assert live_last(by["h64-d2-b1-s8-n7-c5"]) < 0
    assert live_last(by["h128-d2-b1-s16-n10-c4"]) == 1
    assert (64 // 16 * 1) % 8 != 0                                    # n_chunks = 1 at S = 8: padded tasks


@pytest.mark.parametrize("case", NC.CHUNK_CASES, ids=[c.id for c in NC.CHUNK_CASES])
def test_stash_size(case):
    lib = _lib.load()
    assert lib.cips3d_nerf_bwd_fused_stash_floats(case.B, case.S, case.N, case.hidden, case.depth, case.n_chunks) == NC.stash_floats(case)
