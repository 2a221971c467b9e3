"""Cases, fp64 reference and error bounds of the NeRF backward (csrc/nerf_bwd_fused.hip, csrc/nerf_bwd.hip): d loss / d(FiLM
table) and d loss / d(cam_poses).  Shared by test_nerf_bwd_cases_host.py (CPU: the reference is the oracle's render, its gradients
are those of finite differences, the bound rejects every mutant) and test_gpu_nerf_bwd_chunks.py (the kernels).  Imports no GPU
code.

The reference is a plain torch expression of the render, generic in its dtype, built from the oracle's pieces (oracle/path.py:
camera_params, rays_in_world, z_vals, ray_points, normalize_points, volume_integration).  It differs from siren_points in one
point: the FiLM table film[B, D+1, 2, H] is a LEAF, h = sin(film[:, l, 0] * affine(h) + film[:, l, 1]) -- the kernels' own input
and the tensor whose gradient they return.  Evaluated in float64 it is the oracle; in float32 on the CPU it is "a correct fp32
implementation"; with a `mutant` it is a subtly wrong one.  Every input (weights, poses, table, upstream gradients) is an fp32
tensor, so the kernels and the reference see the same numbers.

Loss: scale * (sum(features tF) + 3 sum(thumb tT)  [+ sum(mask tM) + 10 sum(depth tD) + 10 sum(xyz tX) with `geo`]).

Error of a gradient: max-abs difference from fp64 over a SLICE, divided by the fp64 max-abs of the slice.  A slice of d film is
one (layer, gamma | beta) over batch and channels; d cam_poses is one slice.
Bound of a slice: K * max(e32, FLOOR), e32 = the CPU fp32 reference's own error on that slice; FLOOR = 1e-5 is the typical level
of e32, so that a lucky draw does not tighten a case.  K = 8: the split-fp16 products of the matrix cores keep 22 of fp32's 24
bits (4 x), another summation order and float atomics give 2 x.  K_CAP = 32 is the most any case may be given after analysis;
the host test proves that even at the cap every mutant is rejected.

Mutants (what a chunking error of the fused backward would do to d film; the point network is evaluated a second time with
film.detach() and spliced in with torch.where, so d cam_poses is not changed by any of them):
    last     the last live sample of the last non-empty chunk (sample N - 1) does not reach d film
    first1   the first sample of chunk 1 does not reach it            (cases with n_chunks >= 2)
    group    one 16-ray group of one sample of one view does not reach it
    twice    the last sample counts twice: a missing `live` gate behind the clamp sk = min(sg, N - 1)
"""
import functools
import math

import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, weights
from oracle import path as O

F32, F64 = torch.float32, torch.float64
K, K_CAP, FLOOR = 8.0, 32.0, 1e-5
LOCS = [[0.25, 0.1], [-0.4, -0.05], [0.1, 0.2], [0.0, 0.0]]
WAVES, RAYS = 8, 16                  # waves of a workgroup, rays of a wave task (csrc/nerf_mlp.h)


class Case:
    def __init__(self, hidden, depth, B, S, N, n_chunks=None, static=False, perturb=True, scale=1.0, geo=False, seed=3):
        self.hidden, self.depth, self.B, self.S, self.N, self.n_chunks = hidden, depth, B, S, N, n_chunks
        self.static, self.perturb, self.scale, self.geo, self.seed = static, perturb, scale, geo, seed

    @property
    def id(self):
        s = f"h{self.hidden}-d{self.depth}-b{self.B}-s{self.S}-n{self.N}"
        return s + (f"-c{self.n_chunks}" if self.n_chunks else "") + ("-geo" if self.geo else "")

    @property
    def chunk(self):
        return math.ceil(self.N / self.n_chunks)

    def cfg(self):
        return configs.tiny_G_cfg(self.hidden, self.depth, 1) if self.hidden < 256 else configs.ffhq_G_cfg(256, self.depth)

    def mutants(self):
        return ("last", "group", "twice") + (("first1",) if self.n_chunks and self.n_chunks >= 2 else ())


# (hidden, depth, B, S, N, n_chunks): the smallest shapes that reach each regime of the fused backward's sample loop
CHUNK_CASES = [
    Case(32, 2, 2, 8, 7, 1),                          # whole ray per wave; 4 tasks padded to 8: half of every workgroup is dead
    Case(32, 2, 2, 8, 7, 2),                          # chunk 4, one dead sample
    Case(64, 3, 3, 12, 7, 3),                         # chunk 3, two dead samples; 27 tasks padded to 32
    Case(64, 2, 1, 8, 7, 5),                          # chunk 2, the fifth chunk wholly beyond N
    Case(128, 2, 1, 16, 10, 4, static=True, scale=1e3),   # chunk 3, the last chunk has one live sample
    Case(256, 2, 2, 16, 9, 2, scale=1e-5),            # launch_fused<16,4>, chunk 5
    Case(256, 8, 1, 8, 5, 2),                         # depth >= 8: launch_fused<16,2> (the two-tile slab), chunk 3
    Case(32, 1, 1, 8, 5, 2, perturb=False),           # no hidden MFMA layer, chunk 3
    Case(64, 2, 2, 8, 7, 3, geo=True),                # with the d_mask, d_xyz upstreams
]
# (hidden, depth, B, S, N): dispatch edges of the materialised sequence (csrc/nerf_bwd.hip)
MATERIALISED_CASES = [
    Case(32, 2, 1, 6, 2),        # R = 36: no multiple of 16, 32 or 64; N = 2 is the smallest composite_par_kernel launch
    Case(32, 2, 1, 6, 32),       # 1024 threads, 28 KB of LDS: the largest one-sample-per-thread launch
    Case(32, 2, 1, 6, 33),       # the per-ray composite_kernel; three samples per camera-chain slice: slices 11..15 empty
    Case(32, 2, 2, 10, 17),      # R = 100; two samples per camera-chain slice: slices 9..15 empty
]
ALL_CASES = CHUNK_CASES + MATERIALISED_CASES


def stash_floats(case):
    """cips3d_nerf_bwd_fused_stash_floats: the tasks of a view padded to whole workgroups, a full chunk of rows for each"""
    groups = math.ceil(case.S * case.S / RAYS)
    tasks = math.ceil(groups * case.n_chunks / WAVES) * WAVES
    return case.B * tasks * case.chunk * case.depth * 16 * case.hidden


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _renderer_weights(hidden, depth, seed):
    G = pkg.build_generator(Case(hidden, depth, 1, 8, 1).cfg(), "cpu", seed=seed)
    return {k: v.detach().clone() for k, v in G.state_dict().items() if k.startswith("renderer.")}


def film_of_styles(sd, styles, D):
    """the FiLM table of the oracle's film_siren (gamma: 15 x + 30, beta: 0.25 x) -> [B, D+1, 2, H]"""
    net = "renderer.network"
    rows = []
    for l in range(D + 1):
        p = f"{net}.pts_linears.{l}" if l < D else f"{net}.views_linears"
        rows.append(torch.stack([15.0 * O._affine(sd, p + ".gamma", styles[:, l]) + 30.0,
                                 0.25 * O._affine(sd, p + ".beta", styles[:, l])], 1))
    return torch.stack(rows, 1)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """everything a run of the case reads, fp32 on the CPU; never modified"""
    B, S, N, D, H = case.B, case.S, case.N, case.depth, case.hidden
    sd = _renderer_weights(H, D, case.seed)
    cam, focal, near, far = O.camera_params(torch.tensor(LOCS[:B]), S, 6, 0.12)[:4]
    rnd = lambda tag, shape: weights.det_normal(f"nbc.{tag}.{case.id}", shape, 1.0, case.seed)
    styles = 0.5 * rnd("styles", (B, D + 1, sd["renderer.network.pts_linears.0.gamma.weight"].shape[1]))
    t = {"sd": sd, "cam": cam, "focal": focal, "near": near, "far": far, "styles": styles,
         "film": film_of_styles(sd, styles, D),
         "u": weights.det_unit_uniform(f"nbc.u.{case.id}", (B, S, S, 1), case.seed) if case.perturb else None,
         "tF": rnd("tF", (B, H, S, S)), "tT": rnd("tT", (B, 3, S, S))}
    if case.geo:
        t.update(tM=rnd("tM", (B, S, S)), tD=rnd("tD", (B, S, S)), tX=rnd("tX", (B, 3, S, S)))
    return t


def upstreams(case, t):
    """the upstream gradients of the loss, as the kernels take them: d_features, d_thumb, (d_mask [2,B,S,S], d_xyz) or None"""
    s = case.scale
    geo = (s * torch.stack([t["tM"], 10.0 * t["tD"]]), s * 10.0 * t["tX"]) if case.geo else (None, None)
    return s * t["tF"], s * 3.0 * t["tT"], geo[0], geo[1]


# ------------------------------------------------------------------------------------------------------------------ render
def point_network(sd, pts_n, viewdirs, film, D):
    """siren_points with the FiLM table as its input: pts_n (B,R,N,3), viewdirs (B,R,3), film (B,D+1,2,H)"""
    net = "renderer.network"
    gb = lambda l, k: film[:, l, k][:, None, None, :]
    h = pts_n
    for l in range(D):
        h = torch.sin(gb(l, 0) * O._affine(sd, f"{net}.pts_linears.{l}", h) + gb(l, 1))
    sdf = O._affine(sd, net + ".sigma_linear", h)
    dirs = viewdirs.unsqueeze(-2).expand(*h.shape[:-1], 3)
    feat = torch.sin(gb(D, 0) * O._affine(sd, net + ".views_linears", torch.cat([h, dirs], -1)) + gb(D, 1))
    return O._affine(sd, net + ".rgb_linear", feat), sdf, feat


def mutant_mask(case, mutant):
    """[B, R, N] bool: the points whose path to d film the mutant changes"""
    m = torch.zeros(case.B, case.S * case.S, case.N, dtype=torch.bool)
    if mutant in ("last", "twice"):
        m[:, :, case.N - 1] = True
    elif mutant == "first1":
        m[:, :, case.chunk] = True
    elif mutant == "group":
        m[case.B - 1, RAYS:2 * RAYS, min(1, case.N - 1)] = True
    else:
        raise ValueError(mutant)
    return m


def render(case, t, dtype, film, cam, mutant=None):
    """-> dict(features [B,H,S,S], thumb [B,3,S,S], mask [B,S,S], depth [B,S,S], xyz [B,3,S,S]) in `dtype`"""
    B, S, N, D = case.B, case.S, case.N, case.depth
    R = S * S
    c = lambda v: None if v is None else v.to(dtype)
    sd = {k: v.to(dtype) for k, v in t["sd"].items()}
    near, far = c(t["near"]), c(t["far"])
    rays_o, rays_d, viewdirs = O.rays_in_world(c(t["focal"]), S, cam, case.static)
    z = O.z_vals(near, far, B, S, S, N, c(t["u"]))
    pts = O.ray_points(rays_o, rays_d, z).reshape(B, R, N, 3)
    rays_d, viewdirs, z = rays_d.reshape(B, R, 3), viewdirs.reshape(B, R, 3), z.reshape(B, R, N)
    pts_n = O.normalize_points(pts, near, far)
    out = point_network(sd, pts_n, viewdirs, film, D)
    if mutant is not None:
        cut = point_network(sd, pts_n, viewdirs, film.detach(), D)      # same values, no path to the table
        m = mutant_mask(case, mutant).unsqueeze(-1)
        if mutant == "twice":                                            # 2 live - cut: the table's share twice, the points' once
            out = tuple(torch.where(m, 2.0 * a - b, a) for a, b in zip(out, cut))
        else:
            out = tuple(torch.where(m, b, a) for a, b in zip(out, cut))
    rgb, sdf, feat = out
    rgb_map, feature_map, xyz, mask = O.volume_integration(rgb, sdf, feat, z, rays_d, pts, sd["renderer.sigmoid_beta"])
    to_img = lambda v: v.transpose(1, 2).reshape(B, v.shape[-1], S, S)
    return {"features": to_img(feature_map), "thumb": to_img(rgb_map), "mask": to_img(mask)[:, 0], "depth": to_img(mask)[:, 1],
            "xyz": to_img(xyz)}


def loss(case, t, maps):
    c = lambda v: v.to(maps["features"].dtype)
    v = (maps["features"] * c(t["tF"])).sum() + 3.0 * (maps["thumb"] * c(t["tT"])).sum()
    if case.geo:
        v = v + (maps["mask"] * c(t["tM"])).sum() + 10.0 * (maps["depth"] * c(t["tD"])).sum() + 10.0 * (maps["xyz"] * c(t["tX"])).sum()
    return case.scale * v


def loss_of(case, t, dtype, film, cam, mutant=None):
    return loss(case, t, render(case, t, dtype, film, cam, mutant))


def grads(case, dtype, mutant=None):
    """(d film [B,D+1,2,H], d cam_poses [B,3,4]) in `dtype`, by autograd"""
    t = inputs(case)
    film, cam = (t[k].to(dtype, copy=True).requires_grad_(True) for k in ("film", "cam"))
    df, dc = torch.autograd.grad(loss_of(case, t, dtype, film, cam, mutant), [film, cam])
    return df.detach(), dc.detach()


# ------------------------------------------------------------------------------------------------------------------ bound
def slice_names(case):
    return [f"film.{l}.{nm}" for l in range(case.depth + 1) for nm in ("gamma", "beta")] + ["cam"]


def slice_errors(case, got, ref):
    """{slice: max-abs difference / fp64 max-abs}; got = (d film, d cam) of any dtype / device, ref = the fp64 pair"""
    gf, gc = (g.detach().double().cpu() for g in got)
    rf, rc = ref
    err = {}
    for l in range(case.depth + 1):
        for k, nm in ((0, "gamma"), (1, "beta")):
            err[f"film.{l}.{nm}"] = float((gf[:, l, k] - rf[:, l, k]).abs().max() / rf[:, l, k].abs().max())
    err["cam"] = float((gc.reshape(rc.shape) - rc).abs().max() / rc.abs().max())
    return err


@functools.lru_cache(maxsize=None)
def reference(case):
    """(fp64 gradients, {slice: max(e32, FLOOR)}): computed once per case and kept unchanged"""
    ref = grads(case, F64)
    assert all(float(r.abs().max()) > 0 and bool(torch.isfinite(r).all()) for r in ref)
    e32 = slice_errors(case, grads(case, F32), ref)
    return ref, {k: max(v, FLOOR) for k, v in e32.items()}


def ratios(case, got):
    """{slice: err / max(e32, FLOOR)}: inside the bound where <= K"""
    ref, unit = reference(case)
    err = slice_errors(case, got, ref)
    return {k: (err[k] / unit[k] if math.isfinite(err[k]) else math.inf) for k in err}


def worst(case, got):
    """(largest ratio, its slice)"""
    r = ratios(case, got)
    k = max(r, key=r.get)
    return r[k], k
