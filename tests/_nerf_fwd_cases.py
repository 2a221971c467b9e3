"""Cases, fp64 reference and error bound of the NeRF forward (csrc/nerf.hip: nerf_render_kernel in every instantiation
cips3d_nerf_render can launch, the fused finish and both stand-alone finish kernels).  Shared by test_nerf_fwd_cases_host.py (CPU:
the reference is the oracle's render, the cases are well conditioned, the bound rejects every mutant, the planners put every case
where the table below says) and test_gpu_nerf_fwd.py (the kernels).  Imports no GPU code.

Inputs and reference are those of tests/_nerf_bwd_cases.py: the generator's own renderer weights, the oracle's pieces
(oracle/path.py), and the FiLM table film[B, D+1, 2, H] as a LEAF (VolumeFeatureRenderer.render / forward take it as `film=`), so
that the kernel and the reference read the same fp32 numbers.  Evaluated in float64 the expression is the oracle; in float32 on
the CPU it is "a correct fp32 implementation"; with a `mutant` it is a subtly wrong one.

Maps, per case, in ray order: features [B,H,R], thumb [B,3,R], mask [B,R], depth [B,R], xyz [B,3,R], sdf [B,R,N] (the sigma head's
output: a distance, or the raw density of a with_sdf=False renderer).

Error of a map: max-abs and RMS of (map - fp64) over the whole map.  e32: the same of the CPU fp32 reference.
Bound (the rule of test_gpu_sdf_grad.py): RMS <= 2 x max(e32_rms, floor), max <= 4 x max(e32_max, floor), floor = 2^-23 x the
map's fp64 max-abs -- one fp32 ulp of its largest value; e32 of `mask` is 4.5e-9 on rays that end in the background, less than
any fp32 implementation can promise.  K_OF may give one case its own factors with the analysis beside it, never above K_CAP =
(4, 8); the host test proves that every mutant is rejected even at the cap.

Calm table: the deep cases multiply film[:, 1:D, 0] (the hidden layers' gamma) by 0.5.  With the stock table the fp32
reference's own error on `features` grows about 1.35 x per layer (8e-6 at D = 2, 9e-5 at D = 11, 2.6e-4 at D = 16, 2.4e-2 at
D = 42) and a lost fp16 low half of one tile disappears in it; with the hidden gammas halved the network contracts, e32 stays at
1e-6 and the same mutant stands out by two orders of magnitude.

Mutants (applied to the fp32 reference):
    xlo        the activations entering the LAST HIDDEN layer are rounded to fp16 for the first 16 output units: a lost
               w_hi x_lo product of one o-tile (D = 1: there is no hidden MFMA layer, the view layer takes its place)
    xlo_view   the same at the view layer
    wlo        the weights of the view layer's first o-tile rounded to fp16 at the layer's power-of-two scale (max |2^s W| in
               [512, 1024)): a lost w_lo x_hi product
    dead       sample N - 1 enters every sum a second time with its own weight (cases with ceil(N / n_chunks) n_chunks > N).
               This is the VISIBLE form of a missing `live` gate behind sk = min(sg, N - 1).  The literal form -- the dead sample
               composited behind the last one -- cannot be seen by any bound: the last sample has delta = 1e10, its alpha is 1
               and the transmittance behind it is 1e-10 T.  What a missing gate would really break is the sdf store at sample
               index >= N, which test_gpu_nerf_fwd.py's store discipline and the sdf map catch.
    softplus   log(1 + exp(x)) in place of F.softplus (raw-density cases): 0 below x = -16.6, where the last sample
               (delta = 1e10) still carries the ray's remaining transmittance

What this pin cannot see: a SUBTLE error in an early layer of a deep, contracting network is damped by about 0.5 per layer under
the calm table.  Early layers are pinned by the shallow cases, where layer 1 is the last hidden layer.  A GROSS per-layer error
(wrong slab, wrong scale index, wrong table row) still arrives at the output far above the bound.
"""
import functools
import math

import torch
import torch.nn.functional as F

import _nerf_bwd_cases as NC
from cips_3dplusplus_amd import weights
from oracle import path as O

F32, F64 = torch.float32, torch.float64
K, K_CAP = (2.0, 4.0), (4.0, 8.0)            # (RMS, max) factors: the rule, and the most a case may be given
# case id -> {map: (k_rms, k_max) <= K_CAP}, each with its analysis (test_nerf_fwd_cases_host.py re-derives it from the reference)
K_OF = {
    # sigmoid_beta = 0.001, `mask` (the last sample's weight): 98 % of the squared e32 sits on ONE ray (view 0, ray 7), whose
    # sample 2 lies 5.5 beta in front of the surface (sdf = +0.0055): d mask / d sdf = 123 there and 0.1 at every other sample of
    # the ray.  The fp32 reference's sdf error at that one sample happens to be 2.2e-8 -- its error over the sdf map is 1.1e-7
    # RMS, 5.2e-7 max -- so e32(mask) = 2.7e-6 is a lucky draw: a correct fp32 implementation whose sdf error at the sample is
    # just the map's RMS lands at 123 x 1.1e-7 = 1.4e-5, 5 x e32, and the plain factors would refuse it.  The sdf map itself is
    # held to the plain factors in this case, and so is every other map; `mask` gets the cap, at which the host test still
    # rejects every mutant of the case.
    "s-h64-d2-b2-s5-n7-c3-beta0.001": {"mask": (4.0, 8.0)},
}
MAPS = ("features", "thumb", "mask", "depth", "xyz", "sdf")
WAVES, RAYS, LDS_BYTES = 8, 16, 160 * 1024    # csrc/nerf_mlp.h; the LDS of a gfx950 workgroup


class Case:
    """key: the row of the table in test_gpu_nerf_fwd.py's docstring.  S: S x S camera rays; R: explicit geometry (pts, rays_d,
    viewdirs, z from the caller).  fused / tps: the route the planners must choose (checked on the host)."""

    def __init__(self, key, hidden, depth, B, N, n_chunks, fused, S=None, R=None, tps=None, static=False, perturb=True, calm=False,
                 exact=False, with_sdf=True, beta=None, bias=None, seed=3):
        assert (S is None) != (R is None)
        self.key, self.hidden, self.depth, self.B, self.N, self.n_chunks = key, hidden, depth, B, N, n_chunks
        self.S, self.R_explicit, self.fused, self.tps = S, R, fused, tps or (4 if hidden == 256 else 2)
        self.static, self.perturb, self.calm, self.exact = static, perturb, calm, exact
        self.with_sdf, self.beta, self.bias, self.seed = with_sdf, beta, bias, seed

    @property
    def explicit(self):
        return self.R_explicit is not None

    @property
    def R(self):
        return self.R_explicit if self.explicit else self.S * self.S

    @property
    def id(self):
        s = f"{self.key}-h{self.hidden}-d{self.depth}-b{self.B}-" + (f"r{self.R}x" if self.explicit else f"s{self.S}")
        s += f"-n{self.N}-c{self.n_chunks}"
        for flag, tag in ((self.calm, "calm"), (self.exact, "f32"), (self.static, "static"), (not self.perturb, "nou")):
            s += f"-{tag}" if flag else ""
        s += f"-beta{self.beta:g}" if self.beta is not None else ""
        s += "-raw" if not self.with_sdf else ""
        return s + (f"-bias{self.bias:g}" if self.bias is not None else "")

    @property
    def chunk(self):
        return math.ceil(self.N / self.n_chunks)

    @property
    def dead_samples(self):
        return self.chunk * self.n_chunks - self.N

    def base(self):
        """the case of _nerf_bwd_cases whose weights, camera, styles and table this one starts from"""
        return NC.Case(self.hidden, self.depth, self.B, self.S or 7, self.N, self.n_chunks, static=self.static, perturb=self.perturb,
                       seed=self.seed)

    def mutants(self):
        m = ("xlo", "xlo_view", "wlo") + (("dead",) if self.dead_samples > 0 else ())
        return m + (("softplus",) if not self.with_sdf and self.bias is not None and self.bias <= -17.0 else ())


C = Case
CASES = [
    C("a", 32, 1, 2, 5, 2, False, S=5),                       # no hidden MFMA layer; table < 1024 floats; R = 25: scalar finish
    C("b", 32, 2, 1, 1, 1, False, S=4),                       # N = 1: the only sample is the last one
    C("c", 32, 10, 2, 7, 4, True, S=5),                       # first depth at which NT = 2 fuses; two groups per workgroup
    C("d", 64, 1, 1, 6, 2, False, S=6),                       # table still too small to fuse; R = 36: vector finish
    C("e", 64, 2, 3, 7, 3, False, S=7),                       # 3 does not divide 8: part route; R = 49; 12 tasks padded to 16
    C("f", 64, 3, 2, 9, 8, True, S=5),                        # the unrolled NC = 8 form; chunks 5 .. 7 wholly beyond N
    C("g", 64, 4, 1, 8, 1, True, S=4),                        # one chunk: one live wave of eight; odd hidden layer + a pair
    C("h", 128, 2, 1, 10, 4, True, S=6, static=True),         # NC = 4; second half of the second workgroup idle
    C("i", 128, 5, 2, 3, 2, True, S=4, perturb=False),
    C("j", 256, 2, 2, 9, 2, True, S=5),                       # four-tile slabs, four groups per workgroup
    C("k", 256, 3, 1, 5, 5, False, S=4),                      # odd depth at NT = 16: pairs only; part route
    C("l", 256, 9, 1, 4, 4, True, S=4, calm=True),            # fused finish, LDS exactly full
    C("m", 256, 10, 1, 4, 2, False, S=5, calm=True),          # fuse refused by LDS size; four-tile unfused exactly full
    C("n", 256, 11, 1, 4, 2, False, S=5, tps=2, calm=True),   # launch_render<16, 2>, first depth
    C("o", 256, 16, 1, 3, 1, False, S=4, tps=2, calm=True),   # the two-tile form with a larger table
    C("p", 256, 2, 1, 5, 2, True, S=5, exact=True),           # the F32 instantiation
    C("p", 256, 11, 1, 5, 2, False, S=5, tps=2, calm=True, exact=True),      # ... and its own two-tile fallback
    C("q", 32, 2, 2, 5, 2, False, R=37),                      # XG instantiation; R odd and ragged; scalar finish
    C("q", 256, 2, 2, 5, 2, True, R=37),
    C("r", 64, 2, 1, 3, 1, True, R=1),                        # one ray
]
CASES += [C("s", 64, 2, 2, 7, nc, nc == 4, S=5, beta=beta) for beta in (0.01, 0.001) for nc in (3, 4)]      # hard surface
CASES += [C("t", h, 2, 2, 7, nc, nc == 4, S=5, with_sdf=False, bias=bias)
          for h in (64, 256) for nc in (3, 4) for bias in (-20.0, 0.0, 25.0)]
CASES += [C("t", 64, 2, 2, 7, 4, True, S=5, with_sdf=False, bias=bias) for bias in (-8.0, -11.0, -14.0)]    # across the fix's switch
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
STORE_CASES = [c for c in CASES if c.key in "acefq"]


# ------------------------------------------------------------------------------------------------------------------ planners
def table_floats(H, L):
    """nerf_table_floats (csrc/nerf_mlp.h): the FiLM table and the small weight tables of a workgroup"""
    return L * 2 * H + 10 * H


def ring_floats(H, tps, fuse):
    """nerf_ring_floats: two weight slabs, or the partial exchange of the fused finish where that is larger"""
    xf = WAVES * RAYS * (H + 4)
    return xf if fuse and xf > 2 * 16 * H * tps else 2 * 16 * H * tps


def lds_bytes(H, D, tps, fuse):
    return 4 * (ring_floats(H, tps, fuse) + table_floats(H, D + 1))


def plan(H, D, n_chunks):
    """(fused, tps) as nerf_fuse_plan and cips3d_nerf_render's switch decide them; tps None: refused"""
    tps0 = 4 if H == 256 else 2
    fused = WAVES % n_chunks == 0 and table_floats(H, D + 1) >= WAVES * 8 * RAYS and lds_bytes(H, D, tps0, True) <= LDS_BYTES
    for tps in ((4, 2) if H == 256 else (2,)):
        if lds_bytes(H, D, tps, fused) <= LDS_BYTES:
            return fused, tps
    return fused, None


def part_floats(case):
    return case.n_chunks * case.B * (case.hidden + 8) * case.R


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(case):
    """everything a run of the case reads, fp32 on the CPU; never modified.  sd carries the overrides of the case."""
    t = dict(NC.inputs(case.base()))
    B, N, D = case.B, case.N, case.depth
    sd = dict(t["sd"])
    if case.beta is not None:
        sd["renderer.sigmoid_beta"] = torch.tensor([case.beta])
    if case.bias is not None:
        sd["renderer.network.sigma_linear.bias"] = torch.tensor([case.bias])
    t["sd"] = sd
    if case.calm:
        film = t["film"].clone()
        film[:, 1:D, 0] *= 0.5
        t["film"] = film
    if case.explicit:
        # rays of the 7 x 7 camera, the first R of them; depths of the caller's own: one jittered sample per stratum
        R = case.R
        rays_o, rays_d, viewdirs = (v.reshape(B, 49, 3)[:, :R].contiguous() for v in O.rays_in_world(t["focal"], 7, t["cam"]))
        jit = weights.det_unit_uniform(f"nfc.z.{case.id}", (B, R, N), case.seed)
        near, far = t["near"].view(B, 1, 1), t["far"].view(B, 1, 1)
        z = (near + (far - near) * (torch.arange(N).view(1, 1, N) + 0.9 * jit) / N).contiguous()
        t.update(rays_d=rays_d, viewdirs=viewdirs, z=z, pts=O.ray_points(rays_o, rays_d, z).contiguous(), u=None)
    return t


# ------------------------------------------------------------------------------------------------------------------ render
def _h16(x):
    return x.half().to(x.dtype)


def _first_tile(y, y_mut):
    return torch.cat([y_mut[..., :16], y[..., 16:]], -1)


def point_network(sd, pts_n, viewdirs, film, D, mutant=None):
    """NC.point_network with the MLP mutants: pts_n (B,R,N,3), viewdirs (B,R,3), film (B,D+1,2,H) -> rgb, sdf, feat"""
    net = "renderer.network"
    gb = lambda l, k: film[:, l, k][:, None, None, :]
    h = pts_n
    for l in range(D):
        p = f"{net}.pts_linears.{l}"
        y = O._affine(sd, p, h)
        if mutant == "xlo" and D >= 2 and l == D - 1:
            y = _first_tile(y, O._affine(sd, p, _h16(h)))
        h = torch.sin(gb(l, 0) * y + gb(l, 1))
    sdf = O._affine(sd, net + ".sigma_linear", h)
    H = h.shape[-1]
    dirs = viewdirs.unsqueeze(-2).expand(*h.shape[:-1], 3)
    Wv, bv = sd[net + ".views_linears.weight"], sd[net + ".views_linears.bias"]
    y = F.linear(torch.cat([h, dirs], -1), Wv, bv)
    if mutant == "xlo_view" or (mutant == "xlo" and D == 1):
        y = _first_tile(y, F.linear(torch.cat([_h16(h), dirs], -1), Wv, bv))
    elif mutant == "wlo":
        e = math.frexp(float(Wv[:, :H].abs().max()))[1]          # max = f 2^e, f in [0.5, 1): 2^(10 - e) max in [512, 1024)
        s = 2.0 ** (10 - e)
        Wm = Wv.clone()
        Wm[:16, :H] = _h16(Wv[:16, :H] * s) / s
        y = F.linear(torch.cat([h, dirs], -1), Wm, bv)
    feat = torch.sin(gb(D, 0) * y + gb(D, 1))
    return O._affine(sd, net + ".rgb_linear", feat), sdf, feat


def integrate(rgb, sdf, feat, z, rays_d, pts, beta, with_sdf=True, mutant=None):
    """O.volume_integration (the host test holds the two together) with the compositing mutants"""
    dnorm = rays_d.norm(dim=-1, keepdim=True)
    delta = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(dnorm, 1e10)], dim=-1) * dnorm
    if with_sdf:
        sigma = torch.sigmoid(-sdf / beta) / beta
    elif mutant == "softplus":
        sigma = torch.where(sdf > 20.0, sdf, torch.log(1.0 + torch.exp(sdf)))
    else:
        sigma = F.softplus(sdf)
    alpha = 1 - torch.exp(-sigma * delta.unsqueeze(-1))
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1, :]), 1.0 - alpha + 1e-10], dim=-2), dim=-2)[..., :-1, :]
    w = alpha * trans
    ws = torch.cat([w, w[..., -1:, :]], -2) if mutant == "dead" else w
    again = (lambda v: torch.cat([v, v[..., -1:, :]], -2)) if mutant == "dead" else (lambda v: v)
    rgb_map = -1 + 2 * (ws * torch.sigmoid(again(rgb))).sum(-2)
    feature_map = (ws * again(feat)).sum(-2)
    xyz = (ws * again(pts)).sum(-2)
    mask = torch.cat([w[..., -1, :], -xyz.norm(dim=-1, keepdim=True)], dim=-1)
    return rgb_map, feature_map, xyz, mask


def geometry(case, t, dtype):
    """pts (B,R,N,3), rays_d (B,R,3), viewdirs (B,R,3), z (B,R,N) in `dtype`"""
    B, N, R = case.B, case.N, case.R
    c = lambda v: None if v is None else v.to(dtype)
    if case.explicit:
        return c(t["pts"]), c(t["rays_d"]), c(t["viewdirs"]), c(t["z"])
    S = case.S
    rays_o, rays_d, viewdirs = O.rays_in_world(c(t["focal"]), S, c(t["cam"]), case.static)
    z = O.z_vals(c(t["near"]), c(t["far"]), B, S, S, N, c(t["u"]))
    pts = O.ray_points(rays_o, rays_d, z)
    return pts.reshape(B, R, N, 3), rays_d.reshape(B, R, 3), viewdirs.reshape(B, R, 3), z.reshape(B, R, N)


def render_maps(case, dtype, mutant=None, film=None):
    """-> {features [B,H,R], thumb [B,3,R], mask [B,R], depth [B,R], xyz [B,3,R], sdf [B,R,N]} in `dtype`; film: another table
    than the case's own (the host test hands in the fp64 table of the styles)"""
    t = inputs(case)
    sd = {k: v.to(dtype) for k, v in t["sd"].items()}
    pts, rays_d, viewdirs, z = geometry(case, t, dtype)
    pts_n = O.normalize_points(pts, t["near"].to(dtype), t["far"].to(dtype))
    rgb, sdf, feat = point_network(sd, pts_n, viewdirs, (t["film"] if film is None else film).to(dtype), case.depth, mutant)
    rgb_map, feature_map, xyz, mask = integrate(rgb, sdf, feat, z, rays_d, pts, sd["renderer.sigmoid_beta"], case.with_sdf, mutant)
    tr = lambda v: v.transpose(1, 2).contiguous()
    return {"features": tr(feature_map), "thumb": tr(rgb_map), "mask": mask[..., 0], "depth": mask[..., 1], "xyz": tr(xyz),
            "sdf": sdf[..., 0]}


# ------------------------------------------------------------------------------------------------------------------ bound
def err_stats(got, ref):
    """(max-abs, RMS) of got - ref over the whole map; inf for a non-finite map"""
    d = got.detach().double().cpu().reshape(ref.shape) - ref
    if not bool(torch.isfinite(d).all()):
        return math.inf, math.inf
    return float(d.abs().max()), float(d.square().mean().sqrt())


@functools.lru_cache(maxsize=None)
def reference(case):
    """(fp64 maps, {map: (e32_max, e32_rms)}, {map: floor}): computed once per case and kept unchanged"""
    ref = render_maps(case, F64)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    r32 = render_maps(case, F32)
    e32 = {k: err_stats(r32[k], ref[k]) for k in MAPS}
    floor = {k: 2.0 ** -23 * float(ref[k].abs().max()) for k in MAPS}
    return ref, e32, floor


def ratios(case, got):
    """{map: (max error / max(e32_max, floor), RMS error / max(e32_rms, floor))}; got: {map: tensor shaped like the reference's}"""
    ref, e32, floor = reference(case)
    out = {}
    for k in MAPS:
        g_max, g_rms = err_stats(got[k], ref[k])
        out[k] = (g_max / max(e32[k][0], floor[k]), g_rms / max(e32[k][1], floor[k]))
    return out


def factors(case, name):
    k_rms, k_max = K_OF.get(case.id, {}).get(name, K)
    assert K[0] <= k_rms <= K_CAP[0] and K[1] <= k_max <= K_CAP[1]
    return k_rms, k_max


def violations(case, got, k=None):
    """[(map, statistic, ratio, factor)] of everything outside the bound; k: the same factors for every map (the caps)"""
    bad = []
    for name, (r_max, r_rms) in ratios(case, got).items():
        k_rms, k_max = k or factors(case, name)
        if not r_max <= k_max:
            bad.append((name, "max", r_max, k_max))
        if not r_rms <= k_rms:
            bad.append((name, "rms", r_rms, k_rms))
    return bad


def ratio_line(case, got):
    r = ratios(case, got)
    return " ".join(f"{k}={r[k][0]:.2f}/{r[k][1]:.2f}" for k in MAPS)
