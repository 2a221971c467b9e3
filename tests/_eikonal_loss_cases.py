"""Shared recipe of the eikonal-loss tests (test_eikonal_loss_host.py, test_gpu_eikonal_loss.py): the oracle -- the two loss
values, d L / d film and d L / d styles by double backward through the trunk in a chosen dtype -- and a torch restatement of the
arithmetic csrc/nerf_eikonal.hip performs (forward-mode pass, seeds, reverse sweep).  Inputs come from _sdf_grad_cases.

L = lam_e mean((|d sdf / d pts| - 1)^2) + lam_m mean(exp(-beta |sdf|)) over all B R N points.

VALUE_FLOOR.  The kernel-level tests bound each of the two loss VALUES by 4 x max(the fp32 oracle's relative error against fp64,
VALUE_FLOOR): a scalar's fp32 error is one draw, and on some cases the fp32 oracle happens to land within 1e-8 of fp64, so a bare
ratio would be fragile.  The floor is the worst relative error of the fp32 restatement (`restatement(..., torch.float32)`, on the
CPU) against the fp64 oracle over KERNEL_CASES + the camera case, both values:  python tests/_eikonal_loss_cases.py  prints the
table it was taken from.  Worst entry: the eikonal value of the one-point case at D = 6, 8.22e-06 (its fp32 oracle: 1.02e-05); the
other entries lie between 1.5e-09 and 7.0e-06.
"""
import os
import sys

import torch

if __name__ == "__main__":          # run as a script from anywhere: the repository root holds the package and the oracle
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cips_3dplusplus_amd import weights
from oracle import path as O

import _sdf_grad_cases as SG

H = SG.H
BETA = 100.0
# (D, B, R, N) of the explicit-form kernel cases
KERNEL_CASES = [(D, B, R, N) for D in (2, 6, 8) for (B, R, N) in ((2, 37, 5), (1, 1, 1), (3, 16, 24), (1, 4099, 3))] + [(16, 1, 37, 5)]
CAMERA_CASE = dict(D=6, B=2, S=8, N=5)
VALUE_FLOOR = 8.3e-6     # 8.218e-06, the worst fp32-restatement relative error over the case list, rounded up


def case_inputs(D, B, R, N):
    return SG.explicit_inputs(B, R, N, D, tag=f"eik{R}")


def camera_case_inputs(dt=torch.float64):
    c = CAMERA_CASE
    locs = torch.tensor([[0.3, 0.1], [-0.2, 0.05]])[:c["B"]]
    cam = O.camera_params(locs, c["S"], 6, 0.12)
    u = weights.det_unit_uniform("eikcam.u", (c["B"], c["S"] * c["S"]), c["S"])
    styles = weights.det_normal("eikcam.styles", (c["B"], c["D"] + 1, H), 0.5, c["D"])
    return cam, u, styles, SG.camera_inputs(cam, c["S"], c["N"], u, False, dt, c["D"], styles)


def _cast(sd, inp, dt):
    sdd = {k: v.to(dt) if v.is_floating_point() else v for k, v in sd.items()}
    c = {k: v.detach().to(dt) for k, v in inp.items()}
    return sdd, c


def film_of(sdd, styles, D, prefix="renderer.network"):
    """gamma (15 x + 30) and beta (0.25 x) of the D point layers from the styles -> [B, D, 2, H] (cips3d/volume_renderer.py:66-67)."""
    rows = []
    for l in range(D):
        p = f"{prefix}.pts_linears.{l}"
        rows.append(torch.stack([15.0 * O._affine(sdd, p + ".gamma", styles[:, l]) + 30.0,
                                 0.25 * O._affine(sdd, p + ".beta", styles[:, l])], 1))
    return torch.stack(rows, 1)


def trunk_sdf(sdd, film, pts, near, far, D, prefix="renderer.network"):
    """sdf (B, P, 1) of the points pts (B, P, 3): the trunk of oracle.path.siren_points with gamma / beta given (film [B, D, 2, H])."""
    h = O.normalize_points(pts, near, far)
    for l in range(D):
        pre = O._affine(sdd, f"{prefix}.pts_linears.{l}", h)
        h = torch.sin(film[:, l, 0].unsqueeze(1) * pre + film[:, l, 1].unsqueeze(1))
    return O._affine(sdd, prefix + ".sigma_linear", h)


def oracle(sd, inp, D, dt, lam_e=1.0, lam_m=1.0, beta=BETA):
    """dict(eik, ms: the unweighted means (python floats of dtype dt's arithmetic), dfilm [B, D+1, 2, H] (view row zero), dstyles
    [B, D+1, style_dim]) of L by double backward, everything in dtype dt."""
    sdd, c = _cast(sd, inp, dt)
    B = c["pts"].shape[0]
    with torch.enable_grad():
        styles = c["styles"].clone().requires_grad_(True)
        film = film_of(sdd, styles, D)
        pts = c["pts"].reshape(B, -1, 3).clone().requires_grad_(True)
        sdf = trunk_sdf(sdd, film, pts, c["near"], c["far"], D)
        g, = torch.autograd.grad(sdf, pts, torch.ones_like(sdf), create_graph=True)
        eik = ((g.norm(dim=-1) - 1) ** 2).mean()
        ms = torch.exp(-beta * sdf.abs()).mean()
        dfilm, dstyles = torch.autograd.grad(lam_e * eik + lam_m * ms, [film, styles], allow_unused=True)
    dfilm = torch.zeros_like(film) if dfilm is None else dfilm
    dstyles = torch.zeros_like(styles) if dstyles is None else dstyles
    full = torch.zeros(B, D + 1, 2, film.shape[-1], dtype=dt)
    full[:, :D] = dfilm
    return dict(eik=float(eik.detach()), ms=float(ms.detach()), dfilm=full, dstyles=dstyles.detach(), sdf=sdf.detach())


def restatement(sd, inp, D, dt, lam_e=1.0, lam_m=1.0, beta=BETA):
    """The kernel's arithmetic in torch ops of dtype dt, no autograd: forward-mode pass storing (a_l, A_l^j), the seeds, the reverse
    sweep.  -> dict(eik, ms, dfilm [B, D+1, 2, H])."""
    sdd, c = _cast(sd, inp, dt)
    pre = "renderer.network"
    with torch.no_grad():
        B = c["pts"].shape[0]
        film = film_of(sdd, c["styles"], D)
        pts = c["pts"].reshape(B, -1, 3)
        P = pts.shape[1]
        s = (2 / (c["far"] - c["near"])).reshape(B, 1, 1)
        Ws = [sdd[f"{pre}.pts_linears.{l}.weight"] for l in range(D)]
        bs = [sdd[f"{pre}.pts_linears.{l}.bias"] for l in range(D)]
        w_s, b_s = sdd[pre + ".sigma_linear.weight"][0], sdd[pre + ".sigma_linear.bias"]
        a_l, A_l, z_l = [], [], []
        x = T = None
        for l in range(D):
            gm, bt = film[:, l, 0].unsqueeze(1), film[:, l, 1].unsqueeze(1)
            if l == 0:
                a = (pts * s) @ Ws[0].t() + bs[0]                                        # [B, P, H]
                A = (s.unsqueeze(-1) * Ws[0].t().reshape(1, 1, 3, -1)).expand(B, P, 3, -1)   # [B, P, 3, H]
            else:
                a = x @ Ws[l].t() + bs[l]
                A = T @ Ws[l].t()
            z = gm * a + bt
            x = torch.sin(z)
            T = (torch.cos(z) * gm).unsqueeze(2) * A
            a_l.append(a); A_l.append(A); z_l.append(z)
        sdf = x @ w_s + b_s                                                                  # [B, P]
        g = T @ w_s                                                                          # [B, P, 3]
        M = B * P
        nrm = g.norm(dim=-1)
        em = torch.exp(-beta * sdf.abs())
        eik, ms = ((nrm - 1) ** 2).mean(), em.mean()
        coef = torch.where(nrm > 0, lam_e * 2 * (nrm - 1) / nrm.clamp_min(torch.finfo(dt).tiny), torch.zeros_like(nrm))
        gbar = coef.unsqueeze(-1) * g / M
        sbar = -lam_m * beta * torch.sign(sdf) * em / M
        xbar = sbar.unsqueeze(-1) * w_s                                                      # [B, P, H]
        Tbar = gbar.unsqueeze(-1) * w_s                                                      # [B, P, 3, H]
        dfilm = torch.zeros(B, D + 1, 2, film.shape[-1], dtype=dt)
        for l in range(D - 1, -1, -1):
            gm = film[:, l, 0].unsqueeze(1)
            sn, cs = torch.sin(z_l[l]), torch.cos(z_l[l])
            Q = (Tbar * A_l[l]).sum(2)
            zbar = xbar * cs - Q * sn * gm
            dfilm[:, l, 0] = (zbar * a_l[l] + Q * cs).sum(1)
            dfilm[:, l, 1] = zbar.sum(1)
            if l > 0:
                xbar = (zbar * gm) @ Ws[l]
                Tbar = (Tbar * (cs * gm).unsqueeze(2)) @ Ws[l]
    return dict(eik=float(eik), ms=float(ms), dfilm=dfilm)


def rel(x, ref):
    return abs(x - ref) / max(abs(ref), 1e-300)


if __name__ == "__main__":
    worst = 0.0
    todo = [(f"D={D} B={B} R={R} N={N}", D, case_inputs(D, B, R, N)) for D, B, R, N in KERNEL_CASES]
    # (the camera case's fp32 side generates its rays and points in fp32 too, as the kernel does)
    todo.append(("camera", CAMERA_CASE["D"], camera_case_inputs()[3]))
    for name, D, inp in todo:
        sd = SG.synth_renderer_sd(D)
        inp32 = camera_case_inputs(torch.float32)[3] if name == "camera" else inp
        o64 = oracle(sd, inp, D, torch.float64)
        o32 = oracle(sd, inp32, D, torch.float32)
        r32 = restatement(sd, inp32, D, torch.float32)
        r64 = restatement(sd, inp, D, torch.float64)
        e = [rel(r32[k], o64[k]) for k in ("eik", "ms")]
        eo = [rel(o32[k], o64[k]) for k in ("eik", "ms")]
        worst = max(worst, *e)
        n_max, n_rms = SG.err_stats(o32["dfilm"], o64["dfilm"])
        k_max, k_rms = SG.err_stats(r32["dfilm"], o64["dfilm"])
        x_max, _ = SG.err_stats(r64["dfilm"], o64["dfilm"])
        print(f"{name}: eik {o64['eik']:.6g} ms {o64['ms']:.6g} | restatement fp32 rel err eik {e[0]:.2e} ms {e[1]:.2e} | fp32 oracle "
              f"{eo[0]:.2e} {eo[1]:.2e} | dfilm ratios max {k_max / max(n_max, 1e-300):.2f} rms {k_rms / max(n_rms, 1e-300):.2f} | "
              f"fp64 restatement vs oracle {x_max:.1e} (largest {float(o64['dfilm'].abs().max()):.3g})")
    print(f"worst fp32 restatement relative error of a value: {worst:.3e}")
