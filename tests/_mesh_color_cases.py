"""Shared recipe of the mesh-colour tests (test_mesh_color_host.py, test_gpu_mesh_color.py): a numpy restatement of the
contract of include/cips3d_hip.h (cips3d_mesh_vertex_colors) in a chosen precision, on top of _mesh_raster_cases' meshes, camera
and brute-force rasteriser.  fp64 is the yardstick; fp32 is the restatement whose own error against fp64 scales the kernel's
allowance (DESIGN 9.2's ratio rule: max <= 4 x, RMS <= 2 x).

A (view, vertex) pair is left out of the comparison when one of its decisions sits on a tie -- `tie` below; a vertex with any
such pair is left out of the colour comparison.  At most CAP of the pairs of a case may be left out."""
import functools

import numpy as np

import _mesh_raster_cases as MR

FRAME_SCALE = 0.24
DEFAULT_DEPTH_TOL = FRAME_SCALE / 128       # mesh.vertex_colors' default: one cell of a 128^3 volume
TIE_Z = 1e-6                                # |z - (z* + depth_tol)| below this: excluded
TIE_FACING = 1e-6                           # |n . d| below this: excluded
CAP = 0.03


def images(n, R, seed=0):
    """[n,3,R,R] fp32 in [-1, 1]: a smooth function of (view, channel, row, column) plus noise."""
    rng = np.random.RandomState(1000 * seed + 10 * n + R)
    y, x = np.meshgrid(np.linspace(0, 1, R), np.linspace(0, 1, R), indexing="ij")
    k = np.arange(n)[:, None, None, None]
    c = np.arange(3)[None, :, None, None]
    smooth = 0.6 * np.sin(3.1 * x[None, None] + 0.7 * k + 1.3 * c) * np.cos(2.3 * y[None, None] - 0.5 * c + 0.3 * k)
    img = np.clip(smooth + 0.35 * rng.uniform(-1, 1, (n, 3, R, R)), -1, 1).astype(np.float32)
    img.setflags(write=False)
    return img


def project(verts, azim, elev, S, fov_deg, dist, znear, dt):
    """The rasteriser's vertex pass (csrc/mesh_raster.hip, as _mesh_raster_cases.rasterize restates it) in dtype dt ->
    (x_p, y_p, z, kept by znear, eye C)."""
    V = np.asarray(verts).astype(dt)
    C, x_ax, y_ax, z_ax, s = MR.camera(azim, elev, fov_deg, dist, dt)
    d = V - C
    pv = np.stack([d @ x_ax, d @ y_ax, d @ z_ax], 1).astype(dt)
    half = dt(0.5) * dt(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = (dt(1) - s * pv[:, 0] / pv[:, 2]) * half - dt(0.5)
        sy = (dt(1) - s * pv[:, 1] / pv[:, 2]) * half - dt(0.5)
    vz = pv[:, 2]
    return sx, sy, vz, (vz >= dt(znear)) & (vz > 0), C


def bilinear(img, u, v, dt):
    """img [3,R,R] at (u, v) [M] with clamp to edge -> [M,3], in the kernel's order of operations."""
    R = img.shape[-1]
    u, v = np.clip(u, dt(0), dt(R - 1)), np.clip(v, dt(0), dt(R - 1))
    fx0, fy0 = np.floor(u), np.floor(v)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, R - 1), np.minimum(y0 + 1, R - 1)
    fx, fy = (u - fx0)[:, None], (v - fy0)[:, None]
    I = np.moveaxis(img.astype(dt), 0, -1)                   # [R,R,3]
    top = (dt(1) - fx) * I[y0, x0] + fx * I[y0, x1]
    bot = (dt(1) - fx) * I[y1, x0] + fx * I[y1, x1]
    return ((dt(1) - fy) * top + fy * bot).astype(dt)


def vertex_colors(verts, faces, normals, imgs, views, S, power=2, depth_tol=DEFAULT_DEPTH_TOL, fill=0.0, fov_deg=12.0, dist=1.0,
                  znear=0.01, dt=np.float64):
    """The contract in dtype dt -> dict: colors [V,3], weight [V], seen [V] int, and per (view, vertex) [n,V]: w, faces_view
    (visible and c > 0), tie (a decision of the pair sits on a tie: see the module docstring)."""
    V = np.asarray(verts).astype(dt)
    N = np.asarray(normals).astype(dt)
    n, nv, R = len(views), len(V), imgs.shape[-1]
    acc, wsum, seen = np.zeros((nv, 3), dt), np.zeros(nv, dt), np.zeros(nv, np.int64)
    w_all, faces_view, tie = np.zeros((n, nv), dt), np.zeros((n, nv), bool), np.zeros((n, nv), bool)
    tol = dt(depth_tol)
    for k, (az, el) in enumerate(views):
        ras = MR.rasterize(verts, faces, az, el, S, fov_deg=fov_deg, dist=dist, znear=znear, dt=dt)
        sx, sy, vz, kept, C = project(verts, az, el, S, fov_deg, dist, znear, dt)
        with np.errstate(invalid="ignore"):
            cj, ci = np.rint(sx), np.rint(sy)
            on = kept & (cj >= 0) & (cj <= S - 1) & (ci >= 0) & (ci <= S - 1)
        j, i = np.where(on, cj, 0).astype(np.int64), np.where(on, ci, 0).astype(np.int64)
        zstar = np.where(ras["hit"], ras["zbuf"], np.inf).astype(dt)[i, j]
        visible = on & (vz <= zstar + tol)
        d = C - V
        d = d / np.maximum(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), dt(1e-12))[:, None]
        c = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2]
        fv = visible & (c > 0)
        w = c.copy()
        for _ in range(1, power):
            w = w * c
        w = np.where(fv, w, 0).astype(dt)
        take = w > 0
        u = (sx[take] + dt(0.5)) * dt(R) / dt(S) - dt(0.5)
        v = (sy[take] + dt(0.5)) * dt(R) / dt(S) - dt(0.5)
        rgb = bilinear(imgs[k], u, v, dt)
        acc[take] = acc[take] + w[take, None] * rgb
        wsum[take] = wsum[take] + w[take]
        seen += fv
        w_all[k], faces_view[k] = w, fv
        # ties: the rounding to a pixel, the pixel's owner, the depth test, the facing test
        with np.errstate(invalid="ignore"):
            half = lambda t: np.abs(t - np.floor(t) - 0.5) < MR.EDGE_TOL          # noqa: E731
            near_frame = kept & (sx > -1) & (sx < S) & (sy > -1) & (sy < S)
            t = near_frame & (half(sx) | half(sy))
            t |= on & MR.excluded(ras)[i, j]
            t |= on & (np.abs(vz - (zstar + tol)) < TIE_Z)
            t |= on & (np.abs(c) < TIE_FACING)
            t |= np.abs(vz - dt(znear)) < TIE_Z
        tie[k] = t
    with np.errstate(divide="ignore", invalid="ignore"):
        colors = np.where(wsum[:, None] > 0, acc / wsum[:, None], dt(fill)).astype(dt)
    return dict(colors=colors, weight=wsum, seen=seen, w=w_all, faces_view=faces_view, tie=tie)


# name -> (mesh, views, S, R, power, depth_tol, znear): every case the GPU test compares with this yardstick.  The first two are
# the parity cases; the others the edge inputs (one view, a near plane that cuts the mesh, the ends of the power range, a
# one-texel image, a one-pixel frame)
CASES = {
    "coarse": ("coarse", MR.VIEWS, 64, 40, 2, DEFAULT_DEPTH_TOL, 0.01),
    "subpixel": ("subpixel", MR.VIEWS, 48, 64, 1, 5e-4, 0.01),
    "one_view": ("coarse", MR.VIEWS[1:], 64, 40, 2, DEFAULT_DEPTH_TOL, 0.01),
    "znear": ("coarse", MR.VIEWS, 64, 40, 2, DEFAULT_DEPTH_TOL, 0.95),
    "power1": ("coarse", MR.VIEWS, 64, 40, 1, DEFAULT_DEPTH_TOL, 0.01),
    "power8": ("coarse", MR.VIEWS, 64, 40, 8, DEFAULT_DEPTH_TOL, 0.01),
    "R1": ("coarse", MR.VIEWS, 64, 1, 2, DEFAULT_DEPTH_TOL, 0.01),
    "S1": ("coarse", MR.VIEWS, 1, 40, 2, DEFAULT_DEPTH_TOL, 0.01),
}


@functools.lru_cache(maxsize=None)
def case(name, dt_name):
    """vertex_colors() of CASES[name] with images(len(views), R); cached, shared by the tests: do not write."""
    kind, views, S, R, power, depth_tol, znear = CASES[name]
    v, f, n, _ = MR.two_spheres(kind)
    return vertex_colors(v, f, n, images(len(views), R), views, S, power=power, depth_tol=depth_tol, znear=znear,
                         dt=getattr(np, dt_name))


def albedo_u8(face, shade, attr):
    """cips3d_mesh_albedo_frame in fp64: face [n,S,S], shade [n,S,S], attr [n,3,S,S] -> (uint8 [n,3,S,S], near [n,3,S,S]: 255 x
    value lies within 2^-10 of a half-integer, where the rounding to a byte may go either way)."""
    val = 255 * np.clip(np.asarray(shade, np.float64)[:, None] * (np.asarray(attr, np.float64) + 1) / 2, 0, 1)
    hit = (np.asarray(face) >= 0)[:, None]
    u8 = np.where(hit, np.floor(val + 0.5), 255).astype(np.uint8)
    near = hit & (np.abs(val - np.floor(val) - 0.5) < 2.0 ** -10)
    return u8, near
