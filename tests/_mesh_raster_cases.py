"""Shared recipe of the mesh-rasteriser tests (test_mesh_raster_host.py, test_gpu_mesh_raster.py): the two-sphere meshes and a
brute-force rasteriser in numpy that loops every face over every pixel and evaluates the contract of include/cips3d_hip.h
(cips3d_mesh_rasterize / cips3d_mesh_resolve) in a chosen precision: fp64 is the yardstick, fp32 is the restatement whose own
error against fp64 scales the kernel's allowance (DESIGN 9.2's ratio rule: max <= 4 x, RMS <= 2 x)."""
import functools

import numpy as np

VIEWS = ((0.4, 0.1), (-0.77, 0.2))          # (azim, elev) radians; fov 12 degrees, dist 1
EDGE_TOL = 2.0 ** -13                       # px: 16 ulp of the largest pixel coordinate at S = 64
DEPTH_TOL = 1e-6                            # the two nearest covering depths closer than this: excluded
PHONG = dict(ka=0.1, kd=0.65, ks=0.2, shininess=64.0)


def uv_sphere(radius, centre, n_lat, n_lon):
    """n_lat latitude bands x n_lon longitude steps: two poles, n_lat - 1 rings, pole fans.  Outward winding."""
    v = [(0.0, radius, 0.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            v.append((radius * np.sin(th) * np.sin(ph), radius * np.cos(th), radius * np.sin(th) * np.cos(ph)))
    v.append((0.0, -radius, 0.0))
    south = len(v) - 1
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon      # noqa: E731
    f = []
    for j in range(n_lon):
        f.append((0, ring(1, j), ring(1, j + 1)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    for j in range(n_lon):
        f.append((south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    return np.asarray(v, np.float64) + np.asarray(centre, np.float64), np.asarray(f, np.int64)


@functools.lru_cache(maxsize=None)
def two_spheres(kind):
    """"coarse": 10x14 and 5x7 (V 158, F 308); "subpixel": 40x56 and 20x28 (V 2720, F 5432).  The small sphere partly occludes
    the large one.  Vertices are rounded to fp32 (what the kernel sees); unit vertex normals; one attribute set [V,3]."""
    a, b = {"coarse": ((10, 14), (5, 7)), "subpixel": ((40, 56), (20, 28))}[kind]
    v0, f0 = uv_sphere(0.08, (0.0, 0.0, 0.0), *a)
    v1, f1 = uv_sphere(0.03, (0.03, 0.01, 0.09), *b)
    n = np.concatenate([v0 / 0.08, (v1 - np.asarray((0.03, 0.01, 0.09))) / 0.03]).astype(np.float32)
    v = np.concatenate([v0, v1]).astype(np.float32)
    f = np.concatenate([f0, f1 + len(v0)])
    rng = np.random.RandomState(len(v))
    attr = rng.randn(len(v), 3).astype(np.float32)
    for arr in (v, f, n, attr):
        arr.setflags(write=False)
    return v, f, n, attr


def camera(azim, elev, fov_deg, dist, dt):
    """(C, x_ax, y_ax, z_ax, s) of the reference's create_cameras, evaluated in dtype dt."""
    az, el, fov, dist = (dt(x) for x in (azim, elev, fov_deg, dist))
    C = np.array([dist * (np.cos(el) * np.sin(az)), dist * np.sin(el), dist * (np.cos(el) * np.cos(az))], dt)
    z_ax = -C / np.sqrt((C * C).sum(dtype=dt))
    x_ax = np.cross(np.array([0, 1, 0], dt), z_ax).astype(dt)
    x_ax = x_ax / np.sqrt((x_ax * x_ax).sum(dtype=dt))
    y_ax = np.cross(z_ax, x_ax).astype(dt)
    s = dt(1) / np.tan(fov * dt(np.pi / 360))
    return C, x_ax, y_ax, z_ax, s


def rasterize(verts, faces, azim, elev, S, fov_deg=12.0, dist=1.0, znear=0.01, dt=np.float64, attrs=None, normals=None,
              light=None, phong=PHONG):
    """Brute force, every face over every pixel, in dtype dt -> dict of [S,S] maps: face (-1 empty), zbuf, bary [S,S,3] (-1
    empty), gap (second-nearest minus nearest covering depth; inf with one cover), edge (distance in px from the pixel centre to
    the nearest boundary of ANY face), and, when given, attr [C,S,S] (nan where empty) / shade [S,S] (1 where empty)."""
    V = np.asarray(verts).astype(dt)
    C, x_ax, y_ax, z_ax, s = camera(azim, elev, fov_deg, dist, dt)
    d = V - C
    pv = np.stack([d @ x_ax, d @ y_ax, d @ z_ax], 1).astype(dt)
    half = dt(0.5) * dt(S)
    sx = (dt(1) - s * pv[:, 0] / pv[:, 2]) * half - dt(0.5)
    sy = (dt(1) - s * pv[:, 1] / pv[:, 2]) * half - dt(0.5)
    vz = pv[:, 2]
    ok = (vz >= dt(znear)) & (vz > 0)
    py, px = np.meshgrid(np.arange(S, dtype=dt), np.arange(S, dtype=dt), indexing="ij")
    face = np.full((S, S), -1, np.int64)
    z1 = np.full((S, S), np.inf, dt)
    z2 = np.full((S, S), np.inf, dt)
    bary = np.full((S, S, 3), -1, dt)
    edge = np.full((S, S), np.inf, dt)
    for fi, (i0, i1, i2) in enumerate(np.asarray(faces)):
        if not (ok[i0] and ok[i1] and ok[i2]):
            continue
        ax, ay, bx, by, cx, cy = sx[i0], sy[i0], sx[i1], sy[i1], sx[i2], sy[i2]
        area = (bx - ax) * (cy - ay) - (cx - ax) * (by - ay)
        if not abs(area) > 0:
            continue
        for (ux, uy), (wx, wy) in (((ax, ay), (bx, by)), ((bx, by), (cx, cy)), ((cx, cy), (ax, ay))):
            ex, ey = wx - ux, wy - uy
            t = np.clip(((px - ux) * ex + (py - uy) * ey) / max(ex * ex + ey * ey, dt(1e-300) if dt is np.float64 else dt(1e-30)), 0, 1)
            edge = np.minimum(edge, np.hypot(px - (ux + t * ex), py - (uy + t * ey)))
        dax, day, dbx, dby, dcx, dcy = ax - px, ay - py, bx - px, by - py, cx - px, cy - py
        e0, e1, e2 = dbx * dcy - dcx * dby, dcx * day - dax * dcy, dax * dby - dbx * day
        inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) if area > 0 else ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        if not inside.any():
            continue
        b0, b1, b2 = e0 / area, e1 / area, e2 / area
        iz0, iz1, iz2 = dt(1) / vz[i0], dt(1) / vz[i1], dt(1) / vz[i2]
        with np.errstate(divide="ignore", invalid="ignore"):
            z = dt(1) / ((b0 * iz0 + b1 * iz1) + b2 * iz2)
            w = np.stack([(b0 * iz0) * z, (b1 * iz1) * z, (b2 * iz2) * z], -1)
        z = np.where(inside, z, np.inf).astype(dt)
        win = z < z1                                   # faces come in ascending order: equal depths stay with the lower index
        z2 = np.where(win, z1, np.minimum(z2, z))
        bary[win] = w[win]
        face[win] = fi
        z1 = np.where(win, z, z1)
    hit = face >= 0
    out = dict(face=face, zbuf=np.where(hit, z1, -1).astype(dt), bary=bary, gap=z2 - np.where(hit, z1, 0), edge=edge, hit=hit)
    F = np.asarray(faces)
    idx = F[np.where(hit, face, 0)]                    # [S,S,3]
    if attrs is not None:
        A = np.asarray(attrs).astype(dt)
        a = ((bary[..., 0:1] * A[idx[..., 0]] + bary[..., 1:2] * A[idx[..., 1]]) + bary[..., 2:3] * A[idx[..., 2]])
        out["attr"] = np.where(hit[None], np.moveaxis(a, -1, 0), np.nan)
    if normals is not None:
        N = np.asarray(normals).astype(dt)
        L = np.asarray(light).astype(dt)
        interp = lambda T: (bary[..., 0:1] * T[idx[..., 0]] + bary[..., 1:2] * T[idx[..., 1]]) + bary[..., 2:3] * T[idx[..., 2]]   # noqa: E731
        unit = lambda x: x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), dt(1e-12))                                      # noqa: E731
        n, p = unit(interp(N)), interp(V)
        l, v = unit(L - p), unit(C - p)
        c = (n * l).sum(-1)
        r = dt(2) * c[..., None] * n - l
        vr = np.maximum((v * r).sum(-1), 0)
        spec = np.where(c > 0, vr ** dt(phong["shininess"]), 0)
        sh = (dt(phong["ka"]) + dt(phong["kd"]) * np.maximum(c, 0)) + dt(phong["ks"]) * spec
        out["shade"] = np.where(hit, sh, 1).astype(dt)
    return out


@functools.lru_cache(maxsize=None)
def case(kind, view, S, dt_name, extras=False):
    """rasterize() of a two-sphere mesh from VIEWS[view] (or an (azim, elev) pair); cached, shared by the tests: do not write."""
    v, f, n, attr = two_spheres(kind)
    az, el = VIEWS[view] if isinstance(view, int) else view
    kw = {}
    if extras:
        kw = dict(attrs=attr, normals=n, light=light_of(az))
    return rasterize(v, f, az, el, S, dt=getattr(np, dt_name), **kw)


def light_of(azim):
    return np.array([5 * np.sin(azim), 0.0, 5 * np.cos(azim)])


def excluded(ref64):
    """Pixels left out of the face-id comparison: the centre within EDGE_TOL px of a face boundary, or the two nearest
    covering depths closer than DEPTH_TOL."""
    return (ref64["edge"] < EDGE_TOL) | (ref64["hit"] & (ref64["gap"] < DEPTH_TOL))


def err_stats(x, ref64, mask):
    """(max, rms) of x - ref64 over mask, in fp64."""
    d = (np.asarray(x, np.float64) - np.asarray(ref64, np.float64))[mask]
    if d.size == 0:
        return 0.0, 0.0
    return float(np.abs(d).max()), float(np.sqrt((d * d).mean()))


def check_ratio(name, got, ref32, ref64, mask):
    """The ratio rule: the kernel's error against fp64 is at most 4 x (max) / 2 x (RMS) the fp32 restatement's own."""
    n_max, n_rms = err_stats(ref32, ref64, mask)
    k_max, k_rms = err_stats(got, ref64, mask)
    print(f"{name}: kernel max {k_max:.3e} rms {k_rms:.3e} | fp32 restatement max {n_max:.3e} rms {n_rms:.3e} | ratios max "
          f"{k_max / max(n_max, 1e-300):.2f} rms {k_rms / max(n_rms, 1e-300):.2f}")
    assert k_rms <= 2 * n_rms, f"{name}: RMS error {k_rms:.3e} > 2 x {n_rms:.3e}"
    assert k_max <= 4 * n_max, f"{name}: max error {k_max:.3e} > 4 x {n_max:.3e}"
    return k_max / max(n_max, 1e-300), k_rms / max(n_rms, 1e-300)


def subdivide_np(verts, faces):
    """numpy restatement of mesh.subdivide's contract."""
    V = len(verts)
    edges = sorted({(min(a, b), max(a, b)) for tri in faces for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))})
    mid = {e: V + k for k, e in enumerate(edges)}
    nv = np.concatenate([verts, np.array([(verts[a] + verts[b]) * 0.5 for a, b in edges]).reshape(-1, 3)])
    m = lambda a, b: mid[(min(a, b), max(a, b))]      # noqa: E731
    nf = []
    for a, b, c in faces:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return nv, np.asarray(nf, np.int64)
