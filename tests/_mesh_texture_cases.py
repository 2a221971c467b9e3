"""Shared recipe of the mesh-texture tests (test_mesh_texture_host.py, test_gpu_mesh_texture.py): numpy restatements of the
contracts of include/cips3d_hip.h (the atlas layout, cips3d_mesh_fill_colors, cips3d_mesh_texture_bake,
cips3d_mesh_textured_frame) on top of _mesh_raster_cases' meshes and brute-force rasteriser and _mesh_color_cases' images,
projection and bilinear sample.  fp64 is the yardstick; fp32 is the restatement whose own error against fp64 scales the kernel's
allowance (the ratio rule: max <= 4 x, RMS <= 2 x).

A (view, texel) pair is left out of the comparison when one of its decisions sits on a tie -- _mesh_color_cases' conditions,
applied to the texel's surface point; a texel with any such pair is left out of the colour comparison.  At most MC.CAP of the
pairs of a case may be left out."""
import functools
import math

import numpy as np

import _mesh_color_cases as MC
import _mesh_raster_cases as MR


# ------------------------------------------------------------------------------------------------ atlas layout
def layout(F, T, cols=None):
    """(cols, rows, Wt, Ht) of the atlas of F faces."""
    cells = (F + 1) // 2
    if cols is None:
        cols = max(1, math.ceil(math.sqrt(cells * T / (T + 1))))
    rows = -(-cells // cols)
    return cols, rows, cols * (T + 1), rows * T


def classify(F, T, cols, rows):
    """Per texel [Ht,Wt]: face (-1: unowned), gutter, and the lattice point (li, lj) in fp64 (exact: halves)."""
    m = T - 2
    y, x = np.meshgrid(np.arange(rows * T), np.arange(cols * (T + 1)), indexing="ij")
    cx, i = x // (T + 1), x % (T + 1)
    cy, j = y // T, y % T
    c = cy * cols + cx
    d = i + j
    lower = d <= m + 1
    gutter = (d == m + 1) | (d == m + 2)
    face = np.where(lower, 2 * c, 2 * c + 1)
    li = np.where(lower, i, T - i) - 0.5 * gutter
    lj = np.where(lower, j, T - 1 - j) - 0.5 * gutter
    owned = face < F
    return np.where(owned, face, -1), gutter & owned, li.astype(np.float64), lj.astype(np.float64)


def bary(li, lj, T, dt):
    m = dt(T - 2)
    b1 = np.clip(li.astype(dt) / m, dt(0), dt(1))
    b2 = np.clip(lj.astype(dt) / m, dt(0), dt(1))
    b0 = np.maximum(dt(0), (dt(1) - b1) - b2)
    return b0, b1, b2


def corner_uv(F, T, cols):
    """[F,3,2] fp64: the faces' corner UVs in continuous texel coordinates."""
    f = np.arange(F)
    c = f // 2
    ox, oy = (c % cols) * (T + 1), (c // cols) * T
    m = T - 2
    lo = np.stack([np.stack([ox + 0.5, oy + 0.5], -1), np.stack([ox + 0.5 + m, oy + 0.5], -1), np.stack([ox + 0.5, oy + 0.5 + m], -1)], 1)
    hi = np.stack([np.stack([ox + T + 0.5, oy + T - 0.5], -1), np.stack([ox + T + 0.5 - m, oy + T - 0.5], -1),
                   np.stack([ox + T + 0.5, oy + T - 0.5 - m], -1)], 1)
    return np.where((f % 2 == 0)[:, None, None], lo, hi).astype(np.float64)


def bilinear_footprint(x, y, Wt, Ht):
    """The texels a bilinear fetch at the continuous texel position (x, y) reads with non-zero weight (taps clamped to the
    atlas): a list of (column, row)."""
    u, v = x - 0.5, y - 0.5
    x0, y0 = math.floor(u), math.floor(v)
    fx, fy = u - x0, v - y0
    taps = []
    for yy, wy in ((y0, 1 - fy), (y0 + 1, fy)):
        for xx, wx in ((x0, 1 - fx), (x0 + 1, fx)):
            if wx * wy != 0:
                taps.append((min(max(xx, 0), Wt - 1), min(max(yy, 0), Ht - 1)))
    return taps


# ------------------------------------------------------------------------------------------------ fill
def fill(colors, weight, faces, iters):
    """cips3d_mesh_fill_colors, exactly: (colors [V,3] fp32, filled [V] int32)."""
    col = np.array(colors, np.float32)
    filled = np.where(np.asarray(weight) > 0, 0, -1).astype(np.int32)
    F = np.asarray(faces, np.int64)
    for r in range(1, iters + 1):
        S = np.zeros((len(col), 3), np.int64)
        n = np.zeros(len(col), np.int64)
        q = np.rint(col * np.float32(1048576.0)).astype(np.int64)
        for a in range(3):
            for b in ((a + 1) % 3, (a + 2) % 3):
                take = (filled[F[:, a]] < 0) & (filled[F[:, b]] >= 0)
                np.add.at(S, F[take, a], q[F[take, b]])
                np.add.at(n, F[take, a], 1)
        hit = n > 0
        if not hit.any():
            break
        col[hit] = (S[hit].astype(np.float64) / (n[hit].astype(np.float64) * 1048576.0)[:, None]).astype(np.float32)
        filled[hit] = r
    return col, filled


def strip(n):
    """A triangle strip of n + 1 columns of two vertices: vertex 2k at (k, 0), 2k + 1 at (k, 1); faces (2k, 2k+2, 2k+1) and
    (2k+1, 2k+2, 2k+3)."""
    v = np.array([(k, y, 0.0) for k in range(n + 1) for y in (0.0, 1.0)], np.float32)
    f = np.array([t for k in range(n) for t in ((2 * k, 2 * k + 2, 2 * k + 1), (2 * k + 1, 2 * k + 2, 2 * k + 3))], np.int64)
    return v, f


def graph_distance(n_verts, faces, sources):
    """Edge distance of every vertex to the nearest source (-1: unreachable)."""
    adj = [set() for _ in range(n_verts)]
    for a, b, c in np.asarray(faces):
        adj[a] |= {b, c}; adj[b] |= {a, c}; adj[c] |= {a, b}
    dist = np.full(n_verts, -1, np.int64)
    front = [int(s) for s in sources]
    dist[front] = 0
    while front:
        nxt = []
        for a in front:
            for b in adj[a]:
                if dist[b] < 0:
                    dist[b] = dist[a] + 1
                    nxt.append(b)
        front = nxt
    return dist


# ------------------------------------------------------------------------------------------------ bake
@functools.lru_cache(maxsize=None)
def raster(kind, face0, n_faces, view, S, znear, dt_name):
    """The brute-force rasterisation of the faces [face0, face0 + n_faces) (n_faces None: to the end) of a two-sphere mesh;
    cached, shared: do not write."""
    if face0 == 0 and n_faces is None and znear == 0.01 and view in MR.VIEWS:
        return MR.case(kind, MR.VIEWS.index(view), S, dt_name)
    v, f, _, _ = MR.two_spheres(kind)
    return MR.rasterize(v, f[face0:][:n_faces], view[0], view[1], S, znear=znear, dt=getattr(np, dt_name))


def bake(kind, views, S, R, T, cols=None, face0=0, n_faces=None, power=2, depth_tol=MC.DEFAULT_DEPTH_TOL, znear=0.01, fill_value=0.0,
         vertex_colors=None, filled=None, dt=np.float64):
    """cips3d_mesh_texture_bake in dtype dt -> dict: texture [3,Ht,Wt], weight [Ht,Wt], seen [Ht,Wt] int, owned [Ht,Wt], tie
    [n,Ht,Wt] (a decision of the (view, texel) pair sits on a tie), fallback [Ht,Wt] (an owned texel no view sees whose corners
    are all filled), layout (cols, rows, Wt, Ht)."""
    verts, faces, normals, _ = MR.two_spheres(kind)
    faces = faces[face0:][:n_faces]                   # (all vertices stay: the rasteriser projects them, nothing draws them)
    F = len(faces)
    cols, rows, Wt, Ht = layout(F, T, cols)
    face, _, li, lj = classify(F, T, cols, rows)
    owned = face >= 0
    fo = face[owned]
    b0, b1, b2 = (b[owned][:, None] for b in bary(li, lj, T, dt))
    V, N = verts.astype(dt), normals.astype(dt)
    i0, i1, i2 = faces[fo, 0], faces[fo, 1], faces[fo, 2]
    P = ((b0 * V[i0] + b1 * V[i1]) + b2 * V[i2]).astype(dt)
    Nn = ((b0 * N[i0] + b1 * N[i1]) + b2 * N[i2]).astype(dt)
    Nn = Nn / np.maximum(np.sqrt((Nn[:, 0] * Nn[:, 0] + Nn[:, 1] * Nn[:, 1]) + Nn[:, 2] * Nn[:, 2]), dt(1e-12))[:, None]
    imgs = MC.images(len(views), R)
    M = len(P)
    acc, wsum, seen = np.zeros((M, 3), dt), np.zeros(M, dt), np.zeros(M, np.int64)
    tie = np.zeros((len(views), M), bool)
    tol = dt(depth_tol)
    for k, view in enumerate(views):
        ras = raster(kind, face0, n_faces, tuple(view), S, znear, np.dtype(dt).name)
        sx, sy, vz, kept, C = MC.project(P, view[0], view[1], S, 12.0, 1.0, znear, dt)
        with np.errstate(invalid="ignore"):
            cj, ci = np.rint(sx), np.rint(sy)
            on = kept & (cj >= 0) & (cj <= S - 1) & (ci >= 0) & (ci <= S - 1)
        j, i = np.where(on, cj, 0).astype(np.int64), np.where(on, ci, 0).astype(np.int64)
        zstar = np.where(ras["hit"], ras["zbuf"], np.inf).astype(dt)[i, j]
        visible = on & (vz <= zstar + tol)
        d = C - P
        d = d / np.maximum(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), dt(1e-12))[:, None]
        c = (Nn[:, 0] * d[:, 0] + Nn[:, 1] * d[:, 1]) + Nn[:, 2] * d[:, 2]
        fv = visible & (c > 0)
        w = c.copy()
        for _ in range(1, power):
            w = w * c
        w = np.where(fv, w, 0).astype(dt)
        take = w > 0
        u = (sx[take] + dt(0.5)) * dt(R) / dt(S) - dt(0.5)
        v = (sy[take] + dt(0.5)) * dt(R) / dt(S) - dt(0.5)
        acc[take] = acc[take] + w[take, None] * MC.bilinear(imgs[k], u, v, dt)
        wsum[take] = wsum[take] + w[take]
        seen += fv
        with np.errstate(invalid="ignore"):
            half = lambda t: np.abs(t - np.floor(t) - 0.5) < MR.EDGE_TOL          # noqa: E731
            near_frame = kept & (sx > -1) & (sx < S) & (sy > -1) & (sy < S)
            t = near_frame & (half(sx) | half(sy))
            t |= on & MR.excluded(ras)[i, j]
            t |= on & (np.abs(vz - (zstar + tol)) < MC.TIE_Z)
            t |= on & (np.abs(c) < MC.TIE_FACING)
            t |= np.abs(vz - dt(znear)) < MC.TIE_Z
        tie[k] = t
    with np.errstate(divide="ignore", invalid="ignore"):
        colour = np.where(wsum[:, None] > 0, acc / wsum[:, None], dt(fill_value)).astype(dt)
    fb = np.zeros(M, bool)
    if vertex_colors is not None:
        Cv = np.asarray(vertex_colors).astype(dt)
        fb = (wsum == 0) & (filled[i0] >= 0) & (filled[i1] >= 0) & (filled[i2] >= 0)
        mix = ((b0 * Cv[i0] + b1 * Cv[i1]) + b2 * Cv[i2]).astype(dt)
        colour[fb] = mix[fb]
    out = dict(texture=np.full((3, Ht, Wt), dt(fill_value)), weight=np.zeros((Ht, Wt), dt), seen=np.zeros((Ht, Wt), np.int64),
               owned=owned, tie=np.zeros((len(views), Ht, Wt), bool), fallback=np.zeros((Ht, Wt), bool), layout=(cols, rows, Wt, Ht))
    out["texture"][:, owned] = colour.T
    out["weight"][owned], out["seen"][owned], out["fallback"][owned] = wsum, seen, fb
    out["tie"][:, owned] = tie
    return out


# name -> bake()'s arguments: the parity cases first, then the edge inputs
_C = dict(kind="coarse", views=MR.VIEWS, S=64, R=40, T=4)
CASES = {
    "coarse_T4": dict(_C),
    "coarse_T8": dict(_C, T=8),
    "subpixel_T3": dict(kind="subpixel", views=MR.VIEWS, S=48, R=64, T=3, power=1, depth_tol=5e-4),
    "odd_F": dict(_C, n_faces=307),
    "cols1": dict(_C, cols=1),
    "cols7": dict(_C, cols=7, n_faces=300),          # 150 cells: 21 rows of 7 and a last row of 3
    "one_view": dict(_C, views=MR.VIEWS[1:]),
    "znear": dict(_C, znear=0.95),
    "power8": dict(_C, power=8),
    "R1": dict(_C, R=1),
    "S1": dict(_C, S=1),
    "F1": dict(_C, face0=100, n_faces=1),            # (face 0 touches the pole, which projects onto a pixel boundary: a tie)
}
PARITY = ("coarse_T4", "coarse_T8", "subpixel_T3")
FILL = 0.375


@functools.lru_cache(maxsize=None)
def case(name, dt_name):
    """bake() of CASES[name] with fill 0.375; cached, shared by the tests: do not write."""
    return bake(fill_value=FILL, dt=getattr(np, dt_name), **CASES[name])


def synthetic_texture(F, T, cols, rows, seed=0, poison=40.0):
    """(texture [3,Ht,Wt] fp32, c [F,3]): every owned and gutter texel of face f holds c[f], random in [-1, 1], so that
    neighbouring faces differ; unowned texels hold `poison`, far outside the range, so that a fetch that touches one shows."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(-1, 1, (F, 3)).astype(np.float32)
    face, _, _, _ = classify(F, T, cols, rows)
    tex = np.where(face[None] >= 0, c[np.maximum(face, 0)].transpose(2, 0, 1), np.float32(poison)).astype(np.float32)
    return tex, c
