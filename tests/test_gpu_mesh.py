"""Geometry export on the GPU (csrc/mesh.hip, cips_3dplusplus_amd/mesh.py): frustum alignment against the reference's
recorded output, marching cubes against the numpy oracle of tests/test_mesh_host.py, and the renderer-only surface
extraction against the renderer and the CPU oracle."""
import numpy as np
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import _lib, configs, hip, mesh, weights
from cips_3dplusplus_amd.camera import Camera
from conftest import maxdiff
from oracle import path as O
from test_mesh_host import (ALIGN_FP64_BAR, ALIGN_LARGE, ALIGN_SMALL, align_case, align_fp64, align_samples, apply_affine,
                            assert_closed_oriented, euler, mc_numpy, mc_numpy_full, random_field, sphere, torus)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def cu(t):
    return t.to(DEV)


def _mc(A, level=0.0, affine=None):
    v, f = hip.marching_cubes(cu(torch.from_numpy(np.ascontiguousarray(A))), level, affine)
    assert f.dtype == torch.int64 and v.dtype == torch.float32
    return v.cpu().numpy(), f.cpu().numpy()


# ------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("tag", ["a", "b"])
def test_align_volume_matches_reference(golden, tag):
    fx = golden("mesh_align")
    vin, ref = fx[f"align.{tag}.in"], fx[f"align.{tag}.out"]
    near, far = float(fx[f"align.{tag}.near"]), float(fx[f"align.{tag}.far"])
    out = mesh.align_volume(cu(vin), near, far).cpu()
    assert out.shape == ref.shape
    # out-of-frustum mask bit for bit: the reference writes exactly 1 there; the inside values are samples
    mask = (ref == 1.0)
    assert mask.any() and (~mask).any()
    assert torch.equal(out[mask], ref[mask])
    assert maxdiff(out, ref) < 1e-6
    out4 = mesh.align_volume(cu(vin[..., 0]), near, far).cpu()
    assert torch.equal(out4, out[..., 0])


@pytest.mark.parametrize("tag", ALIGN_LARGE + ALIGN_SMALL)
def test_align_volume_sizes_match_reference(golden, tag):
    """The reference's recorded output at the production size (128^3), at a large non-cubic size and at degenerate sizes
    (tests/golden/mesh_align_sizes.npz): the mask bit for bit, the values below 1e-6; and the fp64 statement of the
    header's definition (test_mesh_host.align_fp64) over the whole volume, at the bar the reference itself meets."""
    fx = golden("mesh_align_sizes")
    vol, near, far = align_case(fx, tag)
    out = mesh.align_volume(cu(vol), near, far).cpu()
    assert out.shape == vol.shape
    if tag in ALIGN_LARGE:
        assert np.array_equal(np.packbits((out == 1.0).numpy()), fx[f"{tag}.mask"].numpy())
        pairs = align_samples(fx, tag, out)
    else:
        assert torch.equal(out == 1.0, fx[f"{tag}.out"] == 1.0)
        pairs = [("out", fx[f"{tag}.out"], out)]
    err = {what: maxdiff(got, ref) for what, ref, got in pairs}
    ref64, mask64 = align_fp64(vol, near, far)
    err64 = maxdiff(out, ref64)
    print(f"align {tag}: kernel - reference = {max(err.values()):.3e}, kernel - fp64 = {err64:.3e} (bar {ALIGN_FP64_BAR[tag]:.3e})")
    assert all(ref.shape == got.shape and ref.numel() > 0 for _, ref, got in pairs)
    assert max(err.values()) < 1e-6, err
    assert torch.equal(out == 1.0, mask64)
    assert err64 <= ALIGN_FP64_BAR[tag]


def test_align_volume_wrapper_forms():
    base = cu(weights.det_normal("align_wrapper", (2, 10, 9, 11, 1), 1.0, 3))
    want = mesh.align_volume(base, 0.8, 1.2)
    # a non-contiguous view of the same values
    nc = base.permute(0, 3, 2, 1, 4).contiguous().permute(0, 3, 2, 1, 4)
    assert not nc.is_contiguous() and torch.equal(nc, base)
    got = mesh.align_volume(nc, 0.8, 1.2)
    assert got.shape == base.shape and torch.equal(got, want)
    wide = cu(weights.det_normal("align_wrapper_wide", (2, 10, 9, 11, 2), 1.0, 4))
    assert torch.equal(mesh.align_volume(wide[..., :1], 0.8, 1.2), mesh.align_volume(wide[..., :1].contiguous(), 0.8, 1.2))
    # the 4-D form
    got4 = mesh.align_volume(base[..., 0], 0.8, 1.2)
    assert got4.shape == base.shape[:4] and torch.equal(got4, want[..., 0])
    assert torch.equal(mesh.align_volume(nc[..., 0], 0.8, 1.2), want[..., 0])
    # out=: written in place, nothing else allocated for the result
    buf = torch.full_like(base[..., 0], -7.0)
    ret = hip.align_volume(base[..., 0].contiguous(), 0.8, 1.2, out=buf)
    assert ret is buf and torch.equal(buf, want[..., 0])


def test_reference_vertex_frame(golden):
    fx = golden("mesh_align")
    sdf = fx["mc.in"]
    _, h, w, d, _ = sdf.shape
    # the array the reference meshes is sdf[0, ..., 0].permute(1, 0, 2): x <-> w, y <-> h, z <-> d
    assert torch.equal(fx["mc.sdf_vol"], sdf[0, ..., 0].permute(1, 0, 2))
    vi = fx["mc.verts_index"].numpy()
    aff = mesh.reference_affine(h, w, d)
    ours = np.stack([vi[:, a] * np.float32(aff[a][0]) + np.float32(aff[a][1]) for a in range(3)], 1)
    assert np.abs(ours - fx["mc.verts_out"].numpy()).max() < 1e-6


# ------------------------------------------------------------------------------------------------ marching cubes = oracle
FIELDS = {
    "random_12": lambda: random_field((12, 12, 12), 0),
    "random_nc": lambda: random_field((9, 17, 13), 1),
    "random_big": lambda: random_field((40, 33, 70), 2),
    "sphere_nc": lambda: sphere(24, 30, 20, 8.3),
    "torus": lambda: torus(32, 9.0, 3.5),
    "noisy": lambda: np.random.default_rng(5).standard_normal((7, 5, 6)).astype(np.float32),
}


@pytest.mark.parametrize("name", list(FIELDS))
def test_marching_cubes_equals_oracle(name):
    A = FIELDS[name]()
    h, w, d = A.shape
    for affine in (None, mesh.reference_affine(h, w, d)):
        v, f = _mc(A, 0.0, affine)
        rv, rf = mc_numpy(A, 0.0, affine)
        assert v.shape == rv.shape and f.shape == rf.shape
        assert len(f) > 0
        assert np.abs(v - rv).max() < 1e-6
        assert np.array_equal(f, rf)


def test_marching_cubes_level():
    A = sphere(20, 20, 20, 4.0)
    v, f = _mc(A, 2.5)
    rv, rf = mc_numpy(A, 2.5)
    assert np.array_equal(f, rf) and np.abs(v - rv).max() < 1e-6
    r = np.linalg.norm(v - 9.5, axis=1)
    assert np.abs(r - 6.5).max() < 0.5


def test_sphere_geometry():
    r = 20.0
    v, f = _mc(sphere(64, 64, 64, r))
    c = 31.5
    assert np.abs(np.linalg.norm(v - c, axis=1) - r).max() < 0.5
    tri = v[f].astype(np.float64) - c
    vol = np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6
    exact = 4 / 3 * np.pi * r ** 3
    assert vol > 0 and abs(vol - exact) < 0.01 * exact
    assert_closed_oriented(f)
    assert euler(v, f) == 2


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_planes_land_on_their_axis(axis):
    h, w, d = 10, 12, 14
    i, j, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(d), indexing="ij")
    coord = (j, i, k)[axis].astype(np.float32)         # x <-> j, y <-> i, z <-> k
    v, f = _mc(coord - 4.25)
    assert len(f) > 0
    assert np.abs(v[:, axis] - 4.25).max() < 1e-6
    # the reference frame maps that index plane to the expected coordinate
    vr, _ = _mc(coord - 4.25, 0.0, mesh.reference_affine(h, w, d))
    n = (w, h, d)[axis]
    want = (4.25 / n - 0.5) * 0.24 * (1 if axis == 0 else -1)
    assert np.abs(vr[:, axis] - want).max() < 1e-6


def test_empty_volumes_and_refusals():
    for val in (1.0, -1.0):
        A = cu(torch.full((1, 6, 7, 8, 1), val))
        v, f = hip.marching_cubes(A[0, ..., 0].contiguous())
        assert v.shape == (0, 3) and f.shape == (0, 3)
        assert mesh.extract_mesh_with_marching_cubes(A) is None
    with pytest.raises(RuntimeError):
        hip.marching_cubes(cu(torch.zeros(1, 8, 8)))
    with pytest.raises(RuntimeError):
        hip.marching_cubes(cu(torch.zeros(8, 8, 1)))


def test_two_runs_are_bit_identical():
    A = cu(torch.from_numpy(random_field((48, 40, 56), 9)))
    v1, f1 = hip.marching_cubes(A, 0.1, mesh.reference_affine(48, 40, 56))
    v2, f2 = hip.marching_cubes(A, 0.1, mesh.reference_affine(48, 40, 56))
    assert torch.equal(v1, v2) and torch.equal(f1, f2)
    a1, a2 = mesh.align_volume(A[None]), mesh.align_volume(A[None])
    assert torch.equal(a1, a2)


# ------------------------------------------------------------------------------------------------ where the loops wrap
TILE = 2048                 # points per tile (csrc/mesh.hip MC_TILE)
SCAN_ROUND = 256            # tiles per round of the tile scan (one per thread of its workgroup)
GRID_CAP = 8192             # workgroups of the grid-stride kernels (mc_grid)


def normal_field(shape, seed):
    """Unit-normal samples with open borders: crossings everywhere, the surface runs into every border plane."""
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def two_spheres(shape, c0, r0, c1, r1):
    return np.minimum(sphere(*shape, r0, c0), sphere(*shape, r1, c1))


def last_layer_field(shape, seed, planes):
    """Positive everywhere but on the last lattice plane of each axis: negative there (`planes` False: every crossing
    edge runs from index n - 2 to n - 1 of its axis), or unit-normal there (`planes` True: crossings also on the edges
    inside the three planes i = h - 1, j = w - 1, k = d - 1, whose points are the lower corner of no cell)."""
    rng = np.random.default_rng(seed)
    A = (np.abs(rng.standard_normal(shape)) + 0.1).astype(np.float32)
    B = rng.standard_normal(shape).astype(np.float32) if planes else -A
    for sl in ((-1, slice(None), slice(None)), (slice(None), -1, slice(None)), (slice(None), slice(None), -1)):
        A[sl] = B[sl]
    return A


def on_border(v, shape):
    h, w, d = shape
    return ((v[:, 0] == 0) | (v[:, 0] == w - 1) | (v[:, 1] == 0) | (v[:, 1] == h - 1) | (v[:, 2] == 0) | (v[:, 2] == d - 1))


def assert_open_edges_on_border(v, f, shape):
    """Every edge used by exactly one triangle has both ends on a border plane of the volume (index-space vertices)."""
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = e.min(1) * np.int64(len(v)) + e.max(1)
    uniq, n = np.unique(key, return_counts=True)
    assert n.max() <= 2
    once = uniq[n == 1]
    assert len(once) > 0
    ends = np.concatenate([once // len(v), once % len(v)])
    assert on_border(v[ends], shape).all()


def assert_equals_oracle(A, level=0.0, nonfinite=False):
    """The bars of test_marching_cubes_equals_oracle, in index space and in the reference's frame; the oracle runs once.
    -> (verts, faces, oracle's vert_point, vert_axis, face_point)."""
    h, w, d = A.shape
    rv, rf, vp, va, fp = mc_numpy_full(A, level)
    for affine in (None, mesh.reference_affine(h, w, d)):
        v, f = _mc(A, level, affine)
        want = rv if affine is None else apply_affine(rv.copy(), affine)
        assert v.shape == want.shape and f.shape == rf.shape
        assert np.array_equal(f, rf)
        if len(f):
            assert f.min() >= 0 and f.max() < len(v)
        if nonfinite:
            assert np.array_equal(np.isnan(v), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.array_equal(np.isinf(v), np.isinf(want)) and not np.isinf(want).any()
            assert np.abs(v[ok] - want[ok]).max() < 1e-6
        elif len(v):
            assert np.abs(v - want).max() < 1e-6
        if affine is None:
            v0, f0 = v, f
    return v0, f0, vp, va, fp


LARGE_FIELDS = {
    # name: (field, tiles above, closed surface's Euler characteristic or None for an open-bordered field)
    "spheres_128": (lambda: two_spheres((128, 128, 128), (45, 40, 38), 28.0, (85, 90, 92), 26.0), 4 * SCAN_ROUND - 1, 4),
    "normal_128": (lambda: normal_field((128, 128, 128), 21), 4 * SCAN_ROUND - 1, None),
    "normal_ragged": (lambda: normal_field((100, 131, 83), 22), 2 * SCAN_ROUND, None),
}


@pytest.mark.parametrize("name", list(LARGE_FIELDS))
def test_marching_cubes_equals_oracle_past_one_scan_round(name):
    """More than 256 tiles: mc_scan_tiles_kernel carries its running totals from round to round (four rounds at the
    production size 128^3, three at 100 x 131 x 83 with a ragged last tile)."""
    field, tiles_above, chi = LARGE_FIELDS[name]
    A = field()
    n_tiles = -(-A.size // TILE)
    assert n_tiles > tiles_above
    v, f, vp, _, fp = assert_equals_oracle(A)
    assert len(f) > 0
    rounds = np.unique(vp // (TILE * SCAN_ROUND))
    assert len(rounds) == -(-n_tiles // SCAN_ROUND)            # vertices in every round of the scan
    if chi is None:
        assert len(np.unique(vp // TILE)) == n_tiles           # crossings fill every tile, the first and the last included
        assert vp.min() < TILE and vp.max() >= (n_tiles - 1) * TILE
        assert_open_edges_on_border(v, f, A.shape)
    else:
        assert not on_border(v, A.shape).any()
        assert_closed_oriented(f)
        assert euler(v, f) == chi
    if name == "normal_ragged":
        assert A.size % TILE != 0 and len({*A.shape}) == 3


def test_marching_cubes_equals_oracle_past_the_grid_cap():
    """More than 8192 tiles: the second trip of the grid-stride loops of mc_classify_kernel and mc_emit_verts_kernel
    (with their __syncthreads() inside the loop) and of mc_emit_faces_kernel.  The second sphere lies wholly in rows whose
    points come after 8192 tiles."""
    shape = (300, 256, 256)
    A = two_spheres(shape, (127.5, 80.0, 127.5), 60.0, (140.0, 278.0, 110.0), 18.0)
    n_tiles = -(-A.size // TILE)
    assert n_tiles > GRID_CAP
    v, f, vp, _, fp = assert_equals_oracle(A)
    second = vp >= GRID_CAP * TILE
    assert second.any() and (~second).any()
    assert (fp >= GRID_CAP * TILE).any() and (fp < GRID_CAP * 256).any()
    # the second sphere is whole: its vertices are exactly those of the second trip
    assert np.array_equal(second, v[:, 1] > 250)
    assert np.abs(np.linalg.norm(v[second] - np.array([140.0, 278.0, 110.0], np.float32), axis=1) - 18.0).max() < 0.5
    assert not on_border(v, shape).any()
    assert_closed_oriented(f)
    assert euler(v, f) == 4


@pytest.mark.parametrize("shape", [(8, 16, 16), (16, 16, 16), (2, 2, 512), (2, 2, 2), (2, 3, 2)])
def test_marching_cubes_equals_oracle_at_tile_multiples(shape):
    """Point counts of exactly one and two tiles (no ragged tail), and the smallest volumes."""
    A = normal_field(shape, 23)
    if A.size >= TILE:
        assert A.size in (TILE, 2 * TILE)
    v, f, vp, _, _ = assert_equals_oracle(A)
    assert len(f) > 0
    assert len(np.unique(vp // TILE)) == -(-A.size // TILE)
    assert_open_edges_on_border(v, f, A.shape)


@pytest.mark.parametrize("planes", [False, True])
def test_marching_cubes_equals_oracle_in_the_last_layer(planes):
    shape = (11, 19, 13)
    h, w, d = shape
    A = last_layer_field(shape, 24, planes)
    v, f, vp, va, _ = assert_equals_oracle(A)
    assert len(f) > 0
    # every vertex lies in the last layer of cells
    assert ((v[:, 0] >= w - 2) | (v[:, 1] >= h - 2) | (v[:, 2] >= d - 2)).all()
    i, j, k = np.unravel_index(vp, shape)
    if not planes:
        # every crossing edge ends at the last lattice point of its axis
        assert (np.where(va == 0, j == w - 2, np.where(va == 1, i == h - 2, k == d - 2))).all()
        for a in range(3):
            assert (va == a).any()
    else:
        # edges inside each of the three planes whose points start no cell, in both in-plane directions
        for plane, axes in ((i == h - 1, (0, 2)), (j == w - 1, (1, 2)), (k == d - 1, (0, 1))):
            for a in axes:
                assert (plane & (va == a)).any()


# ------------------------------------------------------------------------------------------------ the emit call's bounds
def test_emit_bounds_every_store():
    """max_verts / max_faces bound every store (include/cips3d_hip.h): the buffers here are larger than the bound, so what
    the guards keep out is the test's own memory."""
    lib = _lib.load()
    A = cu(torch.from_numpy(normal_field((24, 30, 40), 25)))
    h, w, d = A.shape
    assert A.numel() > 10 * TILE
    ws, totals = hip.marching_cubes_count(A, 0.0)
    V, F = (int(x) for x in totals.cpu())
    assert V > 1000 and F > 1000
    full_v, full_f = hip.marching_cubes_emit(A, 0.0, ws, V, F)
    rv, rf = mc_numpy(A.cpu().numpy())
    assert np.array_equal(full_f.cpu().numpy(), rf) and np.abs(full_v.cpu().numpy() - rv).max() < 1e-6
    full_v, full_f = full_v.view(torch.int32), full_f
    pad, vs, fs = 64, -12345.0, -7
    for mv, mf in ((V, F), (V - 1, F), (V, F - 1), (V // 2, F // 3), (0, F), (V, 0), (0, 0)):
        vb = torch.full((V + pad, 3), vs, device=DEV)
        fb = torch.full((F + pad, 3), fs, dtype=torch.int32, device=DEV)
        rc = lib.cips3d_marching_cubes_emit(_lib.dev_ptr(A), h, w, d, 0.0, None, ws.data_ptr(), vb.data_ptr(), fb.data_ptr(), mv, mf,
                                            _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (mv, mf)
        assert (vb[mv:] == vs).all() and (fb[mf:] == fs).all(), (mv, mf)
        assert torch.equal(vb[:mv].view(torch.int32), full_v[:mv]), (mv, mf)
        assert torch.equal(fb[:mf], full_f[:mf]), (mv, mf)


# ------------------------------------------------------------------------------------------------ the inside rule's edges
@pytest.mark.parametrize("level", [0.0, 0.1])
def test_samples_equal_to_the_level_are_outside(level):
    """A == level is outside (inside is A < level): t = 0 or t = 1 on its edges, zero-area triangles allowed.  0.1 is not
    an fp32 number: the library compares with float(0.1), which the field holds."""
    rng = np.random.default_rng(26)
    A = normal_field((20, 22, 18), 27) + np.float32(level)
    hit = rng.random(A.shape) < 0.15
    A[hit] = np.float32(level)
    if level == 0.0:
        neg = rng.random(A.shape) < 0.05
        A[neg] = np.float32(-0.0)
        assert np.signbit(A[neg]).all() and (A[neg] == 0).all()
    assert (A == np.float32(level)).mean() > 0.1
    v, f, vp, va, _ = assert_equals_oracle(A, level)
    assert len(f) > 0
    # vertices that sit exactly on a lattice point: both t = 0 and t = 1 occur
    i, j, k = np.unravel_index(vp, A.shape)
    t = v[np.arange(len(v)), va] - np.where(va == 0, j, np.where(va == 1, i, k))
    assert (t == 0).any() and (t == 1).any() and ((t > 0) & (t < 1)).any()
    tri = v[f]
    assert (np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) == 0).any()


def test_levels_below_inside_and_above_the_range():
    A = sphere(20, 20, 20, 4.0)
    for level in (float(A.min()) - 1.0, float(A.min())):           # nothing is below the minimum: no inside point
        v, f = _mc(A, level)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    for level in (float(A.max()) + 1.0, float(np.nextafter(A.max(), np.float32(np.inf)))):     # every point inside
        v, f = _mc(A, level)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    for level in (-3.0, 0.1, 2.5, float(A.max())):
        v, f, _, _, _ = assert_equals_oracle(A, level)
        assert len(f) > 0


def test_non_finite_samples():
    """NaN and +inf are outside, -inf is inside.  An edge with a non-finite end carries whatever the contract's
    t = (level - A_a) / (A_b - A_a) gives (NaN, or the finite end for +inf at the upper end); the faces and every vertex
    between two finite samples are untouched by it."""
    A = normal_field((16, 18, 20), 28)
    spots = {np.nan: [(3, 4, 5), (10, 12, 3), (15, 17, 19), (0, 0, 0)],
             np.inf: [(6, 9, 14), (12, 3, 8), (0, 17, 10)],
             -np.inf: [(8, 6, 2), (13, 14, 16), (15, 0, 7)]}
    for val, where in spots.items():
        for p in where:
            A[p] = val
    pts = np.array([p for where in spots.values() for p in where])
    gap = np.abs(pts[:, None] - pts[None]).max(-1) + 100 * np.eye(len(pts), dtype=np.int64)
    assert gap.min() >= 2                                           # no lattice edge joins two of them
    v, f, vp, va, _ = assert_equals_oracle(A, 0.0, nonfinite=True)
    assert len(f) > 0 and f.min() >= 0 and f.max() < len(v)
    flat = A.reshape(-1)
    h, w, d = A.shape
    upper = vp + np.where(va == 0, d, np.where(va == 1, w * d, 1))
    finite_edge = np.isfinite(flat[vp]) & np.isfinite(flat[upper])
    assert np.isfinite(v[finite_edge]).all()
    assert np.isnan(v[~finite_edge]).any() and np.isfinite(v[~finite_edge]).all(1).any()
    assert 0 < (~finite_edge).sum() <= 6 * len(pts)


# ------------------------------------------------------------------------------------------------ surface_mesh
def test_surface_mesh_tiny_generator():
    cfg = configs.tiny_G_cfg(hidden=32, N_layers_renderer=2)
    G = pkg.build_generator(cfg, DEV, seed=5)
    sd = {k: v.detach().cpu() for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    zs = [torch.randn(1, 32, generator=g), torch.randn(1, 32, generator=g)]
    nb = O.create_noise_bufs(cfg, 8, generator=g)
    ncfg = dict(N_samples=6, perturb=False, static_viewdirs=False)
    e, f, n, fa, _ = Camera.generate_camera_params(8, DEV, locations=cu(torch.tensor([[0.2, -0.05]])))

    def forward():
        return G(zs=[cu(z) for z in zs], cam_poses=e, focals=f, img_size=8, near=n, far=fa,
                 noise_bufs=[cu(b) for b in nb], nerf_cfg=ncfg, return_xyz=True)

    before = forward()
    S, N = 12, 10
    style_r, _ = G.mapping_renderer([cu(zs[0])], 1, None)
    locs = torch.zeros(1, 2)
    cam = Camera.generate_camera_params(S, DEV, locations=cu(locs))
    _, _, sdf_r, _, _ = G.renderer.render(cam[0], cam[1], cam[2], cam[3], style_r, S, N, return_sdf=True)
    aligned_r = mesh.align_volume(sdf_r)
    inside = aligned_r[0, ..., 0][aligned_r[0, ..., 0] != 1.0]
    level = float(inside.median())

    out = mesh.surface_mesh(G, zs=[cu(zs[0])], resolution=S, N_samples=N, level=level)
    assert torch.equal(out["sdf"], sdf_r)
    # the volume agrees with the CPU oracle's renderer
    D = cfg["renderer_cfg"]["N_layers_renderer"]
    st = style_r.cpu()
    ocam = O.camera_params(locs, S, 6, 0.12)
    rays_o, rays_d, vd = O.rays_in_world(ocam[1], S, ocam[0], False)
    z = O.z_vals(ocam[2], ocam[3], 1, S, S, N, None)
    pts = O.ray_points(rays_o, rays_d, z)
    R = S * S
    r_sdf = O.renderer_forward(sd, "renderer", pts.reshape(1, R, N, 3), rays_d.reshape(1, R, 3), vd.reshape(1, R, 3),
                               z.reshape(1, R, N), ocam[2], ocam[3], st, D)[2]
    assert maxdiff(out["sdf"].cpu(), r_sdf.reshape(1, S, S, N, 1)) < 5e-5
    # the mesh is the oracle's on the aligned volume
    assert torch.equal(out["aligned"], aligned_r)
    A = aligned_r[0, ..., 0].cpu().numpy()
    rv, rf = mc_numpy(A, level, mesh.reference_affine(S, S, N))
    assert out["meshes"][0] is not None and len(rf) > 0
    v, fc = out["meshes"][0]
    assert np.abs(v.cpu().numpy() - rv).max() < 1e-6
    assert np.array_equal(fc.cpu().numpy(), rf)
    # nothing leaks into the forward's plans or tables
    after = forward()
    for k in ("rgb", "thumb_rgb", "xyz", "mask", "depth"):
        assert torch.equal(before[k], after[k]), k


@pytest.mark.parametrize("truncation", [1, 0.7])
def test_surface_mesh_batch_of_views(truncation):
    """A batch of three views with their own z, location and level: every row equals, bit for bit, the batch-1 call on that
    row, and the rows differ from one another."""
    cfg = configs.tiny_G_cfg(hidden=32, N_layers_renderer=2)
    G = pkg.build_generator(cfg, DEV, seed=5)
    B, S, N = 3, 12, 10
    zs = cu(weights.det_normal("surface_mesh_batch.z", (B, 32), 1.0, 7))
    locs = cu(torch.tensor([[0.2, -0.05], [-0.3, 0.1], [0.0, 0.15]]))
    if truncation < 1:
        w = G._run_style(zs)
        G.style_render_mean = cu(weights.det_normal("surface_mesh_batch.mean", (1, w.shape[1]), 0.5, 8))
        G.style_decoder_mean = torch.zeros_like(G.style_render_mean)
    kw = dict(truncation=truncation, resolution=S, N_samples=N)
    first = mesh.surface_mesh(G, zs=[zs], locations=locs, **kw)
    assert first["sdf"].shape == first["aligned"].shape == (B, S, S, N, 1) and len(first["meshes"]) == B
    if truncation < 1:
        plain = mesh.surface_mesh(G, zs=[zs], locations=locs, resolution=S, N_samples=N)
        assert not torch.equal(plain["sdf"], first["sdf"])
    levels = []
    for b in range(B):
        vol = first["aligned"][b, ..., 0]
        assert (vol == 1.0).any() and (vol != 1.0).any()
        levels.append(float(vol[vol != 1.0].median()))
    got = []
    for b in range(B):
        out = mesh.surface_mesh(G, zs=[zs], locations=locs, level=levels[b], **kw)
        one = mesh.surface_mesh(G, zs=[zs[b:b + 1]], locations=locs[b:b + 1], level=levels[b], **kw)
        assert torch.equal(out["sdf"], first["sdf"]) and torch.equal(out["aligned"], first["aligned"])
        assert one["sdf"].shape == (1, S, S, N, 1) and len(one["meshes"]) == 1
        assert torch.equal(out["sdf"][b], one["sdf"][0])
        assert torch.equal(out["aligned"][b], one["aligned"][0])
        assert out["meshes"][b] is not None and one["meshes"][0] is not None
        for x, y in zip(out["meshes"][b], one["meshes"][0]):
            assert x.shape == y.shape and x.shape[0] > 0 and torch.equal(x, y)
        # and it is the oracle's mesh of that row
        rv, rf = mc_numpy(out["aligned"][b, ..., 0].cpu().numpy(), levels[b], mesh.reference_affine(S, S, N))
        assert np.abs(out["meshes"][b][0].cpu().numpy() - rv).max() < 1e-6
        assert np.array_equal(out["meshes"][b][1].cpu().numpy(), rf)
        got.append(out["meshes"][b])
    for a in range(B):
        for b in range(a + 1, B):
            assert not torch.equal(first["sdf"][a], first["sdf"][b])
            assert not torch.equal(first["aligned"][a], first["aligned"][b])
            assert got[a][0].shape != got[b][0].shape or not torch.equal(got[a][0], got[b][0])
    # the location reaches the renderer: the same z from another view is another volume
    moved = mesh.surface_mesh(G, zs=[zs[:1]], locations=locs[1:2], level=levels[0], **kw)
    assert not torch.equal(moved["sdf"][0], first["sdf"][0])


def test_surface_mesh_ffhq_d2_at_128():
    G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=1)
    out = mesh.surface_mesh(G, zs=[torch.randn(1, G.z_dim, generator=torch.Generator().manual_seed(0)).to(DEV)])
    assert out["sdf"].shape == (1, 128, 128, 128, 1)
    assert torch.isfinite(out["aligned"]).all()
    vol = out["aligned"][0, ..., 0]
    level = float(vol[vol != 1.0].median())
    for lv in (0.0, level):
        m = mesh.extract_mesh_with_marching_cubes(out["aligned"], lv)
        if m is None:
            assert lv == 0.0 and ((vol < 0).all() or (vol >= 0).all())
            continue
        v, f = m
        assert f.min() >= 0 and f.max() < v.shape[0]
        assert torch.isfinite(v).all()
        assert v.abs().max() <= 0.12 + 1e-6
