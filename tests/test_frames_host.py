"""Frame resampling on the host (no GPU): the numpy mirror `frames._resize_u8_host` -- the oracle of tests/test_gpu_frames.py --
equals Pillow's `Image.resize` byte for byte, live and against the committed fixture; the coefficient tables keep their
invariants; `compose_panels` and the inversion's target preprocessing on CPU tensors equal Pillow's pictures pasted / scaled
the reference's way.  Integer arithmetic: every comparison is exact."""
import math
import os

import numpy as np
import pytest
import torch

from cips_3dplusplus_amd import frames

import _frames_cases as FC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_resize.npz")


@pytest.mark.parametrize("flt", FC.FILTERS)
@pytest.mark.parametrize("case", FC.SMALL + FC.PILLOW_ONLY, ids=lambda c: c[0])
def test_host_mirror_equals_pillow(case, flt):
    name, (H, W), size = case
    a = FC.image(name, H, W)
    got = frames._resize_u8_host(a, size, flt)
    ref = FC.pillow_resize(a, size, flt)
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert int((got != ref).sum()) == 0


def test_host_mirror_equals_rgb_mode_pillow():
    """Pillow filters the bands of an RGB picture independently: the planar layout loses nothing."""
    from PIL import Image
    a = FC.image("rgb_mode", 33, 47)
    ref = np.asarray(Image.fromarray(a[0].transpose(1, 2, 0), "RGB").resize((9, 8), Image.LANCZOS)).transpose(2, 0, 1)
    assert np.array_equal(frames._resize_u8_host(a, (8, 9), Image.LANCZOS)[0], ref)


@pytest.mark.parametrize("flt", FC.FILTERS)
def test_host_mirror_equals_committed_fixture(flt):
    gold = np.load(GOLDEN)
    for name, (H, W), size in FC.SMALL:
        a = gold[f"{name}/in"]
        assert np.array_equal(a, FC.image(name, H, W, C=1)), name
        assert np.array_equal(frames._resize_u8_host(a, size, flt), gold[f"{name}/{flt}"]), (name, flt)


@pytest.mark.parametrize("flt", FC.FILTERS)
def test_coefficient_tables(flt):
    support = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0, "lanczos": 3.0}[flt]
    pairs = {(I, O) for _, (H, W), (oh, ow) in FC.SMALL + FC.PILLOW_ONLY for I, O in ((H, oh), (W, ow))} | {(1, 1), (2, 1000)}
    for I, O in sorted(pairs):
        bounds, coeffs = frames.resample_coeffs(I, O, flt)
        assert bounds.dtype == torch.int32 and coeffs.dtype == torch.int32
        ksize = 2 * math.ceil(support * max(I / O, 1.0)) + 1
        assert tuple(bounds.shape) == (O, 2) and tuple(coeffs.shape) == (O, ksize) == (O, frames.ksize_of(I, O, flt))
        xmin, n = bounds[:, 0].numpy().astype(np.int64), bounds[:, 1].numpy().astype(np.int64)
        assert (xmin >= 0).all() and (n >= 1).all() and (n <= ksize).all() and (xmin + n <= I).all()
        # the kernels bound a tile's input window by its first and last output: both ends of the windows never move back
        assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all()
        c = coeffs.numpy().astype(np.int64)
        assert all((c[i, n[i]:] == 0).all() for i in range(O))
        # normalised weights: the fixed-point coefficients of a window sum to 2^22 up to their n roundings
        assert (np.abs(c.sum(1) - (1 << 22)) <= n).all()
        # Pillow's bound: |sum p k| stays inside int32 for every 8-bit input
        assert (255 * np.abs(c).sum(1) + (1 << 21) < 2 ** 31).all()
    assert frames.resample_coeffs(7, 13, flt)[1] is not None and frames.resample_coeffs(7, 13, flt.upper())[0].shape[0] == 13


def test_unknown_filter_and_bad_sizes():
    with pytest.raises(ValueError):
        frames.resample_coeffs(4, 4, "nearest")
    with pytest.raises(ValueError):
        frames.resize_u8(torch.zeros(1, 1, 4, 4, dtype=torch.uint8), (0, 4))
    with pytest.raises(TypeError):
        frames.resize_u8(torch.zeros(1, 1, 4, 4, dtype=torch.int32), 4)


def test_fp32_source_is_quantised_like_rgb_to_uint8():
    x = torch.tensor([-3.0, -1.0, -0.5, 0.0, 1 / 255, 0.5, 1.0, 7.0, 2 / 255 - 1, 1 - 1 / 255]).float()
    x = torch.cat([x, torch.linspace(-1.1, 1.1, 90)]).reshape(1, 1, 10, 10)
    q = torch.from_numpy(np.rint((np.clip(x.numpy(), -1, 1).astype(np.float32) + np.float32(1)) * np.float32(127.5)).astype(np.uint8))
    assert torch.equal(frames.resize_u8(x, 10), q)
    assert torch.equal(frames.resize_u8(x, (7, 23), "bicubic"), frames.resize_u8(q, (7, 23), "bicubic"))


@pytest.mark.parametrize("nrow", [None, 2])
def test_compose_panels_cpu_equals_pillow_paste(nrow):
    n = 2
    panes = [torch.from_numpy(FC.image(f"pane{i}", s, s, 3, n)) for i, s in enumerate((32, 8, 16))]
    got = frames.compose_panels(panes, resample="lanczos", nrow=nrow)
    cols = 3 if nrow is None else nrow
    rows = -(-3 // cols)
    assert got.shape == (n, 3, rows * 32, cols * 32) and got.dtype == torch.uint8
    ref = np.full(tuple(got.shape), 255, np.uint8)
    for i, p in enumerate(panes):
        r, c = divmod(i, cols)
        ref[:, :, r * 32:(r + 1) * 32, c * 32:(c + 1) * 32] = FC.pillow_resize(p.numpy(), (32, 32), "lanczos")
    assert np.array_equal(got.numpy(), ref)
    # into a given block, non-square cells
    block = torch.full((n, 3, 2 * 10, 2 * 24), 7, dtype=torch.uint8)
    out = frames.compose_panels(panes, size=(10, 24), resample="bilinear", nrow=2, out=block)
    assert out is block and bool((block[:, :, 10:, 24:] == 255).all())
    assert np.array_equal(block[:, :, :10, 24:].numpy(), FC.pillow_resize(panes[1].numpy(), (10, 24), "bilinear"))


def test_target_images_from_u8():
    """`StyleGAN2Projector_Flip._get_target_image`: centre crop to the short side, LANCZOS to S^2, / 255, - 0.5, * 2; the flip."""
    from PIL import Image
    a = FC.image("target", 45, 70)[0]                              # [3, 45, 70]
    pil = Image.fromarray(a.transpose(1, 2, 0), "RGB")
    left = int(round((70 - 45) / 2.0))
    pil = pil.crop((left, 0, left + 45, 45)).resize((32, 32), Image.LANCZOS)
    t_np = np.array(pil, dtype=np.float32).transpose([2, 0, 1]) / 255.
    t = (torch.from_numpy(t_np) - 0.5) * 2
    f_np = np.array(pil.transpose(Image.FLIP_LEFT_RIGHT), dtype=np.float32).transpose([2, 0, 1]) / 255.
    ref = torch.stack([t, (torch.from_numpy(f_np) - 0.5) * 2], 0)
    got = frames.target_images_from_u8(torch.from_numpy(a), 32)
    assert got.shape == (2, 3, 32, 32) and got.dtype == torch.float32
    assert torch.equal(got, ref)
    crop = frames.center_crop_resize(torch.from_numpy(a), 45)
    assert torch.equal(crop, torch.from_numpy(a[:, :, left:left + 45]))
