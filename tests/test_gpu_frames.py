"""Frame resampling on the device (csrc/frame_resample.hip) against the host mirror `frames._resize_u8_host`, which
tests/test_frames_host.py holds to Pillow.  Integer arithmetic: every comparison is exact, zero differing bytes, all four
filters.  The shapes are the smallest at which a kernel can still go wrong: clamped windows, both ends of the pixel clamp, odd
and non-square sizes in both directions, a skipped pass, sizes around the fused route's tile, ragged row ends for the dword
loads, the threshold between the fused and the two-launch route, batches and channel counts, outputs inside a larger block."""
import numpy as np
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import configs, frames, hip

import _frames_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 201


def dev_resize(a, size, flt, **kw):
    return frames.resize_u8(torch.from_numpy(np.ascontiguousarray(a)).to(DEV), size, flt, **kw).cpu().numpy()


def same(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    assert int((got != ref).sum()) == 0, what


@pytest.mark.parametrize("flt", FC.FILTERS)
@pytest.mark.parametrize("case", FC.SMALL, ids=lambda c: c[0])
def test_device_equals_host_mirror(case, flt):
    name, (H, W), size = case
    a = FC.image(name, H, W)
    same(dev_resize(a, size, flt), frames._resize_u8_host(a, size, flt), (name, flt))


@pytest.mark.parametrize("flt", FC.FILTERS)
def test_sizes_around_the_tile(flt):
    """Output heights and widths one below, at and one above the fused route's tile; up- and down-scaling into them."""
    th, tw, _ = frames.tile()
    up = FC.image("tile_up", 9, 11, 1)
    down = FC.image("tile_down", 2 * th + 5, 2 * tw + 7, 1)
    for oh in (th - 1, th, th + 1):
        for ow in (tw - 1, tw, tw + 1):
            for a in (up, down):
                assert frames.resample_route(a.shape[-2:], (oh, ow), flt) == "fused"
                same(dev_resize(a, (oh, ow), flt), frames._resize_u8_host(a, (oh, ow), flt), (oh, ow, a.shape))


@pytest.mark.parametrize("flt", FC.FILTERS)
@pytest.mark.parametrize("W", [61, 63, 64, 65])
def test_input_row_ends(W, flt):
    """Input rows of 61, 63, 64 and 65 bytes: dword loads must stop at the row's last whole dword.  As a contiguous tensor
    (pitch W: dwords only when W % 4 == 0), and as a view of rows padded to 68 bytes (dwords, ragged end)."""
    a = FC.image(f"rowend{W}", 10, W, 2)
    wide = torch.full((1, 2, 10, 68), SENTINEL, dtype=torch.uint8)
    wide[..., :W] = torch.from_numpy(a)
    view = wide.to(DEV)[..., :W]
    for size in ((23, 2 * W + 1), (7, 29), (10, 90), (21, W)):
        ref = frames._resize_u8_host(a, size, flt)
        same(dev_resize(a, size, flt), ref, (W, size, "contiguous"))
        same(frames.resize_u8(view, size, flt).cpu().numpy(), ref, (W, size, "padded rows"))
        same(frames.resize_u8(view, size, flt, route="two_launch").cpu().numpy(), ref, (W, size, "padded rows, two launches"))
    odd = wide.to(DEV)[..., 1:W]                      # a source pointer that is no multiple of 4
    same(frames.resize_u8(odd, (17, 40), flt).cpu().numpy(), frames._resize_u8_host(a[..., 1:], (17, 40), flt), (W, "offset 1"))


@pytest.mark.parametrize("flt", FC.FILTERS)
def test_routes(flt):
    """257 x 3 -> 2 x 3 puts more input rows under an output row than the fused route stages: it must take two launches.  A
    fused-eligible shape forced through both routes gives the same bytes.  One-axis and no-axis shapes take one launch."""
    _, _, max_rows = frames.tile()
    assert 257 > max_rows
    assert frames.resample_route((257, 3), (2, 3), flt) == "two_launch"          # (its width does not change: that pass is skipped)
    assert frames.resample_route((257, 3), (2, 4), flt) == "two_launch"          # (both passes, through the workspace)
    assert frames.resample_route((256 * 40, 8), (40, 9), flt) == "two_launch"
    assert frames.resample_route((64, 64), (1024, 1024), flt) == "fused"
    assert frames.resample_route((512, 512), (1024, 1024), flt) == "fused"
    for hw, size in (((40, 64), (80, 64)), ((64, 40), (64, 80)), ((9, 11), (9, 11))):     # a pass to skip: nothing to fuse
        assert frames.resample_route(hw, size, flt) == "two_launch"
    a = FC.image("tall", 257, 3)
    same(dev_resize(a, (2, 4), flt), frames._resize_u8_host(a, (2, 4), flt), "257x3 -> 2x4")
    with pytest.raises(RuntimeError):
        dev_resize(a, (2, 4), flt, route="fused")
    for name, (H, W), size in (("mixed", (100, 80), (37, 64)), ("odd_up", (7, 5), (13, 17)), ("odd_down", (33, 47), (8, 9)),
                               ("two_tiles", (50, 70), (45, 150))):
        b = FC.image(name, H, W)
        assert frames.resample_route((H, W), size, flt) == "fused"
        ref = frames._resize_u8_host(b, size, flt)
        same(dev_resize(b, size, flt, route="fused"), ref, (name, "fused"))
        same(dev_resize(b, size, flt, route="two_launch"), ref, (name, "two_launch"))


def test_tall_down_with_and_without_a_horizontal_pass():
    """257 x 3 -> 2 x 3 keeps its width, so of the two launches only the vertical one runs; with the width changed as well the
    same rows go through the workspace."""
    a = FC.image("tall_down", 257, 3)
    for flt in FC.FILTERS:
        same(dev_resize(a, (2, 3), flt), frames._resize_u8_host(a, (2, 3), flt), flt)
        same(dev_resize(a, (2, 5), flt), frames._resize_u8_host(a, (2, 5), flt), flt)
        assert frames.resample_route((257, 3), (2, 5), flt) == "two_launch"


@pytest.mark.parametrize("flt", FC.FILTERS)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_batches_and_channels(C, flt):
    a = FC.image(f"batch{C}", 19, 23, C, n=3)
    for size in ((40, 31), (6, 50), (19, 50)):
        got = dev_resize(a, size, flt)
        same(got, frames._resize_u8_host(a, size, flt), (C, size))
        same(dev_resize(a[1:2], size, flt), got[1:2], (C, size, "sample 1 alone"))


@pytest.mark.parametrize("flt", FC.FILTERS)
def test_out_is_a_cell_of_a_larger_block(flt):
    """`out=` a cell of a block: the cell equals the stand-alone result, every other byte of the block keeps the sentinel.  Cell
    offsets and widths that allow dword stores (multiples of 4) and that forbid them."""
    a = FC.image("cell", 12, 10, 3, n=2)
    for (oh, ow), (top, left), (BH, BW) in (((24, 32), (8, 16), (40, 64)), ((24, 32), (3, 5), (31, 41)), ((7, 9), (1, 2), (9, 12)),
                                           ((12, 20), (0, 4), (12, 28)), ((25, 10), (2, 8), (30, 20))):
        ref = frames._resize_u8_host(a, (oh, ow), flt)
        for route in ("auto", "two_launch"):
            block = torch.full((2, 3, BH, BW), SENTINEL, dtype=torch.uint8, device=DEV)
            cell = block[:, :, top:top + oh, left:left + ow]
            ret = frames.resize_u8(torch.from_numpy(a).to(DEV), (oh, ow), flt, out=cell, route=route)
            assert ret.data_ptr() == cell.data_ptr()
            host = block.cpu().numpy()
            same(host[:, :, top:top + oh, left:left + ow], ref, (oh, ow, route))
            host[:, :, top:top + oh, left:left + ow] = SENTINEL
            assert bool((host == SENTINEL).all()), f"{(oh, ow, top, left, route)}: a byte outside the cell was written"


@pytest.mark.parametrize("flt", FC.FILTERS)
def test_fp32_source(flt):
    """An fp32 source equals resize_u8(hip.rgb_to_uint8(x)): values outside [-1, 1], exactly +-1, halves between two levels."""
    g = torch.Generator().manual_seed(5)
    x = 1.3 * (2 * torch.rand(2, 3, 16, 20, generator=g) - 1)
    x[0, 0, 0, :8] = torch.tensor([-1.0, 1.0, -7.0, 7.0, 0.0, 1 / 255, -1 + 1 / 255, 1 - 3 / 255])
    xd = x.to(DEV)
    q = hip.rgb_to_uint8(xd)
    assert torch.equal(q.cpu(), torch.from_numpy(frames._quantize_host(x.numpy())))
    for size in ((16, 20), (33, 47), (5, 6), (16, 50), (40, 20)):
        got = frames.resize_u8(xd, size, flt)
        assert torch.equal(got, frames.resize_u8(q, size, flt)), size
        same(got.cpu().numpy(), frames._resize_u8_host(x, size, flt).numpy(), size)
    assert torch.equal(frames.resize_u8(xd, (33, 47), flt, route="two_launch"), frames.resize_u8(q, (33, 47), flt))


def test_thumbnail_and_preview_ratios_at_size():
    """The demo's own shapes once, lanczos: 64^2 -> 1024^2 fp32 thumbnail, 512^2 -> 1024^2, the 1024^2 -> 256^2 preview."""
    for name, (H, W), size in FC.PILLOW_ONLY[:3]:
        a = FC.image(name, H, W, 1)
        same(dev_resize(a, size, "lanczos"), frames._resize_u8_host(a, size, "lanczos"), name)


@pytest.mark.parametrize("flt", ["lanczos", "bilinear"])
def test_compose_panels(flt):
    n = 2
    panes = [torch.from_numpy(FC.image(f"pane{i}", s, s, 3, n)) for i, s in enumerate((32, 8, 16))]
    panes[1] = (panes[1].float() / 127.5 - 1)                    # the thumbnail arrives as fp32
    dev = [p.to(DEV) for p in panes]
    got = frames.compose_panels(dev, resample=flt)
    assert got.shape == (n, 3, 32, 96) and got.dtype == torch.uint8 and got.is_cuda
    same(got.cpu().numpy(), frames.compose_panels(panes, resample=flt).numpy(), "one row")
    got2 = frames.compose_panels(dev, resample=flt, nrow=2)
    assert got2.shape == (n, 3, 64, 64)
    same(got2.cpu().numpy(), frames.compose_panels(panes, resample=flt, nrow=2).numpy(), "nrow=2")
    assert bool((got2[:, :, 32:, 32:] == 255).all())
    assert torch.equal(got2[:, :, :32, :32], dev[0])
    block = torch.full((n, 3, 20, 36), SENTINEL, dtype=torch.uint8, device=DEV)
    frames.compose_panels(dev, size=(20, 12), resample=flt, out=block)
    same(block.cpu().numpy(), frames.compose_panels(panes, size=(20, 12), resample=flt).numpy(), "given block")


def test_target_images_on_device():
    a = torch.from_numpy(FC.image("target", 45, 70)[0])
    assert torch.equal(frames.target_images_from_u8(a.to(DEV), 32).cpu(), frames.target_images_from_u8(a, 32))


# ------------------------------------------------------------------------------------------------ the sequence
_SEQ = {}


def _sequence(gather, lanes, n_frames=2, **extra):
    from cips_3dplusplus_amd.multiview import sample_multi_view
    key = (gather, lanes, n_frames, tuple(sorted(extra.items())))
    if key not in _SEQ:
        if "G" not in _SEQ:
            G = pkg.build_generator(configs.ffhq_G_cfg(256, 2), DEV, seed=3)
            g = torch.Generator(device=DEV).manual_seed(11)
            zs = [torch.randn(1, 256, device=DEV, generator=g), torch.randn(1, 256, device=DEV, generator=g)]
            nb = [torch.randn(b.shape, device=DEV, generator=g) for b in G.create_noise_bufs(32, DEV)]
            G.style_render_mean = 0.1 * torch.randn(1, 256, device=DEV, generator=g)
            G.style_decoder_mean = 0.1 * torch.randn(1, 512, device=DEV, generator=g)
            _SEQ["G"] = (G, zs, nb)
        G, zs, nb = _SEQ["G"]
        cam_cfg = {"img_size": 32, "fov_ang": 12, "dist_radius": 0.12}
        out = sample_multi_view(G, cam_cfg, {"static_viewdirs": False}, zs, view_mode="yaw", N_frames=n_frames, truncation_ratio=0.7,
                                N_samples=12, noise_bufs=nb, gather=gather, lanes=lanes, **extra)
        torch.cuda.synchronize()
        _SEQ[key] = out
    return _SEQ[key]


def test_sample_multi_view_panel():
    """FFHQ 256^2 weights at 32^2 rays x 12 samples, 2 frames: the panel is compose_panels of the separately gathered panes; the
    panes are byte-identical to a call without "panel"; 1 and 2 lanes agree; the panel alone can be gathered."""
    full = ("rgb", "thumb_rgb", "shaded", "panel")
    out = _sequence(full, 2)
    base = _sequence(full[:3], 2)
    assert set(out) == set(full) | {"trajectory"} and set(base) == set(full[:3]) | {"trajectory"}
    R = out["rgb"].shape[-1]
    assert out["panel"].shape == (2, 3, R, 3 * R) and out["panel"].dtype == torch.uint8 and out["panel"].is_contiguous()
    for k in full[:3]:
        assert torch.equal(out[k], base[k]), k
    ref = frames.compose_panels([out["rgb"], out["thumb_rgb"], out["shaded"]], size=R, resample="lanczos")
    assert torch.equal(out["panel"], ref)
    host = frames.compose_panels([out[k].cpu() for k in full[:3]], size=R, resample="lanczos")
    assert torch.equal(out["panel"].cpu(), host)
    one = _sequence(full, 1)
    for k in full:
        assert torch.equal(one[k], out[k]), k
    alone = _sequence(("panel",), 2)
    assert set(alone) == {"panel", "trajectory"} and torch.equal(alone["panel"], out["panel"])
    two = _sequence(("panel",), 2, panel=("shaded", "rgb"), panel_resample="bilinear")
    assert torch.equal(two["panel"], frames.compose_panels([out["shaded"], out["rgb"]], size=R, resample="bilinear"))
    # the yaw trajectory starts and ends at the same camera, so two frames are one picture twice: three frames, whose middle
    # one differs, show that every frame's panel sits in its own slice of the block
    three = _sequence(full, 2, n_frames=3)
    assert not torch.equal(three["rgb"][0], three["rgb"][1])
    assert torch.equal(three["panel"], frames.compose_panels([three[k] for k in full[:3]], size=R, resample="lanczos"))
    for k in full:
        assert torch.equal(_sequence(full, 1, n_frames=3)[k], three[k]), k
