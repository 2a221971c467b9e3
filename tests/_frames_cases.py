"""The case list of the frame-resampling tests, shared by the host tests (against Pillow and the committed fixture) and the GPU
tests (against the host mirror).  A case is (name, (H, W), (oh, ow)); `image(name, H, W, C)` is its uint8 input."""
import numpy as np

FILTERS = ("box", "bilinear", "bicubic", "lanczos")

# small shapes: both lists below and the committed fixture (tests/golden/frames_resize.npz) use them
SMALL = [
    ("one_pixel", (1, 1), (5, 3)),                 # every bound clamps
    ("checker3", (3, 3), (64, 64)),                # 0 / 255 checker: over- and undershoot reach both ends of the clamp
    ("odd_up", (7, 5), (13, 17)),
    ("odd_down", (33, 47), (8, 9)),
    ("mixed", (100, 80), (37, 64)),                # one axis up, one down
    ("rows_only", (40, 64), (80, 64)),             # the horizontal pass is skipped
    ("cols_only", (64, 40), (64, 80)),             # the vertical pass is skipped
    ("thumb_ratio", (16, 16), (256, 256)),         # the thumbnail's ratio of 16, reduced
    ("down4", (64, 64), (16, 16)),
    ("tall_down", (257, 3), (2, 3)),               # more input rows under one output row than the fused route stages
    ("same", (9, 11), (9, 11)),                    # nothing to filter
    ("zeros", (12, 10), (31, 29)),
    ("ones", (12, 10), (5, 23)),
]
# the shapes the issue's definition was checked on against Pillow (host test only: the large ones take the host a while)
PILLOW_ONLY = [
    ("thumb_1024", (64, 64), (1024, 1024)),
    ("shaded_1024", (512, 512), (1024, 1024)),
    ("preview_256", (1024, 1024), (256, 256)),
    ("up_64_256", (64, 64), (256, 256)),
    ("down_256_64", (256, 256), (64, 64)),
    ("photo_224", (1000, 700), (224, 224)),
]


def image(name, H, W, C=3, n=1):
    """The case's input, [n, C, H, W] uint8: deterministic, from the name."""
    if name == "checker3" or name.startswith("checker"):
        yy, xx = np.mgrid[0:H, 0:W]
        a = (((yy + xx) % 2) * 255).astype(np.uint8)
        return np.ascontiguousarray(np.broadcast_to(a, (n, C, H, W)))
    if name == "zeros":
        return np.zeros((n, C, H, W), np.uint8)
    if name == "ones":
        return np.full((n, C, H, W), 255, np.uint8)
    seed = sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, C, H, W), dtype=np.uint8)


def pillow_resize(a, size, resample):
    """[n, C, H, W] uint8 -> Pillow's resize of every channel (mode 'L'), the definition itself."""
    from PIL import Image
    flt = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[resample]
    oh, ow = size
    out = np.empty(a.shape[:2] + (oh, ow), np.uint8)
    for i in range(a.shape[0]):
        for c in range(a.shape[1]):
            out[i, c] = np.asarray(Image.fromarray(a[i, c], "L").resize((ow, oh), flt))
    return out
