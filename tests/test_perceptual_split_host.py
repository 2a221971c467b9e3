"""CPU-only checks of the split-fp16 mode of the VGG16 conv perceptual loss (csrc/vgg_split.hip, perceptual.VGG16ConvLoss(...,
precision="split_fp16")): the C ABI, the size contract, the order the split weights are packed in, and the accuracy of the
split arithmetic itself, restated with torch ops (the GPU numerics are tests/test_gpu_perceptual_split.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _perceptual_cases as PC
from cips_3dplusplus_amd import _lib, perceptual
from cips_3dplusplus_amd.perceptual import VGG16ConvLoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cips3d_vgg_split_supported", "cips3d_vgg_split_range_bytes", "cips3d_vgg_split_pack", "cips3d_vgg_split_features",
       "cips3d_vgg_split_loss_forward", "cips3d_vgg_split_loss_backward")


def test_new_symbols_sizes_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} not declared in the header"
        assert s in _lib.EXPORTED and hasattr(raw, s), s
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 36
    assert ctypes.sizeof(_lib.VggSplitCtx) == lib.cips3d_sizeof_struct(14)
    assert ctypes.sizeof(_lib.VggSplitIO) == lib.cips3d_sizeof_struct(15)
    # the existing structs keep their sizes and ids
    assert ctypes.sizeof(_lib.VggCtx) == lib.cips3d_sizeof_struct(12)
    assert ctypes.sizeof(_lib.VggIO) == lib.cips3d_sizeof_struct(13)
    # one word per (tensor, sample), activations and gradients
    assert lib.cips3d_vgg_split_range_bytes(1) == 2 * 13 * 4 and lib.cips3d_vgg_split_range_bytes(3) == 2 * 13 * 3 * 4
    assert lib.cips3d_vgg_split_range_bytes(0) == -1


def test_size_contract_is_the_exact_mode_s():
    lib = _lib.load()
    for args, want in (((1, 16, 16), 0), ((2, 80, 48), 0), ((1, 8, 8), -2), ((1, 72, 64), -2), ((1, 64, 60), -2),
                       ((0, 16, 16), -1), ((2, 256, 256), 0), ((2, 72, 64), -2)):
        assert lib.cips3d_vgg_split_supported(*args) == lib.cips3d_vgg_supported(*args) == want, args


def test_null_pointers_are_bad_arguments_and_the_size_contract_comes_first():
    lib = _lib.load()
    assert lib.cips3d_vgg_split_pack(None, None, 13, None) == -1
    assert lib.cips3d_vgg_split_features(None, None, None) == -1
    assert lib.cips3d_vgg_split_loss_forward(None, None, None) == -1
    assert lib.cips3d_vgg_split_loss_backward(None, None, None) == -1
    ctx, sio = _lib.VggSplitCtx(), _lib.VggSplitIO()
    assert lib.cips3d_vgg_split_pack(ctypes.byref(ctx), None, 13, None) == -1
    srcs = (ctypes.c_void_p * _lib.VGG_CONVS)()
    assert lib.cips3d_vgg_split_pack(ctypes.byref(ctx), srcs, 14, None) == -1
    assert lib.cips3d_vgg_split_pack(ctypes.byref(ctx), srcs, 2, None) == -1                       # no w_amax, no weights
    calls = (lib.cips3d_vgg_split_features, lib.cips3d_vgg_split_loss_forward, lib.cips3d_vgg_split_loss_backward)
    for call in calls:
        assert call(ctypes.byref(ctx), ctypes.byref(sio), None) == -1                               # io.x is null
    io = sio.io
    io.x, io.B, io.H, io.W, io.n_convs = 64, 1, 16, 16, 14                                          # (never dereferenced)
    for call in calls:
        assert call(ctypes.byref(ctx), ctypes.byref(sio), None) == -1                               # n_convs outside [1, 13]
    io.n_convs, io.H = 2, 24
    for call in calls:
        assert call(ctypes.byref(ctx), ctypes.byref(sio), None) == -2                               # the size contract comes first
    io.H = 16
    for call in calls:
        assert call(ctypes.byref(ctx), ctypes.byref(sio), None) == -1                               # no range words, no weights


def test_precision_is_a_validated_argument():
    net = VGG16ConvLoss("vgg16_conv_random", precision="split_fp16")
    assert net.precision == "split_fp16"
    assert VGG16ConvLoss("vgg16_conv_random").precision == "fp32_exact"
    assert VGG16ConvLoss("vgg16_conv_random", precision="fp32_exact").precision == "fp32_exact"
    for bad in ("fp16", "split", None, 16):
        with pytest.raises(ValueError, match="precision"):
            VGG16ConvLoss("vgg16_conv_random", precision=bad)
    with pytest.raises(RuntimeError, match="GPU"):          # no CPU path in this mode either
        net(torch.zeros(1, 3, 16, 16))


def operand_from_fragments(packed, M, K):
    """W[m][k][tap] (fp64, hi + lo) read back from the fragment order as the kernel's lanes read it: fragment (mt, ks, tap), half,
    lane 16 q + i, element j  ->  m = 16 mt + i, k = 32 ks + 8 q + j."""
    flat = packed.reshape(-1)
    W = np.zeros((M, K, 9))
    for mt in range(M // 16):
        for ks in range(K // 32):
            for tap in range(9):
                base = ((mt * (K // 32) + ks) * 9 + tap) * 2 * 512
                for half in range(2):
                    frag = flat[base + half * 512: base + (half + 1) * 512].astype(np.float64).reshape(4, 16, 8)     # q, i, j
                    for q in range(4):
                        W[mt * 16:(mt + 1) * 16, ks * 32 + 8 * q: ks * 32 + 8 * q + 8, tap] += frag[q]
    return W


def test_packing_order_reproduces_conv2d_and_its_data_gradient():
    g = torch.Generator().manual_seed(11)
    cout, cin = 96, 64                                   # M != K in both forms, several fragments along each
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.037
    w[5, 7, 1, 2] = 1.9                                  # the maximum: 2^0 <= 1.9 < 2^1 -> e = -14
    fwd, bwd, e = perceptual.split_pack_reference(w.numpy())
    assert e == -14 and fwd.dtype == np.float16 and fwd.size == bwd.size == 2 * 9 * cout * cin
    hi_max = np.abs(fwd[:, :, :, 0].astype(np.float64)).max()
    assert 2.0 ** 14 <= hi_max < 2.0 ** 15               # hi lies high in fp16's normal range
    w64 = w.double()
    bound = 2.0 ** -22 * float(w64.abs().max())
    Wf = operand_from_fragments(fwd, cout, cin) * 2.0 ** e                 # [o][c][tap]
    Wb = operand_from_fragments(bwd, cin, cout) * 2.0 ** e                 # [c][o][tap] = w[o][c][8 - tap]
    assert np.abs(Wf - w64.numpy().reshape(cout, cin, 9)).max() <= bound
    assert np.abs(Wb - w64.numpy().reshape(cout, cin, 9)[:, :, ::-1].transpose(1, 0, 2)).max() <= bound
    # as operands of a plain correlation both forms give conv2d and its data gradient
    x = torch.randn(2, cin, 7, 5, generator=g).double().requires_grad_(True)
    out = F.conv2d(x, w64, padding=1)
    gout = torch.randn(out.shape, generator=g).double()
    out.backward(gout)
    got = F.conv2d(x.detach(), torch.from_numpy(Wf).reshape(cout, cin, 3, 3), padding=1)
    assert float((got - out.detach()).abs().max()) <= bound * float(x.detach().abs().sum(dim=1).max()) * 9
    got_g = F.conv2d(gout, torch.from_numpy(Wb).reshape(cin, cout, 3, 3), padding=1)
    assert float((got_g - x.grad).abs().max()) <= bound * float(gout.abs().sum(dim=1).max()) * 9


def flush16(t):
    """fp16 of t with subnormal results flushed to zero, back in fp32."""
    h = t.half().float()
    return torch.where(h.abs() < 2.0 ** -14, torch.zeros_like(h), h)


def split(t, e):
    """(hi, lo) fp32 tensors holding the fp16 halves of t * 2^-e; e broadcastable."""
    s = t * torch.pow(torch.tensor(2.0), -e)
    hi = flush16(s)
    return hi, flush16(s - hi)


def exponent(m):
    """e with m 2^-e in [2^14, 2^15), per element of m."""
    return torch.floor(torch.log2(m.double())).float() - 14


def split_forward(x, ws, layers):
    """The arithmetic of csrc/vgg_split.hip with torch ops in fp32: conv 0 plain; convs 1 .. : operand = relu / pool of the
    pre-ReLU tensor, one power of two per sample from max|z|, one per layer from max|w|, three fp32-accumulated products."""
    want = {f"features_{PC.CONV_INDEX[l]}": l for l in range(13)}
    last = max(want[k] for k in layers)
    h = ((x + 1) / 2 - torch.tensor(PC.MEAN).view(1, 3, 1, 1)) / torch.tensor(PC.STD).view(1, 3, 1, 1)
    z = F.conv2d(h, ws[0][0], ws[0][1], padding=1)
    taps = {"features_0": z} if "features_0" in layers else {}
    for l in range(1, last + 1):
        ex = exponent(z.abs().amax(dim=(1, 2, 3))).view(-1, 1, 1, 1)
        h = F.relu(z)
        if PC.POOL_BEFORE[l]:
            h = F.max_pool2d(h, 2)
        ew = exponent(ws[l][0].abs().max())
        xh, xl = split(h, ex)
        wh, wl = split(ws[l][0], ew)
        acc = F.conv2d(xh, wl, padding=1) + F.conv2d(xl, wh, padding=1) + F.conv2d(xh, wh, padding=1)
        z = acc * torch.pow(torch.tensor(2.0), ex + ew) + ws[l][1].view(1, -1, 1, 1)
        name = f"features_{PC.CONV_INDEX[l]}"
        if name in layers:
            taps[name] = z
    return taps


@pytest.mark.parametrize("name", ["smallest_16x16", "inner_taps_2x32x48"])
def test_split_arithmetic_is_as_accurate_as_fp32(name):
    """The claim the GPU accuracy rule rests on: the split arithmetic errs about as much as torch's fp32 against fp64."""
    c = PC.case(name)
    with torch.no_grad():
        taps = split_forward(c["x"], c["ws"], c["layers"])
    for k in c["layers"]:
        ref64 = c["taps64"][k]
        e_split = float((taps[k].double() - ref64).abs().max())
        e_32 = float((c["taps32"][k].double() - ref64).abs().max())
        print(f"{name} {k}: |split - fp64| {e_split:.3e}  |fp32 - fp64| {e_32:.3e}  ratio {e_split / e_32:.2f}")
        assert e_split <= 2 * e_32, (k, e_split, e_32)
