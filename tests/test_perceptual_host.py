"""CPU-only checks of the VGG16 conv perceptual loss: C ABI hygiene, the size contract, the torchvision-layout loader and the
module's tables (perceptual.VGG16ConvLoss; the GPU numerics are tests/test_gpu_perceptual.py)."""
import ctypes
import os
import re

import pytest
import torch

import _perceptual_cases as PC
from cips_3dplusplus_amd import _lib, perceptual
from cips_3dplusplus_amd.perceptual import VGG16ConvLoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cips3d_vgg_supported", "cips3d_vgg_channels", "cips3d_vgg_stride", "cips3d_vgg_partial_bytes", "cips3d_vgg_pack",
       "cips3d_vgg_features", "cips3d_vgg_loss_forward", "cips3d_vgg_loss_backward")


def test_new_symbols_and_abi_version():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, header), f"{s} not declared in the header"
        assert s in _lib.EXPORTED and hasattr(raw, s), s
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 35
    assert ctypes.sizeof(_lib.VggCtx) == lib.cips3d_sizeof_struct(12)
    assert ctypes.sizeof(_lib.VggIO) == lib.cips3d_sizeof_struct(13)
    assert int(re.search(r"#define\s+CIPS3D_VGG_CONVS\s+(\d+)", header).group(1)) == _lib.VGG_CONVS == 13
    assert [lib.cips3d_vgg_channels(l) for l in range(13)] == list(perceptual.CHANNELS) == list(PC.CHANNELS)
    assert [lib.cips3d_vgg_stride(l) for l in range(13)] == [1, 1, 2, 2, 4, 4, 4, 8, 8, 8, 16, 16, 16]


def test_size_contract_is_decided_on_the_host():
    lib = _lib.load()
    assert lib.cips3d_vgg_supported(1, 16, 16) == 0
    assert lib.cips3d_vgg_supported(2, 80, 48) == 0
    assert lib.cips3d_vgg_supported(1, 8, 8) == -2            # below 16
    assert lib.cips3d_vgg_supported(1, 72, 64) == -2          # 72 is no multiple of 16
    assert lib.cips3d_vgg_supported(1, 64, 60) == -2
    assert lib.cips3d_vgg_supported(0, 16, 16) == -1
    from cips_3dplusplus_amd import hip
    assert hip.vgg_supported(2, 256, 256) and not hip.vgg_supported(2, 72, 64)
    with pytest.raises(RuntimeError, match="multiples of 16"):
        hip.vgg_check_supported(1, 64, 60)


def test_null_pointers_are_bad_arguments():
    lib = _lib.load()
    assert lib.cips3d_vgg_pack(None, None, 13, None) == -1
    assert lib.cips3d_vgg_features(None, None, None) == -1
    assert lib.cips3d_vgg_loss_forward(None, None, None) == -1
    assert lib.cips3d_vgg_loss_backward(None, None, None) == -1
    ctx, io = _lib.VggCtx(), _lib.VggIO()
    assert lib.cips3d_vgg_pack(ctypes.byref(ctx), None, 13, None) == -1
    assert lib.cips3d_vgg_features(ctypes.byref(ctx), ctypes.byref(io), None) == -1           # io.x is null
    io.x, io.B, io.H, io.W, io.n_convs = 64, 1, 16, 16, 14                                      # (never dereferenced)
    assert lib.cips3d_vgg_features(ctypes.byref(ctx), ctypes.byref(io), None) == -1           # n_convs outside [1, 13]
    io.n_convs, io.H = 2, 24
    assert lib.cips3d_vgg_features(ctypes.byref(ctx), ctypes.byref(io), None) == -2           # the size contract comes first
    io.H = 16
    assert lib.cips3d_vgg_features(ctypes.byref(ctx), ctypes.byref(io), None) == -1           # no weights, no outputs
    assert lib.cips3d_vgg_loss_forward(ctypes.byref(ctx), ctypes.byref(io), None) == -1
    assert lib.cips3d_vgg_loss_backward(ctypes.byref(ctx), ctypes.byref(io), None) == -1


def test_torchvision_layout_loader():
    ws = PC.weights()
    sd = PC.state_dict(ws)
    assert any(k.startswith("classifier.") for k in sd)
    net = VGG16ConvLoss("vgg16_conv", weights=sd)
    for (w, b), (w0, b0) in zip(net.conv_weights(), ws):
        assert torch.equal(w, w0) and torch.equal(b, b0)
    back = net.state_dict_torchvision()
    assert sorted(back) == sorted(k for k in sd if k.startswith("features."))
    assert all(torch.equal(back[k], sd[k]) for k in back)
    missing = {k: v for k, v in sd.items() if k != "features.17.bias"}
    with pytest.raises(KeyError, match="features.17.bias"):
        VGG16ConvLoss("vgg16_conv", weights=missing)
    bad = dict(sd)
    bad["features.5.weight"] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(ValueError, match="features.5.weight"):
        VGG16ConvLoss("vgg16_conv", weights=bad)


def test_loader_reads_a_checkpoint_file(tmp_path):
    sd = PC.state_dict(PC.weights())
    path = tmp_path / "vgg16.pth"
    torch.save(sd, path)
    net = VGG16ConvLoss("vgg16_conv", weights=str(path))
    assert torch.equal(net.conv_weights()[12][0], sd["features.28.weight"])


def test_model_names():
    with pytest.raises(RuntimeError) as e:
        VGG16ConvLoss("vgg16_conv")
    assert "vgg16_conv_random" in str(e.value) and "weights=" in str(e.value)
    with pytest.raises(NotImplementedError):
        VGG16ConvLoss("vgg16_relu")
    with pytest.raises(NotImplementedError):
        VGG16ConvLoss("vgg16_conv_random", use_stat_loss=True)
    with pytest.raises(ValueError):
        VGG16ConvLoss("vgg19_conv")
    a = VGG16ConvLoss("vgg16_conv_random", generator=torch.Generator().manual_seed(5))
    b = VGG16ConvLoss("vgg16_conv_random", generator=torch.Generator().manual_seed(5))
    c = VGG16ConvLoss("vgg16_conv_random", generator=torch.Generator().manual_seed(6))
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a.conv_weights(), b.conv_weights()))
    assert not torch.equal(a.conv_weights()[0][0], c.conv_weights()[0][0])
    # the reference's initialisation: N(0, 2 / fan_out), zero bias
    for (w, bias), cout in zip(a.conv_weights(), perceptual.CHANNELS):
        assert float(bias.abs().max()) == 0.0
        assert abs(float(w.std()) / (2.0 / (9 * cout)) ** 0.5 - 1) < 0.08
    torch.manual_seed(3)
    d = VGG16ConvLoss("vgg16_conv_random")
    torch.manual_seed(3)
    e = VGG16ConvLoss("vgg16_conv_random")
    assert torch.equal(d.conv_weights()[7][0], e.conv_weights()[7][0])


def test_tables_tap_map_and_vector_length():
    net = VGG16ConvLoss("vgg16_conv_random")
    assert net.layers == ["features_2", "features_7", "features_14", "features_21", "features_28"]
    assert net.loss_w_dict == net.loss_weight("vgg16_conv_1024") == PC.W_1024
    assert net.loss_weight("vgg16_conv_256")["features_7"] == 0.0006
    assert net.loss_weight("vgg16_relu_1024")["features_28"] == 0.007
    assert net.loss_weight("vgg16_relu_256")["features_21"] == 0.002
    assert perceptual.TAP_CONV == {f"features_{n}": l for l, n in enumerate(PC.CONV_INDEX)}
    assert [perceptual.TAP_CONV[k] for k in net.layers] == [1, 3, 6, 9, 12] and net.n_convs == 13
    # 64 S^2 + 128 (S/2)^2 + 256 (S/4)^2 + 512 (S/8)^2 + 512 (S/16)^2 = 122 S^2
    assert perceptual.feature_length(256, 256, net.layers) == 122 * 256 * 256 == 7995392
    assert perceptual.feature_length(64, 64, net.layers) == 122 * 64 * 64 == 499712
    short = VGG16ConvLoss("vgg16_conv_random", layers=["features_2", "features_7"], loss_w_dict={"features_2": 1.0, "features_7": 2.0})
    assert short.n_convs == 4 and short.layers == ["features_2", "features_7"] and short.loss_w_dict["features_7"] == 2.0
    assert perceptual.feature_length(128, 128, short.layers) == 64 * 128 * 128 + 128 * 64 * 64
    with pytest.raises(ValueError):
        VGG16ConvLoss("vgg16_conv_random", layers=["features_3"])
    # no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        net(torch.zeros(1, 3, 16, 16))


def test_oracle_matches_an_nn_sequential_vgg16():
    """The functional oracle of the GPU tests against the module form the reference builds (vgg_per_loss.py:93-110)."""
    from torch import nn
    ws = PC.weights()
    layers, l = [], 0
    for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512):
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            conv = nn.Conv2d(ws[l][0].shape[1], v, kernel_size=3, padding=1)
            conv.weight.data.copy_(ws[l][0]); conv.bias.data.copy_(ws[l][1])
            layers += [conv, nn.ReLU(inplace=False)]
            l += 1
    seq = nn.Sequential(*layers)
    assert [i for i, m in enumerate(seq) if isinstance(m, nn.Conv2d)] == list(PC.CONV_INDEX)
    x = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1
    h = ((x + 1) / 2 - torch.tensor(PC.MEAN).view(1, 3, 1, 1)) / torch.tensor(PC.STD).view(1, 3, 1, 1)
    taps = PC.oracle_taps(x, ws, PC.DEFAULT_LAYERS, torch.float32)
    with torch.no_grad():
        for i, m in enumerate(seq):
            h = m(h)
            if f"features_{i}" in taps:
                assert torch.allclose(h, taps[f"features_{i}"], rtol=0, atol=1e-5 * float(h.abs().max()))
