"""Host checks of LPIPS (cips_3dplusplus_amd/perceptual.py, csrc/lpips.hip): the C ABI's declarations, struct sizes and the
argument checks that are decided on the host, the constructor's errors, the parsing of the lpips package's lin weights, and the
errors of CPU tensors and unsupported sizes.  Nothing here launches a kernel."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import _lpips_cases as LC
import _perceptual_cases as PC
from cips_3dplusplus_amd import _lib, perceptual as PP, projector as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cips3d_lpips_head", "cips3d_lpips", "cips3d_lpips_split", "cips3d_lpips_supported",
                "cips3d_lpips_partial_bytes")


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in _lib.EXPORTED and s in _lib._SIGS and hasattr(raw, s), s
    m = re.search(r"#define\s+CIPS3D_ABI_VERSION\s+(\d+)", header)
    assert lib.cips3d_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 39
    build = __import__("cips_3dplusplus_amd.build", fromlist=["SOURCES"])
    assert "lpips.hip" in build.SOURCES and "-fno-slp-vectorize" in build.FILE_FLAGS["lpips.hip"]


def test_struct_sizes_agree():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.LpipsIO) == lib.cips3d_sizeof_struct(16)
    assert _lib._struct_table()[16] is _lib.LpipsIO
    assert int(re.search(r"#define\s+CIPS3D_LPIPS_LAYERS\s+(\d+)",
                         open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()).group(1)) == _lib.LPIPS_LAYERS == 5


def test_size_contract_and_scratch():
    lib = _lib.load()
    sup = lib.cips3d_lpips_supported
    assert sup(1, 16, 16) == 0 and sup(3, 80, 48) == 0 and sup(1, 1024, 1024) == 0
    assert sup(1, 24, 16) == -2 and sup(1, 16, 24) == -2 and sup(1, 8, 8) == -2
    assert sup(0, 16, 16) == -1 and sup(1, 0, 16) == -1 and sup(1, 16, -16) == -1
    pb = lib.cips3d_lpips_partial_bytes
    assert pb(1) > 0 and pb(1) % 8 == 0 and pb(3) == 3 * pb(1) and pb(0) == -1


def _aligned(buf):
    return (ctypes.addressof(buf) + 255) // 256 * 256


def test_head_argument_errors_do_not_launch():
    f = _lib.load().cips3d_lpips_head
    buf = (ctypes.c_uint8 * 4096)()
    p = _aligned(buf)                                      # (host memory: a launch would fault, the checks come first)
    assert f(None, p, p, 1, 64, 1, 1, None, p, p, None) == -1
    assert f(p, None, p, 1, 64, 1, 1, None, p, p, None) == -1
    assert f(p, p, None, 1, 64, 1, 1, None, p, p, None) == -1
    assert f(p, p, p, 1, 64, 1, 1, None, None, p, None) == -1
    assert f(p, p, p, 1, 64, 1, 1, None, p, None, None) == -1
    assert f(p, p, p, 0, 64, 1, 1, None, p, p, None) == -1
    assert f(p, p, p, 1, 64, 0, 1, None, p, p, None) == -1
    for C in (0, 3, 32, 96, 1024):
        assert f(p, p, p, 1, C, 1, 1, None, p, p, None) == -1, C
    assert f(p, p, p, 1, 64, 65536, 65536, None, p, p, None) == -2


def _vgg_io(B, H, W, p, n_convs=13):
    io = _lib.VggIO()
    io.x, io.B, io.H, io.W, io.n_convs, io.normalize = p, B, H, W, n_convs, 1
    return io


def _lpips_io(trunk, B, p, row=0, targets=0):
    lio = _lib.LpipsIO()
    lio.trunk = ctypes.addressof(trunk) if trunk is not None else None
    for k in range(5):
        lio.lin[k] = p
        if k < targets:
            lio.target[k] = p
    lio.partial, lio.record, lio.row, lio.B = p, p, row, B
    return lio


@pytest.mark.parametrize("split", (False, True))
def test_whole_metric_argument_errors_do_not_launch(split):
    lib = _lib.load()
    f = lib.cips3d_lpips_split if split else lib.cips3d_lpips
    buf = (ctypes.c_uint8 * 4096)()
    p = _aligned(buf)
    ctx = (_lib.VggSplitCtx if split else _lib.VggCtx)()

    def trunk(B, H, W, n_convs=13):
        io = _vgg_io(B, H, W, p, n_convs)
        if not split:
            return io
        sio = _lib.VggSplitIO()
        ctypes.memmove(ctypes.addressof(sio), ctypes.addressof(io), ctypes.sizeof(io))
        return sio

    def call(lio, ctx_=ctx):
        return f(ctypes.byref(ctx_) if ctx_ is not None else None, ctypes.byref(lio) if lio is not None else None, None)

    t = trunk(2, 16, 16)
    assert call(None) == -1 and call(_lpips_io(t, 1, p), None) == -1
    assert call(_lpips_io(None, 1, p)) == -1                               # no trunk io
    assert call(_lpips_io(t, 0, p)) == -1                                  # B < 1
    assert call(_lpips_io(t, 1, p, row=-1)) == -1                          # a negative row
    assert call(_lpips_io(t, 2, p)) == -1                                  # the pair form needs a trunk batch of 2 B
    assert call(_lpips_io(t, 1, p, targets=3)) == -1                       # some but not all targets
    assert call(_lpips_io(t, 1, p, targets=5)) == -1                       # the prepared form needs a trunk batch of B
    assert call(_lpips_io(trunk(2, 16, 16, n_convs=12), 1, p)) == -1       # the trunk cut short of relu5_3
    for field in ("partial", "record"):
        lio = _lpips_io(t, 1, p)
        setattr(lio, field, None)
        assert call(lio) == -1, field
    lio = _lpips_io(t, 1, p)
    lio.lin[4] = None
    assert call(lio) == -1
    assert call(_lpips_io(trunk(2, 24, 16), 1, p)) == -2                   # outside the size contract
    assert call(_lpips_io(trunk(2, 16, 40), 1, p)) == -2
    # everything of the head is in order, the trunk's own io is not (no z buffers): its check answers, nothing launched
    assert call(_lpips_io(t, 1, p)) == -1
    lio = _lpips_io(t, 1, p)
    lio.heads_only = 1                                                     # the heads alone need the maps that are not there
    assert call(lio) == -1


def test_constructor_errors():
    ws, lins = PC.weights(), LC.lin_weights()
    sd, lsd = PC.state_dict(ws), LC.lin_state_dict(lins)
    with pytest.raises(RuntimeError, match="lin_weights="):
        PP.LPIPS("vgg")
    with pytest.raises(RuntimeError, match="vgg16 checkpoint"):
        PP.LPIPS("vgg", lin_weights=lsd)
    with pytest.raises(RuntimeError, match="vgg.pth"):
        PP.LPIPS("vgg", weights=sd)
    for name in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError, match=name):
            PP.LPIPS(name)
    with pytest.raises(ValueError, match="net must be"):
        PP.LPIPS("resnet")
    with pytest.raises(ValueError, match="precision"):
        PP.LPIPS("vgg_random", precision="bf16")
    missing = {k: v for k, v in lsd.items() if k != "lin3.model.1.weight"}
    with pytest.raises(KeyError, match="lin3.model.1.weight"):
        PP.LPIPS("vgg", weights=sd, lin_weights=missing)
    wrong = dict(lsd)
    wrong["lin2.model.1.weight"] = torch.zeros(1, 128, 1, 1)
    with pytest.raises(ValueError, match="lin2.model.1.weight"):
        PP.LPIPS("vgg", weights=sd, lin_weights=wrong)
    sig = inspect.signature(PP.LPIPS.__init__).parameters
    assert [n for n in sig][1:] == ["net", "weights", "lin_weights", "generator", "precision"]
    assert sig["net"].default == "vgg" and sig["precision"].default == "fp32_exact"


def test_lin_parsing_ignores_extra_keys_and_keeps_the_values(tmp_path):
    ws, lins = PC.weights(), LC.lin_weights()
    lsd = LC.lin_state_dict(lins)
    assert set(lsd) - {f"lin{k}.model.1.weight" for k in range(5)}         # (the fixture does carry extra keys)
    net = PP.LPIPS("vgg", weights=PC.state_dict(ws), lin_weights=lsd, precision="split_fp16")
    assert net.precision == net.trunk.precision == "split_fp16" and net.trunk.n_convs == 13
    for w, ref, c in zip(net.lin_weights(), lins, PP.LPIPS_CHANNELS):
        assert tuple(w.shape) == (c,) and torch.equal(w, ref)
    for (w, b), (rw, rb) in zip(net.trunk.conv_weights(), ws):
        assert torch.equal(w, rw) and torch.equal(b, rb)
    path = tmp_path / "vgg_lin.pth"                                        # a path works like a dict
    torch.save(lsd, path)
    net2 = PP.LPIPS("vgg", weights=PC.state_dict(ws), lin_weights=str(path))
    assert all(torch.equal(a, b) for a, b in zip(net2.lin_weights(), lins))
    rnd = PP.LPIPS("vgg_random", generator=torch.Generator().manual_seed(1))
    assert all(bool((w >= 0).all()) and tuple(w.shape) == (c,) for w, c in zip(rnd.lin_weights(), PP.LPIPS_CHANNELS))
    assert PP.LPIPS_CONVS == LC.LPIPS_CONVS and PP.LPIPS_CHANNELS == LC.CHANNELS


def test_cpu_tensors_and_bad_sizes_raise():
    net = PP.LPIPS("vgg_random", generator=torch.Generator().manual_seed(1))
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(x, x)
    with pytest.raises(RuntimeError, match="GPU only"):
        net.prepare(x)
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(3, 16, 16, dtype=torch.uint8), x)
    with pytest.raises(RuntimeError, match="GPU only"):
        PP.LPIPSLog(net, x, 4)
    with pytest.raises(ValueError, match="multiples of 16"):
        net(torch.zeros(1, 3, 24, 16), torch.zeros(1, 3, 24, 16))
    with pytest.raises(ValueError, match="multiples of 16"):
        net.prepare(torch.zeros(3, 16, 24))
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        net(torch.zeros(1, 1, 16, 16), x)
    with pytest.raises(ValueError, match="float32"):
        net(x.double(), x)
    with pytest.raises(ValueError, match="one image"):
        PP.LPIPSLog(net, torch.zeros(2, 3, 16, 16), 4)
    with pytest.raises(ValueError, match="capacity"):
        PP.LPIPSLog(net, x, 0)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        PP.lpips_layer_distance(torch.zeros(1, 64, 2, 2), torch.zeros(1, 64, 2, 2), torch.zeros(64))
    with pytest.raises(ValueError, match="one shape"):
        PP.lpips_layer_distance(torch.zeros(1, 64, 2, 2), torch.zeros(1, 64, 2, 3), torch.zeros(64))


def test_project_wplus_has_the_reference_keyword():
    sig = inspect.signature(P.FlipProjector.project_wplus).parameters
    assert sig["lpips_metric"].default is None
    proj = P.FlipProjector(G=None, device="cpu")                           # (raises before the generator is touched)
    net = PP.LPIPS("vgg_random", generator=torch.Generator().manual_seed(1))
    with pytest.raises(ValueError, match="lpips_metric needs target_images"):
        proj.project_wplus({"img_size": 8}, {}, lambda rgb, thumb: rgb.sum(), N_steps_pose=1, lpips_metric=net)
    with pytest.raises(ValueError, match="perceptual.LPIPS instance"):
        proj.project_wplus({"img_size": 8}, {}, lambda rgb, thumb: rgb.sum(), N_steps_pose=1, lpips_metric=object(),
                           target_images=torch.zeros(1, 3, 16, 16))
