"""Every compiled form of chain_gemm_kernel (csrc/chain.hip, the chain_forms table) against stored bits.

The exits of the chain GEMM (planes, planes16, fp32 and bf16 NCHW), its epilogue, the folded ToRGB, the range tracking and the
riding fold are template arguments of the kernel: a launch runs the instantiation compiled for exactly what it does, or the generic
one that decides at run time.  None of that may change a bit.  tests/golden/chain_exits/<case>.npz holds what ONE launch of the
library of the commit in front of that change -- one body, every branch at run time, addresses rebuilt per wave -- wrote for the
seeded inputs of tests/_chain_exit_cases.py: the output (planes or NCHW), out_exp, out_pmax, the rgb_part slots, the amax slots and
the riding fold's image, as sha256 of the bytes plus the bytes themselves (large arrays: a strided sample, to locate a mismatch).
tests/golden/chain_exits/make_chain_exits.py regenerates them from a library given by path.

Cases: B = 1 and 2; Cin, Cout in {64, 128} and 256 -> 512; HW = 128 (one pixel block), 192 (a ragged second block) and 64^2 for the one
shape inside the half-chip window (both tiles, the hint on and off: eight ToRGB slots of four 16-row tiles); the hint outside its
window; each exit with and without the epilogue, the fold and the range workspace; shared, per-sample and no noise; with and
without patch maxima of the input.  Each case launches twice; both launches equal the fixture.
Refusals: a launch no row of the table takes returns CIPS3D_E_UNSUPP and writes nothing.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from cips_3dplusplus_amd import _lib, hip

import _chain_exit_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_exits")
E_UNSUPP = -2                                     # CIPS3D_E_UNSUPP (include/cips3d_hip.h)


@pytest.mark.parametrize("case", EC.CASES, ids=EC.IDS)
def test_chain_exit_equals_the_stored_bits(case):
    fx = np.load(os.path.join(GOLDEN, case.id + ".npz"))
    t = EC.inputs(case)
    assert bytes(fx["inputs.sha256"]).hex() == EC.inputs_digest(t), "the seeded inputs are not the ones the fixture was made from"
    names = sorted(k[:-len(".sha256")] for k in fx.files if k.endswith(".sha256") and k != "inputs.sha256")
    for call in range(2):
        res = EC.run(case, t, hip, DEV)
        torch.cuda.synchronize()
        assert sorted(res) == names, (sorted(res), names)
        for k in names:
            got = EC.raw_bytes(res[k])
            assert got.size == int(fx[f"{k}.nbytes"]), f"{k}: {got.size} bytes, fixture {int(fx[f'{k}.nbytes'])}"
            if hashlib.sha256(got.tobytes()).digest() == bytes(fx[f"{k}.sha256"]):
                continue
            # locate it: the first differing 32-bit word of what the fixture kept
            if f"{k}.bytes" in fx.files:
                want, have, step = fx[f"{k}.bytes"].view(np.uint32), got.view(np.uint32), 1
            else:
                want, have, step = fx[f"{k}.sample"], got.view(np.uint32)[::EC.SAMPLE_STEP], EC.SAMPLE_STEP
            bad = np.nonzero(want != have)[0]
            where = (f"{bad.size} of {want.size} kept words differ, the first at word {int(bad[0]) * step}: "
                     f"{int(have[bad[0]]):#010x} for {int(want[bad[0]]):#010x}") if bad.size else "outside the kept sample"
            pytest.fail(f"{case.id} ({case.form}), call {call}: {k} differs from the fixture -- {where}")


def _raw_args(B, Cin, Cout, HW):
    x = torch.zeros(B, Cin // 8, 2, HW, 8, device=DEV, dtype=torch.float16)
    w = torch.zeros(B * Cout * Cin, device=DEV)
    o = torch.full((B, Cout, HW), -77.5, device=DEV)
    return x, w, o


def test_a_launch_outside_the_table_is_unsupported_and_enqueues_nothing():
    """What no row of chain_forms takes: a riding fold on the planes16 kernel (no CF_RIDE row, and its generic row has no riding
    branch), and patch maxima of more than 512 input channels under a tracked planes exit (one load per wave holds 64 entries).  The
    generic rows take every other combination the entry points accepted before the exits were compiled apart."""
    lib = _lib.load()
    B, Cin, Cout, HW = 1, 64, 64, 128
    x, w, o = _raw_args(B, Cin, Cout, HW)
    part, rout = torch.zeros(1, 1, 3, 64, device=DEV), torch.full((1, 3, 64), -77.5, device=DEV)
    job = _lib.ReduceJob()
    job.part, job.out = part.data_ptr(), rout.data_ptr()
    job.n4, job.HW4, job.slot_stride, job.n_slots, job.n_bias = 48, 16, 192, 1, 0
    rg = _lib.Range()
    rg.ride = C.addressof(job)
    rc = lib.cips3d_modconv1x1_planes16(x.data_ptr(), w.data_ptr(), o.data_ptr(), 0, B, Cin, Cout, HW, 0, None, 0, None, None, None,
                                        None, None, C.byref(rg), hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E_UNSUPP
    assert bool((o == -77.5).all()) and bool((rout == -77.5).all()), "a refused launch wrote something"
    # the same job rides on the split kernel: the launch form exists there
    exps = torch.zeros(B, 1, device=DEV, dtype=torch.int32)
    rg2, _k = hip._range(x_exp=exps)
    rg2.ride = C.addressof(job)
    rc = lib.cips3d_modconv1x1_planes(x.data_ptr(), w.data_ptr(), o.data_ptr(), 0, B, Cin, Cout, HW, 0, None, 0, None, None, None,
                                      None, None, C.byref(rg2), hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool((o == 0).all()) and bool((rout == 0).all())
    # tracked planes out of 576 channels with patch maxima
    x, w, o = _raw_args(1, 576, 64, 128)
    op = torch.full((1, 8, 2, 128, 8), -77.5, device=DEV, dtype=torch.float16)
    pmax, lconst = torch.ones(1, 2, 36, device=DEV), torch.ones(1, 4, device=DEV)
    oexp = torch.full((1, 1), -12345, device=DEV, dtype=torch.int32)
    rg3, _k3 = hip._range(x_exp=exps, x_pmax=pmax, lconst=lconst, out_exp=oexp)
    rc = lib.cips3d_modconv1x1_planes(x.data_ptr(), w.data_ptr(), op.data_ptr(), 1, 1, 576, 64, 128, 0, None, 0, None, None, None,
                                      None, None, C.byref(rg3), hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E_UNSUPP
    assert bool((op == -77.5).all()) and int(oexp[0, 0]) == -12345, "a refused launch wrote something"
