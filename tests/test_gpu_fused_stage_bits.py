"""Every compiled form of fused_up_conv_kernel (csrc/fused_stage.hip, the stage_forms table) against stored bits.

What a launch of the fused decoder stage does -- both noise maps, ToRGB, the kind of skip image, the out2 store, range tracking,
max |y_next| measured or bounded, the uint8 image -- is a template argument of the kernel: a launch runs the instantiation compiled
for exactly that, or the generic one of its base shape that decides at run time; the tile index comes from a launcher-supplied
shift or reciprocal and every address is a uniform base plus a 32-bit lane offset.  None of that may change a bit.
tests/golden/fused_stage_bits/<case>.npz holds what ONE launch of the library of the commit in front of that change -- one body,
every feature a run-time branch, a division and 64-bit addresses per lane -- wrote for the seeded inputs of
tests/_fused_stage_bits_cases.py: out2, rgb (fp32 or uint8), y_next (fp32 or bf16) and the next_amax array, as sha256 of the bytes
plus the bytes themselves (large arrays: a strided sample, to locate a mismatch), and the digest of the inputs.
tests/golden/fused_stage_bits/make_fused_stage_bits.py regenerates them from a library given by path.

Cases: those of tests/_fused_stage_cases.py (CASES in fp32, bf16, bf16 storage, split with and without the range workspace;
YB_CASES; U8_CASES with the uint8 image) -- which the generic forms take, apart from a few -- and the feature set of every row of
stage_forms, each where tiles_x is a power of two and where it is not (B = 2, sample 0 at 2^9 times sample 1, per-sample noise).
Each case launches twice; both launches equal the fixture.  Every launch the entry points accept has a form (the generic rows
decide at run time), so there is no refusal of the table's own to check; what the entry points refuse is in
tests/test_gpu_fused_stage.py.
"""
import hashlib
import os

import numpy as np
import pytest

from cips_3dplusplus_amd import _lib, hip

import _fused_stage_bits_cases as BC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_stage_bits")


@pytest.mark.parametrize("case", BC.CASES, ids=BC.IDS)
def test_fused_stage_equals_the_stored_bits(case):
    fx = np.load(os.path.join(GOLDEN, case.id + ".npz"))
    t = BC.inputs(case)
    assert bytes(fx["inputs.sha256"]).hex() == BC.inputs_digest(t), "the seeded inputs are not the ones the fixture was made from"
    names = sorted(k[:-len(".sha256")] for k in fx.files if k.endswith(".sha256") and k != "inputs.sha256")
    for call in range(2):
        res = BC.run(case, t, hip, _lib)
        assert sorted(res) == names, (sorted(res), names)
        for k in names:
            got = BC.raw_bytes(res[k])
            assert got.size == int(fx[f"{k}.nbytes"]), f"{k}: {got.size} bytes, fixture {int(fx[f'{k}.nbytes'])}"
            if hashlib.sha256(got.tobytes()).digest() == bytes(fx[f"{k}.sha256"]):
                continue
            # locate it: the first differing 32-bit word of what the fixture kept
            if f"{k}.bytes" in fx.files:
                want, have, step = fx[f"{k}.bytes"].view(np.uint32), got.view(np.uint32), 1
            else:
                step = BC.sample_step(got.size)
                want, have = fx[f"{k}.sample"], got.view(np.uint32)[::step]
            bad = np.nonzero(want != have)[0]
            where = (f"{bad.size} of {want.size} kept words differ, the first at word {int(bad[0]) * step}: "
                     f"{int(have[bad[0]]):#010x} for {int(want[bad[0]]):#010x}") if bad.size else "outside the kept sample"
            pytest.fail(f"{case.id} ({case.form}), call {call}: {k} differs from the fixture -- {where}")


def test_the_rows_cover_both_forms_of_the_tile_division():
    """every launch the rows of stage_forms are compiled for runs where tiles_x is a power of two (a shift) and where it is not (the
    reciprocal)"""
    seen = {}
    for c in BC.ROWS:
        seen.setdefault((c.form, c.run), set()).add(BC.tiles_x(c) & (BC.tiles_x(c) - 1) == 0)
    assert len(seen) == 36 and all(v == {True, False} for v in seen.values()), seen
