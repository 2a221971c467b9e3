"""Regenerates the fixtures of tests/test_gpu_fused_stage_bits.py: one <case id>.npz per case of tests/_fused_stage_bits_cases.py,
holding what ONE launch of the given library wrote for the case's seeded inputs (needs a GPU).

    python tests/golden/fused_stage_bits/make_fused_stage_bits.py PATH/TO/libcips3d_hip.so [OUT_DIR]

The committed files come from the library of the commit in front of the one that compiled the features of fused_up_conv_kernel
apart and moved its addressing to uniform bases: they pin that change, and every later one, to the bits the single
run-time-branching kernel produced.  The library is loaded as it is (no staleness check, no rebuild) through the Python binding of
the tree this script stands in, so it has to export that tree's C ABI; for a library of an older ABI (the committed fixtures: ABI
45) run the script from a checkout of that library's commit, with this file, tests/_fused_stage_bits_cases.py and
tests/_fused_stage_cases.py copied in.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    lib_path = os.path.abspath(sys.argv[1])
    out_dir = sys.argv[2] if len(sys.argv) > 2 else HERE
    from cips_3dplusplus_amd import _lib, build
    _lib.LIB_PATH = lib_path
    build.up_to_date = lambda: True               # load the given file as it is
    from cips_3dplusplus_amd import hip
    import _fused_stage_bits_cases as BC
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for case in BC.CASES:
        t = BC.inputs(case)
        first = {k: BC.raw_bytes(v).copy() for k, v in BC.run(case, t, hip, _lib).items()}
        again = {k: BC.raw_bytes(v) for k, v in BC.run(case, t, hip, _lib).items()}
        for k in first:
            assert np.array_equal(first[k], again[k]), f"{case.id}: {k} differs between two launches of the same library"
        fx = BC.record({k: torch.from_numpy(v) for k, v in first.items()})
        fx["inputs.sha256"] = np.frombuffer(bytes.fromhex(BC.inputs_digest(t)), dtype=np.uint8)
        path = os.path.join(out_dir, case.id + ".npz")
        np.savez_compressed(path, **fx)
        total += os.path.getsize(path)
        print(f"{case.id:64s} {os.path.getsize(path):8d} bytes  {sorted(k for k in first)}  {case.form}")
    print(f"{len(BC.CASES)} fixtures, {total} bytes, library {lib_path}")


if __name__ == "__main__":
    main()
