"""Regenerates the fixtures of tests/test_gpu_chain_exits.py: one <case id>.npz per case of tests/_chain_exit_cases.py, holding what
ONE launch of the given library wrote for the case's seeded inputs (needs a GPU).

    python tests/golden/chain_exits/make_chain_exits.py PATH/TO/libcips3d_hip.so [OUT_DIR]

The committed files come from the library of the commit in front of the one that compiled the exits of chain_gemm_kernel apart:
they pin that change, and every later one, to the bits the single run-time-branching kernel produced.  The library is loaded as it
is (no staleness check, no rebuild), so a library of another commit can be given; it has to export today's C ABI.
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
    import _chain_exit_cases as EC
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for case in EC.CASES:
        t = EC.inputs(case)
        first = {k: EC.raw_bytes(v).copy() for k, v in EC.run(case, t, hip).items()}
        again = {k: EC.raw_bytes(v) for k, v in EC.run(case, t, hip).items()}
        torch.cuda.synchronize()
        for k in first:
            assert np.array_equal(first[k], again[k]), f"{case.id}: {k} differs between two launches of the same library"
        fx = EC.record({k: torch.from_numpy(v) for k, v in first.items()})
        fx["inputs.sha256"] = np.frombuffer(bytes.fromhex(EC.inputs_digest(t)), dtype=np.uint8)
        path = os.path.join(out_dir, case.id + ".npz")
        np.savez_compressed(path, **fx)
        total += os.path.getsize(path)
        print(f"{case.id:64s} {os.path.getsize(path):8d} bytes  {sorted(k for k in first)}")
    print(f"{len(EC.CASES)} fixtures, {total} bytes, library {lib_path}")


if __name__ == "__main__":
    main()
