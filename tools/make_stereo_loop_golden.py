#!/usr/bin/env python3
"""Records what tests/test_gpu_stereo_loop_bits.py compares bit for bit: the outputs of every case of that test for both
stereo solvers, from whatever build of the library is loaded (CALIB_LM_LIBRARY picks another one than the product's).
Run it on the GPU with the build BEFORE a change that must keep the stereo solvers' results:

    python3 tools/make_stereo_loop_golden.py [output directory, default tests/golden/stereo_loop]

Every case runs twice; nothing is written for a case whose two runs differ. One small .npz per case: the small outputs
as arrays, the SHA-256 of each large one, and the SHA-256 of the case's inputs. Nothing but this repository is read."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_stereo_loop_bits as cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN_DIR
    os.makedirs(out, exist_ok=True)
    for case in cases.CASES:
        one, two = cases.packed(cases.runCase(case)), cases.packed(cases.runCase(case))
        if sorted(one) != sorted(two) or any(one[k].tobytes() != two[k].tobytes() for k in one):
            raise SystemExit(f"{cases.caseId(case)}: two runs of the same build differ")
        path = os.path.join(out, cases.caseId(case) + ".npz")
        np.savez_compressed(path, inputs=np.array(cases.inputDigest(case)), **one)
        print(f"{path}: {sorted(one)}, iterations {int(one['iters'].ravel()[0]) if 'iters' in one else '-'}, "
              f"{os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
