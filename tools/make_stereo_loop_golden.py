#!/usr/bin/env python3
"""Records what a bit test of the solvers on the shared LM loop compares: the outputs of every case of
tests/test_gpu_stereo_loop_bits.py (both stereo solvers, the default) or of tests/test_gpu_rig_loop_bits.py (both rig
solvers), from whatever build of the library is loaded (CALIB_LM_LIBRARY picks another one than the product's). Run it
on the GPU with the build BEFORE a change that must keep the solvers' results:

    python3 tools/make_stereo_loop_golden.py [cases module, default test_gpu_stereo_loop_bits] [output directory,
                                              default the module's GOLDEN_DIR]

Every case runs twice; nothing is written for a case whose two runs differ, or that ends singular. One small .npz per
case: the small outputs as arrays, the SHA-256 of each large one, and the SHA-256 of the case's inputs. Nothing but this
repository is read."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    cases = importlib.import_module(sys.argv[1] if len(sys.argv) > 1 else "test_gpu_stereo_loop_bits")
    out = sys.argv[2] if len(sys.argv) > 2 else cases.GOLDEN_DIR
    os.makedirs(out, exist_ok=True)
    refused = []
    for case in cases.CASES:
        one, two = cases.packed(cases.runCase(case)), cases.packed(cases.runCase(case))
        if sorted(one) != sorted(two) or any(one[k].tobytes() != two[k].tobytes() for k in one):
            raise SystemExit(f"{cases.caseId(case)}: two runs of the same build differ")
        if any(k.startswith("singular") for k in one):
            refused.append(cases.caseId(case))
            print(f"{cases.caseId(case)}: {sorted(one)}: a singular call records nothing to compare", flush=True)
            continue
        path = os.path.join(out, cases.caseId(case) + ".npz")
        np.savez_compressed(path, inputs=np.array(cases.inputDigest(case)), **one)
        print(f"{path}: {sorted(one)}, iterations {int(one['iters'].ravel()[0]) if 'iters' in one else '-'}, "
              f"{os.path.getsize(path)} bytes", flush=True)
    if refused:
        raise SystemExit(f"not recorded: {refused}")


if __name__ == "__main__":
    main()
