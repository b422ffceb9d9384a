#!/usr/bin/env python3
"""Records what tests/test_gpu_stream_trim.py compares bit for bit: P, sse and the trace of lmBegin / lmRun(3) / lmEnd of
every case of that test, from whatever build of the library is loaded (CALIB_LM_LIBRARY picks another one than the
product's). Run it on the GPU with the build BEFORE a change that must keep the stream kernel's results:

    python3 tools/make_stream_trim_golden.py [output directory, default tests/golden/stream_trim]

One small .npz per case: sse, P, trace, and the SHA-256 of the case's inputs (so that a test failure says whether the
shard or the kernel changed). Nothing but this repository is read."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_stream_trim as cases  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN_DIR
    os.makedirs(out, exist_ok=True)
    for key in [k for k in os.environ if k.startswith("CALIB_") and k != "CALIB_LM_LIBRARY"]:
        del os.environ[key]
    for case in cases.CASES:
        sh = cases.makeCaseShard(case)
        sse, P, trace = cases.runCase(case, sh)
        sse2, P2, trace2 = cases.runCase(case, sh)
        if sse.tobytes() != sse2.tobytes() or P.tobytes() != P2.tobytes() or trace.tobytes() != trace2.tobytes():
            raise SystemExit(f"{cases.caseId(case)}: two runs of the same build differ")
        path = os.path.join(out, cases.caseId(case) + ".npz")
        np.savez_compressed(path, sse=sse, P=P, trace=trace, inputs=np.array(cases.inputDigest(sh)))
        print(f"{path}: {trace.shape[0]} iterations, sse {float(sse):.9e}, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
