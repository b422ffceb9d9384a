#!/usr/bin/env python3
"""Wall time of one refine call of each solver on the shared LM loop (refineStereo, refineStereoJoint, refineRig,
refineRigJoint): what the host side of a handle-less call costs -- checks, uploads, launches, read-backs -- on top of its
kernels.

    python tools/time_solver_front.py [--views 17] [--iters 20] [--warmup 5] [--calls 21]

The problem is tools/time_rig.py's (200 points per camera and view, radtan throughout, pixel noise 0.1) with two cameras
for the stereo solvers and four for the rig solvers; the joint solvers start from the cameras the others hold fixed. A
call runs --iters iterations under a stop rule that never fires and ends in a device-to-host copy, so the host clock
around it is a synchronised time. Per solver: --warmup calls, then the median of --calls calls. One JSON line; to compare
two trees, run each tree's copy of this tool in a fresh process, alternating."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import time_rig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=17)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=21)
    args = ap.parse_args()
    from camera_calibration_amd import engine, rig

    pair, Ps0 = time_rig.problem(args.views, 2)
    four, Pr0 = time_rig.problem(args.views, 4)
    Pj0 = np.concatenate((pair[0][1], pair[1][1], Ps0))
    Pq0 = rig.packJoint([cam[1] for cam in four], Pr0)
    K, never = args.iters, time_rig.NEVER
    solvers = {"stereo": lambda: engine.refineStereo(*pair, Ps0, K, **never),
               "stereo_joint": lambda: engine.refineStereoJoint(*pair, Pj0, K, **never),
               "rig": lambda: engine.refineRig(four, Pr0, K, **never),
               "rig_joint": lambda: engine.refineRigJoint(four, Pq0, K, **never)}
    doc = {"tool": "tools/time_solver_front.py", "tree": ROOT, "views": args.views, "iters": K, "calls": args.calls,
           "median_ms": {}, "min_ms": {}}
    for name, call in solvers.items():
        for _ in range(args.warmup):
            assert call()[2] == K
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        doc["median_ms"][name], doc["min_ms"][name] = round(float(np.median(ms)), 4), round(min(ms), 4)
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
