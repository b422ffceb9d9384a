#!/usr/bin/env python3
"""Time one LM round of the joint rig refinement (calib_refine_rig_joint) beside two baselines on the same data: the
rig-only round of this tree (calib_refine_rig, the cameras held) and the rounds of the pairwise joint stereo refinements
(calib_refine_stereo_joint) of the pairs (0, c): what a user without calib_refine_rig_joint runs.

    python tools/time_rig_joint.py [--views 10000] [--cameras 4] [--iters 10] [--out FILE]

The problem is tools/time_rig.py's: --views views x --cameras cameras x 200 points (a 20 x 10 board seen whole by every
camera), radtan throughout, pixel noise 0.1. The times come from kernel traces of the tool's own: it starts itself three
times under rocprofv3 --kernel-trace, each a run of its own in a fresh process -- `--profile-run joint` is one
calib_refine_rig_joint call, `rig` one calib_refine_rig call, `pairs` the N - 1 calib_refine_stereo_joint calls -- each
call of --iters iterations under a stop rule that never fires, so every kernel of a round is dispatched iters + 1 times
per call. Per kernel the median duration of its dispatches; a round is the sum of its five kernels' medians; the pairs'
figure is the sum over the N - 1 pairs. Host time (allocation, upload, launches) is not in these figures."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_rig import NEVER, problem, traceMedians  # noqa: E402


def traced(which, args):
    """this tool's --profile-run `which` under rocprofv3 --kernel-trace in a fresh process -> the trace's path"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix=f"time_rig_joint_{which}_")
    subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", which, "--", sys.executable,
                    os.path.abspath(__file__), "--profile-run", which, "--views", str(args.views), "--cameras",
                    str(args.cameras), "--iters", str(args.iters)], check=True, stdout=subprocess.DEVNULL)
    found = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if len(found) != 1:
        raise RuntimeError(f"expected one kernel trace under {out}, found {found}")
    return found[0], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--cameras", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--profile-run", choices=["joint", "rig", "pairs"])
    ap.add_argument("--out")
    args = ap.parse_args()
    M, N, K = args.views, args.cameras, args.iters

    if args.profile_run:
        from camera_calibration_amd import engine, rig
        cams, Pr0 = problem(M, N)
        S = 6 * (N - 1)
        if args.profile_run == "joint":
            Pq0 = rig.packJoint([cam[1] for cam in cams], Pr0)
            assert engine.refineRigJoint(cams, Pq0, K, **NEVER)[2] == K
        elif args.profile_run == "rig":
            assert engine.refineRig(cams, Pr0, K, **NEVER)[2] == K
        else:
            for c in range(1, N):
                Pj0 = np.concatenate((cams[0][1], cams[c][1], Pr0[6 * (c - 1):6 * c], Pr0[S:]))
                assert engine.refineStereoJoint(cams[0], cams[c], Pj0, K, **NEVER)[2] == K
        return

    doc = {"tool": "tools/time_rig_joint.py", "views": M, "cameras": N, "points_per_camera_and_view": 200, "iters": K,
           "shared_unknowns": 10 * N + 6 * (N - 1)}
    keep = {"joint": lambda n: n.startswith("rig_joint_"),
            "rig": lambda n: (n.startswith("rig_") and not n.startswith("rig_joint_")) or "RigLayout" in n,
            "pairs": lambda n: n.startswith("stereo_") and "RigLayout" not in n}
    rounds = {}
    for which in ("joint", "rig", "pairs"):
        path, tmp = traced(which, args)
        kernels = traceMedians(path, keep[which])
        shutil.rmtree(tmp, ignore_errors=True)
        rounds[which] = sum(v["median_us"] for v in kernels.values())
        doc[which] = {"kernels": kernels, "round_us": round(rounds[which], 2)}
    doc["pairs"]["round_us_one_pair"] = doc["pairs"].pop("round_us")
    doc["pairs"]["round_us_all_pairs"] = round((N - 1) * rounds["pairs"], 2)
    doc["joint_over_rig_only"] = round(rounds["joint"] / rounds["rig"], 4)
    doc["joint_over_pairs"] = round(rounds["joint"] / ((N - 1) * rounds["pairs"]), 4)
    doc["note"] = ("round = sum of the per-kernel median durations of a kernel trace (each kernel runs once a round); the "
                   "pairs' medians are over the dispatches of all N - 1 calls; host time is in no figure")
    if args.out:
        json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
