#!/usr/bin/env python3
"""Time one LM round of the robust joint rig refinement (calib_refine_rig_robust) under Huber and under Cauchy beside the
plain joint round (calib_refine_rig_joint) of the same tree on the same data.

    python tools/time_rig_robust.py [--views 10000] [--cameras 4] [--iters 10] [--scale 1.0] [--out FILE]

The problem is tools/time_rig.py's: --views views x --cameras cameras x 200 points (a 20 x 10 board seen whole by every
camera), radtan throughout, pixel noise 0.1. The times come from kernel traces of the tool's own: it starts itself three
times under rocprofv3 --kernel-trace, each a run of its own in a fresh process -- `--profile-run plain` is one
calib_refine_rig_joint call, `huber` and `cauchy` one calib_refine_rig_robust call each at --scale pixels -- each call of
--iters iterations under a stop rule that never fires, so every kernel of a round is dispatched iters + 1 times per call.
Per kernel the median, the smallest and the largest duration of its dispatches; a round is the sum of its five kernels'
medians. Only the blocks kernel differs between the three rounds: the spread of the other four is the trace's own. Host
time (allocation, upload, launches) is not in these figures."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_rig import NEVER, problem, shortName, traceMedians  # noqa: E402

RUNS = ("plain", "huber", "cauchy")


def traced(which, args):
    """this tool's --profile-run `which` under rocprofv3 --kernel-trace in a fresh process -> the trace's path"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix=f"time_rig_robust_{which}_")
    subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", which, "--", sys.executable,
                    os.path.abspath(__file__), "--profile-run", which, "--views", str(args.views), "--cameras",
                    str(args.cameras), "--iters", str(args.iters), "--scale", str(args.scale)], check=True,
                   stdout=subprocess.DEVNULL)
    found = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if len(found) != 1:
        raise RuntimeError(f"expected one kernel trace under {out}, found {found}")
    return found[0], out


def traceSpread(path, keep):
    """per kernel of the trace whose name keep() accepts: the smallest and the largest duration (us)"""
    per = {}
    for row in csv.DictReader(open(path)):
        name = shortName(row.get("Kernel_Name") or row.get("Name") or "")
        if keep(name):
            per.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {n: (round(min(v), 2), round(max(v), 2)) for n, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--cameras", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--profile-run", choices=RUNS)
    ap.add_argument("--out")
    args = ap.parse_args()
    M, N, K = args.views, args.cameras, args.iters

    if args.profile_run:
        from camera_calibration_amd import engine, rig
        cams, Pr0 = problem(M, N)
        Pq0 = rig.packJoint([cam[1] for cam in cams], Pr0)
        if args.profile_run == "plain":
            assert engine.refineRigJoint(cams, Pq0, K, **NEVER)[2] == K
        else:
            assert engine.refineRigRobust(cams, Pq0, K, (args.profile_run, args.scale), **NEVER)[2] == K
        return

    doc = {"tool": "tools/time_rig_robust.py", "views": M, "cameras": N, "points_per_camera_and_view": 200, "iters": K,
           "scale_px": args.scale, "shared_unknowns": 10 * N + 6 * (N - 1)}

    def keep(n):
        return n.startswith("rig_joint_")
    rounds = {}
    for which in RUNS:
        path, tmp = traced(which, args)
        kernels = traceMedians(path, keep)
        for n, (lo, hi) in traceSpread(path, keep).items():
            kernels[n]["min_us"], kernels[n]["max_us"] = lo, hi
        shutil.rmtree(tmp, ignore_errors=True)
        rounds[which] = sum(v["median_us"] for v in kernels.values())
        doc[which] = {"kernels": kernels, "round_us": round(rounds[which], 2)}
    doc["huber_over_plain"] = round(rounds["huber"] / rounds["plain"], 4)
    doc["cauchy_over_plain"] = round(rounds["cauchy"] / rounds["plain"], 4)
    doc["note"] = ("round = sum of the per-kernel median durations of a kernel trace (each kernel runs once a round); host "
                   "time is in no figure")
    if args.out:
        json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
