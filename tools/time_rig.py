#!/usr/bin/env python3
"""Time one LM round of the multi-camera rig refinement (calib_refine_rig) beside the rounds of the rig-only stereo
refinement (calib_refine_stereo) of the pairs (0, c) on the same data: what a user without calib_refine_rig runs.

    python tools/time_rig.py [--views 10000] [--cameras 4] [--iters 20] [--out FILE]

--views views x --cameras cameras x 200 points (a 20 x 10 board seen whole by every camera), radtan throughout, pixel
noise 0.1. The times come from kernel traces of the tool's own: it starts itself twice under rocprofv3 --kernel-trace,
each a run of its own in a fresh process -- `--profile-run rig` is one calib_refine_rig call, `--profile-run pairs` the
N - 1 calib_refine_stereo calls of the pairs (0, c) -- each call of --iters iterations under a stop rule that never
fires, so every kernel of a round is dispatched iters + 1 times per call. Per kernel the median duration of its
dispatches; a round is the sum of its five kernels' medians; the pairs' figure is the sum over the N - 1 pairs. Host time
(allocation, upload, launches) is not in these figures: the calls are handle-less and spend it alike."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A_B = np.array([[520.0, 0.0, 330.0], [0.0, 515.0, 250.0], [0.0, 0.0, 1.0]])
K_B = (-0.3, 0.1, 0.01, -0.02, 0.02)
NEVER = dict(lamMin=0.0, lamMax=float("inf"), errMin=-1.0)
WIDTH = 19 * 0.03
# camera c >= 1: Euler angles in degrees, then its offset
RIGS = np.array([[2.0, -3.0, 1.5, -0.2 * WIDTH, 0.01, 0.005], [-2.5, 2.0, -1.0, 0.2 * WIDTH, 0.01, -0.005],
                 [1.5, 3.0, 2.0, 0.005, -0.2 * WIDTH, 0.005], [-1.0, -2.5, 1.0, 0.005, 0.2 * WIDTH, 0.005],
                 [3.0, 1.0, -2.0, -0.2 * WIDTH, -0.2 * WIDTH, 0.0], [-2.0, -1.5, -1.5, 0.2 * WIDTH, 0.2 * WIDTH, 0.0],
                 [1.0, 2.5, -2.5, -0.2 * WIDTH, 0.2 * WIDTH, 0.005]])


def problem(M, N):
    """-> (cameras as engine.refineRig takes them, Pr0)"""
    import camera_calibration_amd as cca
    from camera_calibration_amd import engine, stereo, synthetic

    def project(A, W, k, offs, model):
        eng = cca.RefineEngine("radtan", "f64")
        try:
            eng.setProblem(offs, None, model)
            return eng.evaluate(synthetic.composeP(A, W, k), wantY=True)["y"]
        finally:
            eng.close()
    corners = synthetic.checkerboardCorners(20, 10, 0.03)
    n = corners.shape[0]
    W0 = synthetic.sampleBoardPosesInCamera(corners, np.arange(M))
    offs = np.arange(M + 1, dtype=np.int64) * n
    model = np.ascontiguousarray(np.tile(corners, (M, 1)))
    rng = np.random.default_rng(11)
    cams = []
    for c in range(N):
        A, k = (synthetic.RADTAN_A, synthetic.RADTAN_K) if c == 0 else (A_B, K_B)
        T = np.eye(4) if c == 0 else stereo.parametersToPoses(RIGS[c - 1])[0]
        uv = project(A, T @ W0, k, offs, model) + rng.normal(0, 0.1, (M * n, 2))
        cams.append((engine.MODEL_IDS["radtan"], synthetic.composeP(A, W0[:0], k), offs, uv, model))
    PrTrue = np.concatenate((RIGS[:N - 1].ravel(), stereo.posesToParameters(W0).ravel()))
    return tuple(cams), PrTrue * (1 + 1e-3 * rng.standard_normal(PrTrue.shape))


def shortName(name):
    return re.sub(r"\(.*", "", re.sub(r"^void\s+", "", name).replace("calib::", "")).strip()


def traceMedians(path, keep):
    """per kernel of a rocprofv3 kernel trace whose name keep() accepts: dispatches, median and total duration (us)"""
    per = {}
    for r in csv.DictReader(open(path)):
        name = shortName(r.get("Kernel_Name") or r.get("Name") or "")
        if keep(name):
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return {n: {"dispatches": len(d), "median_us": round(float(np.median(d)), 2), "total_us": round(float(np.sum(d)), 1)}
            for n, d in sorted(per.items())}


def traced(which, args):
    """this tool's --profile-run `which` under rocprofv3 --kernel-trace in a fresh process -> the trace's path"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix=f"time_rig_{which}_")
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--profile-run", choices=["rig", "pairs"])
    ap.add_argument("--out")
    args = ap.parse_args()
    M, N, K = args.views, args.cameras, args.iters

    if args.profile_run:
        from camera_calibration_amd import engine
        cams, Pr0 = problem(M, N)
        S = 6 * (N - 1)
        if args.profile_run == "rig":
            assert engine.refineRig(cams, Pr0, K, **NEVER)[2] == K
        else:
            for c in range(1, N):
                Ps0 = np.concatenate((Pr0[6 * (c - 1):6 * c], Pr0[S:]))
                assert engine.refineStereo(cams[0], cams[c], Ps0, K, **NEVER)[2] == K
        return

    doc = {"tool": "tools/time_rig.py", "views": M, "cameras": N, "points_per_camera_and_view": 200, "iters": K}
    path, tmp = traced("rig", args)
    rig = traceMedians(path, lambda n: n.startswith("rig_") or "RigLayout" in n)
    shutil.rmtree(tmp, ignore_errors=True)
    path, tmp = traced("pairs", args)
    pairs = traceMedians(path, lambda n: n.startswith("stereo_") and "RigLayout" not in n)
    shutil.rmtree(tmp, ignore_errors=True)
    doc["rig"] = {"kernels": rig, "round_us": round(sum(v["median_us"] for v in rig.values()), 2)}
    pairRound = sum(v["median_us"] for v in pairs.values())
    doc["pairs"] = {"kernels": pairs, "round_us_one_pair": round(pairRound, 2),
                    "round_us_all_pairs": round((N - 1) * pairRound, 2)}
    doc["rig_over_pairs"] = round(doc["rig"]["round_us"] / ((N - 1) * pairRound), 4)
    doc["note"] = ("round = sum of the per-kernel median durations of a kernel trace (each kernel runs once a round); the "
                   "pairs' medians are over the dispatches of all N - 1 calls; host time is in neither figure")
    if args.out:
        json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
