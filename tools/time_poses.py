#!/usr/bin/env python3
"""Time the per-view pose-only refinement (calib_refine_poses) on benchmark-shaped shards.

    python tools/time_poses.py [--configs c3 c2] [--repeat 5] [--max-iters 20]

Per config one JSON line: views, points, mean iterations per view, the call's wall time in ms (best and median of
--repeat; the call is handle-less, so the time INCLUDES allocating and uploading the shard and reading the poses
back) and point-residual-iterations per second (points x mean iterations / best time). Beside it, the global LM loop
with every shared parameter fixed (RefineEngine.setFixedShared("all")) on the same data and start poses: resident
(refine alone, the shard already in HBM) and including calib_set_problem -- the form that shares one lambda and one
accept decision between all views and runs the Schur / reduce / L x L machinery for nothing.
Data: synthetic.makeShard (the camera is the config's true one, the start poses its perturbed ones)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import camera_calibration_amd as cca                      # noqa: E402
from camera_calibration_amd import engine, synthetic      # noqa: E402


def timed(fn, repeat):
    ts, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c3", "c2"])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-iters", type=int, default=20)
    ap.add_argument("--views", type=int, default=None, help="views per shard (default: the config's)")
    args = ap.parse_args()
    for tag in args.configs:
        sh = synthetic.makeShard(tag, numViews=args.views, noiseSigma=0.0)
        offs, s, m = sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"]
        modelId = engine.MODEL_IDS[sh["model"]]
        L = engine.NUM_SHARED[modelId]
        shared, poses0 = sh["Ptrue"][:L], sh["P0"][L:].reshape(-1, 6)
        engine.refinePoses(modelId, shared, poses0, offs, s, m, args.max_iters)          # warm-up: code object, clocks
        best, med, (sse, poses, iters, status) = timed(
            lambda: engine.refinePoses(modelId, shared, poses0, offs, s, m, args.max_iters), args.repeat)
        # the global loop on the same start point, all shared parameters fixed
        P0 = np.concatenate((shared, poses0.ravel()))
        eng = cca.RefineEngine(sh["model"], "f64")
        eng.setFixedShared("all")
        upBest, upMed, _ = timed(lambda: eng.setProblem(offs, s, m), args.repeat)
        eng.refine(P0, 60)
        gBest, gMed, (gsse, PG, gIters, _) = timed(lambda: eng.refine(P0, 60), args.repeat)
        eng.close()
        MN = int(offs[-1])
        print(json.dumps({
            "config": tag, "model": sh["model"], "views": int(offs.shape[0] - 1), "points": MN,
            "max_iters": args.max_iters, "mean_iters_per_view": float(iters.mean()), "max_iters_of_a_view": int(iters.max()),
            "failed_views": int((status != 0).sum()), "sum_sse": float(np.nansum(sse)), "max_view_sse": float(np.nanmax(sse)),
            "ms": round(best, 3), "ms_median": round(med, 3),
            "point_residual_iterations_per_s": MN * float(iters.mean()) / (best * 1e-3),
            "global_fixed_all": {"iters": int(gIters), "sse": float(gsse), "ms_resident": round(gBest, 3),
                                 "ms_resident_median": round(gMed, 3), "ms_set_problem": round(upBest, 3),
                                 "max_pose_diff": float(np.abs(PG[L:].reshape(-1, 6) - poses).max())},
        }))


if __name__ == "__main__":
    main()
