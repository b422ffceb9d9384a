#!/usr/bin/env python3
"""Time one LM round of the stereo refinement (calib_refine_stereo) beside the nearest existing workload.

    python tools/time_stereo.py [--views 10000] [--repeat 7] [--iters 20 120]

Stereo: --views views x (200 + 200) points (a 20 x 10 board seen whole by both cameras), radtan / radtan, pixel noise
0.1. The call is handle-less (it allocates, uploads, runs and reads back), so one round is taken as a SLOPE: the call
is timed with two iteration counts under a stop rule that never fires (lam_min = 0, lam_max = inf, err_min = -1: every
call runs exactly its max_iters rounds, plus the bootstrap round), and ms per round = (t(K2) - t(K1)) / (K2 - K1) --
the host clock around calls that end in a device synchronise, best and median of --repeat. The intercept (allocation,
upload, bootstrap, read-back) is reported beside it.
Mono: the global LM loop with every shared parameter fixed (RefineEngine.setFixedShared("all")) on the same views of
camera a, --views x 200 points, resident in HBM, the same slope; the comparison figure is TWO such rounds (one per
camera's worth of points). One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import camera_calibration_amd as cca                      # noqa: E402
from camera_calibration_amd import engine, stereo, synthetic      # noqa: E402

A_B = np.array([[520.0, 0.0, 330.0], [0.0, 515.0, 250.0], [0.0, 0.0, 1.0]])
K_B = (-0.3, 0.1, 0.01, -0.02, 0.02)
NEVER = dict(lamMin=0.0, lamMax=float("inf"), errMin=-1.0)


def project(A, W, k, offs, model):
    eng = cca.RefineEngine("radtan", "f64")
    try:
        eng.setProblem(offs, None, model)
        return eng.evaluate(synthetic.composeP(A, W, k), wantY=True)["y"]
    finally:
        eng.close()


def timed(fn, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts)), out


def slope(call, k1, k2, repeat):
    call(k1)                                               # warm-up: code objects, clocks
    b1, m1, o1 = timed(lambda: call(k1), repeat)
    b2, m2, o2 = timed(lambda: call(k2), repeat)
    assert o1 == k1 and o2 == k2, f"the loop stopped early: {o1} of {k1}, {o2} of {k2} iterations"
    return {"iters": [k1, k2], "best_ms": [round(b1, 3), round(b2, 3)], "median_ms": [round(m1, 3), round(m2, 3)],
            "ms_per_round": (b2 - b1) / (k2 - k1), "ms_per_round_of_medians": (m2 - m1) / (k2 - k1),
            "intercept_ms": b1 - k1 * (b2 - b1) / (k2 - k1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--iters", type=int, nargs=2, default=[20, 120])
    args = ap.parse_args()
    M, (k1, k2) = args.views, args.iters
    corners = synthetic.checkerboardCorners(20, 10, 0.03)
    N = corners.shape[0]
    Wa = synthetic.sampleBoardPosesInCamera(corners, np.arange(M))
    rig = np.array([2.0, -3.0, 1.5, -0.2 * 19 * 0.03, 0.01, 0.005])
    T = stereo.parametersToPoses(rig)[0]
    offs = np.arange(M + 1, dtype=np.int64) * N
    model = np.ascontiguousarray(np.tile(corners, (M, 1)))
    rng = np.random.default_rng(11)
    uvA = project(synthetic.RADTAN_A, Wa, synthetic.RADTAN_K, offs, model) + rng.normal(0, 0.1, (M * N, 2))
    uvB = project(A_B, T @ Wa, K_B, offs, model) + rng.normal(0, 0.1, (M * N, 2))
    sharedA = synthetic.composeP(synthetic.RADTAN_A, Wa[:0], synthetic.RADTAN_K)
    sharedB = synthetic.composeP(A_B, Wa[:0], K_B)
    PsTrue = np.concatenate((rig, stereo.posesToParameters(Wa).ravel()))
    Ps0 = PsTrue * (1 + 1e-3 * rng.standard_normal(PsTrue.shape))
    camA = (engine.MODEL_IDS["radtan"], sharedA, offs, uvA, model)
    camB = (engine.MODEL_IDS["radtan"], sharedB, offs, uvB, model)

    st = slope(lambda k: engine.refineStereo(camA, camB, Ps0, k, **NEVER)[2], k1, k2, args.repeat)
    sse, Ps, iters, trace, ab = engine.refineStereo(camA, camB, Ps0, 50)
    st.update({"converged_run": {"iters": iters, "sse": sse, "accepted": int(trace[:, 4].sum()),
                                 "max_rig_error": float(np.abs(Ps[:6] - rig).max())}})

    eng = cca.RefineEngine("radtan", "f64")
    eng.setFixedShared("all")
    eng.setProblem(offs, uvA, model)
    P0 = np.concatenate((sharedA, Ps0[6:]))
    mono = slope(lambda k: eng.refine(P0, k, **NEVER)[2], k1, k2, args.repeat)
    eng.close()
    print(json.dumps({
        "tool": "tools/time_stereo.py", "views": M, "points_per_view": [N, N], "models": ["radtan", "radtan"],
        "stereo": st, "mono_fixed_all": mono, "two_mono_rounds_ms": 2 * mono["ms_per_round"],
        "stereo_over_two_mono_rounds": st["ms_per_round"] / (2 * mono["ms_per_round"]),
        "note": "ms_per_round = slope of the call's host-clock time between the two iteration counts (best of repeat); "
                "the stereo call is handle-less, its intercept holds allocation, upload, bootstrap round and read-back; "
                "the mono loop runs on a resident problem"}))


if __name__ == "__main__":
    main()
