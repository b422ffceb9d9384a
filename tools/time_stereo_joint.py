#!/usr/bin/env python3
"""Time one LM round of the joint stereo refinement (calib_refine_stereo_joint) beside the rig-only round
(calib_refine_stereo) on the problem of tools/time_stereo.py.

    python tools/time_stereo_joint.py [--views 10000] [--repeat 7] [--iters 20 120] [--rig-only-tree DIR] [--out FILE]
    rocprofv3 --kernel-trace -d OUT -o joint -- python tools/time_stereo_joint.py --profile-run
    python tools/time_stereo_joint.py --merge FILE --trace OUT/<host>/joint_kernel_trace.csv [--bench-ab FILE2]

--views views x (200 + 200) points (a 20 x 10 board seen whole by both cameras), radtan / radtan, pixel noise 0.1. Both
calls are handle-less (they allocate, upload, run and read back), so a round is a SLOPE: the call is timed with two
iteration counts under a stop rule that never fires (every call runs exactly its max_iters rounds plus the bootstrap
round), ms per round = (t(K2) - t(K1)) / (K2 - K1), best and median of --repeat; the intercept is reported beside it.
--rig-only-tree: the rig-only slope is taken in a child process that imports the package of that tree (a built checkout
of the parent commit) on the same device, right after this process's own measurements. --profile-run: one joint call of --iters[0] rounds
and nothing else, for a kernel trace taken in a run of its own. --merge: add the per-kernel medians of such a trace (and
the ms_per_step lists of an A/B file of bench.py lines, if given) to the JSON a first run wrote."""
import argparse
import csv
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:                                   # the child of --rig-only-tree: that tree's package
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)

A_B = np.array([[520.0, 0.0, 330.0], [0.0, 515.0, 250.0], [0.0, 0.0, 1.0]])
K_B = (-0.3, 0.1, 0.01, -0.02, 0.02)
NEVER = dict(lamMin=0.0, lamMax=float("inf"), errMin=-1.0)


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


def problem(M):
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
    shared0 = np.concatenate((sharedA, sharedB)) * (1 + 1e-3 * rng.standard_normal(20))
    return N, camA, camB, Ps0, np.concatenate((shared0, Ps0)), rig


def shortName(name):
    return re.sub(r"\(.*", "", re.sub(r"^void\s+", "", name).replace("calib::", "")).strip()


def traceMedians(path):
    """per kernel of a rocprofv3 kernel trace: dispatches, median and total duration in microseconds"""
    per = {}
    for r in csv.DictReader(open(path)):
        name = shortName(r.get("Kernel_Name") or r.get("Name") or "")
        per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return {n: {"dispatches": len(d), "median_us": round(float(np.median(d)), 2), "total_us": round(float(np.sum(d)), 1)}
            for n, d in sorted(per.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--iters", type=int, nargs=2, default=[20, 120])
    ap.add_argument("--rig-only-tree")
    ap.add_argument("--tree")
    ap.add_argument("--rig-only-child", action="store_true")
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--merge")
    ap.add_argument("--trace")
    ap.add_argument("--bench-ab")
    args = ap.parse_args()
    M, (k1, k2) = args.views, args.iters

    if args.merge:
        doc = json.load(open(args.merge))
        if args.trace:
            kern = traceMedians(args.trace)
            joint = {n: v for n, v in kern.items() if n.startswith("stereo_joint_") or "JointLayout" in n}   # + the shared back-substitution
            rounds = max(v["dispatches"] for v in joint.values()) if joint else 0
            doc["kernel_trace"] = {"run": f"one calib_refine_stereo_joint call of {doc['joint']['iters'][0]} iterations "
                                          "under rocprofv3 --kernel-trace, a run of its own", "kernels": joint,
                                   "sum_of_medians_us": round(sum(v["median_us"] for v in joint.values()), 2),
                                   "rounds_in_trace": rounds}
        if args.bench_ab:
            ab = {"parent": [], "this": []}
            for ln in open(args.bench_ab):
                tag, _, line = ln.partition(" ")
                if tag in ab and line.strip().startswith("{"):
                    d = json.loads(line)
                    ab[tag].append(d.get("ms_per_step", d.get("timing", {}).get("ms_per_step")))
            doc["bench_ab"] = {"command": "bench.py --gpus 1 --steps 20 --warmup 5, parent and this tree alternating, "
                                          "parent first", "ms_per_step": ab}
        json.dump(doc, open(args.merge, "w"), indent=1)
        print(json.dumps(doc))
        return

    from camera_calibration_amd import engine
    N, camA, camB, Ps0, Pj0, rig = problem(M)
    if args.profile_run:
        engine.refineStereoJoint(camA, camB, Pj0, k1, **NEVER)
        return
    rigOnly = slope(lambda k: engine.refineStereo(camA, camB, Ps0, k, **NEVER)[2], k1, k2, args.repeat)
    if args.rig_only_child:
        print(json.dumps(rigOnly))
        return
    jt = slope(lambda k: engine.refineStereoJoint(camA, camB, Pj0, k, **NEVER)[2], k1, k2, args.repeat)
    sse, Pj, iters, trace, ab = engine.refineStereoJoint(camA, camB, Pj0, 50)
    jt["converged_run"] = {"iters": iters, "sse": sse, "accepted": int(trace[:, 4].sum()),
                           "max_rig_error": float(np.abs(Pj[20:26] - rig).max())}
    doc = {"tool": "tools/time_stereo_joint.py", "views": M, "points_per_view": [N, N], "models": ["radtan", "radtan"],
           "joint": jt, "rig_only_this_library": rigOnly}
    ref = rigOnly
    if args.rig_only_tree:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rig-only-child", "--tree", args.rig_only_tree,
                              "--views", str(M), "--repeat", str(args.repeat), "--iters", str(k1), str(k2)], check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        ref = doc["rig_only_parent_tree"] = json.loads(out.strip().splitlines()[-1])
    doc["joint_over_rig_only"] = jt["ms_per_round"] / ref["ms_per_round"]
    doc["note"] = ("ms_per_round = slope of the call's host-clock time between the two iteration counts (best of repeat); "
                   "both calls are handle-less, their intercepts hold allocation, upload, bootstrap round and read-back; "
                   "joint_over_rig_only uses the parent tree's rig-only round when one was given")
    if args.out:
        json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
