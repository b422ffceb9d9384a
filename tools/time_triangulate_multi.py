#!/usr/bin/env python3
"""Time triangulate_multi_kernel beside triangulate_kernel from a rocprofv3 kernel trace of a run of its own.

    python tools/time_triangulate_multi.py --out profiles/triangulate_multi.json

starts `rocprofv3 --kernel-trace` (no counters in the same run) on a CHILD process -- this script again, with
--device-only, after the `--` -- reads the trace the child leaves and prints the summary. This process itself never
opens the GPU.

Workload (--device-only): 10^6 points 0.5 .. 1.5 m in front of a rig of four cameras (radtan, fisheye, radtan, fisheye),
0.5 px noise, every camera seeing every point:
  a  calib_triangulate_multi with N = 4                           (4 10^6 seen observations)
  b  calib_triangulate on the pixels of cameras 0 and 1          (2 10^6; triangulate_kernel<0, 1>)
  c  calib_triangulate_multi with N = 2 on those same pairs      (2 10^6)
each --repeat + 1 times, a then b then c. The trace's rows are grouped by kernel; triangulate_multi_kernel's dispatches
are told apart by their order (the first --repeat + 1 are a). Each group's first dispatch is dropped (code object load,
clocks) and the MEDIAN duration of the rest is reported, with us per 10^6 seen observations for each, c against b -- what
the run-time camera loop and the run-time model switch cost where the pair kernel has neither -- and a against c per
observation."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POINTS = 1000000
RIG_DEG = ((2.0, -3.0, 1.5), (-2.5, 2.0, -1.0), (1.5, 3.0, 2.0))
RIG_T = ((-0.08, 0.008, 0.004), (0.08, 0.008, -0.004), (0.004, -0.08, 0.004))


def shortName(name):
    name = name.replace("void calib::", "").replace("calib::", "")
    return name.split("(")[0].strip()


def readTrace(path):
    """kernel name (template arguments kept) -> durations in us, in dispatch order"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    for r in rows:
        name = shortName(r.get("Kernel_Name") or r.get("Name") or "")
        if "triangulate" not in name and "undistort_points_kernel" not in name:
            continue
        groups.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return groups


def stats(durs, observations=None):
    kept = durs[1:] if len(durs) > 1 else durs
    out = {"median_us": round(float(np.median(kept)), 2), "dispatches": len(kept),
           "range_us": [round(float(min(kept)), 2), round(float(max(kept)), 2)]}
    if observations:
        out["us_per_million_seen_observations"] = round(out["median_us"] * 1e6 / observations, 2)
    return out


def summarise(groups, repeat):
    multi = [v for k, v in groups.items() if "triangulate_multi_kernel" in k]
    pair = [(k, v) for k, v in groups.items() if k.startswith("triangulate_kernel")]
    if len(multi) != 1 or len(pair) != 1 or len(multi[0]) != 2 * (repeat + 1) or len(pair[0][1]) != repeat + 1:
        raise SystemExit(f"unexpected trace: {[(k, len(v)) for k, v in groups.items()]}")
    a = stats(multi[0][:repeat + 1], 4 * POINTS)
    c = stats(multi[0][repeat + 1:], 2 * POINTS)
    b = stats(pair[0][1], 2 * POINTS)
    key = "us_per_million_seen_observations"
    return {"points": POINTS, "triangulate_multi_kernel_4_cameras": a, "triangulate_multi_kernel_2_cameras": c,
            "triangulate_kernel": dict(b, kernel=pair[0][0]),
            "multi_2_cameras_over_pair_kernel": round(c["median_us"] / b["median_us"], 3),
            "per_observation_4_cameras_over_2_cameras": round(a[key] / c[key], 3),
            "per_observation_4_cameras_over_pair_kernel": round(a[key] / b[key], 3),
            "undistort_points_kernels_median_us": {k: stats(v)["median_us"] for k, v in groups.items()
                                                   if "undistort_points_kernel" in k}}


def runWorkload(repeat):
    import camera_calibration_amd as cca
    from camera_calibration_amd import mathutils as mu
    from camera_calibration_amd import synthetic
    names = ("radtan", "fisheye", "radtan", "fisheye")
    focal = {"radtan": 1000.0, "fisheye": 1600.0}
    coeff = {"radtan": synthetic.RADTAN_K, "fisheye": synthetic.FISHEYE_K}
    model = {"radtan": cca.RadialTangentialModel(), "fisheye": cca.FisheyeModel()}
    cams = [(m, np.array([[focal[m], 0.0, 959.5], [0.0, focal[m], 539.5], [0.0, 0.0, 1.0]]), coeff[m]) for m in names]
    T = np.tile(np.eye(4), (4, 1, 1))
    T[1:, :3, :3] = mu.eulerToRotationMatrices(np.array(RIG_DEG))
    T[1:, :3, 3] = RIG_T
    rng = np.random.default_rng(0)
    Z = rng.uniform(0.5, 1.5, POINTS)
    X = np.column_stack((rng.uniform(-0.3, 0.3, POINTS) * Z, rng.uniform(-0.2, 0.2, POINTS) * Z, Z))
    uv = np.stack([model[m].projectWithDistortion(A, X @ Tc[:3, :3].T + Tc[:3, 3], k) + rng.normal(0.0, 0.5, (POINTS, 2))
                   for (m, A, k), Tc in zip(cams, T)])
    report = {}
    print(json.dumps({"points": POINTS, "cameras": names, "repeat": repeat}), flush=True)
    for _ in range(repeat + 1):
        got, status = cca.triangulateMulti(cams, T, uv, returnStatus=True)
    report["four_cameras"] = (got, status)
    for _ in range(repeat + 1):
        got, status = cca.triangulate(cams[0], cams[1], T[1, :3, :3].copy(), T[1, :3, 3].copy(), uv[0], uv[1],
                                      returnStatus=True)
    report["pair_call"] = (got, status)
    for _ in range(repeat + 1):
        got, status = cca.triangulateMulti(cams[:2], T[:2], uv[:2], returnStatus=True)
    report["two_cameras"] = (got, status)
    for tag, (got, status) in report.items():
        ok = status == 0
        rel = np.linalg.norm(got[ok] - X[ok], axis=1) / np.linalg.norm(X[ok], axis=1)
        print(json.dumps({"call": tag, "status_counts": np.bincount(status, minlength=5).tolist(),
                          "median_rel_distance_to_the_noise_free_point": float(np.median(rel))}), flush=True)
    ok = (report["pair_call"][1] == 0) & (report["two_cameras"][1] == 0)
    d = np.linalg.norm(report["pair_call"][0][ok] - report["two_cameras"][0][ok], axis=1) / np.linalg.norm(X[ok], axis=1)
    print(json.dumps({"max_rel_distance_two_cameras_to_pair_call": float(d.max())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device-only", action="store_true", help="run the workload: what this script puts under rocprofv3")
    ap.add_argument("--trace", default=None, help="read this rocprofv3 kernel trace CSV instead of making one")
    ap.add_argument("--out", default=None, help="JSON file to write the summary to")
    ap.add_argument("--timeout", type=float, default=540.0, help="seconds the traced child may take")
    args = ap.parse_args()
    if args.device_only:
        runWorkload(args.repeat)
        return
    trace = args.trace
    if trace is None:
        out = tempfile.mkdtemp(prefix="triangulate_multi_trace_")
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "tm", "--", sys.executable,
               os.path.abspath(__file__), "--device-only", "--repeat", str(args.repeat)]
        child = subprocess.run(cmd, timeout=args.timeout)
        if child.returncode != 0:
            raise SystemExit(f"the traced run ended with status {child.returncode}")
        found = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if len(found) != 1:
            raise SystemExit(f"expected one kernel trace under {out}, found {found}")
        trace = found[0]
    doc = summarise(readTrace(trace), args.repeat)
    doc["method"] = ("rocprofv3 --kernel-trace of one child run (no counters); per kernel the median over the dispatches "
                     "after the first")
    print(json.dumps(doc, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
