#!/usr/bin/env python3
"""Time rectify_map_kernel beside undistort_map_kernel, and triangulate_kernel beside the undistort_points_kernel
launches that feed it, from a rocprofv3 kernel trace of a run of its own.

    rocprofv3 --kernel-trace --output-format csv -d OUT -o rect -- python tools/time_rectify.py --device-only
    python tools/time_rectify.py --trace OUT/<host>/rect_kernel_trace.csv --out profiles/rectify_bench.json

Workload (--device-only): for 1920 x 1080 and 3840 x 2160 and each model -- the cameras of tools/time_undistort.py --
the maps of the camera itself (calib_undistort_maps) and the maps of the same camera rectified for the rig of the tests
(calib_rectify_maps with R1 and the P1 of stereoRectify), --repeat times each, alternating; then 10^6 matched pixel
pairs with 0.5 px noise through calib_triangulate for a radtan / fisheye pair, --repeat times.

--trace reads the per-dispatch rows (Kernel_Name, Start_Timestamp, End_Timestamp, the grid size), groups them by kernel
and grid size -- which tells the two image sizes apart --, drops each group's first dispatch (code object load, clocks)
and reports the MEDIAN duration of the rest, with the ratio of each rectify_map_kernel to the undistort_map_kernel of
the same model and size, and of triangulate_kernel to the two undistort_points_kernel launches of one call."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((1920, 1080), (3840, 2160))
FOCAL = {"radtan": 1000.0, "fisheye": 1600.0}           # at 1920 columns; scaled with the width (time_undistort.py)
PAIRS = 1000000
RIG_DEG, RIG_T = (2.0, -3.0, 1.5), (-0.08, 0.008, 0.004)


def mapGrid(width, height):
    return (width * height + 1023) // 1024 * 256           # work-items: blocks of 256 threads, four elements each


def pointGrid(n):
    return (n + 255) // 256 * 256


def gridOf(row):
    for key in ("Grid_Size_X", "Grid_Size", "grid_size_x"):
        if row.get(key):
            return int(float(row[key]))
    return 0


def shortName(name):
    name = name.replace("void calib::", "").replace("calib::", "")
    return name.split("(")[0].strip()


def readTrace(path):
    """kernel name (template arguments kept) and grid size -> durations in us, in dispatch order"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    for r in rows:
        name = shortName(r.get("Kernel_Name") or r.get("Name") or "")
        if not any(k in name for k in ("rectify_map_kernel", "undistort_map_kernel", "triangulate_kernel",
                                       "undistort_points_kernel")):
            continue
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        groups.setdefault((name, gridOf(r)), []).append(dur)
    return groups


def summarise(groups):
    out = {"map_kernels": [], "triangulation": []}
    med = {}
    for (name, grid), durs in groups.items():
        kept = durs[1:] if len(durs) > 1 else durs
        med[name, grid] = (float(np.median(kept)), len(kept), float(min(kept)), float(max(kept)))
    for width, height in SIZES:
        for model, tag in (("radtan", "<0>"), ("fisheye", "<1>")):
            u = med.get(("undistort_map_kernel" + tag, mapGrid(width, height)))
            r = med.get(("rectify_map_kernel" + tag, mapGrid(width, height)))
            if u and r:
                out["map_kernels"].append({
                    "model": model, "width": width, "height": height, "bytes": width * height * 8,
                    "undistort_map_kernel_median_us": round(u[0], 2), "rectify_map_kernel_median_us": round(r[0], 2),
                    "dispatches": [u[1], r[1]], "undistort_range_us": [round(u[2], 2), round(u[3], 2)],
                    "rectify_range_us": [round(r[2], 2), round(r[3], 2)], "ratio": round(r[0] / u[0], 3),
                    "rectify_tb_per_s": round(width * height * 8 / (r[0] * 1e-6) / 1e12, 3)})
    tri = [(n, v) for (n, g), v in med.items() if "triangulate_kernel" in n and g == pointGrid(PAIRS)]
    inv = [(n, v) for (n, g), v in med.items() if "undistort_points_kernel" in n and g == pointGrid(PAIRS)]
    if tri:
        feed = sum(v[0] for _, v in inv)
        for n, v in tri:
            out["triangulation"].append({
                "kernel": n, "pairs": PAIRS, "median_us": round(v[0], 2), "dispatches": v[1],
                "range_us": [round(v[2], 2), round(v[3], 2)], "ns_per_pair": round(v[0] * 1e3 / PAIRS, 3),
                "undistort_points_kernels_median_us": {k: round(x[0], 2) for k, x in inv},
                "ratio_to_the_two_inverses": round(v[0] / feed, 3) if feed else None})
    return out


def runWorkload(repeat):
    import camera_calibration_amd as cca
    from camera_calibration_amd import mathutils as mu
    from camera_calibration_amd import synthetic
    R = mu.eulerToRotationMatrices(np.array([RIG_DEG]))[0]
    t = np.array(RIG_T)
    models = (("radtan", cca.RadialTangentialModel(), synthetic.RADTAN_K), ("fisheye", cca.FisheyeModel(), synthetic.FISHEYE_K))
    for width, height in SIZES:
        cams = []
        for name, model, k in models:
            focal = FOCAL[name] * width / 1920
            cams.append((name, np.array([[focal, 0.0, (width - 1) / 2], [0.0, focal, (height - 1) / 2], [0.0, 0.0, 1.0]]), k))
        rect = cca.stereoRectify(cams[0], cams[1], R, t, (width, height))
        for (name, model, k), cam, Rc, P in zip(models, cams, (rect.R1, rect.R2), (rect.P1, rect.P2)):
            nanCount = 0
            for _ in range(repeat + 1):
                model.undistortMaps(cam[1], k, (width, height))
                mapx, _ = model.rectifyMaps(cam[1], k, Rc, P, (width, height))
                nanCount = int(np.isnan(mapx).sum())
            print(json.dumps({"model": name, "width": width, "height": height, "rectified_focal": P[0, 0],
                              "map_entries_nan": nanCount}), flush=True)
    # 10^6 pairs: points 0.5 .. 1.5 m in front of camera a, inside a 0.6 rad cone, seen by both cameras
    rng = np.random.default_rng(0)
    Z = rng.uniform(0.5, 1.5, PAIRS)
    X = np.column_stack((rng.uniform(-0.3, 0.3, PAIRS) * Z, rng.uniform(-0.2, 0.2, PAIRS) * Z, Z))
    camA = ("radtan", np.array([[1000.0, 0.0, 959.5], [0.0, 1000.0, 539.5], [0.0, 0.0, 1.0]]), synthetic.RADTAN_K)
    camB = ("fisheye", np.array([[1600.0, 0.0, 959.5], [0.0, 1600.0, 539.5], [0.0, 0.0, 1.0]]), synthetic.FISHEYE_K)
    uvA = models[0][1].projectWithDistortion(camA[1], X, camA[2]) + rng.normal(0.0, 0.5, (PAIRS, 2))
    uvB = models[1][1].projectWithDistortion(camB[1], X @ R.T + t, camB[2]) + rng.normal(0.0, 0.5, (PAIRS, 2))
    for _ in range(repeat + 1):
        got, status = cca.triangulate(camA, camB, R, t, uvA, uvB, returnStatus=True)
    ok = status == 0
    rel = np.linalg.norm(got[ok] - X[ok], axis=1) / np.linalg.norm(X[ok], axis=1)
    print(json.dumps({"pairs": PAIRS, "status_counts": np.bincount(status, minlength=4).tolist(),
                      "median_rel_distance_to_the_noise_free_point": float(np.median(rel))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--device-only", action="store_true", help="run the workload: what to put under rocprofv3")
    ap.add_argument("--trace", default=None, help="rocprofv3 kernel trace CSV of a --device-only run")
    ap.add_argument("--out", default=None, help="JSON file to write the summary to")
    args = ap.parse_args()
    if args.trace:
        doc = summarise(readTrace(args.trace))
        doc["method"] = ("rocprofv3 --kernel-trace of one --device-only run; per kernel and grid size the median over the "
                         "dispatches after the first")
        print(json.dumps(doc, indent=1))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")
        return
    if not args.device_only:
        ap.error("pass --device-only (under rocprofv3) or --trace")
    runWorkload(args.repeat)


if __name__ == "__main__":
    main()
