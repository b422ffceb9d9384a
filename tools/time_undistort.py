#!/usr/bin/env python3
"""Time the undistortion calls and, from a profiled run, their three kernels.

    python tools/time_undistort.py [--repeat 20] [--out profiles/undistort_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o und -- python tools/time_undistort.py --device-only
    python tools/time_undistort.py --rates OUT/.../und_kernel_stats.csv --out profiles/undistort_bench.json
    ... --width 3840 --height 2160 on all three: another image size, merged under "calls_3840x2160" / "kernels_3840x2160"

Workload: a 1920 x 1080 camera of each model (the coefficients of the benchmark configs; focal length 1000 px for
radtan and 1600 px for fisheye, whose theta_d must stay below the 0.80 at which that polynomial turns for every pixel to
have a preimage): the rectify maps (calib_undistort_maps), a 3-channel uint8 image of that size resampled through them
(calib_remap) and 10^6 pixels drawn uniformly from the image taken back to normalised points (calib_undistort_points).

The entry points take HOST arrays, so a call's time -- the host clock around a call that ends in its copy back -- is
mostly allocation and PCIe copies; it is reported as `calls` and is no statement about a kernel. The kernels' own times
come from a rocprofv3 kernel trace of a --device-only run; --rates turns them into each kernel's algorithmic bytes over
its mean duration and the share of the ~6.3 TB/s a streaming kernel reaches on this part:
  undistort_map_kernel     writes 8 B per pixel (two fp32 planes), reads nothing of size;
  remap_kernel             reads 8 B of map and writes C bytes per destination pixel, and reads the source once
                           (H W C bytes: neighbouring pixels share taps, so the rest of the gather is cache traffic);
  undistort_points_kernel  reads 16 B and writes 20 B per point.
--out merges what this run produced ("calls" or "kernels") into the JSON file, keeping the other part."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACHIEVABLE_HBM = 6.3e12
WIDTH, HEIGHT, CHANNELS, POINTS = 1920, 1080, 3, 1000000
FOCAL = {"radtan": 1000.0, "fisheye": 1600.0}           # at 1920 columns; scaled with the width


def kernelBytes(width, height):
    return {"undistort_map_kernel": width * height * 8,
            "remap_kernel": width * height * (8 + CHANNELS) + width * height * CHANNELS,
            "undistort_points_kernel": POINTS * 36}


def stats(ts):
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "n": len(ts)}


def rates(path, width, height):
    """rocprofv3's kernel stats CSV (Name, Calls, TotalDurationNs, AverageNs, ...) of a --device-only run"""
    out = []
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        for key, b in kernelBytes(width, height).items():
            if key in name:
                avg = float(r.get("AverageNs") or 0.0) * 1e-9
                out.append({"kernel": name.split("(")[0], "calls": int(float(r.get("Calls", 0))),
                            "mean_us": round(avg * 1e6, 2), "bytes": b, "tb_per_s": round(b / avg / 1e12, 3),
                            "share_of_achievable_hbm": round(b / avg / ACHIEVABLE_HBM, 3)})
    return sorted(out, key=lambda d: d["kernel"])


def merge(path, key, value, width, height):
    doc = {}
    if os.path.exists(path):
        doc = json.load(open(path))
    doc[key if (width, height) == (WIDTH, HEIGHT) else f"{key}_{width}x{height}"] = value
    doc["workload"] = {"width": WIDTH, "height": HEIGHT, "channels": CHANNELS, "image_dtype": "uint8", "points": POINTS,
                       "achievable_hbm_bytes_per_s": ACHIEVABLE_HBM}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--device-only", action="store_true", help="few calls, no timing: what to put under rocprofv3")
    ap.add_argument("--rates", default=None, help="rocprofv3 kernel stats CSV of a --device-only run")
    ap.add_argument("--out", default=None, help="JSON file to merge the results into")
    ap.add_argument("--width", type=int, default=WIDTH)
    ap.add_argument("--height", type=int, default=HEIGHT)
    args = ap.parse_args()
    width, height = args.width, args.height
    if args.rates:
        rows = rates(args.rates, width, height)
        for r in rows:
            print(json.dumps(r))
        if args.out:
            merge(args.out, "kernels", rows, width, height)
        return
    import camera_calibration_amd as cca
    from camera_calibration_amd import synthetic, undistort
    rng = np.random.default_rng(0)
    image = rng.integers(0, 256, (height, width, CHANNELS), dtype=np.uint8)
    uv = rng.uniform((0.0, 0.0), (width - 1.0, height - 1.0), (POINTS, 2))
    repeat = 5 if args.device_only else args.repeat
    calls = []
    for name, cls, k in (("radtan", cca.RadialTangentialModel, synthetic.RADTAN_K),
                         ("fisheye", cca.FisheyeModel, synthetic.FISHEYE_K)):
        model = cls()
        focal = FOCAL[name] * width / WIDTH
        camera = np.array([[focal, 0.0, (width - 1) / 2], [0.0, focal, (height - 1) / 2], [0.0, 0.0, 1.0]])
        mapx, mapy = model.undistortMaps(camera, k, (width, height))        # warm-up: code objects, clocks
        out = undistort.remap(image, mapx, mapy)
        xy, status = model.undistortPoints(camera, k, uv, returnStatus=True)
        tMap, tRemap, tPts = [], [], []
        for _ in range(repeat):
            t0 = time.perf_counter()
            model.undistortMaps(camera, k, (width, height))
            t1 = time.perf_counter()
            undistort.remap(image, mapx, mapy)
            t2 = time.perf_counter()
            model.undistortPoints(camera, k, uv)
            t3 = time.perf_counter()
            tMap.append((t1 - t0) * 1e3)
            tRemap.append((t2 - t1) * 1e3)
            tPts.append((t3 - t2) * 1e3)
        line = {"model": name, "width": width, "height": height, "focal_px": focal, "calib_undistort_maps": stats(tMap), "calib_remap": stats(tRemap),
                "calib_undistort_points": stats(tPts), "points_not_solved": int(status.sum()),
                "remap_pixels_at_border": int((out == 0).all(axis=2).sum()),
                "note": "host clock around calls on host arrays: allocation + copies + kernel"}
        calls.append(line)
        print(json.dumps(line), flush=True)
    if args.out and not args.device_only:
        merge(args.out, "calls", calls, width, height)


if __name__ == "__main__":
    main()
