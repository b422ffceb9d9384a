#!/usr/bin/env python3
"""Time the uncertainty calls (calib_covariance, calib_view_errors) beside the host route they replace.

    python tools/time_uncertainty.py [--shapes c3 c5shard] [--repeat 20] [--host-repeat 3]
    rocprofv3 --kernel-trace --stats -d OUT -o unc -- python tools/time_uncertainty.py --shapes c5shard --device-only
    python tools/time_uncertainty.py --rates OUT/unc_results.db --shapes c5shard    (one shape per profiled run; the
                                      rocpd database rocprofv3 writes by default, or a kernel-stats CSV of --output-format csv)

Shapes: c3 (10 000 x 200 fisheye) and c5shard (125 000 x 88 radtan, one GPU's shard of c5). Per shape one JSON line.
Both routes run ALTERNATED in one process on the same resident problem, warmed up, the host clock around calls that
synchronise (every call here copies its result back):
  device   RefineEngine.covariance(P) (pose blocks, no cross block) and RefineEngine.viewErrors(P);
  host     the only route before these calls -- calib_normal_eq (every 768-byte record to the host, a C++ loop over
           the views) + the numpy Schur covariance, and calib_eval(out_r) (16 B per point to the host) + numpy
           reduceat sums.
--device-only runs just the device calls (what to put under rocprofv3); --rates turns the kernel timings of
such a run into each new kernel's algorithmic bytes over its mean duration, as a share of the ~6.3 TB/s a streaming
kernel reaches on this part (both kernels are HBM-bound: view_errors reads 40 B per point in fp64, covariance_views
reads 768 B -- 1536 B for a view with an overflow record -- and writes 288 B per view)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACHIEVABLE_HBM = 6.3e12
SHAPES = {"c3": ("c3", None), "c5shard": ("c5", 125000)}


def timed(fn, repeat):
    ts, out = [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts, out


def hostCovariance(eng, P, L):
    """the parent's route: normal equations to the host, Schur covariance in numpy -> (sigma2, Css, Cvv)"""
    B, E, V, g = eng.normalEquations(P)
    sse = eng.evaluate(P)["sse"]
    M = V.shape[0]
    dof = 2 * eng.MN - (L + 6 * M)
    sigma2 = sse / dof
    Vinv = np.linalg.inv(V)
    Y = Vinv @ np.transpose(E, (0, 2, 1))
    S = B - np.einsum("mlj,mjk->lk", E, Y)
    Css = sigma2 * np.linalg.inv(S)
    Cvv = sigma2 * Vinv + Y @ Css @ np.transpose(Y, (0, 2, 1))
    return sigma2, Css, Cvv


def hostViewErrors(eng, P, offs):
    r = eng.evaluate(P, wantR=True)["r"]
    e = np.sum(r * r, axis=1)
    sse = np.add.reduceat(e, offs[:-1])
    return sse, np.sqrt(sse / np.diff(offs)), np.sqrt(np.maximum.reduceat(e, offs[:-1]))


def stats(ts):
    return {"best_ms": round(min(ts), 3), "median_ms": round(float(np.median(ts)), 3), "n": len(ts)}


def rates(path, shape):
    """rocprofv3's kernel stats CSV (Name, Calls, TotalDurationNs, AverageNs, ...) of a --device-only run of ONE shape"""
    import camera_calibration_amd.synthetic as synthetic
    cfgName, views = SHAPES[shape]
    cfg = synthetic.CONFIGS[cfgName]
    M = views or cfg["views"]
    n = cfg["board"][0] * cfg["board"][1]
    nbytes = {"view_errors_kernel": M * n * 40 + M * 24, "covariance_views_kernel": M * (768 + 288)}
    if path.endswith(".db"):        # rocprofv3's default output: the rocpd database, its `kernels` view
        import sqlite3
        rows = [{"Name": n, "Calls": c, "AverageNs": a} for n, c, a in sqlite3.connect(path).execute(
            "select name, count(*), avg(end - start) from kernels group by name")]
    else:
        rows = list(csv.DictReader(open(path)))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        for key, b in nbytes.items():
            if key in name:
                avg = float(r.get("AverageNs") or 0.0) * 1e-9
                print(json.dumps({"shape": shape, "kernel": name.split("(")[0], "calls": int(float(r.get("Calls", 0))),
                                  "mean_us": round(avg * 1e6, 2), "bytes": b, "tb_per_s": round(b / avg / 1e12, 3),
                                  "share_of_achievable_hbm": round(b / avg / ACHIEVABLE_HBM, 3), "bound": "HBM"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["c3", "c5shard"], choices=sorted(SHAPES))
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--host-repeat", type=int, default=3, help="repetitions of the (slow) host route")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--rates", default=None, help="rocprofv3 results (.db, or a kernel stats CSV) of a --device-only run")
    args = ap.parse_args()
    if args.rates:
        if len(args.shapes) != 1:
            ap.error("--rates needs the one shape the profiled run used (--shapes c3 | c5shard)")
        rates(args.rates, args.shapes[0])
        return
    import camera_calibration_amd as cca
    from camera_calibration_amd import engine, synthetic
    for tag in args.shapes:
        cfgName, views = SHAPES[tag]
        sh = synthetic.makeShard(cfgName, numViews=views, noiseSigma=0.1)
        offs, s, m, P = sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"], sh["Ptrue"]
        eng = cca.RefineEngine(sh["model"], "f64")
        eng.setProblem(offs, s, m)
        L, M, MN = eng.L, eng.M, eng.MN
        dev = eng.covariance(P)                                # warm-up: code objects, buffers, clocks
        errs = eng.viewErrors(P)
        tCov, tErr, tHostCov, tHostErr = [], [], [], []
        host = hostErrs = None
        rounds = args.repeat if args.device_only else max(args.repeat, args.host_repeat)
        for i in range(rounds):                                # the routes alternate
            if i < args.repeat:
                tCov += timed(lambda: eng.covariance(P), 1)[0]
                tErr += timed(lambda: eng.viewErrors(P), 1)[0]
            if not args.device_only and i < args.host_repeat:
                t, host = timed(lambda: hostCovariance(eng, P, L), 1)
                tHostCov += t
                t, hostErrs = timed(lambda: hostViewErrors(eng, P, offs), 1)
                tHostErr += t
        out = {"shape": tag, "model": sh["model"], "views": M, "points": MN, "fused_form": eng.fusedForm(),
               "sigma": float(np.sqrt(dev["sigma2"])), "dof": dev["dof"],
               "calib_covariance": stats(tCov), "calib_view_errors": stats(tErr),
               "covariance_views_bytes": M * (768 + 288), "view_errors_bytes": MN * 40 + M * 24}
        if host is not None:
            out["host_normal_eq_numpy_schur"] = stats(tHostCov)
            out["host_eval_r_numpy_reduceat"] = stats(tHostErr)
            out["covariance_speedup"] = round(min(tHostCov) / min(tCov), 1)
            out["view_errors_speedup"] = round(min(tHostErr) / min(tErr), 1)
            sd = np.sqrt(np.einsum("mii->mi", host[2])).ravel()
            out["max_rel_std_diff_vs_host"] = float(max(
                np.abs(dev["std"][:L] / np.sqrt(np.diagonal(host[1])) - 1).max(), np.abs(dev["std"][L:] / sd - 1).max()))
            out["max_rel_view_sse_diff_vs_host"] = float(np.abs(errs["sse"] / hostErrs[0] - 1).max())
        eng.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
