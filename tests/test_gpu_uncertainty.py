"""Calibration uncertainty on the GPU: calib_covariance / calib_cov_local + calib_cov_finish / calib_view_errors
and the Python surface above them, against yardsticks written from the oracle's public pieces
(tests/uncertainty_yardstick.py: the dense Jacobian's QR for the covariance, reduceat over the oracle's residuals
for the per-view errors; the tolerance tol = 1e3 eps kappa is derived there).

fp32 storage has no derivable bound: the deviation from the same fp64 yardstick was measured on an MI355X and the
assertion is 10 x the measured worst case rounded up to a power of ten (F32_* below; the measured figures are in
DESIGN.md section 6)."""
import functools
import os
import socket

import numpy as np
import pytest

import camera_calibration_amd as cca
from camera_calibration_amd import _native as nat
from camera_calibration_amd import engine, fixed, synthetic
from conftest import loadGolden
from oracle import calib_oracle as orc
from uncertainty_yardstick import (bitsOf, checkCovariance, closeSse, correlation, covarianceYardstick,
                                   viewErrorsYardstick)

pytestmark = pytest.mark.gpu

STANDIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fake_rccl", "librccl_standin.so")

# fp32 storage against the fp64 yardstick, measured on an MI355X (worst case over the cases below):
#   covariance (g9 at Pfinal, g5-200 at P0): std / sigma relative 1.26e-5, correlations 1.04e-5 absolute;
#   sigma2 relative 1.35e-5;
#   per-view errors (g9, g5-200, the holed problem): sse relative 1.85e-4, rms relative 9.2e-5, max relative 2.17e-4
# asserted: 10 x the measured worst case, rounded up to a power of ten
F32_COV_TOL = 1e-3          # 10 x 1.26e-5 = 1.3e-4
F32_SIGMA2_RTOL = 1e-3      # 10 x 1.35e-5 = 1.4e-4
F32_VIEW_RTOL = 1e-2        # 10 x 2.17e-4 = 2.2e-3

CASES = {"g2_radtan": ("g2_config1_radtan.npz", "radtan", orc.RADTAN, "Pfinal"),
         "g2_fisheye": ("g2_config1_fisheye.npz", "fisheye", orc.FISHEYE, "Pfinal"),
         "g9": ("g9_noisy.npz", "radtan", orc.RADTAN, "Pfinal"),
         "g5_200": ("g5_ragged200.npz", "radtan", orc.RADTAN, "P0")}
MASK_KEYS = ("none", "gamma_lastk", "all")


def maskOf(key, name):
    names = fixed.sharedNames(engine.MODEL_IDS[name])
    sel = {"none": (), "gamma_lastk": ("gamma", names[-1]), "all": ("all",)}[key]
    return fixed.resolveFixed(names, sel)[0]


def problemOf(case):
    tag, name, model, at = CASES[case]
    g = loadGolden(tag)
    return name, model, g["viewOffsets"], g["sensorPoints"], g["modelPoints"], np.array(g[at], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def yardstickOf(case, mask):
    name, model, offs, s, m, P = problemOf(case)
    return covarianceYardstick(model, P, offs, s, m, bitsOf(mask))


def engineOf(case, dtype="f64", mode="fused", mask=0):
    name, model, offs, s, m, P = problemOf(case)
    eng = cca.RefineEngine(name, dtype)
    eng.setProblem(offs, s, m)
    eng.setLmMode(mode)
    eng.setFixedShared(mask)
    return eng, P


# ---- 1. covariance against the yardstick ------------------------------------------------------------------------
@pytest.mark.parametrize("key", MASK_KEYS)
@pytest.mark.parametrize("mode", ["fused", "two_kernel"])
@pytest.mark.parametrize("case", list(CASES))
def test_covariance_against_the_qr_yardstick(case, mode, key):
    name = CASES[case][1]
    mask = maskOf(key, name)
    F = bitsOf(mask)
    eng, P = engineOf(case, "f64", mode, mask)
    L, M = eng.L, eng.M
    res = eng.covariance(P, wantViews=True, wantCross=True)
    again = eng.covariance(P, wantViews=True, wantCross=True)
    stepped = None
    if key == "none":                                        # the stepping form on one shard is the same computation
        eng.covLocal(P)
        stepped = eng.covFinish(eng.MN, M, wantViews=True, wantCross=True)
    eng.close()
    yard = yardstickOf(case, mask)
    checkCovariance(res, yard, L, F, f"{case} {mode} {key}")
    for k in ("covShared", "covViews", "covCross", "std"):       # fixed-order sums: bitwise reproducible
        assert np.array_equal(res[k], again[k]), k
        if stepped is not None:
            assert np.array_equal(res[k], stepped[k]), k
    assert res["sigma2"] == again["sigma2"]
    assert np.array_equal(res["covShared"], res["covShared"].T)
    assert np.array_equal(res["covViews"], np.transpose(res["covViews"], (0, 2, 1)))
    assert np.array_equal(res["std"][:L], np.sqrt(np.diagonal(res["covShared"])))
    assert np.array_equal(res["std"][L:].reshape(M, 6), np.sqrt(np.einsum("mii->mi", res["covViews"])))
    if key == "all":
        # only the poses are free: dof = 2 n - 6 M and C_vv,i = sigma2 V_i^-1
        name_, model, offs, s, m, _ = problemOf(case)
        assert res["dof"] == 2 * int(offs[-1]) - 6 * M
        assert not res["covShared"].any() and not res["covCross"].any()
        Jc = orc.jacobianCompact(model, P, offs, m)
        r = s - orc.projectAllPoints(model, P, offs, m)
        _, _, V, _ = orc.normalBlocks(model, Jc, r, offs)
        worst = 0.0
        for i in range(M):
            worst = max(worst, np.abs(correlation(res["covViews"][i]) - correlation(np.linalg.inv(V[i]))).max())
        print(f"{case} {mode} all: max |d corr| of C_vv vs sigma2 V^-1 {worst:.3e}")
        assert worst <= yard["tol"]


# ---- 2. the stream form -------------------------------------------------------------------------------------------
def test_covariance_in_the_stream_form(monkeypatch):
    """A uniform c5-shaped shard (88-point views) in the stream form of the fused kernel, where wave starts cut views in
    two records: against the same engine with CALIB_FUSED_STREAM=0 (standard deviations to 1e-12 relative), and --
    the shard being a 500-view slice of the config's views -- against the dense yardstick."""
    sh = synthetic.makeShard(dict(synthetic.CONFIGS["c5"]), viewStart=7, numViews=500, noiseSigma=0.1)
    offs, s, m, P = sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"], sh["Ptrue"]
    outs = {}
    monkeypatch.setenv("CALIB_STREAM_WAVES", "37")          # 11 000 groups in shares of 298: wave starts fall inside views
    for stream in ("1", "0"):
        monkeypatch.setenv("CALIB_FUSED_STREAM", stream)
        eng = cca.RefineEngine("radtan", "f64")
        eng.setProblem(offs, s, m)
        share, waves = eng.fusedForm()
        assert (share > 0) == (stream == "1")
        if stream == "1":
            n4 = 88 // 4
            cut = sum(1 for w in range(1, waves) if (w * share) % n4 != 0 and w * share < 500 * n4)
            print(f"stream form: share {share} groups, {waves} waves, {cut} views cut by a wave start")
            assert cut > 0
        outs[stream] = eng.covariance(P, wantViews=True, wantCross=True)
        eng.close()
    a, b = outs["1"], outs["0"]
    rel = np.abs(a["std"] - b["std"]) / b["std"]
    print(f"stream vs one view per wave: max rel d std {rel.max():.3e}, sigma2 {a['sigma2']:.15e} / {b['sigma2']:.15e}")
    assert rel.max() <= 1e-12
    assert a["dof"] == b["dof"] and abs(a["sigma2"] - b["sigma2"]) <= 1e-12 * b["sigma2"]
    yard = covarianceYardstick(orc.RADTAN, P, offs, s, m)
    checkCovariance(a, yard, 10, (), "stream form, 500 views")


# ---- 3. statistics on g9 ------------------------------------------------------------------------------------------
def test_g9_noise_estimate_and_z_scores():
    """g9 has noise sigma = 0.1 px and 15 views: the noise estimate must come out at 0.1 within five of its own
    standard deviations' worth of slack, |sigma - 0.1| <= 5 * 0.1 / sqrt(2 dof) (= 0.0031; the estimator's spread is
    0.0006, the reference's value 0.09974), every shared parameter of Pfinal within 5 standard deviations of the truth
    (largest |z| of the yardstick: 2.40), rms = 0.140502."""
    g = loadGolden("g9_noisy.npz")
    eng, P = engineOf("g9")
    res = eng.covariance(P)
    errs = eng.viewErrors(P)
    eng.close()
    sigma, dof = np.sqrt(res["sigma2"]), res["dof"]
    A, k = g["Atrue"], g["ktrue"]
    truth = np.array([A[0, 0], A[1, 1], A[0, 1], A[0, 2], A[1, 2]] + list(k))
    z = (P[:10] - truth) / res["std"][:10]
    rms = np.sqrt(errs["sse"].sum() / int(g["viewOffsets"][-1]))
    print(f"g9: sigma {sigma:.6f} dof {dof} max |z| {np.abs(z).max():.3f} rms {rms:.6f}")
    assert abs(sigma - 0.1) <= 5 * 0.1 / np.sqrt(2 * dof)
    assert np.abs(z).max() <= 5.0
    assert abs(rms - 0.140502) <= 5e-7
    assert closeSse(errs["sse"].sum(), res["sigma2"] * dof)


# ---- 4. per-view errors ---------------------------------------------------------------------------------------------
def holedProblem():
    """g2 radtan with view 3 emptied and view 5 cut down to one point"""
    g = loadGolden("g2_config1_radtan.npz")
    offs, s, m = g["viewOffsets"], g["sensorPoints"], g["modelPoints"]
    keep = np.ones(int(offs[-1]), dtype=bool)
    keep[offs[3]:offs[4]] = False
    keep[offs[5] + 1:offs[6]] = False
    n = np.diff(offs).copy()
    n[3], n[5] = 0, 1
    return np.concatenate(([0], np.cumsum(n))).astype(np.int64), s[keep], m[keep], g["P0"]


def checkViewErrors(got, want, label, rtol=None):
    sse, rms, mx = want
    empty = np.isnan(rms)
    dS = np.abs(got["sse"] - sse)
    dM = np.abs(got["max"] - mx)
    with np.errstate(invalid="ignore"):
        dR = np.abs(got["rms"][~empty] - rms[~empty]) / np.where(rms[~empty] > 0, rms[~empty], 1.0)
    print(f"{label}: max d sse {dS.max():.3e} (rel {np.max(dS / np.maximum(sse, 1e-300)):.3e}), max rel d rms "
          f"{dR.max():.3e}, max d max {dM.max():.3e} px (rel {np.max(dM / np.maximum(mx, 1e-300)):.3e})")
    assert np.array_equal(np.isnan(got["rms"]), empty), label
    assert not got["sse"][empty].any() and not got["max"][empty].any(), label
    if rtol is None:
        assert np.all(dS <= np.maximum(1e-9 * sse, 1e-13)), label
        assert np.all(dR <= 1e-9), label
        assert np.all(dM <= 1e-9), label                     # pixels
    else:
        assert np.all(dS <= rtol * sse), label
        assert np.all(dR <= rtol), label
        assert np.all(dM <= rtol * mx), label


@pytest.mark.parametrize("case", ["g9", "g5_200", "holed"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_view_errors_against_the_yardstick(case, dtype):
    if case == "holed":
        name, model = "radtan", orc.RADTAN
        offs, s, m, P = holedProblem()
    else:
        name, model, offs, s, m, P = problemOf(case)
    eng = cca.RefineEngine(name, dtype)
    eng.setProblem(offs, s, m)
    got = eng.viewErrors(P)
    again = eng.viewErrors(P)
    sseAll = eng.evaluate(P)["sse"]
    eng.close()
    for k in ("sse", "rms", "max"):
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    checkViewErrors(got, viewErrorsYardstick(model, P, offs, s, m), f"{case} {dtype}",
                    None if dtype == "f64" else F32_VIEW_RTOL)
    # calib_eval's sum over all points: the same residuals in fp64; in fp32 the two kernels' projections differ by
    # fp32 rounding (the compiler contracts them differently), which the fp32 bar covers
    assert abs(got["sse"].sum() - sseAll) <= (1e-12 if dtype == "f64" else F32_VIEW_RTOL) * sseAll
    if case == "holed":
        assert np.isnan(got["rms"][3]) and got["sse"][3] == 0.0 and got["max"][3] == 0.0
        assert got["rms"][5] == np.sqrt(got["sse"][5]) and abs(got["max"][5] - got["rms"][5]) <= 1e-15 * got["rms"][5]


@pytest.mark.parametrize("case", ["g9", "g5_200"])
def test_covariance_with_fp32_storage(case):
    """fp32 storage evaluates its own Jacobian; sums and everything after them are fp64. Against the fp64 yardstick at
    the measured tolerance (module docstring)."""
    eng, P = engineOf(case, "f32")
    res = eng.covariance(P, wantViews=True, wantCross=True)
    eng.close()
    yard = yardstickOf(case, 0)
    rel = abs(res["sigma2"] - yard["sigma2"]) / yard["sigma2"]
    print(f"{case} f32: rel d sigma2 {rel:.3e}")
    assert res["dof"] == yard["dof"] and rel <= F32_SIGMA2_RTOL
    # (sigma2 has its own fp32 bar above: the yardstick's sse is replaced so that the fp64 bar inside is not applied)
    checkCovariance(res, dict(yard, sse=res["sigma2"] * res["dof"]), eng.L, (), f"{case} f32", tol=F32_COV_TOL)


# ---- 5. errors -----------------------------------------------------------------------------------------------------
def test_error_codes():
    g = loadGolden("g2_config1_radtan.npz")
    offs, s, m, P = g["viewOffsets"], g["sensorPoints"], g["modelPoints"], g["Pfinal"]
    # a view with two points: its 6 x 6 block is singular
    keep = np.ones(int(offs[-1]), dtype=bool)
    keep[offs[4] + 2:offs[5]] = False
    n = np.diff(offs).copy()
    n[4] = 2
    eng = cca.RefineEngine("radtan", "f64")
    eng.setProblem(np.concatenate(([0], np.cumsum(n))).astype(np.int64), s[keep], m[keep])
    with pytest.raises(np.linalg.LinAlgError):
        eng.covariance(P)
    assert np.isfinite(eng.viewErrors(P)["rms"]).all()       # the errors of such a view are well defined
    # 2 n <= free parameters: one view of 7 points (spread over the board) has 14 residuals for 16 parameters
    idx = np.array([0, 4, 8, 22, 27, 45, 53])
    eng.setProblem(np.array([0, 7], dtype=np.int64), s[idx], m[idx])
    with pytest.raises(ValueError):
        eng.covariance(P[:16])
    eng.setFixedShared(("all",))                             # 6 free parameters: dof = 8
    assert eng.covariance(P[:16])["dof"] == 8
    eng.setFixedShared(())
    # covFinish without covLocal, and every call while a stepping LM run is active
    eng.setProblem(offs, s, m)
    with pytest.raises(nat.CalibNativeError, match="calib_cov_local"):
        eng.covFinish(eng.MN, eng.M)
    eng.lmBegin(g["P0"], 5)
    eng.lmRun(2)
    for call in (lambda: eng.covariance(P), lambda: eng.covLocal(P), lambda: eng.covFinish(eng.MN, eng.M),
                 lambda: eng.viewErrors(P)):
        with pytest.raises(nat.CalibNativeError, match="-4"):
            call()
    eng.lmRun(4)
    assert eng.lmEnd()[2] >= 1                               # the run was not disturbed
    assert eng.covariance(P)["dof"] == 2 * eng.MN - eng.K
    eng.close()


# ---- 6. end to end ------------------------------------------------------------------------------------------------
def test_calibrate_camera_extended_on_g9():
    g = loadGolden("g9_noisy.npz")
    offs, s, m = g["viewOffsets"], g["sensorPoints"], g["modelPoints"]
    dets = [(s[a:b].copy(), m[a:b].copy()) for a, b in zip(offs[:-1], offs[1:])]
    maxIters = int(g["maxIters"])
    sse, A, W, k = cca.calibrateCamera(dets, "radtan", maxIters)
    sseX, AX, WX, kX, unc = cca.calibrateCameraExtended(dets, "radtan", maxIters)
    assert sse == sseX and np.array_equal(A, AX) and np.array_equal(k, kX)
    assert len(W) == len(WX) and all(np.array_equal(a, b) for a, b in zip(W, WX))
    cal = cca.Calibrator(cca.RadialTangentialModel())
    out = cal.calibrateExtended(dets, maxIters)
    uploads = cal._resident.uploads
    later = cal.uncertainty(out[1], out[2], out[3], dets)
    assert cal._resident.uploads == uploads                  # the resident problem was used
    cal.close()
    for u in (unc, later):
        assert isinstance(u, cca.CalibrationUncertainty)
        for f in ("stdShared", "covShared", "stdPoses", "covPoses", "perViewRms", "perViewMax"):
            assert np.array_equal(getattr(u, f), getattr(out[4], f)), f
        assert (u.sigma, u.dof, u.rms) == (out[4].sigma, out[4].dof, out[4].rms)
    assert unc.names == cca.RadialTangentialModel().sharedParameterNames()
    assert unc.covPoses.shape == (15, 6, 6) and unc.perViewRms.shape == (15,)
    assert np.array_equal(np.diagonal(unc.correlationShared()), np.ones(10))
    text = unc.summary()
    print(text)
    assert all(sum(ln.startswith(n + " = ") for ln in text.splitlines()) == 1 for n in unc.names)
    # a fixed parameter is honoured and printed as such
    cal = cca.Calibrator(cca.RadialTangentialModel(), fixed={"skew": 0.0})
    uF = cal.calibrateExtended(dets, maxIters)[4]
    cal.close()
    assert uF.stdShared[2] == 0.0 and not uF.covShared[2].any() and "gamma = 0 (fixed)" in uF.summary()
    assert uF.dof == unc.dof + 1


# ---- 7. two ranks on one GPU ------------------------------------------------------------------------------------------
def _freePort():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def _worker(rank, world, port, allreduce, outDir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0", RANK=str(rank),
                      WORLD_SIZE=str(world), CALIB_ALLREDUCE=allreduce, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if allreduce == "direct":
        os.environ["CALIB_RCCL_LIBRARY"] = STANDIN
    import torch.distributed as dist
    from camera_calibration_amd import distributed
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = loadGolden("g9_noisy.npz")
        sse, P, iters, trace, unc = distributed.refineDistributed(
            "radtan", g["Pfinal"], g["viewOffsets"], g["sensorPoints"], g["modelPoints"], 5, uncertainty=True)
        np.savez(os.path.join(outDir, f"r{rank}.npz"), P=P, kind=distributed.refineDistributed.lastAllReduce,
                 sigma2=unc["sigma2"], dof=unc["dof"], covShared=unc["covShared"], covViews=unc["covViews"], std=unc["std"])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("allreduce", ["direct", "torch"])
def test_sharded_uncertainty_two_ranks_on_one_gpu(tmp_path, allreduce):
    """refineDistributed(..., uncertainty=True) with real engines, two fresh child processes on GPU 0, the one sum
    carried by the library's own ncclAllReduce through the stand-in librccl (calib_lm_allreduce between
    calib_cov_local and calib_cov_finish) or by torch.distributed over gloo."""
    import torch.multiprocessing as mp
    if allreduce == "direct" and not os.path.exists(STANDIN):
        pytest.fail(f"{STANDIN} is missing: __graft_entry__.build() (make -C tests/fake_rccl) builds it")
    world = 2
    mp.spawn(_worker, args=(world, _freePort(), allreduce, str(tmp_path)), nprocs=world, join=True)
    outs = [np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(world)]
    for o in outs:
        assert str(o["kind"]) == allreduce
        assert np.array_equal(o["covShared"], outs[0]["covShared"])          # bitwise equal on both ranks
        assert np.array_equal(o["covViews"], outs[0]["covViews"]) and np.array_equal(o["std"], outs[0]["std"])
        assert float(o["sigma2"]) == float(outs[0]["sigma2"]) and int(o["dof"]) == int(outs[0]["dof"])
    o = outs[0]
    P = o["P"]
    g = loadGolden("g9_noisy.npz")
    eng = cca.RefineEngine("radtan", "f64")
    eng.setProblem(g["viewOffsets"], g["sensorPoints"], g["modelPoints"])
    single = eng.covariance(P)
    eng.close()
    tol = yardstickOf("g9", 0)["tol"]                        # kappa of the same Jacobian to working precision
    relStd = np.abs(o["std"] - single["std"]) / single["std"]
    dS = np.abs(correlation(o["covShared"]) - correlation(single["covShared"])).max()
    dV = max(np.abs(correlation(a) - correlation(b)).max() for a, b in zip(o["covViews"], single["covViews"]))
    print(f"two ranks ({allreduce}) vs one process: max rel d std {relStd.max():.3e}, max |d corr| shared {dS:.3e} views "
          f"{dV:.3e}, tol {tol:.3e}")
    assert int(o["dof"]) == single["dof"] and closeSse(float(o["sigma2"]) * single["dof"], single["sigma2"] * single["dof"])
    assert relStd.max() <= tol and dS <= tol and dV <= tol
