"""The initialisation kernels -- dlt_kernel, homography_lm_kernel, extrinsics_kernel, distortion_normal_kernel,
compose_views_kernel / decompose_views_kernel -- on sparse, noisy and many views, against host numpy
(tests/init_yardstick.py; its inputs are checked without a GPU by tests/test_init_yardstick_cpu.py).

What the other GPU tests leave open: they run these kernels on 10 or 15 full 9 x 6 boards, i.e. in workgroup 0 of a
one-workgroup grid with every lane of every view loaded, never in a second 256-thread block, never on a second trip of
distortion_normal_kernel's grid-stride loop, and compare D^T D only through the solved k. Every test prints what it
measured (pytest -s)."""
import numpy as np
import pytest

import camera_calibration_amd as cca
import init_yardstick as iy
from camera_calibration_amd import engine, linearcalibrate as lc, mathutils as mu
from oracle import calib_oracle as orc

pytestmark = pytest.mark.gpu
MODELS = ("radtan", "fisheye")
LM_ERROR_MIN = 1e-12          # src/calibrate.py:16: below this error the LM stops; smaller errors are rounding to it


def reprojections(Hs, v):
    return np.vstack([iy.project(H, m) for H, (s, m) in zip(Hs, iy.detections(v))])


def perView(x, v):
    """max |x| over each view's points"""
    return np.array([np.abs(x[a:b]).max() for a, b in zip(v["offs"][:-1], v["offs"][1:])])


# ---------------------------------------------------------------- DLT
@pytest.mark.parametrize("model,sigma", iy.R_VARIANTS)
def test_dlt_on_sparse_and_noisy_views_vs_the_svd(model, sigma):
    """engine.estimateHomographies(refineIters=0) on R (83 views of 4..130 points, six workgroups) against
    lc.estimateHomographies on its SVD route, at the bars of test_device_homographies_on_the_references_stored_detections:
    per view |H - H_svd| <= 1e-8 max|H_svd| and the view's own model points reproject to 1e-6 px.

    Measured on an MI355X, worst view per variant, |H - H_svd| / max|H_svd| and reprojections in px, with the kernel's 8
    inverse iterations -- and with the 4 it had, where tests/init_yardstick.py's emulation of the algorithm gave the same:
      radtan   0    px  1.60e-14  1.2e-12      4 iterations: 1.31e-07  7.5e-06   (emulation 1.31e-07)
      radtan   0.3  px  9.53e-15  1.5e-12                    1.33e-07  7.7e-06   (1.33e-07)
      radtan   1.5  px  6.74e-15  1.0e-12                    1.47e-07  8.6e-06   (1.47e-07)
      fisheye  0    px  4.61e-15  5.7e-13                    9.98e-08  8.6e-06   (9.98e-08)
      fisheye  0.3  px  1.13e-14  1.4e-12                    1.00e-07  8.6e-06   (1.00e-07)
      fisheye  1.25 px  1.38e-14  1.8e-12                    1.05e-07  9.1e-06   (1.05e-07)"""
    v = iy.problemR(model, sigma)
    assert iy.hostSvdRoute(v)
    Hsvd = iy.hostHomographies(model, sigma)
    H = engine.estimateHomographies(v["offs"], v["s"], v["m"], refineIters=0)
    assert H.shape == (iy.R_NUM_VIEWS, 3, 3)
    rel = np.abs(H - Hsvd).max(axis=(1, 2)) / np.abs(Hsvd).max(axis=(1, 2))
    dy = perView(reprojections(H, v) - reprojections(Hsvd, v), v)
    counts = iy.rCounts()
    print(f"\nDLT {model} {sigma} px: worst |H - H_svd| / max|H_svd| = {rel.max():.2e} (view {rel.argmax()}, "
          f"{counts[rel.argmax()]} points; {int((rel > 1e-8).sum())} views past 1e-8), reprojections {dy.max():.2e} px "
          f"(view {dy.argmax()}, {counts[dy.argmax()]} points)")
    assert np.isfinite(H).all()
    assert np.all(rel <= 1e-8), (rel.max(), np.nonzero(rel > 1e-8)[0])
    assert np.all(dy <= 1e-6), (dy.max(), np.nonzero(dy > 1e-6)[0])
    assert np.all(H[:, 2, 2] == 1.0)
    assert np.array_equal(H, engine.estimateHomographies(v["offs"], v["s"], v["m"], refineIters=0))


def test_dlt_refuses_a_three_point_view_among_good_ones():
    v = iy.problemR("radtan", 0.3)
    offs = v["offs"].copy()
    offs[41] = offs[42] - 3                      # view 40 gains the points view 41 loses: view 41 keeps 3
    assert offs[42] - offs[41] == 3 and np.all(np.diff(offs) >= 3) and (np.diff(offs) < 4).sum() == 1
    with pytest.raises(ValueError, match="at least 4"):          # CALIB_E_INVALID
        engine.estimateHomographies(offs, v["s"], v["m"], refineIters=0)
    with pytest.raises(ValueError, match="at least 4"):
        engine.estimateHomographies(offs, v["s"], v["m"], refineIters=20)


# ---------------------------------------------------------------- LM polish
@pytest.mark.parametrize("model,sigma", iy.R_VARIANTS)
def test_homography_lm_on_sparse_and_noisy_views_vs_the_host(model, sigma):
    """engine.refineHomographies against lc.refineHomographies from the same (host SVD) start, on the views of R where
    the host agrees with itself (iy.undecidedViews lists the others): H to 1e-5, reprojections to 1e-6 px (the bars of
    test_homography_lm_on_device_vs_reference), the view's final error to 1e-9 relative -- of max(error, 1e-12): below
    1e-12 the LM itself stops, and the four-point views end there. Two calls are equal to the bit.

    Measured on an MI355X on the compared views, |H - H_host|, reprojections in px, final error relative:
      radtan   0    px  1.91e-06  1.3e-07  4.4e-14        fisheye  0    px  9.16e-07  8.3e-08  4.9e-14
      radtan   0.3  px  1.66e-06  1.1e-07  1.4e-13        fisheye  0.3  px  8.76e-07  8.0e-08  1.1e-13
      radtan   1.5  px  9.64e-07  8.0e-08  5.3e-14        fisheye  1.25 px  7.43e-07  9.1e-08  5.0e-14
    This test found homography_lm_kernel's accept test too noisy: with residuals m - t / w rounded like any quotient, view 4
    of radtan 1.5 px (16 points, final error 950 px^2, a digit gained per step) had its 7th step, which lowers the error by
    2e-12, rejected for good and ended 1.77e-5 from the host in H. The kernel now forms the residuals from two-double sums
    (DESIGN.md section 2); the view follows the host to 2.3e-13 through all 8 of its iterations."""
    v = iy.problemR(model, sigma)
    H0 = iy.hostHomographies(model, sigma)
    Hh = iy.hostPolish(model, sigma)
    undecided = list(iy.undecidedViews(model, sigma))
    decided = np.setdiff1d(np.arange(iy.R_NUM_VIEWS), undecided)
    Hd = engine.refineHomographies(H0, v["offs"], v["s"], v["m"])
    dH = np.abs(Hd - Hh).max(axis=(1, 2))
    dy = perView(reprojections(Hd, v) - reprojections(Hh, v), v)
    dets = iy.detections(v)
    eD = np.array([iy.viewError(H, s, m) for H, (s, m) in zip(Hd, dets)])
    eH = np.array([iy.viewError(H, s, m) for H, (s, m) in zip(Hh, dets)])
    dE = np.abs(eD - eH) / np.maximum(eH, LM_ERROR_MIN)
    print(f"\nLM polish {model} {sigma} px: {len(undecided)} undecided views skipped {undecided}; on the other "
          f"{len(decided)}: |H - H_host| {dH[decided].max():.2e}, reprojections {dy[decided].max():.2e} px, "
          f"final error {dE[decided].max():.2e} relative"
          + (f"; on the skipped ones {dH[undecided].max():.2e}, {dy[undecided].max():.2e} px, {dE[undecided].max():.2e}"
             if undecided else ""))
    assert len(undecided) <= 0.05 * iy.R_NUM_VIEWS
    assert np.isfinite(Hd).all() and np.all(Hd[:, 2, 2] == 1.0)
    assert np.all(dH[decided] <= 1e-5), np.nonzero(dH > 1e-5)[0]
    assert np.all(dy[decided] <= 1e-6), np.nonzero(dy > 1e-6)[0]
    assert np.all(dE[decided] <= 1e-9), np.nonzero(dE > 1e-9)[0]
    assert np.array_equal(Hd, engine.refineHomographies(H0, v["offs"], v["s"], v["m"]))


@pytest.mark.parametrize("model,sigma", iy.R_VARIANTS)
def test_homography_lm_with_empty_views_spliced_in(model, sigma):
    """The batch of the test above with empty views at the front, in the middle and at the end (check_views allows them
    for the refine entry point; the kernel's loop takes no trip): every other view keeps its bits from the run without
    them, an empty view returns its input over its own [2,2]."""
    v = iy.problemR(model, sigma)
    H0 = iy.hostHomographies(model, sigma)
    Hd = engine.refineHomographies(H0, v["offs"], v["s"], v["m"])
    e, keep, empty, He = iy.withEmptyViews(v, H0)
    out = engine.refineHomographies(He, e["offs"], e["s"], e["m"])
    assert np.array_equal(out[keep], Hd)
    assert np.array_equal(out[empty], He[empty] / He[empty][:, 2:3, 2:3])
    with pytest.raises(ValueError):              # the DLT entry point has no answer for an empty view
        engine.estimateHomographies(e["offs"], e["s"], e["m"], refineIters=0)


# ---------------------------------------------------------------- extrinsics
def test_extrinsics_in_seventeen_blocks_with_scaled_and_negated_homographies():
    """engine.computeExtrinsics on 4 099 views (16 blocks of 256 and 3 threads): the host-polished homographies of R
    at its largest sigma, each copy times its own scale in [0.25, 4], negative on every third. |A^-1 h0| absorbs the
    magnitude. A negative scale negates r0, r1 and t and leaves r2 = r0 x r1: lc.computeExtrinsics (SVD) and the kernel
    (Newton's polar iteration) both return that proper rotation with the board behind the camera. Bars of
    test_device_initialisation_stages_vs_reference: 1e-12 on W, 1e-14 on R R^T - I."""
    H, scale, A = iy.extrinsicsInput()
    Wd = engine.computeExtrinsics(H, A)
    Wh = np.array(lc.computeExtrinsics(H, A))
    assert Wd.shape == (iy.EXT_VIEWS, 4, 4)
    dW = np.abs(Wd - Wh).max(axis=(1, 2))
    R = Wd[:, :3, :3]
    orth = np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max(axis=(1, 2))
    det = np.linalg.det(R)
    print(f"\nextrinsics: |W - W_host| {dW.max():.2e} (view {dW.argmax()}, last block {dW[4096:].max():.2e}), "
          f"R R^T - I {orth.max():.2e}, det R in [{det.min():.15f}, {det.max():.15f}]")
    assert np.all(dW < 1e-12), np.nonzero(dW >= 1e-12)[0][:10]
    assert np.all(orth < 1e-14)
    assert np.all(det > 0)
    assert np.all(Wd[:, 3, :] == np.array([0.0, 0.0, 0.0, 1.0]))
    # the scale leaves nothing behind but its sign
    W1 = engine.computeExtrinsics(H / np.abs(scale)[:, None, None], A)
    assert np.abs(Wd - W1).max() < 1e-12
    neg = scale < 0
    W83 = engine.computeExtrinsics(iy.hostPolish("radtan", iy.R_SIGMAS["radtan"][-1]), A)[np.arange(iy.EXT_VIEWS) % 83]
    flip = np.where(neg[:, None, None], np.array([-1.0, -1.0, 1.0, -1.0]), 1.0)
    assert np.abs(Wd[:, :3, :] - W83[:, :3, :] * flip).max() < 1e-12
    assert np.all((Wd[:, 2, 3] < 0) == neg)      # behind the camera exactly where the scale was negative


# ---------------------------------------------------------------- distortion normal equations
@pytest.mark.parametrize("case", ("empty", "big"))
@pytest.mark.parametrize("model", MODELS)
def test_distortion_normal_equations_vs_longdouble_rows(model, case):
    """engine.distortionNormalEquations against D^T D and D^T Ddot of iy.distortionRows in longdouble.
    empty: R at 0.3 px with empty views at the front, in the middle and at the end, every view with its own pose -- a
    slipped view index shows. big: 4 855 views of 54 points, 262 170 points -- the grid is capped at 1 024 workgroups and
    threads 0..25 of workgroup 0 take a second trip. Bars: DtD[a,b] to 1e-11 sqrt(DtD[a,a] DtD[b,b]) (the columns span
    r^2 .. r^6; a bar on the largest entry would not see the small ones), Dtd[a] to 1e-11 sum_i |D[i,a] Ddot[i]|; the
    solved k to 1e-7 max(1, |k|), the bar of test_device_initialisation_stages_vs_reference."""
    v = iy.distortionCaseEmpty(model) if case == "empty" else iy.distortionCaseBig(model)
    modelId = iy.MODEL_IDS[model]
    DtD, Dtd, barG, barg, r = iy.normalEquationsYardstick(v)
    G, g = engine.distortionNormalEquations(modelId, v["offs"], v["s"], v["m"], v["A"], v["W"])
    ld = np.longdouble
    relG = (np.abs(G.astype(ld) - DtD) / barG).max() * 1e-11
    relg = (np.abs(g.astype(ld) - Dtd) / barg).max() * 1e-11
    kD = np.array(lc.solveDistortionNormalEquations(G, g))
    kY = np.array(lc.solveDistortionNormalEquations(DtD.astype(np.float64), Dtd.astype(np.float64)))
    print(f"\ndistortion sums {model} {case} ({int(v['offs'][-1])} points): DtD {float(relG):.2e} of sqrt(DtD[a,a] DtD[b,b]), "
          f"Dtd {float(relg):.2e} of sum |D Ddot|, k {np.abs(kD - kY).max():.2e} (|k| <= {np.abs(kY).max():.2e})")
    assert r.min() > 1e-3
    assert np.all(np.abs(G.astype(ld) - DtD) <= barG)
    assert np.all(np.abs(g.astype(ld) - Dtd) <= barg)
    assert np.array_equal(G, G.T)
    G2, g2 = engine.distortionNormalEquations(modelId, v["offs"], v["s"], v["m"], v["A"], v["W"])
    assert np.array_equal(G, G2) and np.array_equal(g, g2)
    assert np.abs(kD - kY).max() <= 1e-7 * max(1.0, np.abs(kY).max())
    if case == "empty":                          # the empty views add nothing: the same sums from R without them
        w = iy.problemR(model, 0.3)
        G3, g3 = engine.distortionNormalEquations(modelId, w["offs"], w["s"], w["m"], w["A"], w["W"])
        assert np.array_equal(G, G3) and np.array_equal(g, g3)


# ---------------------------------------------------------------- compose / decompose
def test_compose_decompose_in_seventeen_blocks_with_the_branches_in_the_last():
    """engine.decomposeParameters against orc.eulerToR and engine.composeParameters of those matrices against
    orc.rToEuler on 4 099 random poses and, at indices >= 4 099 of the last 256-thread block, the gimbal-lock rows with
    their neighbours and angles of at most 1e-8 rad. Bars of test_compose_decompose_on_device: 1e-15 on R, 1e-11 degrees
    on the angles; translations bit-exact."""
    angles, t = iy.composeAngles()
    n = angles.shape[0]
    A0 = np.array([[400.0, 0.5, 320.0], [0.0, 410.0, 240.0], [0.0, 0.0, 1.0]])
    for modelId, k0 in ((orc.RADTAN, np.array([-0.5, 0.2, 0.07, -0.03, 0.05])), (orc.FISHEYE, np.array([-0.1, 0.02, 0.0, -0.03]))):
        L = orc.numShared(modelId)
        P = np.concatenate(([400.0, 410.0, 0.5, 320.0, 240.0], k0, np.hstack((angles, t)).ravel()))
        A1, W1, k1 = engine.decomposeParameters(modelId, P)
        Rref = orc.eulerToR(angles)
        dR = np.abs(W1[:, :3, :3] - Rref).max(axis=(1, 2))
        assert np.array_equal(A1, A0) and np.array_equal(k1, k0) and W1.shape == (n, 4, 4)
        assert np.array_equal(W1[:, :3, 3], t) and np.all(W1[:, 3, :] == np.array([0.0, 0.0, 0.0, 1.0]))
        Pback = engine.composeParameters(modelId, A0, mu.posesFromRT(Rref, t), k0)
        back = Pback[L:].reshape(n, 6)
        dA = np.abs(back[:, :3] - orc.rToEuler(Rref)).max(axis=1)
        print(f"\ncompose / decompose (L = {L}, {n} poses): R {dR.max():.2e} (special rows {dR[iy.EXT_VIEWS:].max():.2e}), "
              f"angles {dA.max():.2e} degrees (special rows {dA[iy.EXT_VIEWS:].max():.2e})")
        assert np.all(dR < 1e-15), np.nonzero(dR >= 1e-15)[0][:10]
        assert np.all(dA < 1e-11), np.nonzero(dA >= 1e-11)[0][:10]
        assert np.array_equal(back[:, 3:], t) and np.array_equal(Pback[:L], P[:L])


# ---------------------------------------------------------------- the whole stage
@pytest.mark.parametrize("model", MODELS)
def test_whole_initialisation_on_the_device_vs_all_host(model):
    """lc.estimateCalibrationParametersDevice against lc.estimateCalibrationParameters (all host) on R at 0.3 px. The bar
    is 100 x the host's distance from itself with every view's points permuted (the device sums in a third order and may
    part from the host on an undecided view), floored at 1e-12 and no looser than the existing 1e-5 (A, relative),
    1e-6 (W), 1e-5 (k). Host self-difference / bar / device on an MI355X:
      radtan   A 8.8e-10 / 8.8e-08 / 3.2e-10,  W 4.0e-09 / 4.0e-07 / 4.9e-09,  k 2.0e-10 / 2.0e-08 / 1.9e-10
      fisheye  A 6.6e-10 / 6.6e-08 / 8.6e-11,  W 3.9e-09 / 3.9e-07 / 2.8e-09,  k 2.6e-11 / 2.6e-09 / 2.1e-11"""
    v = iy.problemR(model, iy.STAGE_SIGMA)
    (Ah, Wh, kh), selfDiff, bars = iy.hostStage(model)
    assert all(1e-12 <= b <= e for b, e in zip(bars, iy.STAGE_EXISTING_BARS))
    dm = cca.RadialTangentialModel() if model == "radtan" else cca.FisheyeModel()
    Ad, Wd, kd = lc.estimateCalibrationParametersDevice(dm, v["offs"], v["s"], v["m"])
    diff = iy.stageDifference((Ad, Wd, kd), (Ah, Wh, kh))
    print(f"\nwhole stage {model} {iy.STAGE_SIGMA} px (A rel, W, k): host self-difference "
          + ", ".join(f"{d:.2e}" for d in selfDiff) + "; bars " + ", ".join(f"{b:.2e}" for b in bars)
          + "; device vs host " + ", ".join(f"{d:.2e}" for d in diff))
    assert Wd.shape == (iy.R_NUM_VIEWS, 4, 4) and len(kd) == len(kh)
    assert all(d <= b for d, b in zip(diff, bars)), (diff, bars)
