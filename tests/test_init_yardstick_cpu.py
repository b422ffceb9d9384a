"""The guard of tests/test_gpu_init_kernels.py, no GPU: the inputs of tests/init_yardstick.py take the initialisation
kernels where the GPU tests say they do, and the host references are fit to be compared against. Every test prints what
it measured (pytest -s)."""
import numpy as np
import pytest

import init_yardstick as iy
from camera_calibration_amd import linearcalibrate as lc
from oracle import calib_oracle as orc

MODELS = ("radtan", "fisheye")


def relH(H, Href):
    return float(np.abs(H - Href).max() / np.abs(Href).max())


def test_r_counts_meet_every_pattern_of_the_lane_stride():
    counts = iy.rCounts()
    assert len(counts) == iy.R_NUM_VIEWS == 83 and min(counts) >= 4
    seen = set()
    for n in counts:
        seen |= iy.lanePatterns(n)
    assert iy.R_REQUIRED <= seen, iy.R_REQUIRED - seen
    assert set(counts) == set(iy.R_COUNT_CYCLE)
    # the orientation points of lanePatterns
    assert iy.lanePatterns(4) == {"fewer points than lanes", "exact fit"}
    assert iy.lanePatterns(17) == {"one past one per lane", "last trip with one live lane"}
    assert "last trip with one live lane" in iy.lanePatterns(65) and "around four trips" in iy.lanePatterns(64)
    for model, sigma in iy.R_VARIANTS:
        v = iy.problemR(model, sigma)
        assert np.array_equal(np.diff(v["offs"]), counts) and v["offs"][-1] == v["s"].shape[0] == v["m"].shape[0]
        assert np.isfinite(v["s"]).all()
        assert iy.hostSvdRoute(v)
    assert [len(iy.R_SIGMAS[m]) for m in MODELS] == [3, 3] and all(iy.R_SIGMAS[m][0] == 0.0 for m in MODELS)


def test_r_fills_six_workgroups_and_the_last_holds_three_views():
    blocks, rest = divmod(iy.R_NUM_VIEWS, iy.VIEWS_PER_WORKGROUP)
    assert (blocks + 1, rest) == (6, 3)            # the last wave of the last workgroup has a group that returns at once
    assert iy.EXT_VIEWS == 16 * 256 + 3            # one view per thread: 16 full blocks and 3 threads


def test_sparse_views_keep_the_outer_corners_and_no_view_is_degenerate():
    for model in MODELS:
        numW, numH, spacing = iy.BOARDS[model]
        v = iy.problemR(model, 0.0)
        for s, m in iy.detections(v):
            assert m.shape[0] >= 4 and np.unique(m, axis=0).shape[0] == m.shape[0]
            for corner in ((0, 0), (numW - 1, 0), (0, numH - 1), (numW - 1, numH - 1)):
                assert (np.abs(m[:, :2] - np.array(corner) * spacing).max(axis=1) < 1e-12).any()
            c = m[:, :2] - m[:, :2].mean(axis=0)
            assert np.linalg.svd(c, compute_uv=False)[1] > 0.1        # metres: the points span the plane


def test_host_dlt_is_the_full_svds_null_vector_on_every_view():
    """lc.estimateHomographies against the reference's route restated per view (iy.dltSvd): with 4 points M is 8 x 9
    and the null vector is the ninth row of the full V^T, which a reduced SVD does not return."""
    worst = 0.0
    for model, sigma in iy.R_VARIANTS:
        Hs = iy.hostHomographies(model, sigma)
        for i, (s, m) in enumerate(iy.detections(iy.problemR(model, sigma))):
            Href = iy.dltSvd(s, m)
            worst = max(worst, relH(Hs[i], Href))
            assert relH(Hs[i], Href) <= 1e-12, (model, sigma, i, s.shape[0])
            if s.shape[0] == 4:                    # exact fit: the homography passes through the four points
                assert np.abs(iy.project(Hs[i], m) - s).max() < 1e-9
    print(f"host DLT vs per-view full SVD: worst {worst:.1e} of max|H|")


def test_inverse_iteration_4_misses_the_bar_and_8_is_100x_inside():
    """dlt_kernel's algorithm in numpy against the SVD on R: 4 iterations leave more than 1e-8 of max|H_svd| on some
    view of every variant (so the GPU test can tell the two kernels apart), 8 leave less than 1e-10 on every view."""
    print("\nvariant           lambda1/lambda2   worst |H - H_svd| / max|H_svd|, 4 iterations   8 iterations")
    for model, sigma in iy.R_VARIANTS:
        Hs = iy.hostHomographies(model, sigma)
        e4, e8, ratio = [], [], []
        for i, (s, m) in enumerate(iy.detections(iy.problemR(model, sigma))):
            H4, r = iy.dltInverseIteration(s, m, 4, wantRatio=True)
            e4.append(relH(H4, Hs[i]))
            e8.append(relH(iy.dltInverseIteration(s, m, 8), Hs[i]))
            ratio.append(r)
        print(f"{model:8s} {sigma:4.2f} px   <= {max(ratio):.2e}      {max(e4):.2e} ({sum(e > 1e-8 for e in e4)} views past 1e-8)"
              f"              {max(e8):.2e}")
        assert max(e4) > 1e-8, (model, sigma, max(e4))
        assert max(e8) < 1e-10, (model, sigma, max(e8))
        assert ratio[0] < 1e-12                   # 4 points fit exactly: lambda_1 = 0, only the shift keeps the solve finite


def test_host_polish_agrees_with_itself_on_95_percent_of_the_views():
    """The views on which the GPU test compares the LM polish: at most 5 % of a variant's may be undecided (a
    condition on the inputs; see R_SIGMAS for what it cost)."""
    for model, sigma in iy.R_VARIANTS:
        und = iy.undecidedViews(model, sigma)
        counts = [iy.rCounts()[i] for i in und]
        print(f"{model} {sigma} px: {len(und)} of {iy.R_NUM_VIEWS} views undecided {list(und)} with {counts} points")
        assert len(und) <= 0.05 * iy.R_NUM_VIEWS, (model, sigma, und)


def test_empty_views_are_spliced_in_at_the_front_middle_and_end():
    v = iy.problemR("radtan", 0.3)
    e, keep, empty = iy.withEmptyViews(v)
    counts = np.diff(e["offs"])
    assert list(empty) == [0, 42, 85] and len(counts) == 86 and np.all(counts[empty] == 0)
    assert np.array_equal(counts[keep], iy.rCounts()) and e["W"].shape == (86, 4, 4)
    assert np.array_equal(e["s"], v["s"]) and np.array_equal(e["W"][keep], v["W"])
    assert len({w.tobytes() for w in v["W"]}) == 83                   # a slipped view index picks a different pose


def test_extrinsics_input_scales():
    H, scale, A = iy.extrinsicsInput()
    assert H.shape == (iy.EXT_VIEWS, 3, 3) and np.all(np.abs(scale) >= 0.25) and np.all(np.abs(scale) <= 4.0)
    assert np.all(scale[::3] < 0) and np.all(scale[1::3] > 0) and np.all(scale[2::3] > 0)
    assert len(np.unique(scale)) == iy.EXT_VIEWS
    # what lc.computeExtrinsics does with a negative scale: r0, r1 and t change sign, r2 = r0 x r1 does not -- a proper
    # rotation (turned by 180 degrees about r2) with the board behind the camera
    Hp = np.abs(scale)[:, None, None] * H / scale[:, None, None]
    Wn, Wp = np.array(lc.computeExtrinsics(H, A)), np.array(lc.computeExtrinsics(Hp, A))
    neg = scale < 0
    flip = np.array([-1.0, -1.0, 1.0, -1.0])
    assert np.abs(Wn[neg][:, :3, :] - Wp[neg][:, :3, :] * flip).max() < 1e-12
    assert np.abs(Wn[~neg] - Wp[~neg]).max() < 1e-12
    assert np.all(np.linalg.det(Wn[:, :3, :3]) > 0.999)


@pytest.mark.parametrize("model", MODELS)
def test_distortion_cases(model):
    a, b = iy.distortionCaseEmpty(model), iy.distortionCaseBig(model)
    assert np.diff(b["offs"]).tolist() == [54] * iy.BIG_VIEWS and b["offs"][-1] == 262170
    blocks = -(-262170 // 256)
    assert blocks == 1025 and 262170 - 1024 * 256 == 26      # threads 0..25 of workgroup 0 take a second trip
    assert len({w.tobytes() for w in b["W"]}) == iy.BIG_VIEWS
    for tag, v in (("R + empty views", a), ("4 855 views", b)):
        D, Ddot, r = iy.distortionRows(model, v["A"], v["W"], v["offs"], v["s"], v["m"])
        assert D.dtype == np.longdouble and D.shape == (2 * v["offs"][-1], 5 if model == "radtan" else 4)
        print(f"{model} {tag}: r in [{float(r.min()):.3e}, {float(r.max()):.3f}]")
        assert r.min() > 1e-3                      # the fisheye rows divide by r, in the reference too
        assert np.isfinite(D.astype(np.float64)).all()
    # the rows are lc.estimateDistortion's: same k from the yardstick's sums as from the host's pinv route
    v = iy.problemR(model, 0.3)
    DtD, Dtd, _, _, _ = iy.normalEquationsYardstick(v)
    kY = np.array(lc.solveDistortionNormalEquations(DtD.astype(np.float64), Dtd.astype(np.float64)))
    kH = np.array(lc.estimateDistortion(iy._distortionModel(model), v["A"], iy.detections(v), v["W"]))
    print(f"{model}: k from the yardstick's sums vs lc.estimateDistortion: {np.abs(kY - kH).max():.1e}")
    assert np.abs(kY - kH).max() <= 1e-7 * max(1.0, np.abs(kH).max())


def test_compose_angles_put_the_branches_in_the_last_block():
    angles, t = iy.composeAngles()
    n = angles.shape[0]
    assert angles.shape == t.shape and iy.EXT_VIEWS < n <= 17 * 256
    special = angles[iy.EXT_VIEWS:]
    rad = np.abs(special) * orc.DEG
    assert ((rad <= 1e-8) & (rad > 0)).any(axis=1).sum() >= 4          # the numeric Rodrigues quirk, below its threshold
    assert (np.abs(np.abs(special[:, 1]) - 90.0) == 0).sum() >= 4      # gimbal lock
    near = np.abs(np.abs(special[:, 1]) - 90.0)
    band = np.degrees(np.arccos(1.0 - (1e-8 + 1e-5)))                  # np.isclose(R31, +-1): within 0.256 degrees of +-90
    assert ((near > 0) & (near < band)).sum() >= 4 and ((near > band) & (near <= 0.31)).sum() >= 2     # its neighbours
    assert np.abs(angles[:iy.EXT_VIEWS]).max() < 180.0
    R = orc.eulerToR(angles)
    back = orc.rToEuler(R)
    outside = np.abs(np.abs(angles[:, 1]) - 90.0) > band               # inside the band ry comes back as +-90 exactly
    assert np.abs(orc.eulerToR(back) - R)[outside].max() < 1e-9        # the yardstick's own round trip
    assert 0 < (~outside[:iy.EXT_VIEWS]).sum() < 40                    # some of the random rows fall inside it too


@pytest.mark.parametrize("model", MODELS)
def test_stage_bars_come_from_the_hosts_self_difference(model):
    res, selfDiff, bars = iy.hostStage(model)
    print(f"{model} {iy.STAGE_SIGMA} px: host vs host with permuted points (A rel, W, k) = "
          + ", ".join(f"{d:.2e}" for d in selfDiff) + "; bars " + ", ".join(f"{b:.2e}" for b in bars))
    assert all(b >= 1e-12 for b in bars)
    assert all(b <= e for b, e in zip(bars, iy.STAGE_EXISTING_BARS)), (bars, iy.STAGE_EXISTING_BARS)
    assert np.isfinite(res[0]).all() and res[0][0, 0] > 0 and res[0][1, 1] > 0
