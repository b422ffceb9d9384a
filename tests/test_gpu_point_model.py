"""The per-point camera model on the device against the 50-digit yardstick of tests/golden/point_model/: wide angles
(r up to 1e3, 89.94 degrees off axis), the axis itself, both sides of the r^2 = 1e-16 switch and of the r = 1 seam of the
arctangent, in fp64 and in fp32 storage, through every form of the LM round.

The fixtures are read with numpy only (tests/point_model_yardstick.py); tests/test_point_model_cpu.py checks them
against their generator and shows that the element-wise bar used here can fail.

Bars. fp64 per element: |device - yardstick| <= K * 2^-53 * magnitude with one K per output group and model; fp32 the
same with K32 * 2^-24, on the points whose coordinates are fp32 numbers, r <= 3 (the shared parameters of the fixture
are fp32 numbers too, so nothing is rounded on the way in). K and K32 are 4 x the worst ratio measured on an MI355X,
rounded up to a power of two (DESIGN.md section 2 has the measured figures and where they occurred). Normal equations
in fp64: the suite's 1e-11 of a block's largest entry (g, sum r^2 and the step: beyond what the (u, v) bar lets a
residual move, see test_normal_equations_of_every_form_on_the_wide_angle_shard); in fp32: entry-wise, scaled by sqrt(B_aa B_bb) (E, V likewise)
and g by sum |J_ia r_i|, at 4 x the measured worst.
"""
import functools

import numpy as np
import pytest

import camera_calibration_amd as cca
import point_model_yardstick as pmy
from oracle import calib_oracle as orc
from test_gpu_chunked_rounds import KNOBS, chunkList

# ---- measured on an MI355X (worst ratio -> K = 4 x, rounded up to a power of two); see DESIGN.md section 2 -------------
K_FP64 = {
    "radtan": {"uv": 16, "distorted": 16, "intrinsic": 16, "coefficient": 32, "rotation": 32, "translation": 32},
    "fisheye": {"uv": 32, "distorted": 32, "intrinsic": 32, "coefficient": 128, "rotation": 32, "translation": 32},
}
K_FP32 = {
    "radtan": {"uv": 16, "intrinsic": 16, "coefficient": 32, "rotation": 32, "translation": 32},
    "fisheye": {"uv": 8, "intrinsic": 16, "coefficient": 128, "rotation": 16, "translation": 16},
}
# fp32 normal equations, 4 x the worst measured over the forms: scaled entry error per block kind, relative error of
# sum r^2. On the whole fixture radtan's g and sum r^2 are not held to anything: a point at r = 16.4 projects to 6.5e9 px,
# where one fp32 ulp is 512 px, so fp32 storage has no 0.3 px residual there (measured 2.2e4 and 8.4e4; the bar stays
# for the record). Fisheye's V there is set by the points beyond r = 3, where fp32 cancels s against x^2 sror.
F32_NORMAL = {
    "radtan": {"B": 7.6e-7, "E": 9.6e-7, "V": 3.5e-6, "g": 8.8e4, "sse": 3.4e5},
    "fisheye": {"B": 2.3e-6, "E": 4.8e-6, "V": 5.6e-5, "g": 1.3e-2, "sse": 1.1e-4},
}
# the same on the views without their points beyond r = 3 (radtan's largest projection is then 5.8e4 px, one fp32 ulp
# 0.004 px against the 0.3 px residual: g at the 1e-2 level; fisheye's stays below 2 000 px)
F32_NORMAL_R3 = {
    "radtan": {"B": 2.7e-7, "E": 2.6e-7, "V": 2.1e-6, "g": 7.4e-2, "sse": 2.2e-3},
    "fisheye": {"B": 3.1e-6, "E": 1.1e-6, "V": 5.3e-6, "g": 8.0e-4, "sse": 6.9e-5},
}
K_LIMIT = 256                 # a group that needs more is a finding, not a bar

BLOCK_TOL = 1e-11             # tests/test_gpu_chunked_rounds.py: B, E, V, g of the block's largest yardstick entry
SSE_RTOL = 1e-11
STEP_RTOL = 1e-9              # tests/test_gpu_parity.py: stepDelta against the dense solve
COLUMN_RTOL = 1e-12           # the older column-relative bar
TWO_KERNEL_CHUNK = 200        # three chunks of the ragged layout: 219, 220 and 259 points

pytestmark = pytest.mark.gpu

MODEL_CLASS = {"radtan": cca.RadialTangentialModel, "fisheye": cca.FisheyeModel}


@functools.lru_cache(maxsize=None)
def fixture(name):
    return pmy.loadFixture(name)


def residualSlack(name, prob):
    """how far the (u, v) bar lets a residual sensor - (u, v) move: the device's projection within K ulp of its magnitude,
    the yardstick's own float64 rounding and the subtraction's, half an ulp each"""
    return (K_FP64[name]["uv"] + 1) * pmy.EPS64 * prob["y_mag"]


@functools.lru_cache(maxsize=None)
def problemOf(name, which):
    prob = pmy.problem(fixture(name), which)
    L = pmy.NUM_SHARED[name]
    prob["yard"] = pmy.normalSums(prob["J"], pmy.residuals(prob), prob["offs"], L, dr=residualSlack(name, prob))
    prob["step"], prob["stepSlack"] = pmy.denseStep(prob, L, 1e-3, prob["yard"]["gSlack"])
    for a in prob.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return prob


def makeEngine(monkeypatch, name, prob, dtype="f64", env=(), mode=None):
    """an engine on the problem with the given knobs and no other (knobs are read at calib_create); the caller closes it"""
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, value in dict(env).items():
        monkeypatch.setenv(key, str(value))
    eng = cca.RefineEngine(name, dtype)
    try:
        eng.setProblem(prob["offs"], prob["sensor"], prob["pts"])
        if mode:
            eng.setLmMode(mode)
    except Exception:
        eng.close()
        raise
    return eng


def where(fx, i):
    r = pmy.radius(fx)
    return "a generally posed view" if fx["general"][i] else f"r = {r[i]:.6g}"


def report(label, name, fx, got, K):
    for g, (q, i) in got.items():
        print(f"{label} {name} {g}: worst ratio {q:.2f} at point {i} ({where(fx, i)}), K {K[name][g]}")


# ---------------------------------------------------------------- 2. fp64 per-point values
@functools.lru_cache(maxsize=None)
def evaluated(name, dtype):
    """y, Jc of calib_eval at the fixture's point, once per model and storage type (read-only)"""
    fx = fixture(name)
    prob = pmy.problem(fx, "ragged")
    eng = cca.RefineEngine(name, dtype)
    try:
        eng.setProblem(prob["offs"], prob["sensor"], prob["pts"])
        ev = eng.evaluate(prob["P"], wantY=True, wantR=True, wantJ=True)
        verr = eng.viewErrors(prob["P"])
    finally:
        eng.close()
    for a in list(ev.values()) + list(verr.values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ev, verr


@pytest.mark.parametrize("name", pmy.MODELS)
def test_fp64_block_within_k_ulp_of_the_magnitude(name):
    """RefineEngine.evaluate -> jacobian_kernel: (u, v) and the 2 x C block, element by element"""
    fx = fixture(name)
    ev, _ = evaluated(name, "f64")
    y, J = ev["y"], ev["Jc"]
    got = pmy.groupRatios(name, fx, y=y, J=J)
    report("evaluate", name, fx, got, K_FP64)
    assert np.isfinite(y).all() and np.isfinite(J).all()
    for g, (q, i) in got.items():
        assert K_FP64[name][g] <= K_LIMIT
        assert q <= K_FP64[name][g], (g, q, where(fx, i))
    colRel = pmy.columnRelative(J, fx["J"])
    print(f"{name}: column-relative {colRel.max():.2e}")
    assert colRel.max() < COLUMN_RTOL
    # exact outputs
    for c, row in pmy.STRUCTURAL_ZEROS:
        assert np.all(J[:, row, c] == 0.0), (c, row)
    assert np.all(J[:, 0, 3] == 1.0) and np.all(J[:, 1, 4] == 1.0)
    assert np.array_equal(ev["r"], pmy.problem(fx, "ragged")["sensor"] - y)          # the residual is sensor - projection


@pytest.mark.parametrize("name", pmy.MODELS)
def test_fp64_forward_helpers_within_k_ulp(name):
    """distortPoints / projectWithDistortion -> distort_points_kernel / project_cam_kernel on the identity-posed points,
    whose model point (x, y, 0) under t = (0, 0, 1) is the camera-frame point (x, y, 1)"""
    fx = fixture(name)
    ident = ~fx["general"]
    sh, L = fx["shared"], pmy.NUM_SHARED[name]
    A = np.array([[sh[0], sh[2], sh[3]], [0.0, sh[1], sh[4]], [0.0, 0.0, 1.0]])
    xy = np.ascontiguousarray(fx["pts"][:, :2])
    cam = np.column_stack((xy, np.ones(xy.shape[0])))
    xd = MODEL_CLASS[name]().distortPoints(xy, tuple(sh[5:L]))
    uv = MODEL_CLASS[name]().projectWithDistortion(A, cam, tuple(sh[5:L]))
    got = pmy.groupRatios(name, fx, y=uv, xd=xd, mask=ident)
    report("helpers", name, fx, got, K_FP64)
    assert np.isfinite(xd[ident]).all() and np.isfinite(uv[ident]).all()
    for g, (q, i) in got.items():
        assert q <= K_FP64[name][g], (g, q, where(fx, i))


@pytest.mark.parametrize("name", pmy.MODELS)
def test_view_errors_project_as_the_yardstick_does(name):
    """calib_view_errors projects with project_point and returns sums only: a view's sum |r|^2 and largest |r| against
    the yardstick's, within what the (u, v) bar lets every residual move (K + 1: the subtraction rounds once more)"""
    fx = fixture(name)
    prob = pmy.problem(fx, "ragged")
    _, verr = evaluated(name, "f64")
    r = pmy.residuals(prob).astype(np.float64)
    dr = (K_FP64[name]["uv"] + 1) * pmy.EPS64 * fx["y_mag"]
    offs = prob["offs"]
    worst = 0.0
    for v in range(offs.shape[0] - 1):
        a, b = int(offs[v]), int(offs[v + 1])
        sse = float(np.sum(r[a:b] ** 2))
        bar = float(np.sum(2 * np.abs(r[a:b]) * dr[a:b])) + 4 * (b - a) * pmy.EPS64 * sse
        worst = max(worst, abs(verr["sse"][v] - sse) / bar)
        assert abs(verr["sse"][v] - sse) <= bar, v
        norm = np.sqrt(np.sum(r[a:b] ** 2, axis=1))
        assert abs(verr["max"][v] - norm.max()) <= np.max(np.sum(dr[a:b], axis=1)) + 4 * pmy.EPS64 * norm.max(), v
        assert abs(verr["rms"][v] - np.sqrt(verr["sse"][v] / (b - a))) <= 4 * pmy.EPS64 * verr["rms"][v], v
    print(f"{name}: worst share of the per-view bar {worst:.3f}")


def seamPairs(fx, lo, hi, split):
    """pairs (a, b) of identity-posed points on the same half-axis with lo <= r_a < split <= r_b <= hi"""
    pts, r = fx["pts"], pmy.radius(fx)
    ok = ~fx["general"] & (r >= lo) & (r <= hi) & ((pts[:, 0] == 0) ^ (pts[:, 1] == 0))
    key = np.sign(pts[:, 0]) * 2 + np.sign(pts[:, 1])
    idx = np.flatnonzero(ok)
    return [(a, b) for a in idx for b in idx if key[a] == key[b] and r[a] < split <= r[b]]


@pytest.mark.parametrize("name", pmy.MODELS)
def test_fp64_is_continuous_across_the_switch_and_the_seam(name):
    """across r^2 = 1e-16 (analytic limits below) and across r = 1 (the arctangent's reflection above): between two
    points of one half-axis, s = xd / x and the block change by no more than the yardstick changes plus the two bars"""
    fx = fixture(name)
    ev, _ = evaluated(name, "f64")
    J, Jy, Jm = ev["Jc"], fx["J"], fx["J_mag"]
    L = pmy.NUM_SHARED[name]
    K = np.empty(L + 6)
    for g, cols in pmy.columnGroups(name).items():
        K[cols] = K_FP64[name][g]
    for tag, pairs in (("switch", seamPairs(fx, 0.9e-8, 1.1e-8, 1e-8)), ("seam", seamPairs(fx, 0.999, 1.001, 1.0 + 1e-16))):
        assert len(pairs) >= 4, tag
        worst = 0.0
        for a, b in pairs:
            bar = K * pmy.EPS64 * (Jm[a] + Jm[b])
            jump = np.abs((J[a] - J[b]) - (Jy[a] - Jy[b]))
            assert np.all(jump <= bar), (tag, a, b)
            # s from the distorted point: column 0 holds xd, column 1 yd; on a half-axis one of them is s * r
            c, row = (0, 0) if fx["pts"][a, 0] != 0 else (1, 1)
            sa, sb = J[a, row, c] / fx["pts"][a, c], J[b, row, c] / fx["pts"][b, c]
            ya, yb = Jy[a, row, c] / fx["pts"][a, c], Jy[b, row, c] / fx["pts"][b, c]
            assert abs((sa - sb) - (ya - yb)) <= K[0] * pmy.EPS64 * (abs(ya) + abs(yb)) * 2, (tag, a, b)
            worst = max(worst, float(np.max(np.where(bar > 0, jump / np.where(bar > 0, bar, 1.0), 0.0))))
        print(f"{name} {tag}: {len(pairs)} pairs, worst share of the bar {worst:.3f}")


# ---------------------------------------------------------------- 3. every form of the round
FORMS = {
    "tile": ("ragged", {"CALIB_GRAM_FORM": "tile", "CALIB_FUSED_STREAM": "0"}, None),
    "items2": ("ragged", {"CALIB_ITEMS_PER_WAVE": "2", "CALIB_GRAM_FORM": "tile", "CALIB_FUSED_STREAM": "0"}, None),
    # the plan takes several items per wave on uniform shards with one wave per item only (launch_plan.hpp)
    "items2_uniform": ("stream64", {"CALIB_ITEMS_PER_WAVE": "2", "CALIB_GRAM_FORM": "tile", "CALIB_GRAM_WPI": "1",
                                    "CALIB_FUSED_STREAM": "0"}, None),
    "block": ("ragged", {"CALIB_GRAM_FORM": "block", "CALIB_FUSED_STREAM": "0"}, None),
    "two_kernel": ("ragged", {"CALIB_CHUNK_POINTS": str(TWO_KERNEL_CHUNK)}, "two_kernel"),
    "stream64_w5": ("stream64", {"CALIB_FUSED_STREAM": "1", "CALIB_STREAM_WAVES": "5"}, None),
    "stream64_w7": ("stream64", {"CALIB_FUSED_STREAM": "1", "CALIB_STREAM_WAVES": "7"}, None),
    "stream68_w5": ("stream68", {"CALIB_FUSED_STREAM": "1", "CALIB_STREAM_WAVES": "5"}, None),
    "stream68_w7": ("stream68", {"CALIB_FUSED_STREAM": "1", "CALIB_STREAM_WAVES": "7"}, None),
}


FP64_FORMS = tuple(sorted(FORMS))


def test_the_two_kernel_case_spans_three_chunks():
    offs = pmy.problem(fixture("radtan"), "ragged")["offs"]
    assert [c[1] - c[0] for c in chunkList(TWO_KERNEL_CHUNK, offs)] == [219, 220, 259]


@pytest.mark.parametrize("form", FP64_FORMS)
@pytest.mark.parametrize("name", pmy.MODELS)
def test_normal_equations_of_every_form_on_the_wide_angle_shard(name, form, monkeypatch):
    """B, E, V, g of calib_normal_eq at the fixture's point against longdouble sums of the yardstick's J and r, at the
    suite's 1e-11 of the block's largest entry; sum r^2 to 1e-11; stepDelta at lambda = 1e-3 against the dense solve
    at 1e-9.

    B, E and V are held to exactly that. g, sum r^2 and the step depend on the residual sensor - (u, v), and at these
    angles (u, v) is large: a radtan point at r = 16.4 projects to 6.5e9 px, where one fp64 ulp is 9.5e-7 px -- against a
    0.3 px residual no arithmetic gives g to eleven digits (the float64 restatement of the kernel misses g by 9.6e-5 of
    the largest entry, sum r^2 by 1.7e-8 and the step by 2.5e-8). So the difference counts only beyond what the per-point
    (u, v) bar of test_fp64_block_within_k_ulp_of_the_magnitude lets it be: sum_i |J_ia| dr_i for g, sum_i 2 |r_i| dr_i
    for sum r^2, || |H^-1| gSlack || for the step, with dr_i = (K_uv + 1) 2^-53 magnitude(u_i) (residualSlack). Where
    (u, v) is of the size of the existing shards' the allowance is below the 1e-11 itself."""
    which, env, mode = FORMS[form]
    prob = problemOf(name, which)
    L = pmy.NUM_SHARED[name]
    eng = makeEngine(monkeypatch, name, prob, env=env, mode=mode)
    try:
        share, waves = eng.fusedForm()
        got = eng.normalEquations(prob["P"])
        sse = eng.evaluate(prob["P"])["sse"]
        d = eng.stepDelta(prob["P"], 1e-3)
    finally:
        eng.close()
    if form.startswith("stream"):
        # the stream form was taken; a wave's share of 4-point groups is 39 or 28 (64-point views), 34 or 25 (68): but
        # for 34 groups = two views of 68, its cuts fall inside views
        assert share > 0 and waves in (5, 7), (share, waves)
    else:
        assert share == 0
    yard = prob["yard"]
    ratios = pmy.blockRatios(got, yard, L)
    sseRaw = abs(sse - float(yard["sse"])) / float(yard["sse"])
    sseRel = max(abs(sse - float(yard["sse"])) - float(yard["sseSlack"]), 0.0) / float(yard["sse"])
    stepRaw = np.linalg.norm(d - prob["step"]) / np.linalg.norm(prob["step"])
    stepRel = max(stepRaw - prob["stepSlack"], 0.0)
    gRaw = float(np.max(np.abs(got[3] - yard["g"])) / np.max(np.abs(yard["g"])))
    print(f"{name} {form}: worst |d| / max |block| beyond the allowance " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items())
          + f" | sum r^2 rel {sseRel:.2e} | step rel {stepRel:.2e} || raw: g {gRaw:.2e}, sum r^2 {sseRaw:.2e} (allowance "
          f"{float(yard['sseSlack']) / float(yard['sse']):.2e}), step {stepRaw:.2e} (allowance {prob['stepSlack']:.2e})")
    assert all(np.isfinite(a).all() for a in got)
    for kind, worst in ratios.items():
        assert worst <= BLOCK_TOL, (kind, worst)
    assert sseRel <= SSE_RTOL
    assert stepRel <= STEP_RTOL


# ---------------------------------------------------------------- 4. the inverse at wide angles
def pixels(A, xd):
    return np.stack((A[0, 0] * xd[:, 0] + A[0, 1] * xd[:, 1] + A[0, 2], A[1, 1] * xd[:, 1] + A[1, 2]), axis=1)


def fisheyeCamera():
    sh = fixture("fisheye")["shared"]
    return np.array([[sh[0], sh[2], sh[3]], [0.0, sh[1], sh[4]], [0.0, 0.0, 1.0]])


def test_inverse_at_wide_angles_with_monotone_coefficients():
    """undistortPoints for theta from 0.7 to 1.55 (r up to 48): status 0 everywhere, |x - x_true| within the 2e-14 kappa
    of tests/test_gpu_undistort.py test_inverse_round_trip, kappa = max ||J^-1||_2 from the yardstick's derivative"""
    fx = fixture("fisheye")
    A, k = fisheyeCamera(), tuple(fx["inv_k"])
    x, der = fx["inv_x"], fx["inv_der"]
    Jd = np.stack((np.stack((der[:, 0], der[:, 1]), axis=1), np.stack((der[:, 1], der[:, 2]), axis=1)), axis=1)
    kappaEach = 1.0 / np.linalg.svd(Jd, compute_uv=False)[:, -1]
    kappa = float(kappaEach.max())
    got, status = cca.FisheyeModel().undistortPoints(A, k, pixels(A, fx["inv_xd"]), returnStatus=True)
    err = np.abs(got - x).max(axis=1)
    i = int(np.argmax(err / kappaEach))
    print(f"kappa {kappa:.1f}, max |x - x_true| {err.max():.3e}, bar {2e-14 * kappa:.3e}; worst against its own kappa "
          f"{(err / (2e-14 * kappaEach)).max():.3f} of 2e-14 kappa_i at r = {np.hypot(*x[i]):.3f}")
    assert status.shape == (512,) and not status.any()
    assert err.max() <= 2e-14 * kappa
    assert np.all(err <= 2e-14 * kappaEach)                     # and point by point (measured: 0.022 of it at the worst)


def test_inverse_stops_at_the_fold_of_the_benchmark_coefficients():
    """synthetic.FISHEYE_K: theta poly(theta) turns at the yardstick's root of its derivative. Targets below the turning
    value are solved (the forward model returns them), targets beyond it have no preimage: status 1, NaN"""
    fx = fixture("fisheye")
    A, k = fisheyeCamera(), tuple(fx["fold_k"])
    top = float(fx["fold_theta_d"])
    phi = np.linspace(0.0, 2 * np.pi, 64, endpoint=False) + 0.1
    below = np.linspace(0.05, 0.98, 64) * top
    beyond = np.linspace(1.02, 3.0, 64) * top
    td = np.concatenate((below, beyond))
    xd = np.stack((td * np.cos(np.tile(phi, 2)), td * np.sin(np.tile(phi, 2))), axis=1)
    got, status = cca.FisheyeModel().undistortPoints(A, k, pixels(A, xd), returnStatus=True)
    print(f"fold at theta {float(fx['fold_theta']):.6f}, theta_d {top:.6f}; status below {status[:64].sum()}, beyond {status[64:].sum()}")
    assert not status[:64].any() and status[64:].all()
    assert np.isnan(got[64:]).all() and np.isfinite(got[:64]).all()
    assert np.all(np.arctan(np.hypot(got[:64, 0], got[:64, 1])) < float(fx["fold_theta"]))       # the principal branch
    bx, by = orc.distortPoints(orc.FISHEYE, got[:64, 0], got[:64, 1], k)
    assert np.abs(np.stack((bx, by), axis=1) - xd[:64]).max() <= 64 * 2.0**-52


# ---------------------------------------------------------------- 5. fp32 storage
@pytest.mark.parametrize("name", pmy.MODELS)
def test_fp32_block_within_k32_ulp_of_the_magnitude(name):
    """RefineEngine(name, "f32").evaluate: (u, v) and the block on the points whose coordinates are fp32 numbers, r <= 3"""
    fx = fixture(name)
    ev, _ = evaluated(name, "f32")
    mask = fx["f32_exact"] & (pmy.radius(fx) <= 3.0)
    assert mask.sum() >= 400
    got = pmy.groupRatios(name, fx, y=ev["y"], J=ev["Jc"], eps=pmy.EPS32, mask=mask)
    report("f32 evaluate", name, fx, got, K_FP32)
    assert np.isfinite(ev["y"]).all() and np.isfinite(ev["Jc"]).all()
    for g, (q, i) in got.items():
        assert K_FP32[name][g] <= K_LIMIT
        assert q <= K_FP32[name][g], (g, q, where(fx, i))
    for c, row in pmy.STRUCTURAL_ZEROS:
        assert np.all(ev["Jc"][:, row, c] == 0.0)
    assert np.all(ev["Jc"][:, 0, 3] == 1.0) and np.all(ev["Jc"][:, 1, 4] == 1.0)


FORMS["tile_r3"] = ("ragged_r3",) + FORMS["tile"][1:]
FORMS["two_kernel_r3"] = ("ragged_r3",) + FORMS["two_kernel"][1:]
F32_FORMS = ("tile", "items2", "items2_uniform", "two_kernel", "tile_r3", "two_kernel_r3")


@pytest.mark.parametrize("form", F32_FORMS)
@pytest.mark.parametrize("name", pmy.MODELS)
def test_fp32_normal_equations_against_the_fp64_yardstick(name, form, monkeypatch):
    """fp32 points, J and r: every entry of B, E, V against the yardstick's sums, scaled by the diagonals; g by
    sum |J_ia r_i|; sum r^2 of the round (for fisheye the residual rides in the 16th MFMA column) against sum r^2"""
    which, env, mode = FORMS[form]
    prob = problemOf(name, which)
    L = pmy.NUM_SHARED[name]
    eng = makeEngine(monkeypatch, name, prob, dtype="f32", env=env, mode=mode)
    try:
        got = eng.normalEquations(prob["P"])
        sseRound = eng.refine(prob["P"], 1)[0]                  # the error before the update: the round's own sum r^2
    finally:
        eng.close()
    ratios, at = pmy.scaledRatios(got, prob["yard"], L)
    ratios["sse"] = abs(sseRound - float(prob["yard"]["sse"])) / float(prob["yard"]["sse"])
    bars = (F32_NORMAL_R3 if which == "ragged_r3" else F32_NORMAL)[name]
    print(f"f32 {name} {form}: " + " ".join(f"{k} {v:.3e}" for k, v in ratios.items()) + f" | worst at {at}")
    assert all(np.isfinite(a).all() for a in got)
    for kind, worst in ratios.items():
        assert worst <= bars[kind], (kind, worst)
