"""N-view triangulation on the GPU: calib_triangulate_multi and the Python surface above it, against
tests/multiview_yardstick.py (numpy fp64 restatement of the contract in include/calib_lm.h; the forward model is
always the oracle's distortion, the inverse a numpy Newton). tests/test_multiview_cpu.py guards the yardstick and the
scenes (max-pair sin^2 >= 1e-3, every start in front of every camera).

Where the bars come from:
  noise-free   test_gpu_rectify's: |X - X_true| / |X_true| <= 1e-10 -- the rays meet at sin^2 ~ 0.005, so depth amplifies
               the inverse's 2e-14 kappa by ~1 / sin ~ 14.
  noisy        three checks that do not depend on the iteration path: the yardstick's gradient |J^T r| <= 1e-8 |J| |r|
               (central differences resolve ~1e-10), out_sse = the yardstick's squared residual to 1e-9 relative, out_sse
               <= the error at the start; out_res = the yardstick's residuals to 1e-9 px (the two forward models agree
               to ~1e-12 px).
  pair call    each of the two kernels ends with a last accepted step <= 1e-9 |X|: 2e-9 |X| between them.
  frame, order the same minimiser in another frame / summed in another order: 1e-12 |X|, rounding times the depth's
               amplification.
  covariance   the device Jacobian is analytic, the yardstick's is central differences: 50 times the yardstick's own
               largest disagreement between steps 1e-5 and 3e-5 |X| (computed here, ~2e-9 of a point's largest entry)."""
import numpy as np
import pytest

import camera_calibration_amd as cca
import multiview_yardstick as my
import rectify_yardstick as ry
import rig_yardstick as rk
from camera_calibration_amd import engine

pytestmark = pytest.mark.gpu

EVERYTHING = dict(returnStatus=True, returnError=True, returnCovariance=True, returnResiduals=True)


def relative(X, Xref):
    return np.linalg.norm(X - Xref, axis=1) / np.linalg.norm(Xref, axis=1)


def call(sc, seen=None, uv=None, **kw):
    seen = sc["seen"] if seen is None else seen
    return cca.triangulateMulti(sc["cameras"], sc["T"], sc["uv"] if uv is None else uv, my.maskWords(seen), **kw)


def sameBits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("N", [2, 3, 8])
def test_noise_free_points_are_recovered(N):
    sc = my.scene(N, 3)
    X, status, sse = call(sc, returnStatus=True, returnError=True)
    rel = relative(X, sc["X"])
    print(f"N {N}: {len(X)} points, {sc['seen'].sum(axis=0).min()} .. {sc['seen'].sum(axis=0).max()} cameras a point, status "
          f"sum {status.sum()}, max |X - truth| / |truth| {rel.max():.3e} (bar 1e-10), largest sse {sse.max():.3e}")
    assert X.shape == (54 * 3, 3) and status.dtype == np.int32 and sse.shape == status.shape == (54 * 3,)
    assert not status.any()
    assert rel.max() <= 1e-10
    assert sameBits(call(sc, returnStatus=True, returnError=True), (X, status, sse))


@pytest.mark.parametrize("N", [2, 3, 8])
def test_noisy_points_are_stationary(N):
    sc = my.scene(N, 3, 0.3)
    X, status, sse, res = call(sc, returnStatus=True, returnError=True, returnResiduals=True)
    assert not status.any()
    grad, scale, sseY, rY = my.gradientCheck(sc["cameras"], sc["T"], X, sc["uv"], sc["seen"])
    xy, _ = my.inverse(sc["cameras"], sc["uv"])
    sse0 = my.evaluate(sc["cameras"], sc["T"], my.closestPoint(sc["T"], xy, sc["seen"]), sc["uv"], sc["seen"])[0]
    seen3 = np.broadcast_to(sc["seen"][:, :, None], res.shape)
    dres = np.abs(res - rY)[seen3].max()
    print(f"N {N}: max |J^T r| / (|J| |r|) {(grad / scale).max():.3e} (bar 1e-8), max |sse - yardstick| / yardstick "
          f"{(np.abs(sse - sseY) / sseY).max():.3e} (bar 1e-9), max sse / sse(start) {(sse / sse0).max():.6f}, "
          f"|res - yardstick| {dres:.3e} px (bar 1e-9), |X - truth| / |truth| up to {relative(X, sc['X']).max():.2e}")
    assert (grad <= 1e-8 * scale).all()
    assert (np.abs(sse - sseY) <= 1e-9 * sseY).all()
    assert (sse <= sse0).all()
    assert res.shape == sc["uv"].shape and dres <= 1e-9
    assert np.array_equal(np.isnan(res), ~seen3)


@pytest.mark.parametrize("sigma", [0.0, 0.3])
def test_two_cameras_agree_with_the_pair_call(sigma):
    sc = my.scene(2, 3, sigma)
    both = np.ones_like(sc["seen"])
    X, status = call(sc, both, returnStatus=True)
    T1 = sc["T"][1]
    Xp, statusP = cca.triangulate(sc["cameras"][0], sc["cameras"][1], T1[:3, :3].copy(), T1[:3, 3].copy(), sc["uv"][0],
                                  sc["uv"][1], returnStatus=True)
    rel = relative(X, Xp)
    print(f"sigma {sigma}: max |X_multi - X_pair| / |X| {rel.max():.3e} (bar 2e-9), {(rel == 0).sum()} of {len(rel)} equal")
    assert np.array_equal(status, statusP) and not status.any()
    assert rel.max() <= 2e-9


def test_unseen_pixels_are_never_used():
    sc = my.scene(8, 3, 0.3)
    first = call(sc, **EVERYTHING)
    hidden = ~np.broadcast_to(sc["seen"][:, :, None], sc["uv"].shape)
    for fill in (np.nan, 0.0, 1e300):
        uv = np.where(hidden, fill, sc["uv"])
        assert sameBits(call(sc, uv=uv, **EVERYTHING), first), fill
    # seen=None: a camera sees a point where both coordinates are finite
    byDefault = cca.triangulateMulti(sc["cameras"], sc["T"], list(np.where(hidden, np.nan, sc["uv"])), **EVERYTHING)
    assert sameBits(byDefault, first)


def test_two_of_eight_cameras_equal_a_two_camera_call():
    sc = my.scene(8, 3, 0.3)
    seen = np.zeros_like(sc["seen"])
    seen[[1, 4]] = True
    eight = call(sc, seen, **EVERYTHING)
    pick = [1, 4]
    two = cca.triangulateMulti([sc["cameras"][c] for c in pick], sc["T"][pick], sc["uv"][pick], **EVERYTHING)
    assert not eight[1].any()
    assert sameBits(eight[:4], two[:4])
    assert eight[4][pick].tobytes() == two[4].tobytes() and np.isnan(np.delete(eight[4], pick, axis=0)).all()


def test_optional_outputs_do_not_change_the_others():
    sc = my.scene(3, 3, 0.3)
    X, sse, status, cov, res = engine.triangulateMulti([(rk.MODELS[c[0]], c[1], c[2]) for c in sc["cameras"]], sc["T"],
                                                       sc["uv"], my.maskWords(sc["seen"]), True, True)
    for wantCov, wantRes in ((False, False), (True, False), (False, True)):
        got = engine.triangulateMulti([(rk.MODELS[c[0]], c[1], c[2]) for c in sc["cameras"]], sc["T"], sc["uv"],
                                      my.maskWords(sc["seen"]), wantCov, wantRes)
        assert sameBits(got[:3], (X, sse, status))
        assert (got[3] is None) == (not wantCov) and (got[4] is None) == (not wantRes)
        assert got[3] is None or got[3].tobytes() == cov.tobytes()
        assert got[4] is None or got[4].tobytes() == res.tobytes()


def rigid(w, t):
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = ry.rot(w), t
    return G


def test_the_frame_is_the_callers_choice():
    sc = my.scene(3, 3, 0.3)
    G = rigid([0.3, -0.5, 0.2], [0.4, -0.1, 0.25])
    X = call(sc)
    moved = cca.triangulateMulti(sc["cameras"], sc["T"] @ np.linalg.inv(G), sc["uv"], my.maskWords(sc["seen"]))
    rel = relative(moved, X @ G[:3, :3].T + G[:3, 3])
    print(f"max |X' - G X| / |G X| {rel.max():.3e} (bar 1e-12)")
    assert rel.max() <= 1e-12


def test_camera_order_only_changes_the_sum_order():
    sc = my.scene(8, 3, 0.3)
    X = call(sc)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    again = cca.triangulateMulti([sc["cameras"][c] for c in perm], sc["T"][perm], sc["uv"][perm],
                                 my.maskWords(sc["seen"][perm]))
    rel = relative(again, X)
    print(f"max |X(permuted) - X| / |X| {rel.max():.3e} (bar 1e-12)")
    assert rel.max() <= 1e-12


@pytest.mark.parametrize("N", [2, 3, 8])
def test_covariance_against_the_yardstick(N):
    sc = my.scene(N, 3, 0.3)
    X, status, cov = call(sc, returnStatus=True, returnCovariance=True)
    assert not status.any() and cov.shape == (len(X), 3, 3)
    a = my.covariance(sc["cameras"], sc["T"], X, sc["seen"], 1e-5)
    b = my.covariance(sc["cameras"], sc["T"], X, sc["seen"], 3e-5)
    top = np.abs(a).max(axis=(1, 2))
    own = (np.abs(a - b).max(axis=(1, 2)) / top).max()
    err = np.abs(cov - a).max(axis=(1, 2)) / top
    print(f"N {N}: max |cov - yardstick| / largest entry {err.max():.3e}; the yardstick's two steps differ by {own:.3e}, "
          f"bar {50 * own:.3e}; sqrt of the largest variance {np.sqrt(cov[:, 2, 2].max()):.3e} per pixel")
    assert err.max() <= 50 * own
    assert np.array_equal(cov, cov.transpose(0, 2, 1)) and (np.linalg.eigvalsh(cov) > 0).all()
    X2, cov2 = call(sc, returnCovariance=True, sigma=2.0)
    assert X2.tobytes() == X.tobytes() and np.array_equal(cov2, 4.0 * cov)


def test_sizes_are_prefixes_of_the_largest_call():
    sc = my.scene(3, 10)
    assert sc["uv"].shape[1] >= 513
    full = None
    for n in (513, 257, 256, 255, 1):
        got = cca.triangulateMulti(sc["cameras"], sc["T"], sc["uv"][:, :n], my.maskWords(sc["seen"][:, :n]), **EVERYTHING)
        assert got[0].shape == (n, 3) and got[3].shape == (n, 3, 3) and got[4].shape == (3, n, 2)
        if full is None:
            full = got
            assert not got[1].any() and relative(got[0], sc["X"][:n]).max() <= 1e-10
        assert sameBits(got[:4], [a[:n] for a in full[:4]]) and got[4].tobytes() == full[4][:, :n].tobytes()
    empty = cca.triangulateMulti(sc["cameras"], sc["T"], sc["uv"][:, :0], **EVERYTHING)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,) and empty[4].shape == (3, 0, 2)


def test_statuses():
    sc = my.scene(3, 3)
    cams, T = sc["cameras"], sc["T"]
    n = 12
    uv, seen = np.array(sc["uv"][:, :n]), np.ones((3, n), dtype=bool)
    clean = cca.triangulateMulti(cams, T, uv, my.maskWords(seen), **EVERYTHING)
    assert not clean[1].any()
    seen[:, 1] = False                                                          # nobody saw it
    seen[[0, 2], 2] = False                                                     # one camera saw it
    uv[2, 3] = [np.nan, 100.0]
    uv[1, 4] = [1500.0, 250.0]                                                  # beyond the fisheye model's reach
    assert ry.newtonInverse(cams[1], uv[1, 4:5])[1].tolist() == [1]
    d = np.array([0.1, -0.2, 1.0])                                              # one direction in every camera
    for c in range(3):
        uv[c, 5] = ry.projectCamera(cams[c], (T[c][:3, :3] @ d)[None])[0]
    # point 6: cameras 0 and 1 only, camera 1's ray mirrored about camera 0's (test_triangulation_statuses' recipe)
    R, t = T[1][:3, :3], T[1][:3, 3]
    Xt = sc["X"][6]
    da = np.append(Xt[:2] / Xt[2], 1.0)
    Xb = R @ Xt + t
    db = R.T @ np.append(Xb[:2] / Xb[2], 1.0)
    uv[1, 6] = ry.projectCamera(cams[1], (R @ (2.0 * da - db / db[2]))[None])[0]
    seen[2, 6] = False
    seen[[1, 2], 7] = False                                                     # one camera, and its pixel is NaN: still 4
    uv[0, 7] = np.nan
    xy, inv = my.inverse(cams, np.where(seen[:, :, None], uv, 0.0))
    sin2, X0 = my.maxPairSin2(T, xy, seen), my.closestPoint(T, xy, seen)
    print(f"parallel rays: the yardstick's sin^2 {sin2[5]:.2e}; diverging pair: its start at depth {X0[6, 2]:.3f}, sin^2 "
          f"{sin2[6]:.2e}")
    assert sin2[5] < 1e-14 and X0[6, 2] < 0 and sin2[6] > 1e-6
    X, status, sse, cov, res = cca.triangulateMulti(cams, T, uv, my.maskWords(seen), **EVERYTHING)
    print("statuses", status)
    assert status.tolist() == [0, 4, 4, 1, 1, 2, 2, 4, 0, 0, 0, 0]
    assert my.triangulate(cams, T, uv, seen)["status"].tolist() == status.tolist()
    bad = status != 0
    assert np.isnan(X[bad]).all() and np.isnan(sse[bad]).all() and np.isnan(cov[bad]).all() and np.isnan(res[:, bad]).all()
    good = ~bad
    assert sameBits([X[good], sse[good], cov[good], res[:, good]], [clean[0][good], clean[2][good], clean[3][good],
                                                                    clean[4][:, good]])


def test_rig_calibration_triangulates_every_corner():
    models = ["radtan", "fisheye", "radtan"]
    prob, PrTrue = rk.makeRig(3, 4, models)
    rig = cca.rigCalibrate(rk.detections(prob), rk.cameraTuples(prob, models))
    uv = np.stack(prob["uv"])
    Xtrue = rk.pointsIn0(prob, PrTrue, 0)[0]
    X, status = rig.triangulateAll(uv, returnStatus=True)
    rel = relative(X, Xtrue)
    print(f"rigCalibrate: |T - truth| {np.abs(rig.T - rk.rigTransforms(prob, PrTrue)).max():.3e}; all three cameras: max "
          f"|X - truth| / |truth| {rel.max():.3e} (bar 1e-9)")
    assert not status.any() and rel.max() <= 1e-9
    # cameras 1 and 2 only: the pair call's answer, moved from camera 1's frame into camera 0's
    hidden = uv.copy()
    hidden[0] = np.nan
    X12 = rig.triangulateAll(list(hidden))
    Xpair = rig.triangulate(1, 2, uv[1], uv[2])
    back = np.linalg.inv(rig.T[1])
    rel12 = relative(X12, Xpair @ back[:3, :3].T + back[:3, 3])
    print(f"cameras 1 and 2: max |X - pair call| / |X| {rel12.max():.3e}, |X - truth| / |truth| "
          f"{relative(X12, Xtrue).max():.3e} (bars 1e-9)")
    assert rel12.max() <= 1e-9 and relative(X12, Xtrue).max() <= 1e-9
