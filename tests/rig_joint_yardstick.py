"""Yardstick of the joint rig tests (test infrastructure, not a test file): rig_yardstick's problem with every camera
free, in numpy fp64 on the oracle's camera model.

Pq = (shared_0[L0] | shared_1[L1], rig_1[6] | .. | shared_{N-1}, rig_{N-1}[6] | pose_0[6], .., pose_{M-1}[6]), camera-major.
A problem is rig_yardstick's dict; its "shared" entries are ignored here, the cameras travel in Pq. The dense Jacobian is
rig_yardstick.jacobianDense at those cameras, its rig columns moved to their places in Pq, plus the shared columns
orc.jacobianCompact already returns: camera c's rows carry d/d shared_c. A fixed mask (a Python int, bit s = shared
unknown s, rigs included) removes the columns of the fixed unknowns from the dense problem, which is what editing the
reduced system (unit row, zero column, right-hand side 0) solves; their step is 0."""
import numpy as np

import rig_yardstick as ry
import stereo_joint_yardstick as jy
from oracle import calib_oracle as orc


def layout(prob):
    """-> (S, off (N,), L (N,)): camera c's unknowns start at off[c] -- shared_c (L[c]), then for c >= 1 rig_c (6)"""
    L = [orc.numShared(m) for m in prob["models"]]
    off, s = [], 0
    for c, l in enumerate(L):
        off.append(s)
        s += l + (6 if c else 0)
    return s, off, L


def columnsOfPr(prob):
    """index into Pq's shared part of every rig unknown, in Pr's order (6 (N - 1),)"""
    _, off, L = layout(prob)
    return np.concatenate([np.arange(off[c] + L[c], off[c] + L[c] + 6) for c in range(1, ry.numCameras(prob))])


def split(prob, Pq):
    """-> (the problem at Pq's cameras, Pr)"""
    S, off, L = layout(prob)
    Pq = np.asarray(Pq, dtype=np.float64).ravel()
    shared = [Pq[off[c]:off[c] + L[c]].copy() for c in range(ry.numCameras(prob))]
    return dict(prob, shared=shared), np.concatenate((Pq[columnsOfPr(prob)], Pq[S:]))


def join(prob, Pr, shared=None):
    """Pq of the problem's own cameras (or `shared`) and Pr"""
    S, off, L = layout(prob)
    Pr = np.asarray(Pr, dtype=np.float64).ravel()
    Sr = ry.numRig(prob)
    Pq = np.zeros(S + Pr.shape[0] - Sr)
    for c, sh in enumerate(prob["shared"] if shared is None else shared):
        Pq[off[c]:off[c] + L[c]] = sh
    Pq[columnsOfPr(prob)] = Pr[:Sr]
    Pq[S:] = Pr[Sr:]
    return Pq


def residualVector(prob, Pq):
    return ry.residualVector(*split(prob, Pq))


def error(prob, Pq):
    return ry.error(*split(prob, Pq))


def totalError(prob, Pq):
    return ry.totalError(*split(prob, Pq))


def sharedJacobians(prob, Pq):
    """-> [Js_c (n_c,2,L_c)]: d/d shared_c of camera c's rows"""
    p, Pr = split(prob, Pq)
    rigs, poses = ry._split(p, Pr)
    _, _, L = layout(prob)
    out = [orc.jacobianCompact(p["models"][0], np.concatenate((p["shared"][0], poses.ravel())), p["offs"][0],
                               p["xyz"][0])[:, :, :L[0]]]
    for c in range(1, ry.numCameras(prob)):
        X0, _, _ = ry.pointsIn0(p, Pr, c)
        out.append(orc.jacobianCompact(p["models"][c], np.concatenate((p["shared"][c], rigs[c - 1])), [0, X0.shape[0]],
                                       X0)[:, :, :L[c]])
    return out


def jacobianDense(prob, Pq):
    """(2 sum n_c, S + 6 M): d(projection)/d(Pq), rows as rig_yardstick.jacobianDense"""
    p, Pr = split(prob, Pq)
    S, off, L = layout(prob)
    Sr = ry.numRig(prob)
    Jd = ry.jacobianDense(p, Pr)
    J = np.zeros((Jd.shape[0], S + Jd.shape[1] - Sr))
    J[:, columnsOfPr(prob)] = Jd[:, :Sr]
    J[:, S:] = Jd[:, Sr:]
    r = 0
    for c, Js in enumerate(sharedJacobians(prob, Pq)):
        n = Js.shape[0]
        J[r:r + 2 * n, off[c]:off[c] + L[c]] = Js.reshape(2 * n, L[c])
        r += 2 * n
    return J


def freeColumns(prob, Pq, mask):
    S = layout(prob)[0]
    n = np.asarray(Pq).size
    return np.array([c for c in range(n) if c >= S or not mask >> c & 1], dtype=int)


def stepDense(prob, Pq, lam, mask=0):
    """delta = (J^T J + lam diag J^T J)^-1 J^T r over the free columns, 0 at the fixed ones; dense solve"""
    free = freeColumns(prob, Pq, mask)
    J = jacobianDense(prob, Pq)[:, free]
    JTJ = J.T @ J
    delta = np.zeros(np.asarray(Pq).size)
    delta[free] = np.linalg.solve(JTJ + lam * np.diag(np.diagonal(JTJ)), J.T @ residualVector(prob, Pq))
    return delta


def normalBlocks(prob, Pq):
    """View-vectorised, without the dense Jacobian -> dict B (S,S), E (M,S,6) [shared row, view column], V (M,6,6),
    g (S + 6 M,), sseCam (N,). Per camera the row block is [its columns of the shared part | view columns (6)];
    np.add.at sums the points of a view, the cameras in index order."""
    p, Pr = split(prob, Pq)
    S, off, L = layout(prob)
    M, N = ry.numViews(prob), ry.numCameras(prob)
    Jv0, rest = ry.compactJacobians(p, Pr)
    Js = sharedJacobians(prob, Pq)
    res = ry.residuals(p, Pr)
    B, E, V, g, gv = np.zeros((S, S)), np.zeros((M, S, 6)), np.zeros((M, 6, 6)), np.zeros(S + 6 * M), np.zeros((M, 6))
    for c in range(N):
        vi = orc.pointViewIndex(prob["offs"][c])
        Jv = Jv0 if c == 0 else rest[c - 1][1]
        Jc = Js[c] if c == 0 else np.concatenate((Js[c], rest[c - 1][0]), axis=2)       # (n,2,W)
        sl = slice(off[c], off[c] + Jc.shape[2])
        B[sl, sl] = np.einsum("nki,nkj->ij", Jc, Jc)
        Ec = np.zeros((M, Jc.shape[2], 6))
        np.add.at(Ec, vi, np.einsum("nki,nkj->nij", Jc, Jv))
        E[:, sl] = Ec
        np.add.at(V, vi, np.einsum("nki,nkj->nij", Jv, Jv))
        g[sl] = np.einsum("nki,nk->i", Jc, res[c])
        np.add.at(gv, vi, np.einsum("nki,nk->ni", Jv, res[c]))
    g[S:] = gv.ravel()
    return {"B": B, "E": E, "V": V, "g": g, "sseCam": np.array([float(np.sum(r * r)) for r in res])}


def stepFromBlocks(nb, lam, mask=0):
    """the LM step through the Schur complement of the view blocks: orc.schurStep, or with a mask
    stereo_joint_yardstick.stepFromBlocks (the same elimination with the fixed rows and columns left out)"""
    if not mask:
        return orc.schurStep(nb["B"], nb["E"], nb["V"], nb["g"], lam)
    return jy.stepFromBlocks(nb, lam, mask)


def stepBlocks(prob, Pq, lam, mask=0):
    """any M"""
    return stepFromBlocks(normalBlocks(prob, Pq), lam, mask)


def refineDense(prob, Pq0, maxIters, mask=0, lamInit=orc.LAMBDA_INITIAL, lamMin=orc.LAMBDA_MIN, lamMax=orc.LAMBDA_MAX,
                errMin=orc.PT_ERROR_MIN, step=stepDense):
    """the loop of src/calibrate.py:143-171 on Pq -> (err before the last update, Pq, trace rows (iter, err(P),
    err(P + delta), lambda, accepted, the S shared unknowns before the update))"""
    S = layout(prob)[0]
    Pt = np.array(Pq0, dtype=np.float64).ravel()
    lam, trace, err0 = lamInit, [], None
    for it in range(maxIters):
        delta = step(prob, Pt, lam, mask)
        err0 = totalError(prob, Pt)
        err1 = totalError(prob, Pt + delta)
        accepted = bool(err1 < err0)
        trace.append([it, err0, err1, lam, float(accepted)] + list(Pt[:S]))
        if accepted:
            Pt = Pt + delta
            lam /= 10
        else:
            lam *= 10
        if not (lamMin < lam < lamMax) or err0 < errMin:
            break
    return err0, Pt, np.array(trace)


def covarianceDense(prob, Pq, mask=0):
    """the shared (S,S) block of sigma^2 (Jf^T Jf)^-1 over the free columns, rows and columns of the fixed unknowns
    zero; sigma^2 = sse / (rows - free columns)"""
    S = layout(prob)[0]
    free = freeColumns(prob, Pq, mask)
    J = jacobianDense(prob, Pq)[:, free]
    C = totalError(prob, Pq) / (J.shape[0] - J.shape[1]) * np.linalg.inv(J.T @ J)
    nfree = int(np.sum(free < S))
    out = np.zeros((S, S))
    out[np.ix_(free[:nfree], free[:nfree])] = C[:nfree, :nfree]
    return out


def perturbedShared(prob, intrinsics=0.02, distortion=0.10, seed=5):
    """every camera's shared vector with alpha beta uc vc off by `intrinsics` (relative, random signs; a gamma of 0 stays
    0) and the distortion coefficients by `distortion` (relative)"""
    rng = np.random.default_rng(seed)
    out = []
    for sh in prob["shared"]:
        sh = np.array(sh, dtype=np.float64)
        sign = rng.choice([-1.0, 1.0], sh.shape[0])
        out.append(sh * (1.0 + sign * np.where(np.arange(sh.shape[0]) < 5, intrinsics, distortion)))
    return out


def perturbedJoint(prob, PrTrue, rigDeg, rigFrac, poseDeg, poseFrac, intrinsics=0.02, distortion=0.10, seed=5):
    """Pq with the rigs and the poses off as ry.perturbed puts them and the cameras as perturbedShared"""
    return join(prob, ry.perturbed(prob, PrTrue, rigDeg, rigFrac, poseDeg, poseFrac),
                perturbedShared(prob, intrinsics, distortion, seed))


def cameraMask(prob, cams=None):
    """the mask of every shared (camera) unknown of the listed cameras (None: all): no rig bits"""
    _, off, L = layout(prob)
    mask = 0
    for c in range(ry.numCameras(prob)) if cams is None else cams:
        mask |= ((1 << L[c]) - 1) << off[c]
    return mask


def rigMask(prob, c):
    _, off, L = layout(prob)
    return 0x3f << (off[c] + L[c])


COUNTS = (0, 1, 5, 16, 17, 33, 54, 64, 70)       # of a 10 x 8 board's 80: 33, 64 and 70 for a kernel that batches by 32 and 64


def raggedCounts(N, M, seed=11):
    """test_gpu_rig.raggedCounts, restated: per camera and view a count from COUNTS; every view has at least three points
    in total, and camera 1 misses view 0 (a zero band of E) whatever the draw. Here every camera is free, so each must
    also see enough to fix its own intrinsics: every camera keeps at least three views of 54 points (the first of its
    draw that have fewer are raised)."""
    rng = np.random.default_rng(seed + N)
    counts = rng.choice(COUNTS, size=(N, M))
    counts[1, 0] = 0
    for i in range(M):
        if counts[:, i].sum() < 3:
            counts[(i + 2) % N, i] = 5
    for c in range(N):
        i = 1
        while (counts[c] >= 54).sum() < 3:
            if counts[c, i] < 54:
                counts[c, i] = 54
            i += 2
    assert (counts.sum(axis=0) >= 3).all() and (counts == 0).any() and counts[1, 0] == 0
    return counts.tolist()


M_BLOCKS = 17
# camera 0 is radtan throughout: every view aims camera 0 at one corner, and where that corner lands on the axis to the last
# bit the oracle's fisheye projection is 0 / 0
MODELS_OF = {2: ["radtan", "fisheye"], 3: ["radtan", "fisheye", "fisheye"], 4: ["radtan", "fisheye", "radtan", "fisheye"],
             8: ["radtan", "fisheye", "fisheye", "radtan", "radtan", "fisheye", "radtan", "fisheye"],
             "8r": ["radtan"] * 8}
_cache = {}


def blocksCase(key):
    """the M = 17 ragged problem of the GPU tests at a point away from the solution, with the yardstick's blocks (once):
    key 2, 3, 4, 8 (mixed models) or "8r" (eight radtan cameras, S = 122) -> (problem, counts, Pq, blocks)"""
    if key not in _cache:
        N = len(MODELS_OF[key])
        counts = raggedCounts(N, M_BLOCKS)
        # a 10 x 8 board, of which a camera keeps 70 corners at most: a board with an odd number of rows or columns has
        # a corner on camera 0's axis in every view, where the oracle's fisheye projection is 0 / 0
        prob, PrTrue = ry.makeRig(N, M_BLOCKS, MODELS_OF[key], counts, noiseSigma=0.3, board=(10, 8, 0.05))
        Pq = perturbedJoint(prob, PrTrue, 0.3, 0.02, 0.2, 0.004)
        _cache[key] = (prob, counts, Pq, normalBlocks(prob, Pq))
    return _cache[key]


def noiseFreeCase():
    """N = 4, M = 20, full boards, no noise, rigs 1 degree / 3 %, poses 1 degree / 1 % off, the cameras as
    perturbedShared -> (problem, PqTrue, Pq0, refineDense's result), once"""
    if "free" not in _cache:
        prob, PrTrue = ry.makeRig(4, 20, MODELS_OF[4])
        Pq0 = perturbedJoint(prob, PrTrue, 1.0, 0.03, 1.0, 0.01)
        _cache["free"] = (prob, join(prob, PrTrue), Pq0, refineDense(prob, Pq0, 50))
    return _cache["free"]


def noisyCase():
    """N = 3, M = 8, 0.3 px noise, views missing from every camera -> (problem, PqTrue, Pq0, refineDense's result), once"""
    if "noisy" not in _cache:
        counts = [(54, 30, 0, 54, 17, 54, 54, 40), (54, 54, 40, 0, 54, 9, 54, 54), (20, 0, 54, 54, 0, 33, 54, 54)]
        prob, PrTrue = ry.makeRig(3, 8, ["radtan", "fisheye", "radtan"], counts, noiseSigma=0.3)
        Pq0 = perturbedJoint(prob, PrTrue, 1.0, 0.03, 1.0, 0.01)
        _cache["noisy"] = (prob, join(prob, PrTrue), Pq0, refineDense(prob, Pq0, 50))
    return _cache["noisy"]


def engineCameras(prob):
    return ry.engineCameras(prob)


SIZES_MODELS = ["radtan", "fisheye", "radtan"]


def sizesCase(M):
    """the problem of the GPU size tests: N = 3, 6 to 12 points per camera and view, 0.3 px noise -> (problem, Pq)"""
    rng = np.random.default_rng(M)
    counts = rng.integers(6, 13, size=(3, M)).tolist()
    prob, PrTrue = ry.makeRig(3, M, SIZES_MODELS, counts, noiseSigma=0.3)
    return prob, perturbedJoint(prob, PrTrue, 0.2, 0.01, 0.1, 0.002)
