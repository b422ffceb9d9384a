"""The rig-only and the joint stereo solver share one LM loop: state, decision, stop, partial sums, the camera-b chain
rule and the back-substitution are written once. That is structure, never an operand or an order of operations, so
both solvers keep their bits: every output of every case below is byte for byte what the build BEFORE the fold gave
(tests/golden/stereo_loop/, written by tools/make_stereo_loop_golden.py). A golden file holds the small outputs as
arrays and the SHA-256 of each large one, and a digest of the case's inputs, so that a failure says whether the problem
or the kernels moved.

Cases (both solvers unless noted):
  ragged   the M = 8 problem of test_gpu_stereo_joint.blocksCase, all four model pairs: normal equations, the step at
           lambda 1e-3 and 10, six iterations with trace
  sizes    4 + 4 points per view, M = 1, 2, 17, 257, 4099: the step and three iterations (4099 views are 257 Schur
           and 1025 joint blocks partials: every quarter of the sum runs its 8-wide loop and its tail)
  mask     joint only: the step with both cameras fixed; six iterations with a.gamma = -0.0, b.uc and a's last
           distortion coefficient held
  stop     the ragged radtan / fisheye problem ending on max_iters, on err_min and on lambda leaving its bounds
The singular paths return no numbers: test_singular_* of test_gpu_stereo.py and test_gpu_stereo_joint.py cover them.
"""
import hashlib
import os

import numpy as np
import pytest

import stereo_joint_yardstick as jy
import stereo_yardstick as sy

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "stereo_loop")

PAIRS = [("radtan", "radtan"), ("radtan", "fisheye"), ("fisheye", "radtan"), ("fisheye", "fisheye")]
NA, NB = (7, 0, 16, 3, 33, 70, 54, 40), (5, 9, 0, 17, 64, 70, 0, 60)      # test_gpu_stereo_joint.blocksCase
SIZES = (1, 2, 17, 257, 4099)
SOLVERS = ("rig", "joint")
LARGE = ("E", "V", "g", "delta", "delta_lam10", "P")                        # stored as their SHA-256
LAM_BOUNDS = (1e-5, 1e-1)                                                   # from 1e-3: left after two like decisions

CASES = ([("ragged", pair, solver) for pair in PAIRS for solver in SOLVERS]
         + [("sizes", M, solver) for M in SIZES for solver in SOLVERS]
         + [("mask", "step", "joint"), ("mask", "refine", "joint")]
         + [("stop", how, solver) for how in ("max_iters", "err_min", "lambda") for solver in SOLVERS])


def caseId(case):
    kind, what, solver = case
    what = "-".join(what) if isinstance(what, tuple) else f"M{what}" if kind == "sizes" else what
    return f"{kind}_{what}_{solver}"


_problems = {}


def problemOf(case):
    """-> (problem, Pj): the case's joint problem and start point (built once per problem, never changed)"""
    kind, what, _ = case
    key = ("sizes", what) if kind == "sizes" else ("ragged", what if kind == "ragged" else ("radtan", "fisheye"))
    if key not in _problems:
        if kind == "sizes":
            prob, PsTrue = sy.makeStereo(what, "radtan", "fisheye", noiseSigma=0.3, countsA=[4] * what, countsB=[4] * what)
            Pj = jy.perturbedJoint(prob, PsTrue, 0.2, 0.01, 0.1, 0.002, intrinsics=0.002, distortion=0.01)
        else:
            prob, PsTrue = sy.makeStereo(8, key[1][0], key[1][1], board=(10, 7, 0.05), noiseSigma=0.3, countsA=NA, countsB=NB)
            Pj = jy.perturbedJoint(prob, PsTrue, 1.0, 0.03, 1.0, 0.01)
        _problems[key] = (prob, Pj)
    return _problems[key]


def inputsOf(case):
    """-> (cameras, start point, keyword arguments of the refinement): what the case hands to the engine"""
    kind, what, solver = case
    prob, Pj = problemOf(case)
    kw = {}
    if kind == "mask":
        La, Lb, S = jy.sizes(prob)
        Pj = Pj.copy()
        Pj[2] = -0.0
        kw["fixedMask"] = (1 << La + Lb) - 1 if what == "step" else 1 << 2 | 1 << La + 3 | 1 << La - 1
    if kind == "stop":
        kw = {"max_iters": {}, "err_min": {"errMin": 1e30}, "lambda": {"lamMin": LAM_BOUNDS[0], "lamMax": LAM_BOUNDS[1]}}[what]
    if solver == "rig":
        prob, Pj = jy.split(prob, Pj)
    return sy.engineCameras(prob), Pj, kw


def inputDigest(case):
    cams, P0, kw = inputsOf(case)
    h = hashlib.sha256()
    for cam in cams:
        h.update(repr(cam[0]).encode())
        for a in cam[1:]:
            h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.ascontiguousarray(P0).tobytes())
    h.update(repr(sorted(kw.items())).encode())
    return h.hexdigest()


def runCase(case):
    """-> dict of the case's outputs, every one an array; a call that ends singular leaves `singular` in place of its outputs"""
    from camera_calibration_amd import engine
    kind, what, solver = case
    cams, P0, kw = inputsOf(case)
    joint = solver == "joint"
    normalEq = engine.stereoJointNormalEquations if joint else engine.stereoNormalEquations
    stepDelta = engine.stereoJointStepDelta if joint else engine.stereoStepDelta
    refine = engine.refineStereoJoint if joint else engine.refineStereo
    S = engine.stereoJointShared(*cams) if joint else 6
    out = {}

    def step(name, lam):
        try:
            out[name] = stepDelta(*cams, P0, lam, **({"fixedMask": kw["fixedMask"]} if "fixedMask" in kw else {}))
        except np.linalg.LinAlgError:
            out["singular_" + name] = np.array(1)

    def loop(maxIters):
        try:
            sse, P, iters, trace, ab = refine(*cams, P0, maxIters, **kw)
        except np.linalg.LinAlgError:
            out["singular_refine"] = np.array(1)
            return
        out.update(sse=np.float64(sse), P=P, iters=np.int64(iters), trace=np.ascontiguousarray(trace),
                   sse_ab=np.array(ab, dtype=np.float64))

    if kind == "ragged":
        ne = normalEq(*cams, P0)
        out.update(B=ne["B"], g_shared=ne["g"][:S].copy(), E=ne["E"], V=ne["V"], g=ne["g"],
                   ne_sse_ab=np.array([ne["sseA"], ne["sseB"]]))
        step("delta", 1e-3)
        step("delta_lam10", 10.0)
        loop(6)
    elif kind == "sizes":
        step("delta", 1e-3)
        loop(3)
    elif (kind, what) == ("mask", "step"):
        step("delta", 1e-3)
    elif kind == "mask":
        loop(6)
    else:
        loop(2 if what == "max_iters" else 10)
    return out


def packed(out):
    """the outputs as a golden file keeps them: the large ones as `sha_<name>`"""
    keep = {}
    for name, a in out.items():
        a = np.ascontiguousarray(a)
        if name in LARGE:
            keep["sha_" + name] = np.array(hashlib.sha256(a.tobytes()).hexdigest())
            keep["shape_" + name] = np.array(a.shape, dtype=np.int64)
        else:
            keep[name] = a
    return keep


def test_the_cases_are_the_listed_ones():
    ids = [caseId(c) for c in CASES]
    assert len(set(ids)) == len(ids) == 8 + 10 + 2 + 6
    assert sorted(os.listdir(GOLDEN_DIR)) == sorted(i + ".npz" for i in ids)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=caseId)
def test_both_stereo_solvers_keep_their_bits(case):
    g = np.load(os.path.join(GOLDEN_DIR, caseId(case) + ".npz"), allow_pickle=False)
    assert inputDigest(case) == str(g["inputs"]), "the problem itself differs from the recorded one: not the kernels"
    got = packed(runCase(case))
    assert sorted(got) == sorted(k for k in g.files if k != "inputs"), (sorted(got), g.files)
    kind, what, solver = case
    if "trace" in got:
        tr, iters = got["trace"], int(got["iters"].ravel()[0])
        lam1 = tr[-1, 3] * (0.1 if tr[-1, 4] else 10)
        print(f"{caseId(case)}: {iters} iterations, accepted {int(tr[:, 4].sum())}, sse {got['sse'].ravel()[0]:.9e}, next lambda {lam1:.1e}")
        if kind == "stop":                                   # the case ends the way its name says
            inside = LAM_BOUNDS[0] < lam1 < LAM_BOUNDS[1]
            assert {"max_iters": iters == 2, "err_min": iters == 1, "lambda": iters <= 4 and not inside}[what]
    for name in sorted(got):
        assert got[name].dtype == g[name].dtype and got[name].shape == g[name].shape, name
        assert got[name].tobytes() == g[name].tobytes(), f"{name} differs from the recorded build"
