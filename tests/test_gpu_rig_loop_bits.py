"""The rig solver (N known cameras) and the joint rig solver reach the LM loop of csrc/stereo_loop.hpp through the same
host front end as the two stereo solvers. That front end is structure: which kernels a round launches, with which grids
and arguments, does not depend on how the host code is laid out, so both rig solvers keep their bits. Every output of
every case below is byte for byte what the build BEFORE the front ends were folded gave (tests/golden/rig_loop/, written
by tools/make_stereo_loop_golden.py test_gpu_rig_loop_bits). A golden file holds the small outputs as arrays, the
SHA-256 of each large one and a digest of the case's inputs, as tests/test_gpu_stereo_loop_bits.py explains.

Cases ("rig": every camera known; "joint": the cameras free as well):
  blocks   rig_joint_yardstick.blocksCase (M = 17, ragged, mixed models) at N = 2, 3 and 8, the joint solver also at eight
           radtan cameras (S = 122): normal equations, the step at lambda 1e-3 and 10, six iterations with trace
  sizes    rig_joint_yardstick.sizesCase (N = 3), M = 1, 2, 17, 257, 4099: the step and three iterations; the joint
           solver with every camera bit fixed at M <= 2. 4099 views fill and loop the joint rig's two capped grids (512
           and 128 workgroups) and are 257 Schur partials of the rig solver: the numbers the host's begin computes
  mask     joint only: test_gpu_rig_joint.mixedMask at N = 3, the step and six iterations; at N = 8 the step with camera
           0's skew (bit 2) and camera 7's uc (bit 106) held, so that both words of the host's mask carry a bit
  stop     N = 3 ending on max_iters, on err_min and on lambda leaving its bounds
The singular paths return no numbers: test_singular_* of test_gpu_rig.py and test_gpu_rig_joint.py cover them.
"""
import hashlib
import os

import numpy as np
import pytest

import rig_joint_yardstick as qy
import test_gpu_stereo_loop_bits as stereo_bits
from test_gpu_stereo_loop_bits import LAM_BOUNDS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "rig_loop")

SIZES = (1, 2, 17, 257, 4099)
SOLVERS = ("rig", "joint")
LARGE = stereo_bits.LARGE + ("B",)                                          # (122, 122) at eight radtan cameras

CASES = ([("blocks", key, solver) for key in (2, 3, 8) for solver in SOLVERS] + [("blocks", "8r", "joint")]
         + [("sizes", M, solver) for M in SIZES for solver in SOLVERS]
         + [("mask", "step", "joint"), ("mask", "refine", "joint"), ("mask", "step8", "joint")]
         + [("stop", how, solver) for how in ("max_iters", "err_min", "lambda") for solver in SOLVERS])


def caseId(case):
    kind, what, solver = case
    what = f"M{what}" if kind == "sizes" else f"N{what}" if kind == "blocks" else what
    return f"{kind}_{what}_{solver}"


def mixedMask(prob):
    """test_gpu_rig_joint.mixedMask: camera 0's skew, camera 1's last coefficient, camera 2's principal point, rig 1's tz"""
    import test_gpu_rig_joint
    return test_gpu_rig_joint.mixedMask(prob)


def twoWordMask(prob):
    """camera 0's skew and the last camera's uc: one bit in each word of an N = 8 mask"""
    _, off, _ = qy.layout(prob)
    mask = 1 << 2 | 1 << (off[-1] + 3)
    assert mask & (2 ** 64 - 1) and mask >> 64
    return mask


def inputsOf(case):
    """-> (cameras, start point, keyword arguments of the refinement): what the case hands to the engine. The problems
    are the yardstick's (built once there, never changed)."""
    kind, what, solver = case
    if kind == "sizes":
        prob, Pq = qy.sizesCase(what)
    else:
        prob, _, Pq, _ = qy.blocksCase(what if kind == "blocks" else 8 if what == "step8" else 3)
    kw = {}
    if kind == "sizes" and solver == "joint" and what <= 2:
        kw["fixedMask"] = qy.cameraMask(prob)
    if kind == "mask":
        kw["fixedMask"] = twoWordMask(prob) if what == "step8" else mixedMask(prob)
        if what == "refine":
            Pq = Pq.copy()
            Pq[2] = -0.0
    if kind == "stop":
        kw = {"max_iters": {}, "err_min": {"errMin": 1e30}, "lambda": {"lamMin": LAM_BOUNDS[0], "lamMax": LAM_BOUNDS[1]}}[what]
    if solver == "rig":
        prob, Pq = qy.split(prob, Pq)
    return qy.engineCameras(prob), Pq, kw


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
    normalEq = engine.rigJointNormalEquations if joint else engine.rigNormalEquations
    stepDelta = engine.rigJointStepDelta if joint else engine.rigStepDelta
    refine = engine.refineRigJoint if joint else engine.refineRig
    S = engine.rigJointLayout([cam[0] for cam in cams])[0] if joint else 6 * (len(cams) - 1)
    out = {}

    def step(name, lam):
        try:
            out[name] = stepDelta(cams, P0, lam, **({"fixedMask": kw["fixedMask"]} if "fixedMask" in kw else {}))
        except np.linalg.LinAlgError:
            out["singular_" + name] = np.array(1)

    def loop(maxIters):
        try:
            sse, P, iters, trace, cam = refine(cams, P0, maxIters, **kw)
        except np.linalg.LinAlgError:
            out["singular_refine"] = np.array(1)
            return
        out.update(sse=np.float64(sse), P=P, iters=np.int64(iters), trace=np.ascontiguousarray(trace),
                   sse_cam=np.array(cam, dtype=np.float64))

    if kind == "blocks":
        ne = normalEq(cams, P0)
        out.update(B=ne["B"], g_shared=ne["g"][:S].copy(), E=ne["E"], V=ne["V"], g=ne["g"], ne_sse_cam=ne["sseCam"])
        step("delta", 1e-3)
        step("delta_lam10", 10.0)
        loop(6)
    elif kind == "sizes":
        step("delta", 1e-3)
        loop(3)
    elif kind == "mask" and what != "refine":
        step("delta", 1e-3)
    elif kind == "mask":
        loop(6)
    else:
        loop(2 if what == "max_iters" else 10)
    return out


def packed(out):
    """test_gpu_stereo_loop_bits.packed with this file's LARGE: the large outputs as `sha_<name>` and `shape_<name>`"""
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
    assert len(set(ids)) == len(ids) == 7 + 10 + 3 + 6
    assert sorted(os.listdir(GOLDEN_DIR)) == sorted(i + ".npz" for i in ids)


def test_no_case_was_recorded_as_singular():
    for case in CASES:
        g = np.load(os.path.join(GOLDEN_DIR, caseId(case) + ".npz"), allow_pickle=False)
        assert not [k for k in g.files if k.startswith("singular")], caseId(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=caseId)
def test_both_rig_solvers_keep_their_bits(case):
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
            assert {"max_iters": iters == 2, "err_min": iters == 1, "lambda": iters < 10 and not inside}[what]
    for name in sorted(got):
        assert got[name].dtype == g[name].dtype and got[name].shape == g[name].shape, name
        assert got[name].tobytes() == g[name].tobytes(), f"{name} differs from the recorded build"
