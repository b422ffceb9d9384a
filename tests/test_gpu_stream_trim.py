"""The stream kernel's batch loop loads the next batch's points and staged view constants into the registers of the
current ones, behind their last read, and forms the addresses from the wave's advancing uniform bases and a constant
32-bit lane offset that is clamped to the share's last point. That is addressing, register hand-over and loop
structure -- never an operand or an order of operations -- so the results keep their bits. Checked on the smallest shards at which those can go wrong, forced into the
stream form on an explicit number of waves (the plan then does not depend on the chip):

(a) P, sse and the trace of lmBegin / lmRun(3) / lmEnd are byte-for-byte those recorded from the build BEFORE the
    change (tests/golden/stream_trim/, written by tools/make_stream_trim_golden.py);
(b) the same trace agrees with oracle.c_oracle at the tolerance of tests/test_gpu_parity.py.

What each case covers is computed from the share arithmetic (shareProperties follows the kernel's batch loop on the
host) and asserted: test_cases_cover_the_batch_loop needs no GPU.
"""
import hashlib
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "stream_trim")

ROUNDS = 3           # lmRun(3): the bootstrap round and two iterations
MAX_ITERS = 8
# tests/test_gpu_parity.py:178 (test_config2_full_size_1000x54_vs_c_oracle): the damping column equal, error columns to
TRACE_RTOL = 1e-9

BOARDS = {64: (8, 8, 0.03), 68: (17, 4, 0.03), 200: (20, 10, 0.03)}
# (model, points per view, views, CALIB_STREAM_WAVES)
CASES = [
    (model, n, nv, waves)
    for n, nv, waves in ((64, 32, 32), (64, 32, 31), (64, 32, 12), (64, 32, 5), (64, 32, 1), (68, 40, 14), (200, 24, 9))
    for model in ("fisheye", "radtan") if (model, waves) != ("radtan", 1)
]
REQUIRED = {
    "wave of 1 batch", "wave of 2 batches", "wave of 3 batches", "wave of >= 5 batches",
    "share ends on a batch", "last batch is one group", "last wave is shorter", "wave shorter than a batch",
    "straddling batch, then one-view batch", "one-view batch, then straddling batch",
    "boundary at group 0 of a pass", "boundary at group 7 of a pass", "wave starts inside a view",
}


def caseId(case):
    model, n, nv, waves = case
    return f"{model}_n{n}_v{nv}_w{waves}"


def sharePlan(n, nv, waves):
    """-> (share, waves with work): makePlan's arithmetic for CALIB_FUSED_STREAM=1, CALIB_STREAM_WAVES=waves"""
    groups = nv * (n // 4)
    w = max(1, min(waves, nv))
    share = (groups + w - 1) // w
    return share, (groups + share - 1) // share


def shareProperties(n, nv, waves):
    """what the stream kernel's batch loop meets on this shard: the loop of fused_stream_kernel, wave by wave, on the host"""
    share, nw = sharePlan(n, nv, waves)
    gt = nv * (n // 4)
    props = set()
    for w in range(nw):
        g0 = w * share
        p0, p1 = 4 * g0, 4 * min(g0 + share, gt)
        full = p1 - p0 == 4 * share
        va = p0 // n
        vend = (va + 1) * n
        if p0 != va * n:
            props.add("wave starts inside a view")
        batches = (p1 - p0 + 63) // 64
        props.add({1: "wave of 1 batch", 2: "wave of 2 batches", 3: "wave of 3 batches"}.get(
            batches, "wave of >= 5 batches" if batches >= 5 else "wave of 4 batches"))
        if p1 - p0 < 64:
            props.add("wave shorter than a batch")
        if not full:
            assert w == nw - 1
            props.add("last wave is shorter")
        if full and share % 16 == 0:
            props.add("share ends on a batch")
        if full and share % 16 == 1:
            props.add("last batch is one group")
        before = None                                        # did the batch before this one straddle two views?
        for q0 in range(p0, p1, 64):
            qe = min(q0 + 64, p1)
            strad = q0 < vend < qe
            if before is not None and before != strad:
                props.add("straddling batch, then one-view batch" if before else "one-view batch, then straddling batch")
            before = strad
            for ps in (q0, q0 + 32):
                if ps >= p1:
                    break
                ng = min(32, p1 - ps) >> 2
                jb = (vend - ps) >> 2
                assert jb >= 0
                if jb < ng:
                    if ng == 8:
                        props.add(f"boundary at group {jb} of a pass")
                    vend += n
                    assert ((vend - ps) >> 2) >= ng           # a view is longer than a pass
    return props


def test_cases_cover_the_batch_loop():
    seen = set()
    for model, n, nv, waves in CASES:
        assert n in BOARDS and BOARDS[n][0] * BOARDS[n][1] == n and 24 <= nv <= 40
        seen |= shareProperties(n, nv, waves)
    for model in ("fisheye", "radtan"):                       # both instantiations meet every hand-over
        own = set()
        for m, n, nv, waves in CASES:
            if m == model:
                own |= shareProperties(n, nv, waves)
        assert {"straddling batch, then one-view batch", "one-view batch, then straddling batch",
                "last batch is one group", "wave starts inside a view"} <= own, (model, own)
    assert REQUIRED <= seen, REQUIRED - seen
    # the orientation points of the share arithmetic
    assert sharePlan(64, 32, 32)[0] == 16 and sharePlan(64, 32, 31)[0] == 17 and sharePlan(64, 32, 5)[0] == 103
    assert sharePlan(64, 32, 1)[0] == 512 and sharePlan(200, 24, 9)[0] == 134


# ---------------------------------------------------------------- the runs (shared by the golden tool)
def makeCaseShard(case):
    from camera_calibration_amd import synthetic
    model, n, nv, waves = case
    cfg = dict(synthetic.CONFIGS["c2" if model == "radtan" else "c3"], board=BOARDS[n])
    sh = synthetic.makeShard(cfg, viewStart=7, numViews=nv, noiseSigma=0.05)      # as tests/test_gpu_early_loads.py
    assert sh["pointsPerView"] == n
    return sh


def inputDigest(sh):
    h = hashlib.sha256()
    for key in ("viewOffsets", "sensorPoints", "modelPoints", "P0"):
        h.update(np.ascontiguousarray(sh[key]).tobytes())
    return h.hexdigest()


def runCase(case, sh):
    """lmBegin, lmRun(3), lmEnd in the stream form on the case's waves -> (sse, P, trace). The caller has the
    environment clean of other CALIB_* knobs."""
    import camera_calibration_amd as cca
    model, n, nv, waves = case
    os.environ["CALIB_FUSED_STREAM"] = "1"
    os.environ["CALIB_STREAM_WAVES"] = str(waves)
    try:
        eng = cca.RefineEngine(model, "f64")                  # (knobs are read at calib_create)
    finally:
        del os.environ["CALIB_FUSED_STREAM"], os.environ["CALIB_STREAM_WAVES"]
    try:
        eng.setProblem(sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"])
        assert eng.fusedForm() == sharePlan(n, nv, waves), (eng.fusedForm(), sharePlan(n, nv, waves))
        eng.lmBegin(sh["P0"], MAX_ITERS)
        eng.lmRun(ROUNDS)
        sse, P, iters, trace = eng.lmEnd()
    finally:
        eng.close()
    return np.float64(sse), P, np.ascontiguousarray(trace)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=caseId)
def test_stream_rounds_keep_their_bits_and_agree_with_the_oracle(case, monkeypatch):
    from oracle import c_oracle, calib_oracle as orc
    for key in ("CALIB_FUSED_STREAM", "CALIB_STREAM_WAVES", "CALIB_GRAM_FORM", "CALIB_UPD_LANE_VIEWS", "CALIB_LM_MODE",
                "CALIB_UPD_SMALL_VIEWS", "CALIB_HEAD_LOADS", "CALIB_ITEMS_PER_WAVE", "CALIB_GRAM_WPI"):
        monkeypatch.delenv(key, raising=False)
    model, n, nv, waves = case
    g = np.load(os.path.join(GOLDEN_DIR, caseId(case) + ".npz"), allow_pickle=False)
    sh = makeCaseShard(case)
    assert inputDigest(sh) == str(g["inputs"]), "the shard itself differs from the recorded one: not the stream kernel"
    sse, P, trace = runCase(case, sh)
    # (a) the bits of the build before the change
    assert trace.shape == g["trace"].shape and trace.shape[0] >= 1
    assert sse.tobytes() == g["sse"].tobytes(), (sse, g["sse"])
    assert P.tobytes() == g["P"].tobytes(), f"P differs in {int((P != g['P']).sum())} entries"
    assert trace.tobytes() == g["trace"].tobytes()
    # (b) the C oracle
    assert c_oracle.available()
    om = orc.RADTAN if model == "radtan" else orc.FISHEYE
    sseO, PO, trO = c_oracle.refine(om, sh["P0"], sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"], trace.shape[0])
    k = min(trace.shape[0], trO.shape[0])
    assert k == trace.shape[0]
    print(f"{caseId(case)}: {k} iterations, error columns rel diff "
          f"{np.max(np.abs(trace[:k, 1:3] - trO[:k, 1:3]) / np.abs(trO[:k, 1:3])):.2e}")
    assert np.array_equal(trace[:k, 3], trO[:k, 3]) and np.allclose(trace[:k, 1:3], trO[:k, 1:3], rtol=TRACE_RTOL)
