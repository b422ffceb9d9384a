"""What sits at the edges of an LM round's launches -- the order in which a kernel asks for its inputs and for the LM
state, and where it tests the finished flag (fused_stream_kernel, the y == 2 layer of schur_kernel, lm_update_step) --
changes no operand and no order of operations, so it must not change a bit of the results, and a refinement that is over
must stay untouched by the rounds a host enqueues after it. Checked on two uniform fisheye shards that take the stream
form of the fused kernel and update_backsub_kernel (16 lanes per view): a c3-shaped one (200 points per view) and one with
more views than one trip of that kernel's grid-stride loop covers (2 048 workgroups x 16 views = 32 768). Both end by the
stop rule after accepted AND rejected steps, so both record and both parameter buffers have been the current one."""
import numpy as np
import pytest

import camera_calibration_amd as cca
from camera_calibration_amd import synthetic
from oracle import calib_oracle as orc

pytestmark = pytest.mark.gpu

MAX_ITERS = 200      # the stop rule (lambda leaves [1e-10, 1e10]) ends these refinements long before


def shortViews():
    """64 points per view (one batch of the stream form), more than 32 768 views"""
    cfg = dict(synthetic.CONFIGS["c3"])
    cfg["board"] = (8, 8, 0.03)
    return synthetic.makeShard(cfg, viewStart=0, numViews=33000, noiseSigma=0.1)


def c3Shaped():
    return synthetic.makeShard("c3", viewStart=40, numViews=600, noiseSigma=0.1)


@pytest.fixture(scope="module", params=["c3_shaped_600_views", "short_33000_views"])
def shard(request):
    return request.param, (c3Shaped() if request.param.startswith("c3") else shortViews())


def engineFor(sh, monkeypatch):
    # (knobs are read at calib_create) stream form whatever the view count; neither the small-shard nor the
    # one-lane-per-view update kernel: update_backsub_kernel
    monkeypatch.setenv("CALIB_FUSED_STREAM", "1")
    monkeypatch.setenv("CALIB_UPD_SMALL_VIEWS", "0")
    monkeypatch.setenv("CALIB_UPD_LANE_VIEWS", "1000000000")
    eng = cca.RefineEngine("fisheye", "f64")
    eng.setProblem(sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"])
    assert eng.fusedForm()[0] > 0
    return eng


def test_refinement_is_reproducible_and_untouched_by_rounds_after_its_end(shard, monkeypatch):
    name, sh = shard
    eng = engineFor(sh, monkeypatch)
    try:
        sseA, PA, itA, trA = eng.refine(sh["P0"], MAX_ITERS)
        sseB, PB, itB, trB = eng.refine(sh["P0"], MAX_ITERS)
        print(f"{name}: {itA} iterations, accepted {int(trA[:, 4].sum())}, rejected {int((trA[:, 4] == 0).sum())}, "
              f"last lambda {trA[-1, 3]:.1e}, sse {sseA:.6e}")
        # ended by the stop rule, not by the iteration limit
        assert 0 < itA < MAX_ITERS
        # (c) both record / parameter buffers have been the chosen one: accepted AND rejected steps
        assert (trA[:, 4] == 1).any() and (trA[:, 4] == 0).any()
        # (a) two refinements from the same P0: the same bits
        assert itA == itB and sseA == sseB
        assert np.array_equal(PA, PB) and np.array_equal(trA, trB)
        # (b) the same refinement in the stepping form, then rounds enqueued after its end: nothing moves
        eng.lmBegin(sh["P0"], MAX_ITERS)
        eng.lmRun(itA + 1)                                   # the bootstrap round + itA iterations
        assert eng.lmDone()
        for _ in range(6):                                    # whole rounds, enqueued whatever the host knows
            eng.lmLocal()
            eng.lmUpdate()
        eng.lmRun(3)
        assert eng.lmDone()
        sseC, PC, itC, trC = eng.lmEnd()
        assert itC == itA and sseC == sseA
        assert np.array_equal(PC, PA) and np.array_equal(trC, trA)
    finally:
        eng.close()


def test_the_chosen_inputs_accept_and_reject_on_the_oracle_too():
    """the property (c) relies on belongs to the input, not to the device code: the CPU oracle's loop on the c3-shaped
    shard accepts in its first rounds and rejects at the noise floor (src/calibrate.py:155-168)"""
    sh = c3Shaped()
    from oracle import c_oracle
    args = (orc.FISHEYE, sh["P0"], sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"], 12)
    trace = c_oracle.refine(*args)[2] if c_oracle.available() else orc.refineSchur(*args)[2]
    trace = np.asarray(trace)
    assert (trace[:, 4] == 1).any() and (trace[:, 4] == 0).any()
