"""The LM round's kernels ask for everything they need -- kernel arguments, tables, points, view constants, shared
parameters of both P buffers, the LM state -- before their first wait, and take the state up behind the requests. That
moves loads, never an operand or an order of operations, so results keep their bits; a finished refinement stays
untouched by rounds enqueued after it in EVERY kernel form, and a launch with an explicit P (sel == 0) never looks at the
LM state. Checked here where tests/test_gpu_round_edges.py (stream kernel + 16-lane update kernel, fisheye) does not reach:

* the stream form for BOTH models on a shard of 24 views x 64 points dealt to five waves: radial-tangential uses the
  third 16-byte piece of each lane's op entries, fisheye only the first two; shares of 77 groups cut views, several views
  end inside one wave, and the second workgroup has one valid wave and three invalid ones that still reach the barrier;
* rounds after the end in the tile form (f64 and f32), the block form, and with the small-shard and the one-lane-per-view
  update kernels;
* calib_normal_eq / calib_eval at a given P on a handle whose refinement has ended.
"""
import numpy as np
import pytest

import camera_calibration_amd as cca
from camera_calibration_amd import synthetic
from oracle import calib_oracle as orc

pytestmark = pytest.mark.gpu

MAX_ITERS = 200      # the stop rule (lambda leaves [1e-10, 1e10]) ends these refinements long before


def relIntr(P, Pref, L):
    """max relative error of the shared parameters (as in tests/test_gpu_scale.py)"""
    scale = np.maximum(np.abs(Pref[:L]), 1.0)
    scale[2] = abs(Pref[0])
    return float(np.max(np.abs(P[:L] - Pref[:L]) / scale))


def makeShard(base, board, views, viewStart=7, noise=0.05):
    cfg = dict(synthetic.CONFIGS[base], board=board)
    return synthetic.makeShard(cfg, viewStart=viewStart, numViews=views, noiseSigma=noise)


STREAM_ENV = {"CALIB_FUSED_STREAM": "1", "CALIB_STREAM_WAVES": "5"}


def engine(sh, model, dtype, env, monkeypatch):
    for key in ("CALIB_FUSED_STREAM", "CALIB_STREAM_WAVES", "CALIB_GRAM_FORM", "CALIB_UPD_LANE_VIEWS",
                "CALIB_UPD_SMALL_VIEWS", "CALIB_HEAD_LOADS", "CALIB_ITEMS_PER_WAVE", "CALIB_GRAM_WPI"):
        monkeypatch.delenv(key, raising=False)
    for key, value in env.items():                    # (knobs are read at calib_create)
        monkeypatch.setenv(key, value)
    eng = cca.RefineEngine(model, dtype)
    eng.setProblem(sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"])
    return eng


# ---------------------------------------------------------------- stream form, both models
@pytest.fixture(scope="module", params=["radtan", "fisheye"])
def streamCase(request):
    """the shard and its references, computed once per model and left unchanged"""
    name = request.param
    model = orc.RADTAN if name == "radtan" else orc.FISHEYE
    sh = makeShard("c2" if name == "radtan" else "c3", (8, 8, 0.04 if name == "radtan" else 0.03), 24)
    offs, s, m, P0 = sh["viewOffsets"], sh["sensorPoints"], sh["modelPoints"], sh["P0"]
    from oracle import c_oracle
    Jc = orc.jacobianCompact(model, P0, offs, m)
    blocks = orc.normalBlocks(model, Jc, s - orc.projectAllPoints(model, P0, offs, m), offs)
    if c_oracle.available():
        sseO, PO, trO = c_oracle.refine(model, P0, offs, s, m, 25)
    else:
        sseO, PO, trO = orc.refineSchur(model, P0, offs, s, m, 25)
    return name, model, sh, blocks, (sseO, np.asarray(PO), np.asarray(trO))


def test_stream_form_on_five_waves_against_the_oracle(streamCase, monkeypatch):
    """tolerances: those of test_stream_form_of_the_fused_kernel in tests/test_gpu_scale.py"""
    name, model, sh, (Bo, Eo, Vo, go), (sseO, PO, trO) = streamCase
    L = orc.numShared(model)
    eng = engine(sh, name, "f64", STREAM_ENV, monkeypatch)
    try:
        share, waves = eng.fusedForm()
        assert (share, waves) == (77, 5), (share, waves)     # 384 groups on five waves: two workgroups, three idle waves
        B, E, V, g = eng.normalEquations(sh["P0"])
        errs = [np.abs(x - y).max() / np.abs(y).max() for x, y in ((B, Bo), (V, Vo), (E, Eo), (g, go))]
        sse, P, iters, trace = eng.refine(sh["P0"], 25)
        n = min(5, iters, trO.shape[0])
        print(f"{name}: B/V/E/g rel err {errs}, sse {sse:.6e} vs {sseO:.6e}, intrinsics {relIntr(P, PO, L):.2e}")
        assert errs[0] <= 1e-11 and errs[1] <= 1e-11 and errs[2] <= 1e-11 and errs[3] <= 1e-10
        assert abs(sse - sseO) <= 1e-8 * sseO
        assert np.array_equal(trace[:n, 3], trO[:n, 3]) and np.allclose(trace[:n, 1:3], trO[:n, 1:3], rtol=1e-9)
        assert relIntr(P, PO, L) < 1e-7
    finally:
        eng.close()


def test_stream_form_on_five_waves_is_reproducible(streamCase, monkeypatch):
    name, model, sh, _, _ = streamCase
    eng = engine(sh, name, "f64", STREAM_ENV, monkeypatch)
    try:
        sseA, PA, itA, trA = eng.refine(sh["P0"], 25)
        sseB, PB, itB, trB = eng.refine(sh["P0"], 25)
        assert itA == itB and sseA == sseB
        assert np.array_equal(PA, PB) and np.array_equal(trA, trB)
    finally:
        eng.close()


# ---------------------------------------------------------------- rounds after the end, every other form
def tileShard():
    return makeShard("c2", (9, 6, 0.05), 12)                  # 12 views x 54 points: one batch, the tile form


def blockShard():
    return makeShard("c3", (20, 10, 0.03), 12)                # 12 views x 200 points: the 4x4x4 block form


def streamShard():
    return makeShard("c3", (8, 8, 0.03), 24)


FORMS = {
    "tile_f64": (tileShard, "radtan", "f64", {}),
    "tile_f32": (tileShard, "radtan", "f32", {}),
    "block": (blockShard, "fisheye", "f64", {"CALIB_FUSED_STREAM": "0"}),
    "small_update": (streamShard, "fisheye", "f64", STREAM_ENV),                 # the default at these sizes
    "lane_update": (streamShard, "fisheye", "f64", dict(STREAM_ENV, CALIB_UPD_LANE_VIEWS="1", CALIB_UPD_SMALL_VIEWS="0")),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_rounds_after_the_end_change_nothing(form, monkeypatch):
    make, model, dtype, env = FORMS[form]
    sh = make()
    eng = engine(sh, model, dtype, env, monkeypatch)
    try:
        assert (eng.fusedForm()[0] > 0) == ("CALIB_STREAM_WAVES" in env)
        sseA, PA, itA, trA = eng.refine(sh["P0"], MAX_ITERS)
        print(f"{form}: {itA} iterations, accepted {int(trA[:, 4].sum())}, last lambda {trA[-1, 3]:.1e}, sse {sseA:.6e}")
        assert 0 < itA < MAX_ITERS                            # ended by the stop rule
        eng.lmBegin(sh["P0"], MAX_ITERS)
        eng.lmRun(itA + 1)                                    # the bootstrap round + itA iterations
        assert eng.lmDone()
        for _ in range(6):                                    # whole rounds, enqueued whatever the host knows
            eng.lmLocal()
            eng.lmUpdate()
        assert eng.lmDone()
        sseC, PC, itC, trC = eng.lmEnd()
        assert itC == itA and sseC == sseA
        assert np.array_equal(PC, PA) and np.array_equal(trC, trA)
    finally:
        eng.close()


# ---------------------------------------------------------------- sel == 0 ignores the state
@pytest.mark.parametrize("form", ["tile_f64", "block", "small_update"])
def test_explicit_parameters_ignore_a_finished_state(form, monkeypatch):
    make, model, dtype, env = FORMS[form]
    sh = make()
    P = sh["P0"]
    fresh = engine(sh, model, dtype, env, monkeypatch)
    try:
        want = fresh.normalEquations(P)
        wantEv = fresh.evaluate(P, wantY=True, wantR=True)
    finally:
        fresh.close()
    eng = engine(sh, model, dtype, env, monkeypatch)
    try:
        _, _, iters, _ = eng.refine(P, MAX_ITERS)
        assert 0 < iters < MAX_ITERS                          # the handle's state says "done"
        got = eng.normalEquations(P)
        gotEv = eng.evaluate(P, wantY=True, wantR=True)
        for x, y in zip(got, want):
            assert np.array_equal(x, y)
        assert gotEv["sse"] == wantEv["sse"]
        assert np.array_equal(gotEv["y"], wantEv["y"]) and np.array_equal(gotEv["r"], wantEv["r"])
    finally:
        eng.close()
