"""Two-kernel LM rounds that span several chunks on the device.

In two-kernel mode a round walks the shard's points in chunks of whole views (csrc/shard_layout.hpp): per chunk a
jacobian_kernel launch on [p0, p1), whose compact J goes to a buffer indexed from the chunk's first point, and a
gram_kernel launch on the chunk's items, whose workgroup partials are appended behind those of the chunks before. A
chunk closes at CALIB_CHUNK_POINTS points -- by default 1 << 26, so that everywhere else in the suite a round is one
chunk with origin 0. Here one ragged shard of ~5 000 points per camera model runs at chunk sizes 1, 257 and 1000, and
unset as the control, against oracle.c_oracle on the same inputs at the bars the suite already holds a single chunk to.

What the view sizes make the chunk loop meet (origins of every residue modulo 4, a stale tail in the J buffer, a chunk
that is one view of several items, a shorter chunk behind a longer one, a tile that touches 11 views, ..) is computed
from a restatement of makeShardLayout's chunk rule and asserted: test_cases_cover_the_chunk_loop needs no GPU.

Nothing is asserted bitwise BETWEEN chunk sizes in general: a chunk origin that is no multiple of 4 regroups a view's
points in gram_kernel's 4-point MFMA steps. The one exception is stated at test_normal_equations_against_the_oracle.
"""
import functools

import numpy as np
import pytest

TILE = 256            # kernels.hpp kTile: points per jacobian_kernel workgroup
ITEM = 512            # kernels.hpp kGramChunk: points per gram_kernel item
SINGLE_CHUNK = 1 << 26    # launch_plan.hpp: Knobs::chunk_points when CALIB_CHUNK_POINTS is not set

FIXED_SIZES = (5, 3, 64, 6, 255, 7, 257, 700, 4, 513, 1200, 63, 65, 3, 3, 3, 3, 3, 3, 3, 3, 512, 9)
# ... then 20 sizes drawn once, np.random.default_rng(0).integers(3, 120, 20), and kept as drawn: the chunk list is known
DRAWN_SIZES = (102, 77, 62, 34, 39, 7, 11, 4, 23, 98, 78, 109, 61, 73, 116, 88, 76, 66, 68, 112)
SIZES = np.array(FIXED_SIZES + DRAWN_SIZES, dtype=np.int64)          # in this order, not shuffled
OFFS = np.concatenate(([0], np.cumsum(SIZES))).astype(np.int64)
CHUNK_SIZES = (1, 257, 1000)
MODELS = ("radtan", "fisheye")
# every variable launch_plan.hpp's readKnobs looks at: a case runs with the ones it sets and no other
KNOBS = ("CALIB_CHUNK_POINTS", "CALIB_LM_MODE", "CALIB_HEAD_LOADS", "CALIB_ITEMS_PER_WAVE", "CALIB_UPD_LANE_VIEWS",
         "CALIB_UPD_SMALL_VIEWS", "CALIB_GRAM_FORM", "CALIB_FUSED_STREAM", "CALIB_STREAM_WAVES", "CALIB_GRAM_WPI")

BLOCK_TOL = 1e-11     # of the block's largest yardstick entry: tests/test_gpu_stereo*.py hold B, E, V, g to it
SSE_RTOL = 1e-11      # tests/test_gpu_scale.py, test_random_ragged_views_vs_c_oracle


# ---------------------------------------------------------------- the chunk rule, restated
def chunkList(chunkPoints, offs=OFFS):
    """makeShardLayout's chunks for views without an empty one: whole views, a chunk closes once it holds at least
    chunkPoints points -> [(p0, p1, view0, view1)]"""
    nv = offs.shape[0] - 1
    chunks, v = [], 0
    while v < nv:
        v0 = v
        p0 = p1 = int(offs[v])
        while v < nv and p1 - p0 < chunkPoints:
            v += 1
            p1 = int(offs[v])
        chunks.append((p0, p1, v0, v))
    return chunks


def tileViews(p0, p1, offs=OFFS):
    """views touched by each 256-point tile of [p0, p1), the tiles starting at p0 (jacobian_kernel stages that many)"""
    out = []
    for a in range(p0, p1, TILE):
        b = min(p1, a + TILE) - 1
        va = int(np.searchsorted(offs, a, side="right")) - 1
        vb = int(np.searchsorted(offs, b, side="right")) - 1
        out.append(vb - va + 1)
    return out


def test_cases_cover_the_chunk_loop():
    M, MN = SIZES.shape[0], int(OFFS[-1])
    assert M == 43 and tuple(SIZES[:len(FIXED_SIZES)]) == FIXED_SIZES and 4500 <= MN <= 5500
    assert chunkList(SINGLE_CHUNK) == [(0, MN, 0, M)]                     # the control: one chunk from point 0
    lists = {cp: chunkList(cp) for cp in CHUNK_SIZES}
    for cp, chunks in lists.items():
        assert len(chunks) > 1, cp
        assert chunks[0][0] == 0 and chunks[-1][1] == MN
        assert all(a[1] == b[0] and a[3] == b[2] for a, b in zip(chunks, chunks[1:]))      # whole views, back to back
        assert all(c[1] - c[0] >= cp for c in chunks[:-1])
        # bpart holds n_items + chunks workgroup partials; a chunk's gram launch appends ceil(items / (4 / wpi)) of them
        items = [sum((int(n) + ITEM - 1) // ITEM for n in SIZES[c[2]:c[3]]) for c in chunks]
        for wpi in (1, 2, 4):
            assert sum((i * wpi + 3) // 4 for i in items) <= sum(items) + len(chunks)
    assert [(c[2], c[3]) for c in lists[1]] == [(v, v + 1) for v in range(M)]              # at 1: one chunk per view
    every = [(cp, c) for cp, chunks in lists.items() for c in chunks]
    length = lambda c: c[1] - c[0]                                                        # noqa: E731
    # chunk origins of every residue modulo 4: the 4-point storage groups of gram_kernel are those of p - origin
    assert {c[0] % 4 for _, c in every} == {0, 1, 2, 3}
    assert {c[0] % 4 for c in lists[257]} == {0, 1, 2, 3}                                  # ... also where CALIB_GRAM_WPI varies
    # a stale tail in J: a chunk that ends inside a storage group, and another chunk writes the buffer after it
    assert any(length(a) % 4 for chunks in lists.values() for a in chunks[:-1])
    # a chunk that is a single view of several 512-point items, larger than chunk_points (700 and 1200)
    for n in (700, 1200):
        assert any(c[3] - c[2] == 1 and length(c) == n and n > cp and n > ITEM for cp, c in every), n
    # a chunk strictly shorter than the one before it: J is sized by the longest, and holds its leftovers
    assert any(length(b) < length(a) for chunks in lists.values() for a, b in zip(chunks, chunks[1:]))
    # a last chunk below chunk_points
    assert any(length(chunks[-1]) < cp for cp, chunks in lists.items())
    assert length(lists[257][-1]) < 257 and length(lists[1000][-1]) < 1000
    # a chunk with a 256-point tile that touches at least 8 views (the run of 3-point views)
    assert any(max(tileViews(c[0], c[1])) >= 8 for _, c in every)
    assert max(max(tileViews(c[0], c[1])) for c in lists[257]) >= 8
    # chunk tilings whose largest views-per-tile differs from that of the tiling from point 0 (max_views_per_tile, the
    # LDS size of every jacobian launch, is the maximum over both)
    whole = max(tileViews(0, MN))
    perSize = {cp: max(max(tileViews(c[0], c[1])) for c in chunks) for cp, chunks in lists.items()}
    assert any(span != whole for span in perSize.values()), (whole, perSize)
    # tiles that start where no tile of the single-chunk run starts: p_begin is no multiple of 256
    assert any(c[0] % TILE for _, c in every)
    # the orientation points of the arithmetic
    assert [length(c) for c in lists[1000]][:3] == [1297, 1717, 1005]
    assert [length(c) for c in lists[257]][:6] == [333, 264, 700, 517, 1200, 664]


# ---------------------------------------------------------------- the shard and its yardsticks (computed once, read-only)
class Shard:
    pass


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def shardOf(name):
    """the ragged shard of one camera model, built as tests/test_gpu_scale.py test_random_ragged_views_vs_c_oracle builds
    its own: general 3-D model points, poses of synthetic.sampleBoardPosesInCamera, 0.05 px noise, P0 1e-3 off"""
    from camera_calibration_amd import synthetic
    from oracle import c_oracle, calib_oracle as orc
    assert c_oracle.available(), "oracle/libcalib_oracle.so is not built"
    sh = Shard()
    sh.name = name
    sh.model = orc.RADTAN if name == "radtan" else orc.FISHEYE
    sh.L = orc.numShared(sh.model)
    rng = np.random.default_rng(1 if name == "radtan" else 2)
    M, MN = SIZES.shape[0], int(OFFS[-1])
    cfg = synthetic.CONFIGS["c2" if name == "radtan" else "c3"]
    corners = synthetic.checkerboardCorners(25, 18, 0.02)
    W = synthetic.sampleBoardPosesInCamera(corners, np.arange(100, 100 + M))
    Ptrue = synthetic.composeP(cfg["A"], W, cfg["k"])
    pts = np.vstack([np.column_stack((rng.uniform(0, 0.48, n), rng.uniform(0, 0.34, n), rng.uniform(-0.01, 0.01, n)))
                     for n in SIZES])
    sensor = c_oracle.evaluate(sh.model, Ptrue, OFFS, None, pts)["y"] + rng.normal(0, 0.05, (MN, 2))
    P0 = Ptrue * (1 + 1e-3 * rng.standard_normal(Ptrue.shape[0]))
    sh.offs, sh.pts, sh.sensor, sh.Ptrue, sh.P0 = frozen(OFFS), frozen(pts), frozen(sensor), frozen(Ptrue), frozen(P0)
    return sh


@functools.lru_cache(maxsize=None)
def normalYardstick(name):
    """orc.normalBlocks' four sums on the C oracle's J and r at P0, accumulated in np.longdouble: the yardstick's own
    rounding does not count -> dict B (L,L), E (M,L,6), V (M,6,6), g (K,) [longdouble], sse"""
    from oracle import c_oracle
    sh = shardOf(name)
    L, M = sh.L, SIZES.shape[0]
    eo = c_oracle.evaluate(sh.model, sh.P0, sh.offs, sh.sensor, sh.pts, wantJ=True)
    n = eo["Jc"].shape[0]
    Jr = eo["Jc"].reshape(2 * n, L + 6).astype(np.longdouble)
    rr = eo["r"].reshape(2 * n).astype(np.longdouble)
    Js, Je = Jr[:, :L], Jr[:, L:]
    B = Js.T @ Js
    g = np.empty(L + 6 * M, dtype=np.longdouble)
    g[:L] = Js.T @ rr
    E = np.empty((M, L, 6), dtype=np.longdouble)
    V = np.empty((M, 6, 6), dtype=np.longdouble)
    for i in range(M):
        a, b = 2 * int(sh.offs[i]), 2 * int(sh.offs[i + 1])
        E[i] = Js[a:b].T @ Je[a:b]
        V[i] = Je[a:b].T @ Je[a:b]
        g[L + 6 * i:L + 6 * i + 6] = Je[a:b].T @ rr[a:b]
    return {"B": B, "E": E, "V": V, "g": g, "sse": eo["sse"]}


@functools.lru_cache(maxsize=None)
def loopYardstick(name):
    """-> (c_oracle.step at P0 with lambda 1e-3, c_oracle.refine from P0 over 30 iterations)"""
    from oracle import c_oracle
    sh = shardOf(name)
    do = frozen(c_oracle.step(sh.model, sh.P0, sh.offs, sh.sensor, sh.pts, 1e-3))
    sseO, PO, trO = c_oracle.refine(sh.model, sh.P0, sh.offs, sh.sensor, sh.pts, 30)
    return do, (sseO, frozen(PO), frozen(trO))


def relIntr(P, Pref, L):
    """tests/test_gpu_scale.py relIntr: max relative error of the shared parameters, the skew relative to the focal length"""
    scale = np.maximum(np.abs(Pref[:L]), 1.0)
    scale[2] = abs(Pref[0])
    return float(np.max(np.abs(P[:L] - Pref[:L]) / scale))


def tagOf(chunkPoints):
    return "single" if chunkPoints is None else str(chunkPoints)


def makeEngine(monkeypatch, name, chunkPoints, dtype="f64", wpi=None):
    """a two-kernel engine on the model's shard with CALIB_CHUNK_POINTS = chunkPoints (None: unset) and no other knob but
    CALIB_GRAM_WPI = wpi (knobs are read at calib_create). The caller closes it."""
    import camera_calibration_amd as cca
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    if chunkPoints is not None:
        monkeypatch.setenv("CALIB_CHUNK_POINTS", str(chunkPoints))
    if wpi is not None:
        monkeypatch.setenv("CALIB_GRAM_WPI", str(wpi))
    sh = shardOf(name)
    eng = cca.RefineEngine(name, dtype)
    try:
        eng.setProblem(sh.offs, sh.sensor, sh.pts)
        eng.setLmMode("two_kernel")
    except Exception:
        eng.close()
        raise
    return eng


# ---------------------------------------------------------------- 2. the chunks really run
@pytest.mark.gpu
@pytest.mark.parametrize("chunkPoints", CHUNK_SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_every_chunk_is_launched(name, chunkPoints, monkeypatch):
    """six rounds that cannot end launch jacobian_kernel and gram_kernel once per chunk and round: a knob that was
    silently ignored would leave 6 launches of each and let every other test here pass on one chunk"""
    numChunks = len(chunkList(chunkPoints))
    assert numChunks > 1
    sh = shardOf(name)
    eng = makeEngine(monkeypatch, name, chunkPoints)
    try:
        eng.profileEnable(True, every=1)
        eng.lmBegin(sh.P0, 6, lamMin=0.0, lamMax=float("inf"), errMin=-float("inf"))
        eng.lmRun(6)
        eng.lmDone()
        jac, gram = eng.profileRead(0)[1], eng.profileRead(1)[1]
        sse, P, iters, trace = eng.lmEnd()
    finally:
        eng.close()
    print(f"{name} chunk {chunkPoints}: {numChunks} chunks, {jac} jacobian and {gram} gram launches in 6 rounds")
    assert jac == gram == 6 * numChunks, (jac, gram, numChunks)
    assert np.isfinite(sse) and np.isfinite(P).all()


# ---------------------------------------------------------------- 3. normal equations against the oracle
def blockRatios(got, yard, L):
    """worst |got - yardstick| / max |yardstick| per block kind, every view's E, V and g slice being a block of its own"""
    B, E, V, g = got
    M = E.shape[0]

    def ratio(x, y):
        return float(np.max(np.abs(x.astype(np.longdouble) - y)) / np.max(np.abs(y)))
    gv, gvY = g[L:].reshape(M, 6), yard["g"][L:].reshape(M, 6)
    return {"B": ratio(B, yard["B"]), "g_shared": ratio(g[:L], yard["g"][:L]),
            "E": max(ratio(E[i], yard["E"][i]) for i in range(M)),
            "V": max(ratio(V[i], yard["V"][i]) for i in range(M)),
            "g_view": max(ratio(gv[i], gvY[i]) for i in range(M))}


NORMAL_CASES = ([(name, cp, None) for name in MODELS for cp in CHUNK_SIZES + (None,)]
                + [("radtan", 257, wpi) for wpi in (1, 2, 4)])


@pytest.mark.gpu
@pytest.mark.parametrize("name,chunkPoints,wpi", NORMAL_CASES,
                         ids=[f"{n}-{tagOf(cp)}" + (f"-wpi{w}" if w else "") for n, cp, w in NORMAL_CASES])
def test_normal_equations_against_the_oracle(name, chunkPoints, wpi, monkeypatch):
    """B, g[:L] and every view's E, V, g of calib_normal_eq at P0 within 1e-11 of the block's largest entry of the
    longdouble sums over the C oracle's J and r; the control (CALIB_CHUNK_POINTS unset) goes through the same bars.

    Kept across chunkings, bit for bit: the records E, V, g of the views of a chunk whose origin is a multiple of 4.
    jacobian_kernel computes a point from its own inputs and its view's constants, whatever the tile it falls in, so J
    and r keep their bits; gram_kernel walks an item in the 4-point storage groups of p - origin, split over the item's
    waves by group number, and with origin = 0 (mod 4) those are the groups, the split and the order of the one-chunk
    run. (B and g[:L] sum workgroup partials whose composition follows the chunks' item ranges: no such claim.)"""
    sh, yard = shardOf(name), normalYardstick(name)
    L = sh.L
    eng = makeEngine(monkeypatch, name, chunkPoints, wpi=wpi)
    try:
        got = eng.normalEquations(sh.P0)
        sse = eng.evaluate(sh.P0)["sse"]
    finally:
        eng.close()
    B, E, V, g = got
    ratios = blockRatios(got, yard, L)
    sseRel = abs(sse - yard["sse"]) / yard["sse"]
    print(f"{name} chunk {tagOf(chunkPoints)} wpi {wpi or 'default'}: worst |d| / max |block| "
          + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()) + f" | sum r^2 rel {sseRel:.2e}")
    assert np.isfinite(B).all() and np.isfinite(E).all() and np.isfinite(V).all() and np.isfinite(g).all()
    for kind, worst in ratios.items():
        assert worst <= BLOCK_TOL, (kind, worst)
    assert sseRel <= SSE_RTOL
    assert np.array_equal(V, np.transpose(V, (0, 2, 1)))                     # V[i] is bitwise symmetric


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_views_of_aligned_chunks_keep_the_bits_of_one_chunk(name, monkeypatch):
    """the claim of test_normal_equations_against_the_oracle's docstring: E, V and g of those views, at every chunk size,
    against the single chunk"""
    sh = shardOf(name)
    L = sh.L
    outs = {}
    for cp in (None,) + CHUNK_SIZES:
        eng = makeEngine(monkeypatch, name, cp)
        try:
            outs[cp] = eng.normalEquations(sh.P0)
        finally:
            eng.close()
    ctl = outs[None]
    for cp in CHUNK_SIZES:
        got = outs[cp]
        views = [v for c in chunkList(cp) if c[0] % 4 == 0 for v in range(c[2], c[3])]
        assert views, cp                                                     # the first chunk's at least
        print(f"{name} chunk {cp}: {len(views)} views in chunks of origin 0 (mod 4)")
        for v in views:
            assert np.array_equal(got[1][v], ctl[1][v]) and np.array_equal(got[2][v], ctl[2][v]), (cp, v)
            assert np.array_equal(got[3][L + 6 * v:L + 6 * v + 6], ctl[3][L + 6 * v:L + 6 * v + 6]), (cp, v)


# ---------------------------------------------------------------- 4. step and loop against the C oracle
@pytest.mark.gpu
@pytest.mark.parametrize("chunkPoints", CHUNK_SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_step_and_loop_against_the_c_oracle(name, chunkPoints, monkeypatch):
    """the assertions and bars of tests/test_gpu_scale.py test_random_ragged_views_vs_c_oracle, over several chunks"""
    sh = shardOf(name)
    do, (sseO, PO, trO) = loopYardstick(name)
    eng = makeEngine(monkeypatch, name, chunkPoints)
    try:
        d = eng.stepDelta(sh.P0, 1e-3)
        sse, P, iters, trace = eng.refine(sh.P0, 30)
    finally:
        eng.close()
    n = min(5, iters, trO.shape[0])
    stepRel = np.linalg.norm(d - do) / np.linalg.norm(do)
    print(f"{name} chunk {chunkPoints}: step rel {stepRel:.2e} | {iters} iterations (oracle {trO.shape[0]}), sse rel "
          f"{abs(sse - sseO) / sseO:.2e}, first {n} error columns rel "
          f"{np.max(np.abs(trace[:n, 1:3] - trO[:n, 1:3]) / np.abs(trO[:n, 1:3])):.2e}, intrinsics {relIntr(P, PO, sh.L):.2e}")
    assert stepRel <= 1e-8
    assert abs(sse - sseO) <= 1e-8 * sseO
    assert n >= 1
    assert np.array_equal(trace[:n, 3], trO[:n, 3]) and np.allclose(trace[:n, 1:3], trO[:n, 1:3], rtol=1e-9)
    assert relIntr(P, PO, sh.L) < 1e-7


# ---------------------------------------------------------------- 5. determinism and the done flag
@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_chunked_loop_is_reproducible_and_rounds_after_the_end_change_nothing(name, monkeypatch):
    """Fixed-order sums: two refine calls on fresh engines return the same bytes. And the same bytes come from
    lmBegin / lmRun(iters + 5) / lmEnd, whose last rounds are enqueued after the loop has ended: both kernels of every
    chunk return on the done flag, although the host still launches them."""
    sh = shardOf(name)
    outs = []
    for rep in range(2):
        eng = makeEngine(monkeypatch, name, 257)
        try:
            outs.append(eng.refine(sh.P0, 30))
        finally:
            eng.close()
    (sseA, PA, itA, trA), (sseB, PB, itB, trB) = outs
    assert itA == itB and itA >= 1
    assert np.float64(sseA).tobytes() == np.float64(sseB).tobytes()
    assert PA.tobytes() == PB.tobytes() and np.ascontiguousarray(trA).tobytes() == np.ascontiguousarray(trB).tobytes()
    eng = makeEngine(monkeypatch, name, 257)
    try:
        eng.lmBegin(sh.P0, 30)
        eng.lmRun(itA + 5)                       # checkEvery = 0: every round is enqueued, the loop needs itA + 1 at most
        assert eng.lmDone()
        sseC, PC, itC, trC = eng.lmEnd()
    finally:
        eng.close()
    print(f"{name}: {itA} iterations, {itA + 5} rounds enqueued")
    assert itC == itA
    assert np.float64(sseC).tobytes() == np.float64(sseA).tobytes()
    assert PC.tobytes() == PA.tobytes() and np.ascontiguousarray(trC).tobytes() == np.ascontiguousarray(trA).tobytes()


# ---------------------------------------------------------------- 6. two neighbours of the same path
@pytest.mark.gpu
def test_covariance_over_several_chunks_against_the_qr_yardstick(monkeypatch):
    """calib_covariance runs the same chunk loop (a lambda = 0 round): at the refined P of the radtan shard, chunk size
    257, against tests/uncertainty_yardstick.py at its derived bar, as test_covariance_against_the_qr_yardstick"""
    from uncertainty_yardstick import checkCovariance, covarianceYardstick
    sh = shardOf("radtan")
    eng = makeEngine(monkeypatch, "radtan", 257)
    try:
        sse, P, iters, trace = eng.refine(sh.P0, 30)
        res = eng.covariance(P, wantViews=True, wantCross=True)
        again = eng.covariance(P, wantViews=True, wantCross=True)
    finally:
        eng.close()
    yard = covarianceYardstick(sh.model, P, sh.offs, sh.sensor, sh.pts)
    checkCovariance(res, yard, sh.L, [], "radtan chunk 257 two_kernel")
    for k in ("covShared", "covViews", "covCross", "std"):
        assert np.array_equal(res[k], again[k]), k
    assert res["sigma2"] == again["sigma2"]


@pytest.mark.gpu
@pytest.mark.parametrize("chunkPoints", (257, None), ids=tagOf)
def test_fp32_storage_over_several_chunks_vs_fp64_c_oracle(chunkPoints, monkeypatch):
    """fp32 points / J / r, radtan: the first rows of the trace against the fp64 C oracle at the bar of
    tests/test_gpu_scale.py test_fp32_config_at_full_size_vs_fp64_c_oracle (equal lambda and accept columns, error
    columns to 1e-5), for the single chunk and for chunks of 257 points"""
    sh = shardOf("radtan")
    _, (sseO, PO, trO) = loopYardstick("radtan")
    eng = makeEngine(monkeypatch, "radtan", chunkPoints, dtype="f32")
    try:
        sse, P, iters, trace = eng.refine(sh.P0, 30)
    finally:
        eng.close()
    n = min(4, iters, trO.shape[0])
    assert n >= 1
    print(f"radtan f32 chunk {tagOf(chunkPoints)}: {iters} iterations (oracle {trO.shape[0]}), first {n} rows: lambda "
          f"{trace[:n, 3]} vs {trO[:n, 3]}, accept {trace[:n, 4]} vs {trO[:n, 4]}, error columns rel "
          f"{np.max(np.abs(trace[:n, 1:3] - trO[:n, 1:3]) / np.abs(trO[:n, 1:3])):.2e}")
    assert np.array_equal(trace[:n, 3], trO[:n, 3]) and np.array_equal(trace[:n, 4], trO[:n, 4])
    assert np.allclose(trace[:n, 1:3], trO[:n, 1:3], rtol=1e-5)
