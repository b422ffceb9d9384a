"""Calibration uncertainty, the parts that need no GPU: the C-ABI declares and exports the new entry points, the
CalibrationUncertainty helpers behave on a hand-made covariance, and refineDistributed(..., uncertainty=True) over
gloo -- with a CPU shard double that adds covLocal / covFinish in numpy to tests/shard_double.OracleShardEngine --
returns a shared covariance that is bitwise equal on all ranks, equals the single-shard QR yardstick
(tests/uncertainty_yardstick.py, where the tolerance is derived) and carries the pose blocks in global view order."""
import os
import re
import socket

import numpy as np
import pytest

from camera_calibration_amd import _native as nat
from camera_calibration_amd import uncertainty
from conftest import ROOT, loadGolden
from oracle import calib_oracle as orc
from shard_double import OracleShardEngine
from uncertainty_yardstick import checkCovariance, covarianceYardstick

NEW_SYMBOLS = ("calib_view_errors", "calib_cov_local", "calib_cov_finish", "calib_covariance")


def test_header_declares_and_library_exports_the_uncertainty_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert lib.calib_version() >= 420


def _handMade():
    names = ("alpha", "beta", "gamma", "uc")
    d = np.array([2.0, 0.5, 0.0, 3.0])                      # gamma fixed: zero row and column
    R = np.array([[1.0, 0.3, 0.0, -0.2], [0.3, 1.0, 0.0, 0.5], [0.0, 0.0, 0.0, 0.0], [-0.2, 0.5, 0.0, 1.0]])
    C = R * np.outer(d, d)
    return uncertainty.CalibrationUncertainty(
        sigma=0.1, dof=100, rms=0.14, names=names, stdShared=d.copy(), covShared=C, stdPoses=np.ones((2, 6)),
        covPoses=np.tile(np.eye(6), (2, 1, 1)), perViewRms=np.array([0.1, 0.2]), perViewMax=np.array([0.3, 0.4]),
        values=np.array([500.0, 510.0, 0.0, 320.0]), fixedMask=0b100), R


def test_correlation_of_a_hand_made_covariance():
    u, R = _handMade()
    corr = u.correlationShared()
    assert np.array_equal(np.diagonal(corr), np.ones(4))
    off = ~np.eye(4, dtype=bool)
    assert np.allclose(corr[off], R[off], rtol=0, atol=1e-15)
    assert np.array_equal(corr, corr.T)
    assert not corr[2, [0, 1, 3]].any()                      # the fixed parameter correlates with nothing


def test_summary_prints_one_line_per_name_and_marks_fixed_ones():
    u, _ = _handMade()
    lines = u.summary().splitlines()
    for n in u.names:
        mine = [ln for ln in lines if ln.startswith(n + " = ")]
        assert len(mine) == 1, (n, lines)
        if n == "gamma":
            assert mine[0].endswith("(fixed)") and "±" not in mine[0]
        else:
            assert "±" in mine[0] and "(fixed)" not in mine[0]
    assert "alpha = 500 ± 2" in lines[0]
    assert u.isFixed(2) and not u.isFixed(0)


# ---- the sharded protocol over gloo, CPU shard double ---------------------------------------------------------------
class CovShardEngine(OracleShardEngine):
    """OracleShardEngine + the stepping form of the covariance (include/calib_lm.h: calib_cov_local /
    calib_cov_finish) in numpy, through the Schur route and the reduce-buffer layout of csrc/kernels.hpp"""

    def covLocal(self, P):
        P = np.asarray(P, dtype=np.float64).ravel()
        assert P.shape[0] == self.L + 6 * self.M
        self._covBlocks = self._blocks(P)
        self.red[:self.VA] = self._variant(self._covBlocks, 0.0)
        self.red[self.VA:] = 0.0

    def covFinish(self, totalPoints, totalViews, wantViews=True, wantCross=False):
        L, M = self.L, self.M
        dof = 2 * int(totalPoints) - (L + 6 * int(totalViews))
        if dof <= 0:
            raise ValueError("no degrees of freedom left")
        sigma2 = self.red[2 * L * L + 2 * L + 1] / dof
        S = (self.red[:L * L] - self.red[L * L:2 * L * L]).reshape(L, L)
        Css = sigma2 * np.linalg.inv(S)
        _, E, V, _, _ = self._covBlocks
        Vinv = np.linalg.inv(V) if M else np.zeros((0, 6, 6))
        Y = Vinv @ np.transpose(E, (0, 2, 1))                # (M, 6, L)
        covViews = sigma2 * Vinv + Y @ Css @ np.transpose(Y, (0, 2, 1))
        std = np.concatenate((np.sqrt(np.diagonal(Css)), np.sqrt(np.einsum("mii->mi", covViews)).ravel()))
        return {"sigma2": float(sigma2), "dof": dof, "covShared": Css, "covViews": covViews,
                "covCross": -np.einsum("lk,mjk->mlj", Css, Y) if wantCross else None, "std": std}


def _freePort():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def _worker(rank, world, port, outDir):
    import torch
    import torch.distributed as dist
    from camera_calibration_amd import distributed
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = loadGolden("g9_noisy.npz")
        calls = [0]

        def allReduceFactory(eng):
            buf = torch.from_numpy(eng.red)

            def allReduce():
                calls[0] += 1
                dist.all_reduce(buf, op=dist.ReduceOp.SUM)
            return allReduce

        def factory(o, s, m):
            return CovShardEngine(orc.RADTAN, o, s, m)

        args = ("radtan", g["Pfinal"], g["viewOffsets"], g["sensorPoints"], g["modelPoints"], 2)
        plain = distributed.refineDistributed(*args, engineFactory=factory, allReduceFactory=allReduceFactory)
        callsPlain, calls[0] = calls[0], 0
        out = distributed.refineDistributed(*args, engineFactory=factory, allReduceFactory=allReduceFactory,
                                            uncertainty=True)
        assert len(plain) == 4 and len(out) == 5
        assert np.array_equal(plain[1], out[1])
        unc = out[4]
        np.savez(os.path.join(outDir, f"u{rank}.npz"), P=out[1], callsPlain=callsPlain, callsUnc=calls[0],
                 sigma2=unc["sigma2"], dof=unc["dof"], covShared=unc["covShared"], covViews=unc["covViews"],
                 std=unc["std"])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_refine_distributed_uncertainty_over_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _freePort(), str(tmp_path)), nprocs=world, join=True)
    outs = [np.load(os.path.join(tmp_path, f"u{r}.npz")) for r in range(world)]
    g = loadGolden("g9_noisy.npz")
    offs, s, m = g["viewOffsets"], g["sensorPoints"], g["modelPoints"]
    for o in outs:
        assert np.array_equal(o["covShared"], outs[0]["covShared"])          # bitwise equal on all ranks
        assert np.array_equal(o["covViews"], outs[0]["covViews"]) and np.array_equal(o["std"], outs[0]["std"])
        assert float(o["sigma2"]) == float(outs[0]["sigma2"]) and int(o["dof"]) == int(outs[0]["dof"])
        assert int(o["callsUnc"]) == int(o["callsPlain"]) + 1                 # exactly one more all-reduce
    o = outs[0]
    P = o["P"]
    yard = covarianceYardstick(orc.RADTAN, P, offs, s, m)
    res = {"sigma2": float(o["sigma2"]), "dof": int(o["dof"]), "covShared": o["covShared"], "covViews": o["covViews"],
           "std": o["std"], "covCross": None}
    assert res["covViews"].shape == (15, 6, 6) and res["std"].shape == P.shape
    # global view order: checkCovariance compares view i's block with the yardstick's rows L + 6 i of the GLOBAL problem
    checkCovariance(res, yard, 10, (), f"gloo world {world}")
