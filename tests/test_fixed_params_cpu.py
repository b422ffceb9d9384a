"""Fixed shared parameters and pose-only refinement, the parts that need no GPU: the C-ABI declares and exports
the new entry points, names / aliases / masks resolve as documented, value overrides land in the start point, and
the ranks of refineDistributed agree on the mask or raise together (gloo, CPU shard double)."""
import os
import re
import socket

import numpy as np
import pytest

import camera_calibration_amd as cca
from camera_calibration_amd import _native as nat
from camera_calibration_amd import fixed
from conftest import ROOT, loadGolden

NEW_SYMBOLS = ("calib_set_fixed_shared", "calib_get_fixed_shared", "calib_refine_poses")


def test_header_declares_and_library_exports_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "calib_lm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(calib_[a-z0-9_]+)\s*\(", text))
    lib = nat.loadLibrary()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/calib_lm.h"
        assert n in nat.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert lib.calib_version() >= 410


def test_shared_parameter_names_in_the_order_of_P():
    assert cca.RadialTangentialModel().sharedParameterNames() == (
        "alpha", "beta", "gamma", "uc", "vc", "k1", "k2", "p1", "p2", "k3")
    assert cca.FisheyeModel().sharedParameterNames() == ("alpha", "beta", "gamma", "uc", "vc", "k1", "k2", "k3", "k4")
    assert fixed.sharedNames(nat.MODEL_RADTAN) == cca.RadialTangentialModel().sharedParameterNames()
    assert fixed.sharedNames(nat.MODEL_FISHEYE) == cca.FisheyeModel().sharedParameterNames()


@pytest.mark.parametrize("model,L", [(cca.RadialTangentialModel, 10), (cca.FisheyeModel, 9)])
def test_every_name_and_alias_maps_to_its_bits(model, L):
    names = model().sharedParameterNames()
    for i, n in enumerate(names):
        assert fixed.resolveFixed(names, [n]) == (1 << i, {})
        assert fixed.resolveFixed(names, n) == (1 << i, {})          # one bare name
    allK = sum(1 << i for i in range(5, L))
    want = {"skew": 0b00100, "focal": 0b00011, "principal_point": 0b11000, "intrinsics": 0b11111,
            "distortion": allK, "all": (1 << L) - 1}
    if L == 10:
        want["tangential"] = (1 << 7) | (1 << 8)
    for alias, mask in want.items():
        assert fixed.resolveFixed(names, (alias,))[0] == mask, alias
    assert fixed.resolveFixed(names, ("gamma", names[-1]))[0] == 0b100 | 1 << (L - 1)
    assert fixed.resolveFixed(names, ("γ", "α"))[0] == 0b101             # the reference's own spelling of the symbols
    assert fixed.resolveFixed(names, ()) == (0, {}) and fixed.resolveFixed(names, None) == (0, {})
    # integer masks pass through, bits at or above L do not
    assert fixed.resolveFixed(names, 0b100) == (0b100, {})
    assert fixed.resolveFixed(names, np.int64((1 << L) - 1)) == ((1 << L) - 1, {})
    with pytest.raises(ValueError):
        fixed.resolveFixed(names, 1 << L)
    with pytest.raises(ValueError):
        fixed.resolveFixed(names, -1)
    assert fixed.maskNames(names, 0b100 | 1 << (L - 1)) == ("gamma", names[-1])


def test_unknown_names_raise_value_error_listing_the_valid_ones():
    rad, fish = cca.RadialTangentialModel().sharedParameterNames(), cca.FisheyeModel().sharedParameterNames()
    with pytest.raises(ValueError, match="alpha, beta, gamma, uc, vc, k1, k2, p1, p2, k3"):
        fixed.resolveFixed(rad, ("k7",))
    with pytest.raises(ValueError, match="alpha, beta, gamma, uc, vc, k1, k2, k3, k4"):
        fixed.resolveFixed(fish, ("p1",))
    with pytest.raises(ValueError):
        fixed.resolveFixed(fish, ("tangential",))
    with pytest.raises(ValueError):
        fixed.resolveFixed(rad, {"k4": 0.0})
    with pytest.raises(ValueError):
        fixed.resolveFixed(rad, (3,))                      # names are strings; a mask is a bare integer
    with pytest.raises(ValueError):
        cca.Calibrator(cca.FisheyeModel(), fixed=("p2",))


def test_value_overrides_land_in_the_start_point():
    g = loadGolden("g2_config1_radtan.npz")
    P0 = g["P0"]
    cal = cca.Calibrator(cca.RadialTangentialModel(), fixed={"skew": 0.0, "k3": 0.25, "uc": None})
    assert cal.fixedMask == 0b100 | 1 << 9 | 1 << 3
    P = cal._startPoint(P0)
    assert P is not P0 and P[2] == 0.0 and P[9] == 0.25
    keep = [i for i in range(P0.shape[0]) if i not in (2, 9)]
    assert np.array_equal(P[keep], P0[keep])               # uc was named without a value: the start point's own
    assert P0[2] != 0.0                                    # the caller's array is not written to
    col = cal._startPoint(P0.reshape(-1, 1))               # the (K,1) vector of _composeParameterVector
    assert col.shape == (P0.shape[0], 1) and col[2, 0] == 0.0 and col[9, 0] == 0.25
    # an alias with a value gives it to each of its parameters
    cal.setFixed({"principal_point": 100.0})
    assert cal.fixedMask == 0b11000 and list(cal._startPoint(P0)[3:5]) == [100.0, 100.0]
    # names only: nothing is copied
    cal.setFixed(("gamma",))
    assert cal._startPoint(P0) is P0
    cal.setFixed(())
    assert cal.fixedMask == 0


# ---- refineDistributed over gloo: the ranks agree on the mask or raise together -------------------------------
def _freePort():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def _worker(rank, world, port, case, outDir):
    import torch
    import torch.distributed as dist
    from camera_calibration_amd import distributed
    from oracle import calib_oracle as orc
    from shard_double import OracleShardEngine

    class MaskTaker(OracleShardEngine):
        """takes the mask as a real engine would; this file is about the protocol, the masked step itself is the
        subject of tests/test_gpu_fixed_params.py"""
        received = None

        def setFixedShared(self, mask):
            MaskTaker.received = mask

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = loadGolden("g2_config1_radtan.npz")

        def allReduceFactory(eng):
            buf = torch.from_numpy(eng.red)
            return lambda: dist.all_reduce(buf, op=dist.ReduceOp.SUM)

        engineClass = OracleShardEngine if case == "engine_without_method" else MaskTaker
        fixedShared = {"agree": ("gamma", "k3"), "agree_empty": (), "engine_without_method": ("gamma",),
                       "disagree": ("gamma", "k3") if rank == 0 else ("gamma",),
                       "one_rank_empty": () if rank == 1 else ("skew",),
                       "bad_name_on_rank1": ("gamma", "k9") if rank == 1 else ("gamma",)}[case]
        out = {"error": "", "message": "", "received": -1}
        try:
            distributed.refineDistributed("radtan", g["P0"], g["viewOffsets"], g["sensorPoints"], g["modelPoints"], 3,
                                          engineFactory=lambda o, s, m: engineClass(orc.RADTAN, o, s, m),
                                          allReduceFactory=allReduceFactory, fixedShared=fixedShared)
        except Exception as e:      # noqa: BLE001
            out["error"], out["message"] = type(e).__name__, str(e)
        if MaskTaker.received is not None:
            out["received"] = MaskTaker.received
        np.savez(os.path.join(outDir, f"mask{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["agree", "agree_empty", "disagree", "one_rank_empty", "bad_name_on_rank1",
                                  "engine_without_method"])
def test_refine_distributed_ranks_agree_on_the_mask_or_raise_together(tmp_path, case):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_worker, args=(world, _freePort(), case, str(tmp_path)), nprocs=world, join=True)
    outs = [np.load(os.path.join(tmp_path, f"mask{r}.npz")) for r in range(world)]
    errs = [str(o["error"]) for o in outs]
    if case == "agree":
        assert errs == ["", ""] and [int(o["received"]) for o in outs] == [0b100 | 1 << 9] * 2
    elif case == "agree_empty":
        assert errs == ["", ""] and [int(o["received"]) for o in outs] == [0, 0]
    elif case in ("disagree", "one_rank_empty"):
        assert errs == ["ValueError", "ValueError"]        # on EVERY rank, before any engine was begun
        assert all("disagree" in str(o["message"]) for o in outs)
        assert [int(o["received"]) for o in outs] == [-1, -1]
    elif case == "bad_name_on_rank1":
        assert errs == ["RuntimeError", "ValueError"] and "k9" in str(outs[1]["message"])
    else:
        assert errs == ["TypeError", "TypeError"] and "setFixedShared" in str(outs[0]["message"])
