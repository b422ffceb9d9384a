"""Which shared parameters the LM holds fixed: names, aliases and the bit mask of calib_set_fixed_shared.

The reference refines every parameter (src/calibrate.py:117-171); this is surface beside the drop-in one.
Bit i of the mask is shared parameter i in the order of the parameter vector P (include/calib_lm.h):
alpha, beta, gamma, uc, vc, then the model's distortion coefficients.
"""
import operator
from collections.abc import Mapping

from . import _native as nat

INTRINSIC_NAMES = ("alpha", "beta", "gamma", "uc", "vc")
DISTORTION_NAMES = {nat.MODEL_RADTAN: ("k1", "k2", "p1", "p2", "k3"),      # src/distortion.py:75
                    nat.MODEL_FISHEYE: ("k1", "k2", "k3", "k4")}           # src/distortion.py:195
_SYNONYMS = {"α": "alpha", "β": "beta", "γ": "gamma"}       # DistortionModel.getIntrinsicSymbols spells them so


def sharedNames(modelId):
    """names of the L shared parameters of a model, in the order of P"""
    return INTRINSIC_NAMES + DISTORTION_NAMES[modelId]


def aliases(names):
    """alias -> parameter names, for a model whose shared parameters are `names`"""
    k = tuple(names[5:])
    out = {"skew": ("gamma",), "focal": ("alpha", "beta"), "principal_point": ("uc", "vc"),
           "intrinsics": tuple(names[:5]), "distortion": k, "all": tuple(names)}
    if "p1" in k and "p2" in k:
        out["tangential"] = ("p1", "p2")
    return out


def _indices(names, name):
    if not isinstance(name, str):
        raise ValueError(f"fixed parameter names are strings, got {name!r}")
    name = _SYNONYMS.get(name, name)
    if name in names:
        return (names.index(name),)
    al = aliases(names)
    if name in al:
        return tuple(names.index(n) for n in al[name])
    raise ValueError(f"unknown fixed parameter {name!r}: this model has {', '.join(names)}; "
                     f"aliases {', '.join(sorted(al))}")


def resolveFixed(names, fixed):
    """`fixed` -> (mask, {index: value}).

    fixed: None / empty (nothing fixed), an integer mask, one name, an iterable of names, or a mapping
    name -> value. A parameter named without a value (or with None) keeps the start point's value; one with a
    value has it written into the start point before the loop (applyFixedValues). An alias with a value gives
    that value to each of its parameters. Unknown names raise ValueError listing the valid ones."""
    names = tuple(names)
    L = len(names)
    if fixed is None:
        return 0, {}
    if isinstance(fixed, bool):
        raise ValueError("fixed must be names, a mapping name -> value or an integer mask")
    try:
        mask = operator.index(fixed)
    except TypeError:
        mask = None
    if mask is not None:
        if mask < 0 or mask >> L:
            raise ValueError(f"fixed mask {mask:#x} has bits outside the {L} shared parameters ({', '.join(names)})")
        return mask, {}
    if isinstance(fixed, str):
        fixed = (fixed,)
    items = fixed.items() if isinstance(fixed, Mapping) else ((n, None) for n in fixed)
    mask, values = 0, {}
    for name, value in items:
        for i in _indices(names, name):
            mask |= 1 << i
            if value is not None:
                values[i] = float(value)
    return mask, values


def applyFixedValues(P, values):
    """copy of the parameter vector P (any shape holding K values) with the value overrides written in"""
    import numpy as np
    P = np.array(P, dtype=np.float64, copy=True)
    flat = P.reshape(-1)
    for i, v in values.items():
        flat[i] = v
    return P


def maskNames(names, mask):
    return tuple(n for i, n in enumerate(names) if mask >> i & 1)
