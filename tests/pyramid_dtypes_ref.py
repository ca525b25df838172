"""Numpy restatement of the pyramid semantics for float16 and uint32, the yardstick of
tests/test_pyramid_dtypes_host.py and tests/test_gpu_pyramid_dtypes.py.

tests/pyramid_ref.py already states every method for uint32 (its integer mean works in int64) and stride / min / max / median /
mode for float16 (numpy compares float16 by value).  Its float mean returns float32, so the float16 mean is stated here: the
float64 sum of the valid elements in (z, y, x) order, divided by the count, converted to float16 — numpy converts float64 to
float16 directly, with ONE rounding.  Finite float16 values are multiples of 2^-24 below 2^16, so eight of them sum exactly in
float64 and the count is a power of two: the result is the exact mean rounded once.
"""

import numpy as np

import pyramid_ref as base


def reduce_level(a, method):
    """One level down: (..., Z, Y, X) -> (..., ceil(Z/2), ceil(Y/2), ceil(X/2)), same dtype (float16 or uint32)."""
    a = np.asarray(a)
    if a.dtype not in (np.dtype(np.float16), np.dtype(np.uint32)):
        raise TypeError(f"pyramid_dtypes_ref states float16 and uint32, not {a.dtype}")
    if a.dtype == np.uint32 or method != "mean":
        out = base.reduce_level(a, method)
        assert out.dtype == a.dtype
        return out
    *lead, Z, Y, X = a.shape
    nz, ny, nx = -(-Z // 2), -(-Y // 2), -(-X // 2)
    pad = np.zeros((*lead, 2 * nz, 2 * ny, 2 * nx), np.float16)
    pad[..., :Z, :Y, :X] = a
    ok = np.zeros((2 * nz, 2 * ny, 2 * nx), bool)
    ok[:Z, :Y, :X] = True
    v, ok = base._blocks(pad), np.broadcast_to(base._blocks(ok), (*lead, nz, ny, nx, 8))
    s = np.zeros(v.shape[:-1], np.float64)
    for i in range(8):  # sequentially, in (z, y, x) order
        s = s + np.where(ok[..., i], v[..., i].astype(np.float64), 0.0)
    return (s / ok.sum(-1)).astype(np.float16)  # float64 -> float16: one rounding


def pyramid_ref(vol, levels, method):
    """Levels 1..levels-1, each reduced from the one before it."""
    out, cur = [], np.asarray(vol)
    for _ in range(1, levels):
        cur = reduce_level(cur, method)
        out.append(cur)
    return out


# (z, y, x) order; float64 mean 1 + 2^-11 + 2^-27 -> float16 0x3C01 (1 + 2^-10); through float32 it becomes 1 + 2^-11, a tie, -> 0x3C00
WITNESS = np.array([2, 2, 1 + 2.0 ** -8, 1, 1, 1, 2.0 ** -24, 0], np.float16).reshape(2, 2, 2)
WITNESS_MEAN_BITS = 0x3C01
WITNESS_TWICE_ROUNDED_BITS = 0x3C00
