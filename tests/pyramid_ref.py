"""Numpy restatement of the pyramid semantics, the yardstick of tests/test_pyramid_host.py and
tests/test_gpu_pyramid.py.

Level k of a (..., Z, Y, X) array has extents ceil(n / 2) of level k-1 and voxel (z, y, x) reduces the block
[2z, min(2z + 2, n)) x [2y, ...) x [2x, ...) of level k-1 as stored.  Partial blocks are handled by masks, integer means by exact
integer arithmetic, the float32 mean by a float64 sum in (z, y, x) order rounded once.  Leading axes are batch axes.
"""

import numpy as np

METHODS = ("stride", "mean", "min", "max", "median", "mode")


def _hi(dtype):
    return np.inf if dtype.kind == "f" else np.iinfo(dtype).max


def _lo(dtype):
    return -np.inf if dtype.kind == "f" else np.iinfo(dtype).min


def _blocks(a):
    """(..., Z, Y, X) padded to even extents -> (..., Z/2, Y/2, X/2, 8), the block's elements in (z, y, x) order."""
    *lead, Z, Y, X = a.shape
    b = a.reshape(*lead, Z // 2, 2, Y // 2, 2, X // 2, 2)
    n = len(lead)
    b = b.transpose(*range(n), n, n + 2, n + 4, n + 1, n + 3, n + 5)
    return b.reshape(*lead, Z // 2, Y // 2, X // 2, 8)


def reduce_level(a, method):
    """One level down: (..., Z, Y, X) -> (..., ceil(Z/2), ceil(Y/2), ceil(X/2)), same dtype."""
    a = np.asarray(a)
    dt = a.dtype
    *lead, Z, Y, X = a.shape
    nz, ny, nx = -(-Z // 2), -(-Y // 2), -(-X // 2)
    pad = np.zeros((*lead, 2 * nz, 2 * ny, 2 * nx), dt)
    pad[..., :Z, :Y, :X] = a
    ok = np.zeros((2 * nz, 2 * ny, 2 * nx), bool)
    ok[:Z, :Y, :X] = True
    v, ok = _blocks(pad), np.broadcast_to(_blocks(ok), (*lead, nz, ny, nx, 8))
    cnt = ok.sum(-1)
    if method == "stride":
        return v[..., 0].copy()
    if method == "min":
        return np.where(ok, v, _hi(dt)).min(-1).astype(dt)
    if method == "max":
        return np.where(ok, v, _lo(dt)).max(-1).astype(dt)
    if method == "mean":
        if dt.kind == "f":
            s = np.zeros(v.shape[:-1], np.float64)
            for i in range(8):  # sequentially, in (z, y, x) order
                s = s + np.where(ok[..., i], v[..., i].astype(np.float64), 0.0)
            return (s / cnt).astype(np.float32)
        s = np.where(ok, v.astype(np.int64), 0).sum(-1)
        q = np.floor_divide(s, cnt)
        r = s - q * cnt
        up = (2 * r > cnt) | ((2 * r == cnt) & (q % 2 == 1))  # to nearest, ties to even
        return (q + up).astype(dt)
    if method == "median":  # the lower median
        w = np.sort(np.where(ok, v, _hi(dt)), axis=-1)
        return np.take_along_axis(w, ((cnt - 1) // 2)[..., None], axis=-1)[..., 0].astype(dt)
    if method == "mode":  # the most frequent value, the smallest among ties
        eq = (v[..., :, None] == v[..., None, :]) & ok[..., None, :]
        c = np.where(ok, eq.sum(-1), -1)
        best = c.max(-1, keepdims=True)
        return np.where(c == best, v, _hi(dt)).min(-1).astype(dt)
    raise ValueError(method)


def pyramid_ref(vol, levels, method):
    """Levels 1..levels-1, each reduced from the one before it."""
    out, cur = [], np.asarray(vol)
    for _ in range(1, levels):
        cur = reduce_level(cur, method)
        out.append(cur)
    return out


def level_shape(shape, k):
    s = tuple(int(n) for n in shape)
    for _ in range(k):
        s = tuple(-(-n // 2) for n in s)
    return s


def expected_datasets(ds0, levels):
    """multiscales[0].datasets after a pyramid of `levels` levels: level 0's transforms, Z/Y/X scales times 2^k."""
    out = [ds0]
    for k in range(1, levels):
        trs = []
        for tr in ds0.get("coordinateTransformations", []):
            tr = dict(tr)
            if tr["type"] == "scale":
                tr["scale"] = list(tr["scale"][:-3]) + [s * 2 ** k for s in tr["scale"][-3:]]
            trs.append(tr)
        out.append({"path": str(k), "coordinateTransformations": trs})
    return out
