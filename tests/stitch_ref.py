"""Float64 numpy restatement of the reference's stitch blend (biahub/stitch.py:196-311 write_output_chunk with one chunk per
mosaic) in closed form, in the reference's operation order: out = sum_i x_i * (w_i / (sum_j w_j + 1e-8)), FOV by FOV in list
order.  Test infrastructure: the golden cases (tests/golden/stitch.npz) pin it to the reference bit for bit.

The weight of FOV voxel (z, y, x) is w(d), d = min(y, Y-1-y, x, X-1-x): the 2-D Euclidean distance transform of the FOV's
interior (a complete one-pixel background ring, so the nearest zero lies along an axis); w(0) = 0, w(d) = d ** p otherwise;
a FOV with Y < 3 or X < 3 has no interior and weighs 0 everywhere.
"""

from __future__ import annotations

import numpy as np


def output_shape(shifts, tile_shape):
    """(int(max sz) + Z, int(max sy) + Y, int(max sx) + X) (biahub/stitch.py:167-193)."""
    s = np.asarray(list(shifts), np.float64).reshape(-1, 3)
    return tuple(int(s[:, a].max()) + int(tile_shape[a - 3]) for a in range(3))


def distance_map(Y: int, X: int) -> np.ndarray:
    """(Y, X) float64: d = min(y, Y-1-y, x, X-1-x), all zero when the FOV has no interior."""
    if Y < 3 or X < 3:
        return np.zeros((Y, X))
    y, x = np.arange(Y)[:, None], np.arange(X)[None, :]
    return np.minimum(np.minimum(y, Y - 1 - y), np.minimum(x, X - 1 - x)).astype(np.float64)


def weight_map(Y: int, X: int, exponent: float) -> np.ndarray:
    d = distance_map(Y, X)
    w = np.zeros_like(d)
    np.power(d, float(exponent), out=w, where=d > 0)
    return w


def placements(shifts, fov_shape):
    """floor(shift) per FOV and axis, (n, 3) int64; the shifts are non-negative."""
    s = np.asarray(list(shifts), np.float64).reshape(-1, 3)
    if (s < 0).any():
        raise ValueError("negative shift")
    return np.floor(s).astype(np.int64)


def stitch_ref(fovs, shifts, exponent: float = 1.0, with_bound: bool = False):
    """fovs: list of (Z, Y, X) arrays (or (..., Z, Y, X): leading axes are carried), shifts: (n, 3) floats >= 0.
    Returns the float64 mosaic; with_bound also K (covering FOVs per (z, y, x) voxel, int) and A = sum_i w_i |x_i| / (sum w + 1e-8)."""
    fovs = [np.asarray(f) for f in fovs]
    Z, Y, X = fovs[0].shape[-3:]
    lead = fovs[0].shape[:-3]
    off = placements(shifts, (Z, Y, X))
    mz, my, mx = output_shape(shifts, (Z, Y, X))
    w2 = weight_map(Y, X, exponent)
    sw = np.zeros((mz, my, mx))
    K = np.zeros((mz, my, mx), np.int64)
    boxes = []
    for oz, oy, ox in off:
        box = (slice(oz, oz + Z), slice(oy, oy + Y), slice(ox, ox + X))
        boxes.append(box)
        sw[box] += w2[None]
        K[box] += 1
    out = np.zeros(lead + (mz, my, mx))
    A = np.zeros(lead + (mz, my, mx)) if with_bound else None
    for f, box in zip(fovs, boxes):
        wm = w2[None] / (sw[box] + 1e-8)
        sl = (Ellipsis, *box)
        out[sl] += f * wm
        if with_bound:
            A[sl] += np.abs(f.astype(np.float64)) * wm
    return (out, K, A) if with_bound else out


def stitch_ref_gathered(values, dists, exponent: float):
    """The same blend on gathered inputs: values (m, K) float64 (the covering FOVs' voxels in list order, anything where
    dists < 0), dists (m, K) int (d of each, -1 = this FOV does not cover the voxel).  Returns (out, A, K) of length m."""
    values = np.asarray(values, np.float64)
    dists = np.asarray(dists)
    cov = dists >= 0
    d = np.where(cov, dists, 0).astype(np.float64)
    w = np.zeros_like(d)
    np.power(d, float(exponent), out=w, where=d > 0)
    sw = w.sum(axis=1, keepdims=True)
    wm = w / (sw + 1e-8)
    out = np.zeros(len(values))
    A = np.zeros(len(values))
    for k in range(values.shape[1]):
        v = np.where(cov[:, k], values[:, k], 0.0)
        out += v * wm[:, k]
        A += np.abs(v) * wm[:, k]
    return out, A, cov.sum(axis=1)


def seeded_fovs(seed: int, n: int, shape, dtype) -> list:
    """The inputs of a golden case: n arrays of `shape` ((T, Z, Y, X)), regenerated from the seed."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return [(rng.standard_normal(shape) * 100).astype(dt) for _ in range(n)]
    info = np.iinfo(dt)
    return [rng.integers(info.min, int(info.max) + 1, shape).astype(dt) for _ in range(n)]
