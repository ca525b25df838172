"""float64 restatement of the pairwise registration and position solve behind ``estimate-stitch --pcc-channel-name``
(the reference: biahub/vendor/stitch/tile.py, _dexp_shim.py, graph.py), and the seeded scenes its tests cut
their tiles from.  The numerics are numpy / scipy only and evaluated in float64, so it is what the float32 pipelines (the reference's
and the GPU's) are measured against.  One deliberate difference from the reference: the nominal offset of an edge is
(Y - overlap, 0) for a neighbour below and (0, X - overlap) for one to the right (the reference swaps Y and X).
"""

from __future__ import annotations

import numpy as np
import scipy.ndimage as ndi
from scipy.optimize import minimize

BELOW, RIGHT = 0, 1
SIGMA = 1.5


# ---- scenes -------------------------------------------------------------------------------------------------------------
def scene(seed: int, shape) -> np.ndarray:
    """Smooth background (U(0, 1) blurred with sigma 2, times 200) plus sparse blurred points (0.5 % Bernoulli field blurred
    with sigma 1.5, times 3000), float64."""
    rng = np.random.default_rng(seed)
    smooth = ndi.gaussian_filter(rng.random(shape), 2.0) * 200.0
    points = ndi.gaussian_filter((rng.random(shape) < 0.005).astype(np.float64), 1.5) * 3000.0
    return smooth + points


def as_dtype(tile: np.ndarray, dtype) -> np.ndarray:
    """uint16: plus 100, rounded and clipped; float32: minus 150, so that the minimum is negative."""
    dtype = np.dtype(dtype)
    if dtype == np.uint16:
        return np.clip(np.rint(tile + 100.0), 0, 65535).astype(np.uint16)
    if dtype == np.float32:
        return (tile - 150.0).astype(np.float32)
    raise ValueError(dtype)


def unflip(tile: np.ndarray, flipud: bool, fliplr: bool) -> np.ndarray:
    """What has to be stored so that flipping it gives ``tile``."""
    if fliplr:
        tile = tile[:, ::-1]
    if flipud:
        tile = tile[::-1]
    return np.ascontiguousarray(tile)


def cut_pair(seed: int, tile_yx, relation: int, overlap: int, disp, dtype, flipud=False, fliplr=False):
    """(a, b): tiles of one scene, b at a's position plus the nominal offset of ``relation`` plus ``disp`` (dy, dx), each with
    its own N(0, 5) noise, converted by ``as_dtype`` and stored unflipped."""
    Y, X = tile_yx
    nominal = (Y - overlap, 0) if relation == BELOW else (0, X - overlap)
    pad = 40
    sc = scene(seed, (2 * Y + 2 * pad, 2 * X + 2 * pad))
    rng = np.random.default_rng(seed + 7919)
    tiles = []
    for oy, ox in ((pad, pad), (pad + nominal[0] + disp[0], pad + nominal[1] + disp[1])):
        t = sc[oy:oy + Y, ox:ox + X] + rng.normal(0.0, 5.0, (Y, X))
        tiles.append(unflip(as_dtype(t, dtype), flipud, fliplr))
    return tiles[0], tiles[1]


def well_tiles(seed: int, grid_xy, tile_yx, overlap: int, errors: dict, dtype, flipud=False, fliplr=False) -> dict:
    """{(x, y): tile} of a well cut from one scene: cell (x, y) sits at (y * (Y - overlap), x * (X - overlap)) plus its integer
    error ``errors[(x, y)]`` = (dy, dx) (default none)."""
    Y, X = tile_yx
    nx, ny = grid_xy
    pad = 24
    sc = scene(seed, (ny * Y + 2 * pad, nx * X + 2 * pad))
    rng = np.random.default_rng(seed + 104729)
    out = {}
    for x in range(nx):
        for y in range(ny):
            ey, ex = errors.get((x, y), (0, 0))
            oy, ox = pad + y * (Y - overlap) + ey, pad + x * (X - overlap) + ex
            t = sc[oy:oy + Y, ox:ox + X] + rng.normal(0.0, 5.0, (Y, X))
            out[(x, y)] = unflip(as_dtype(t, dtype), flipud, fliplr)
    return out


# ---- registration of one edge -------------------------------------------------------------------------------------------
def strips(tile_a, tile_b, relation: int, overlap: int, flipud=False, fliplr=False):
    a, b = (np.asarray(t) for t in (tile_a, tile_b))
    if flipud:
        a, b = a[::-1], b[::-1]
    if fliplr:
        a, b = a[:, ::-1], b[:, ::-1]
    if relation == BELOW:
        return a[-overlap:, :], b[:overlap, :]
    return a[:, -overlap:], b[:, :overlap]


def prepare(strip) -> np.ndarray:
    s = np.asarray(strip, np.float64)
    if s.min() < 0:
        s = s - s.min()
    s = ndi.gaussian_filter(s, SIGMA, mode="reflect")
    s = np.log1p(np.log1p(s))
    s = np.abs(ndi.sobel(s, axis=0, mode="reflect")) + np.abs(ndi.sobel(s, axis=1, mode="reflect"))
    return s * np.outer(np.sqrt(np.hanning(s.shape[0])), np.sqrt(np.hanning(s.shape[1])))


def correlation(pa, pb) -> np.ndarray:
    R = np.fft.fft2(pa) * np.conj(np.fft.fft2(pb))
    R = R / (np.abs(R) + 1e-6)
    return np.fft.fftshift(np.fft.ifft2(R).real)


def smoothed_crop(corr):
    """(crop after noise-floor clipping and wrap smoothing, r per axis)."""
    r = tuple(int(0.45 * n) for n in corr.shape)
    c = tuple(n // 2 for n in corr.shape)
    sel = corr[:c[0] - r[0], :c[1] - r[1]].ravel()[::16]
    if sel.size == 0:
        floor = corr.mean()
    else:
        floor = np.quantile(sel, 0.999)
        if not np.isfinite(floor):
            floor = sel.mean()
    crop = corr[c[0] - r[0]:c[0] + r[0], c[1] - r[1]:c[1] + r[1]]
    crop = np.maximum(crop, floor) - floor
    return ndi.gaussian_filter(crop, SIGMA, mode="wrap"), r


def mask_half(crop_shape):
    return tuple(max(8, int(s ** 0.9) // 8) for s in crop_shape)


def shift_confidence(corr):
    sm, r = smoothed_crop(corr)
    peak_at = np.unravel_index(int(np.argmax(sm)), sm.shape)
    peak = float(sm[peak_at])
    masked = sm.copy()
    m = mask_half(sm.shape)
    masked[peak_at[0] - m[0]:peak_at[0] + m[0], peak_at[1] - m[1]:peak_at[1] + m[1]] = 0  # numpy slice rule on purpose
    return (int(peak_at[0]) - r[0], int(peak_at[1]) - r[1]), (peak - float(masked.max())) / (1e-6 + peak)


def peak_margin(corr) -> float:
    """(peak - largest value outside a correctly clipped +-m window) / peak on the smoothed crop."""
    sm, _ = smoothed_crop(corr)
    p = np.unravel_index(int(np.argmax(sm)), sm.shape)
    m = mask_half(sm.shape)
    masked = sm.copy()
    masked[max(p[0] - m[0], 0):p[0] + m[0], max(p[1] - m[1], 0):p[1] + m[1]] = -np.inf
    return float((sm[p] - masked.max()) / sm[p])


def register_strips(strip_a, strip_b) -> dict:
    pa, pb = prepare(strip_a), prepare(strip_b)
    corr = correlation(pa, pb)
    shift, conf = shift_confidence(corr)
    return {"shift": shift, "confidence": conf, "prepared": (pa, pb), "corr": corr}


def register_edge(tile_a, tile_b, relation: int, overlap: int, flipud=False, fliplr=False) -> dict:
    """Steps 3 to 7: the edge's shift carries the nominal offset."""
    sa, sb = strips(tile_a, tile_b, relation, overlap, flipud, fliplr)
    out = register_strips(sa, sb)
    Y, X = np.asarray(tile_a).shape
    nominal = (Y - overlap, 0) if relation == BELOW else (0, X - overlap)
    out["pcc_shift"] = out["shift"]
    out["shift"] = (out["shift"][0] + nominal[0], out["shift"][1] + nominal[1])
    return out


# ---- graph ----------------------------------------------------------------------------------------------------------------
def curve_order(cells):
    """The cells [(x, y)] along the reference's curve over the smallest power-of-two square holding max(coordinate) + 1."""
    present = {(int(x), int(y)) for x, y in cells}
    n = max(max(c) for c in present) + 1
    side = 1
    while side < n:
        side *= 2
    return [c for c in _curve_top_down(side) if c in present]


def _curve_top_down(side):
    """Cell of every index d, lowest level first: level k (size s = 2**k) reads bits 2k, 2k+1 of d and transforms the cell
    built so far inside its s x s square before offsetting it: (rx, ry) = (1, 0) mirrors it in both axes (the textbook Hilbert
    curve also transposes there; the reference does not), (0, 0) transposes it."""
    out = []
    for d in range(side * side):
        x = y = 0
        s, t = 1, d
        while s < side:
            hi, lo = (t >> 1) & 1, t & 1
            rx, ry = hi, lo ^ hi
            if ry == 0 and rx == 1:
                x, y = s - 1 - x, s - 1 - y
            elif ry == 0:
                x, y = y, x
            x, y = x + s * rx, y + s * ry
            t >>= 2
            s *= 2
        out.append((x, y))
    return out


def edge_list(cells):
    order = curve_order(cells)
    present = set(order)
    edges = []
    for x, y in order:
        if (x, y + 1) in present:
            edges.append(((x, y), (x, y + 1), BELOW))
        if (x + 1, y) in present:
            edges.append(((x, y), (x + 1, y), RIGHT))
    return order, edges


def solve_positions(edges, n_tiles, guess_i, guess_j) -> np.ndarray:
    """Step 8: [(ia, ib, (si, sj))] -> (n_tiles, 2) integer positions."""
    A = np.zeros((len(edges) + 1, n_tiles), np.float32)
    rhs = np.zeros((len(edges) + 1, 2), np.float32)
    for k, (ia, ib, s) in enumerate(edges):
        A[k, ia] = -1
        A[k, ib] = 1
        rhs[k] = s
    A[-1, 0] = 1
    A = A.astype(np.float64)
    cols = []
    for axis, guess in enumerate((guess_i, guess_j)):
        yv = rhs[:, axis].astype(np.float64)
        x0 = np.asarray(guess, np.float64)
        res = minimize(lambda x: (1.0 / len(yv)) * float(np.abs(A @ x - yv).sum()), x0, method="L-BFGS-B", tol=1e-5,
                       options=dict(maxiter=10 ** 8, maxfun=10 ** 12, gtol=1e-5, eps=1e-5))
        cols.append(res.x if res.success else x0)
    pos = np.stack(cols, axis=1)
    pos -= pos.min(axis=0)
    return np.trunc(pos).astype(np.int64)


# ---- plates for the command-line tests ------------------------------------------------------------------------------------
CHANNELS = ["GFP", "Phase"]
PLANE = (1, 1)  # (channel index, z index) that holds the tiles; every other plane is zero


def write_plate(store, wells: dict, stage_px: dict, scale_yx=(0.5, 0.25), z_slices: int = 2, chunks_yx=None):
    """An HCS plate with micro-manager stage metadata.  ``wells``: {"row/col": {FOV name: (Y, X) tile}}; ``stage_px``:
    {"row/col/name": (y, x)} stage position in pixels (written in micrometres through ``scale_yx``).  The tile is plane
    z = 1 of channel "Phase".  Returns the position paths in the order of ``wells``."""
    from biahub_amd import io

    keys = [(*well.split("/"), name) for well, fovs in wells.items() for name in fovs]
    first = next(iter(next(iter(wells.values())).values()))
    Y, X = first.shape
    shape = (1, len(CHANNELS), z_slices, Y, X)
    io.create_empty_plate(store, keys, CHANNELS, shape, chunks=(1, 1, 1, *(chunks_yx or (Y, X))), scale=(1, 1, 2.0, *scale_yx),
                          dtype=first.dtype, version="0.4")
    entries = []
    for key in keys:
        name = "/".join(key)
        label = f"{key[0]}{key[1]}-Site_{key[2]}"
        y, x = stage_px[name]
        entries.append({"Label": label, "DefaultXYStage": "XY", "DefaultZStage": "Z", "XY": [1000.0 + x * scale_yx[1], -300.0 + y * scale_yx[0]],
                        "Z": 10.0})
        pos = io.open_ome_zarr(store.joinpath(*key))
        pos.update_zattrs({"omero": {**pos.zattrs["omero"], "name": label}})
        vol = np.zeros(shape[2:], first.dtype)
        vol[PLANE[1]] = wells["/".join(key[:2])][key[2]]
        pos.data.write_volume(0, PLANE[0], vol)
    attrs = io._read_group_attrs(store)
    attrs["Summary"] = {"StagePositions": entries}
    io._write_group(store, io._group_format(store), attrs, "0.4")
    return [store.joinpath(*k) for k in keys]


def expected_translations(wells: dict, stage_px: dict, overlap, flipud=False, fliplr=False, flipxy=False, solver=None) -> dict:
    """What ``estimate-stitch --pcc-channel-name`` has to write for ``write_plate(store, wells, stage_px)``: this module's edge
    shifts, ``solver`` (optimal_positions of the product, or ``solve_positions``) for the positions, then the flips, the
    non-negative shift and the rounding of the metadata path.  z is 0 for every FOV (one stage z)."""
    solver = solver or solve_positions
    out = {}
    for well, fovs in wells.items():
        names = list(fovs)
        a = np.array([[0.0, *stage_px[f"{well}/{n}"]] for n in names])
        a -= a.min(axis=0)
        cells = [(int(n[:3]), int(n[3:])) for n in names]
        _, edges = edge_list(cells)
        if edges:
            index = {c: k for k, c in enumerate(cells)}
            rows = []
            for ca, cb, rel in edges:
                r = register_edge(fovs[names[index[ca]]], fovs[names[index[cb]]], rel, overlap, flipud, fliplr)
                rows.append((index[ca], index[cb], (float(r["shift"][0]), float(r["shift"][1]))))
            pos = np.asarray(solver(rows, len(names), a[:, 1], a[:, 2]), np.float64)
            a[:, 1], a[:, 2] = pos[:, 0], pos[:, 1]
        if fliplr:
            a[:, 2] *= -1
        if flipud:
            a[:, 1] *= -1
        if flipxy:
            a[:, [1, 2]] = a[:, [2, 1]]
        a -= np.minimum(a.min(axis=0), 0)
        for k, n in enumerate(names):
            out[f"{well}/{n}"] = [float(v) for v in np.round(a[k], 2)]
    return out
