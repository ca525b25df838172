"""Refine a well's stitch translations by phase correlation of neighbouring FOVs (reference: ``biahub estimate-stitch
--pcc-channel-name``, biahub/estimate_stitch.py:155-191, biahub/vendor/stitch/tile.py, _dexp_shim.py, graph.py, connect.py).

A FOV's grid cell is read from its name ``XXXYYY`` (column x, row y).  Tiles are visited along the reference's space-filling
curve and every tile is paired with its neighbour below, then with its neighbour to the right.  Each pair is registered on its
overlap strip on the GPU (``csrc/stitch_pcc.hip``, ``bh_stitch_edge_shifts``: all edges of a well in one call);
the edge shifts are then solved for consistent positions by L1 regression (scipy's L-BFGS-B, as the reference runs it), warm
started from the stage positions.

Deviations from the reference: the nominal offset added to an edge's shift is ``Y - overlap`` rows for a
neighbour below and ``X - overlap`` columns for one to the right (the reference swaps the two extents, which is the same for
square tiles); the overlap is an option (the reference fixes 300).
"""

from __future__ import annotations

import ctypes as C
import re

import click
import numpy as np

from . import _lib

BELOW, RIGHT = 0, 1
DEFAULT_OVERLAP = 300
MIN_OVERLAP = 16
_NAME = re.compile(r"^\d{6}$")


def parse_grid_names(names) -> list[tuple[int, int]]:
    """[(x, y)] grid cells of FOV names ``XXXYYY`` or ``row/col/XXXYYY``.  ValueError for a name that is not six digits."""
    cells = []
    for name in names:
        last = str(name).split("/")[-1]
        if not _NAME.match(last):
            raise ValueError(f"{last!r} is not a grid name XXXYYY (three digits of column x, three digits of row y)")
        cells.append((int(last[:3]), int(last[3:])))
    return cells


def _curve_cell(side: int, d: int) -> tuple[int, int]:
    """Cell d of the reference's curve over a side x side grid (side a power of two).  It is the Hilbert construction, two bits
    of d per level from the lowest, except that the quadrant with bits (1, 0) is mirrored in both axes and NOT transposed; the
    textbook curve transposes it too.  The order is kept as the reference has it: it fixes the order of the edges, and through
    them the rows of the position solve."""
    x = y = 0
    s = 1
    while s < side:
        rx = (d >> 1) & 1
        ry = (d ^ rx) & 1
        if ry == 0:
            x, y = (s - 1 - x, s - 1 - y) if rx else (y, x)
        x, y = x + s * rx, y + s * ry
        d >>= 2
        s *= 2
    return x, y


def hilbert_edges(cells) -> tuple[list[tuple[int, int]], list[tuple[tuple[int, int], tuple[int, int], int]]]:
    """(order, edges) of a well's grid cells [(x, y)]: ``order`` lists the cells along the curve over the smallest power-of-two
    square holding max(coordinate) + 1; ``edges`` lists, for every cell in that order, (cell, neighbour, relation) for its
    neighbour below (x, y + 1; BELOW), then its neighbour to the right (x + 1, y; RIGHT), where present."""
    present = {(int(x), int(y)) for x, y in cells}
    if not present:
        return [], []
    n = max(max(c) for c in present) + 1
    side = 1 if n <= 1 else 1 << (n - 1).bit_length()
    order = [c for c in (_curve_cell(side, d) for d in range(side * side)) if c in present]
    edges = []
    for x, y in order:
        for nb, rel in (((x, y + 1), BELOW), ((x + 1, y), RIGHT)):
            if nb in present:
                edges.append(((x, y), nb, rel))
    return order, edges


def edge_shifts(tiles_a, tiles_b, relations, overlap: int = DEFAULT_OVERLAP, flipud: bool = False, fliplr: bool = False,
                return_intermediates: bool = False):
    """Register edge e = (tiles_a[e], tiles_b[e], relations[e]) for all e in one ``bh_stitch_edge_shifts`` call.  The tiles are
    same-shape device (Y, X) tensors (uint8, uint16, int16 or float32; only read).  Returns (shifts (n, 2) float64: (y, x) of b
    relative to a, the nominal offset included; confidences (n,) float64), and with ``return_intermediates`` also the lists of
    prepared strips [(a, b)] and of shifted correlations, float32 device tensors.  ValueError for mismatched tiles, an unknown
    relation, or an overlap below 16 or beyond the tile; RuntimeError without a GPU."""
    import torch

    from .device import _TORCH_TO_DT, empty, get_context, resolve_device

    tiles_a, tiles_b, relations = list(tiles_a), list(tiles_b), [int(r) for r in relations]
    n = len(relations)
    if n < 1 or len(tiles_a) != n or len(tiles_b) != n:
        raise ValueError(f"edge_shifts: {len(tiles_a)} / {len(tiles_b)} tiles for {n} relations (n >= 1)")
    first = tiles_a[0]
    if not all(isinstance(t, torch.Tensor) and t.dim() == 2 for t in tiles_a + tiles_b):
        raise ValueError("edge_shifts expects (Y, X) torch tensors")
    if any(t.shape != first.shape or t.dtype != first.dtype or t.device != first.device for t in tiles_a + tiles_b):
        raise ValueError("edge_shifts: the tiles must share one shape, dtype and device")
    if first.dtype not in _TORCH_TO_DT:
        raise ValueError(f"edge_shifts: dtype {first.dtype} is not supported (uint8, uint16, int16, float32)")
    dev = resolve_device(first.device)
    keep = [t.contiguous() for t in tiles_a + tiles_b]
    Y, X = (int(v) for v in first.shape)
    ctx = get_context(dev)
    shifts, conf = np.zeros((n, 2), np.float64), np.zeros(n, np.float64)
    prepared = corr = None
    p_ptrs = c_ptrs = None
    if return_intermediates:
        shape = [(int(overlap), X) if r == BELOW else (Y, int(overlap)) for r in relations]
        prepared = [(empty(s, torch.float32, dev), empty(s, torch.float32, dev)) for s in shape]
        corr = [empty(s, torch.float32, dev) for s in shape]
        p_ptrs = (C.c_void_p * (2 * n))(*[t.data_ptr() for pair in prepared for t in pair])
        c_ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in corr])
    _lib.check(ctx.lib.bh_stitch_edge_shifts(
        ctx.handle, n, (C.c_void_p * n)(*[t.data_ptr() for t in keep[:n]]), (C.c_void_p * n)(*[t.data_ptr() for t in keep[n:]]),
        (C.c_int32 * n)(*relations), _TORCH_TO_DT[first.dtype], Y, X, int(overlap), int(bool(flipud)), int(bool(fliplr)),
        shifts.ctypes.data_as(C.POINTER(C.c_double)), conf.ctypes.data_as(C.POINTER(C.c_double)), p_ptrs, c_ptrs))
    return (shifts, conf, prepared, corr) if return_intermediates else (shifts, conf)


def check_overlap(overlap: int, tile_yx, relations) -> None:
    """ValueError unless 16 <= overlap <= the tile's extent along the strip axis of every relation in use."""
    for rel, extent, axis in ((BELOW, int(tile_yx[0]), "Y"), (RIGHT, int(tile_yx[1]), "X")):
        if rel in relations and not MIN_OVERLAP <= overlap <= extent:
            raise ValueError(f"overlap {overlap}: expected {MIN_OVERLAP} to {extent}, the tile's {axis} extent")


def pairwise_shifts(fov_paths: dict, channel_index: int, z_index: int = 0, overlap: int = DEFAULT_OVERLAP, flipud: bool = False,
                    fliplr: bool = False, device=None) -> list[dict]:
    """Register the neighbouring FOVs of one well.  ``fov_paths``: {FOV name (its last part XXXYYY): position path}.  Plane
    (t = 0, channel_index, z_index) of every FOV with a neighbour is read once (only the chunks holding that plane) and kept on
    the device; all edges go through one ``edge_shifts`` call.  Returns [{"a": name, "b": name, "cell_a": (x, y), "cell_b":
    (x, y), "relation": BELOW | RIGHT, "shift": (y, x), "confidence": float}] in the curve's edge order ([] for a well without
    neighbours) and echoes the confidences the way the reference prints them."""
    import torch

    from .device import resolve_device, upload
    from .io import open_ome_zarr

    names = list(fov_paths)
    cells = parse_grid_names(names)
    by_cell = dict(zip(cells, names))
    _, edges = hilbert_edges(cells)
    if not edges:
        return []
    dev = resolve_device("cuda" if device is None else device)
    planes: dict = {}
    for cell in dict.fromkeys(c for a, b, _ in edges for c in (a, b)):
        plane = open_ome_zarr(fov_paths[by_cell[cell]]).data.read_plane(0, int(channel_index), int(z_index))
        planes[cell] = upload(plane, dev)[0]
    check_overlap(int(overlap), next(iter(planes.values())).shape, {r for _, _, r in edges})
    shifts, conf = edge_shifts([planes[a] for a, _, _ in edges], [planes[b] for _, b, _ in edges], [r for _, _, r in edges],
                               overlap=overlap, flipud=flipud, fliplr=fliplr)
    del planes
    torch.cuda.synchronize(dev)
    click.echo("Confidence scores:")
    out = []
    for (a, b, rel), s, cf in zip(edges, shifts, conf):
        click.echo(f"{[int(v) for v in a]}: {float(cf):.2f}")
        out.append({"a": by_cell[a], "b": by_cell[b], "cell_a": a, "cell_b": b, "relation": rel,
                    "shift": (float(s[0]), float(s[1])), "confidence": float(cf)})
    return out


def optimal_positions(edges, n_tiles: int, guess_i, guess_j) -> np.ndarray:
    """Consistent tile positions (n_tiles, 2) int64 (i = row offset, j = column offset; per-axis minimum 0) from edge shifts.
    ``edges``: [(index of tile a, index of tile b, (shift_i, shift_j))].  Per axis: minimise mean |A x - y| over x, one row
    x_b - x_a = shift per edge and one row pinning tile 0 to 0, rows held in float32 as the reference builds them, by
    scipy.optimize.minimize (L-BFGS-B, tol = gtol = 1e-5, eps = 1e-5, maxiter 1e8, maxfun 1e12) started from the guess; a solve
    that fails returns its start.  The solver is approximate: a consistent graph can come back a pixel off."""
    from scipy.optimize import minimize

    edges = list(edges)
    A = np.zeros((len(edges) + 1, int(n_tiles)), np.float32)
    y = np.zeros((2, len(edges) + 1), np.float32)
    for row, (ia, ib, shift) in enumerate(edges):
        A[row, ia], A[row, ib] = -1, 1
        y[0, row], y[1, row] = shift[0], shift[1]
    A[-1, 0] = 1
    A64 = A.astype(np.float64)

    def solve(rhs, start):
        rhs64, x0 = rhs.astype(np.float64), np.asarray(start, np.float64)
        beta = 1.0 / len(rhs64)
        res = minimize(lambda x: beta * float(np.linalg.norm(A64 @ x - rhs64, ord=1)), x0, method="L-BFGS-B", tol=1e-5,
                       options={"maxiter": int(1e8), "maxfun": int(1e12), "gtol": 1e-5, "eps": 1e-5})
        return res.x if res.success else x0

    pos = np.stack([solve(y[0], guess_i), solve(y[1], guess_j)], axis=1)
    pos = pos - pos.min(axis=0)
    return np.array([[int(v) for v in row] for row in pos], np.int64).reshape(-1, 2)


def refine_translations(well_fov_paths: dict, pixel_zyx: np.ndarray, channel_index: int, z_index: int = 0,
                        overlap: int = DEFAULT_OVERLAP, flipud: bool = False, fliplr: bool = False, device=None):
    """The refinement of one well inside ``estimate-stitch``: ``well_fov_paths`` {FOV name: position path} in the order of the
    rows of ``pixel_zyx`` (the well's stage positions in pixels, zero-based).  Returns (i, j), the optimised row and column
    positions that replace the y and x columns, or None when the well has no pair of neighbours."""
    names = [str(n).split("/")[-1] for n in well_fov_paths]
    shifts = pairwise_shifts(dict(zip(names, well_fov_paths.values())), channel_index, z_index, overlap, flipud, fliplr, device)
    if not shifts:
        return None
    index = {n: k for k, n in enumerate(names)}
    click.echo("optimizing positions")
    pos = optimal_positions([(index[e["a"]], index[e["b"]], e["shift"]) for e in shifts], len(names), pixel_zyx[:, 1], pixel_zyx[:, 2])
    return pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64)


__all__ = ["BELOW", "RIGHT", "DEFAULT_OVERLAP", "check_overlap", "edge_shifts", "hilbert_edges", "optimal_positions",
           "pairwise_shifts", "parse_grid_names", "refine_translations"]
