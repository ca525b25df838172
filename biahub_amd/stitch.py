"""Stitch a well's FOVs into one mosaic (reference: ``biahub stitch``, biahub/stitch.py:167-311, and the metadata path of
``biahub estimate-stitch``, biahub/estimate_stitch.py:16-64, 118-213).

Every FOV of a well has one shape (Z, Y, X) and a shift (sz, sy, sx) >= 0; FOV voxel m lands at mosaic voxel m + floor(shift).
The mosaic is ``out[o] = sum_i x_i[o] * w_i[o] / (sum_i w_i[o] + 1e-8)`` over the FOVs covering o, in the order of the shifts,
with w = d ** blending_exponent for d = min(y, Y-1-y, x, X-1-x) > 0 and 0 on a FOV's border: the reference's weights (a 2-D
distance transform of the FOV interior) in closed form.  ``stitch_fovs`` blends device volumes in ``csrc/stitch.hip``
(``bh_stitch_blend``, float32 arithmetic); ``stitch_well`` is the per-well job of the ``stitch`` verb.

Deviations from the reference: negative shifts are refused (ValueError) — ``estimate-stitch`` never writes them,
and the reference truncates them toward zero while its ``get_output_shape`` ignores them; settings with ``affine_transform``
but no ``total_translation`` are refused (the reference reads only ``total_translation``); output channel k is input channel
``channels[k]`` (the reference indexes the output with the input's channel index, which works only for a prefix).
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import click
import numpy as np

from . import _lib

IN_DTYPES = ("uint8", "uint16", "int16", "float32")


def get_output_shape(shifts, tile_shape) -> tuple[int, int, int]:
    """(Z, Y, X) of the mosaic: int(max shift) + tile extent per axis (biahub/stitch.py:167-193).  ``shifts``: a dict
    {FOV name: (sz, sy, sx)} as the reference takes, or a sequence of such triples; ``tile_shape``: (..., Z, Y, X)."""
    vals = list(shifts.values()) if isinstance(shifts, dict) else list(shifts)
    s = np.asarray(vals, np.float64).reshape(-1, 3)
    return tuple(int(s[:, a].max()) + int(tile_shape[a - 3]) for a in range(3))


def placements(shifts_zyx) -> np.ndarray:
    """floor(shift) per FOV and axis, (n, 3) int64.  ValueError for an empty list, a shape other than (n, 3), a non-finite or a
    negative shift."""
    s = np.asarray(list(shifts_zyx), np.float64)
    if s.ndim != 2 or s.shape[1] != 3 or len(s) == 0:
        raise ValueError(f"shifts: expected (n, 3) values (z, y, x), n >= 1, got shape {s.shape}")
    if not np.isfinite(s).all():
        raise ValueError("shifts must be finite")
    if (s < 0).any():
        raise ValueError(f"negative shift {s[(s < 0).any(axis=1)][0].tolist()}: shifts are offsets from the mosaic's corner and must "
                         "be >= 0 (estimate-stitch writes them that way)")
    return np.floor(s).astype(np.int64)


def _i64(values):
    flat = [int(v) for v in np.asarray(values).reshape(-1)]
    return (C.c_int64 * len(flat))(*flat)


def build_tile_lists(offsets_zyx, fov_shape, region_origin=None, region_extent=None) -> dict:
    """The launch tiling of ``bh_stitch_blend`` for this geometry, from the library's own host code (no GPU involved):
    ``tile`` (tile_y, tile_x), ``apron_x``, ``grid`` (nty, ntx), ``tile_off`` (nty * ntx + 1) and ``tile_fov``: CSR lists of the
    FOVs whose (y, x) footprint meets each tile, in FOV order.  Tile (ty, tx) is rows [ty * tile_y, (ty + 1) * tile_y) and columns
    [tx * tile_x - apron_x, (tx + 1) * tile_x) of the region, clipped to it."""
    off = np.asarray(offsets_zyx, np.int64).reshape(-1, 3)
    Z, Y, X = (int(v) for v in fov_shape)
    if region_origin is None:
        region_origin = (0, 0, 0)
    if region_extent is None:
        region_extent = tuple(m - o for m, o in zip(get_output_shape(off, (Z, Y, X)), region_origin))
    lib = _lib.load()
    tiling, n = (C.c_int64 * 5)(), C.c_int64()
    args = (len(off), _i64(off), Z, Y, X, _i64(region_origin), _i64(region_extent), tiling)
    _lib.check(lib.bh_stitch_tile_lists(*args, None, None, 0, C.byref(n)))
    tile_off = np.zeros(int(tiling[3] * tiling[4]) + 1, np.int32)
    tile_fov = np.zeros(max(1, n.value), np.int32)
    _lib.check(lib.bh_stitch_tile_lists(*args, tile_off.ctypes.data_as(C.POINTER(C.c_int32)),
                                        tile_fov.ctypes.data_as(C.POINTER(C.c_int32)), len(tile_fov), C.byref(n)))
    return {"tile": (int(tiling[0]), int(tiling[1])), "apron_x": int(tiling[2]), "grid": (int(tiling[3]), int(tiling[4])),
            "tile_off": tile_off, "tile_fov": tile_fov[: n.value]}


def tile_shape() -> tuple[int, int]:
    """(tile_y, tile_x) of the kernel's launch tiles."""
    return build_tile_lists([(0, 0, 0)], (1, 1, 1))["tile"]


def stitch_fovs(fovs, shifts_zyx, blending_exponent: float = 1.0, out_dtype=None, region=None):
    """Blend same-shape device (Z, Y, X) tensors (uint8, uint16, int16 or float32; only read) into the mosaic, or into the box
    ``region = ((z0, y0, x0), (ez, ey, ex))`` of it (voxels of a region that no given FOV covers are 0); returns a float32
    (default) or float16 device tensor.  float32 arithmetic per voxel in list order; a voxel's bits do not depend
    on the region.  Stream-ordered on torch's current stream.  ValueError for negative shifts, mismatched shapes or dtypes, a negative or NaN exponent; RuntimeError without a GPU."""
    import torch

    from .device import _TORCH_TO_DT, empty, get_context, resolve_device

    fovs = list(fovs)
    off = placements(shifts_zyx)
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    if len(fovs) != len(off):
        raise ValueError(f"{len(fovs)} FOVs for {len(off)} shifts")
    if not all(isinstance(f, torch.Tensor) and f.dim() == 3 for f in fovs):
        raise ValueError("stitch_fovs expects a list of (Z, Y, X) torch tensors")
    if any(f.shape != fovs[0].shape or f.dtype != fovs[0].dtype or f.device != fovs[0].device for f in fovs):
        raise ValueError("stitch_fovs: the FOVs must share one shape, dtype and device")
    if fovs[0].dtype not in _TORCH_TO_DT:
        raise ValueError(f"stitch_fovs: dtype {fovs[0].dtype} is not supported ({', '.join(IN_DTYPES)})")
    if out_dtype not in (torch.float32, torch.float16):
        raise ValueError(f"stitch_fovs: out_dtype {out_dtype} (float32 or float16)")
    if not float(blending_exponent) >= 0:
        raise ValueError(f"blending_exponent {blending_exponent} (>= 0)")
    dev = resolve_device(fovs[0].device)
    fovs = [f.contiguous() for f in fovs]
    Z, Y, X = (int(v) for v in fovs[0].shape)
    mosaic = get_output_shape(off, (Z, Y, X))
    origin, extent = ((0, 0, 0), mosaic) if region is None else (tuple(int(v) for v in region[0]), tuple(int(v) for v in region[1]))
    if any(o < 0 or e < 1 for o, e in zip(origin, extent)):  # beyond the given FOVs' mosaic a region is simply uncovered: zeros
        raise ValueError(f"region {origin} + {extent}: the origin must be >= 0 and the extent >= 1")
    out = empty(extent, out_dtype, dev)
    ctx = get_context(dev)
    ptrs = (C.c_void_p * len(fovs))(*[f.data_ptr() for f in fovs])
    _lib.check(ctx.lib.bh_stitch_blend(ctx.handle, len(fovs), ptrs, _i64(off), _TORCH_TO_DT[fovs[0].dtype], Z, Y, X,
                                       float(blending_exponent), _i64(origin), _i64(extent),
                                       _lib.DT_F16 if out_dtype == torch.float16 else _lib.DT_F32, C.c_void_p(out.data_ptr())))
    return out


def plan_bands(offsets_zyx, fov_shape, fov_bytes: int, out_itemsize: int, max_device_bytes) -> list[tuple[int, int]]:
    """[(y0, y1)] bands of the mosaic, in y order, such that the FOVs meeting a band plus the band itself fit ``max_device_bytes``
    (None: one band).  Equal heights, as few bands as fit.  MemoryError when even one-row bands do not fit."""
    off = np.asarray(offsets_zyx, np.int64).reshape(-1, 3)
    Z, Y, X = (int(v) for v in fov_shape)
    mz, my, mx = get_output_shape(off, (Z, Y, X))

    def bands(n):
        edges = [round(i * my / n) for i in range(n + 1)]
        return [(a, b) for a, b in zip(edges[:-1], edges[1:]) if b > a]

    def fits(bs):
        return all(int(((off[:, 1] < b) & (off[:, 1] + Y > a)).sum()) * fov_bytes + mz * (b - a) * mx * out_itemsize
                   <= max_device_bytes for a, b in bs)

    if max_device_bytes is None or len(off) * fov_bytes + mz * my * mx * out_itemsize <= max_device_bytes:
        return [(0, my)]
    n = 2
    while True:
        bs = bands(min(n, my))
        if fits(bs):
            return bs
        if n >= my:
            raise MemoryError(f"max_device_bytes = {max_device_bytes}: the FOVs meeting one mosaic row do not fit")
        n = n + 1 if n < 16 else int(n * 1.5)


def stitch_well(fov_paths, shifts_zyx, output_position_path, channel_indices=None, blending_exponent: float = 1.0,
                max_device_bytes=None, device=None, verbose: bool = False) -> dict:
    """The per-well job of ``stitch``: for every (t, k), read channel ``channel_indices[k]`` of the well's FOVs
    (``read_volume_device``), blend them, and write the float16 (the output array's dtype) mosaic as volume (t, k) of the
    output position, which exists with shape (T, len(channel_indices), *mosaic).

    ``max_device_bytes``: when all FOV volumes plus the mosaic exceed it, the mosaic is computed in y bands; only the FOVs that
    meet a band are resident, each band is one region of ``bh_stitch_blend``, the bands are gathered on the host and written
    there.  A banded run equals the single-launch run bit for bit.  Returns {"bands": n, "mosaic": (Z, Y, X)}."""
    import torch

    from .device import resolve_device, to_host
    from .io import _torch_dtype, open_ome_zarr

    dev = resolve_device("cuda" if device is None else device)
    off = placements(shifts_zyx)
    arrays = [open_ome_zarr(p).data for p in fov_paths]
    if len(arrays) != len(off):
        raise ValueError(f"{len(arrays)} FOVs for {len(off)} shifts")
    T, Cin, Z, Y, X = arrays[0].shape
    if any(a.shape != arrays[0].shape or a.dtype != arrays[0].dtype for a in arrays):
        raise ValueError("stitch_well: the FOVs of a well must share one shape and dtype")
    channel_indices = list(range(Cin)) if channel_indices is None else [int(c) for c in channel_indices]
    out_arr = open_ome_zarr(output_position_path).data
    mosaic = get_output_shape(off, (Z, Y, X))
    if tuple(out_arr.shape) != (T, len(channel_indices), *mosaic):
        raise ValueError(f"{output_position_path}: shape {out_arr.shape}, expected {(T, len(channel_indices), *mosaic)}")
    out_dtype = _torch_dtype(out_arr.dtype)
    if out_dtype not in (torch.float16, torch.float32):
        raise ValueError(f"{output_position_path}: dtype {out_arr.dtype} (float16 or float32)")
    bands = plan_bands(off, (Z, Y, X), Z * Y * X * arrays[0].dtype.itemsize, out_arr.dtype.itemsize, max_device_bytes)

    def load(i, t, c):
        v = arrays[i].read_volume_device(t, c, dev)
        return v if v.dtype in (torch.uint8, torch.uint16, torch.int16, torch.float32) else v.to(torch.float32)

    for t in range(T):
        for k, c in enumerate(channel_indices):
            if verbose:
                click.echo(f"\tStitching t={t}, channel {c}: {len(arrays)} FOVs -> {mosaic}, {len(bands)} band(s)")
            if len(bands) == 1:
                vols = [load(i, t, c) for i in range(len(arrays))]
                out_arr.write_volume_device(t, k, stitch_fovs(vols, off, blending_exponent, out_dtype))
                del vols
                continue
            host = np.zeros(mosaic, out_arr.dtype)
            resident: dict = {}
            for y0, y1 in bands:
                need = [i for i in range(len(arrays)) if off[i, 1] < y1 and off[i, 1] + Y > y0]
                for i in [i for i in resident if i not in need]:
                    del resident[i]
                if need:  # a band no FOV meets stays 0
                    for i in need:
                        if i not in resident:
                            resident[i] = load(i, t, c)
                    # every FOV keeps its mosaic offset and the region picks the band: the FOVs left out cover none of it
                    band = stitch_fovs([resident[i] for i in need], off[need], blending_exponent, out_dtype,
                                       region=((0, y0, 0), (mosaic[0], y1 - y0, mosaic[2])))
                    host[:, y0:y1] = to_host(band)
                    del band
            out_arr.write_volume(t, k, host)
    return {"bands": len(bands), "mosaic": mosaic}


def extract_stage_position(plate_zattrs: dict, position_name: str) -> tuple[float, float, float]:
    """(z, y, x) stage position in micrometres of the entry of ``Summary.StagePositions`` labelled ``position_name``
    (biahub/estimate_stitch.py:16-64): either ``DevicePositions`` (the XY stage gives x, y; every other device adds to z) or
    direct stage keys (``DefaultXYStage`` / ``DefaultZStage`` name the keys).  (0, 0, 0) when no entry has the label."""
    zpos, ypos, xpos = 0, 0, 0
    for sp in plate_zattrs["Summary"]["StagePositions"]:
        if sp["Label"] != position_name:
            continue
        xpos, ypos, zpos = 0, 0, 0
        if "DevicePositions" in sp:
            xy = sp.get("DefaultXYStage", "")
            for dev in sp["DevicePositions"]:
                if dev["Device"] == xy and xy:
                    xpos, ypos = dev["Position_um"]
                elif dev["Device"] != xy:
                    zpos += dev["Position_um"][0]
        else:
            if "DefaultXYStage" in sp and sp["DefaultXYStage"] in sp:
                xpos, ypos = sp[sp["DefaultXYStage"]]
            if "DefaultZStage" in sp and sp["DefaultZStage"] in sp:
                zpos = sp[sp["DefaultZStage"]]
    return zpos, ypos, xpos


def estimate_stitch_translations(stage_zyx: dict, scale_zyx, fliplr=False, flipud=False, flipxy=False, refine=None) -> dict:
    """{FOV name "row/col/fov": [z, y, x] in pixels} from stage positions in micrometres (biahub/estimate_stitch.py:135-206): per
    well, zero-based, divided by the scale, flipped, shifted to non-negative, rounded to 2 decimals.  ``refine(well, names,
    pixel_zyx)``, when given, is called per well before the flips and returns None or (i, j): positions that replace the y and x
    columns (``estimate_stitch.refine_translations``)."""
    wells: dict = {}
    for key, value in stage_zyx.items():
        wells.setdefault("/".join(key.split("/")[:2]), {})[key] = value
    out = {}
    for well_name, well in wells.items():
        a = np.array(list(well.values()), np.float64)
        a -= a.min(axis=0)
        a /= np.asarray(scale_zyx, np.float64)
        refined = refine(well_name, list(well), a) if refine is not None else None
        if refined is not None:
            a[:, 1], a[:, 2] = refined
        if fliplr:
            a[:, 2] *= -1
        if flipud:
            a[:, 1] *= -1
        if flipxy:
            a[:, [1, 2]] = a[:, [2, 1]]
        a -= np.minimum(a.min(axis=0), 0)
        for i, name in enumerate(well):
            out[name] = [float(v) for v in np.round(a[i], 2)]
    return out


__all__ = ["build_tile_lists", "estimate_stitch_translations", "extract_stage_position", "get_output_shape", "placements",
           "plan_bands", "stitch_fovs", "stitch_well", "tile_shape"]
