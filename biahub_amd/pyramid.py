"""Multiscale pyramid levels of OME-Zarr positions (reference: ``biahub pyramid``, biahub/pyramid.py:19-40, which hands the work
to iohub's ``Position.compute_pyramid``).

``downsample_pyramid`` computes levels 1..L-1 of a device volume in ``csrc/pyramid.hip`` (``bh_pyramid_downsample``): each level
halves Z, Y and X (rounding up) and is reduced from the level before it as stored.  ``pyramid`` is the reference's
per-position job; the store side lives in ``io.Position.initialize_pyramid`` / ``compute_pyramid``.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import click

from . import _lib

METHODS = ("stride", "median", "mode", "mean", "min", "max")  # the reference's click.Choice (pyramid.py:55-71)
_METHOD_CODE = {"stride": _lib.DS_STRIDE, "mean": _lib.DS_MEAN, "min": _lib.DS_MIN, "max": _lib.DS_MAX,
                "median": _lib.DS_MEDIAN, "mode": _lib.DS_MODE}
DTYPES = ("uint8", "uint16", "int16", "float32", "float16", "uint32")


def level_shapes(shape, levels: int) -> list[tuple[int, int, int]]:
    """(Z, Y, X) of levels 0..levels-1: every level halves each extent, rounding up (an extent of 1 stays 1)."""
    out = [tuple(int(n) for n in shape)]
    for _ in range(1, levels):
        out.append(tuple((n + 1) // 2 for n in out[-1]))
    return out


def _dtype_name(dtype) -> str:
    """"uint16" for np.dtype("uint16"), np.uint16 and torch.uint16 alike; anything numpy cannot name keeps its own text."""
    text = str(dtype)
    if text.startswith("torch."):
        return text[len("torch."):]
    import numpy as np

    try:
        return np.dtype(dtype).name
    except TypeError:
        return text


def check_args(dtype, levels: int, method: str) -> None:
    """The host-side checks of ``downsample_pyramid``, usable before any read: ValueError naming what is wrong."""
    if method not in _METHOD_CODE:
        raise ValueError(f"pyramid method {method!r}: expected one of {', '.join(METHODS)}")
    if int(levels) < 1:
        raise ValueError(f"levels = {levels}: the pyramid has at least level 0")
    name = _dtype_name(dtype)
    if name not in DTYPES:
        raise ValueError(f"pyramid: dtype {name} is not supported ({', '.join(DTYPES)})")


def downsample_pyramid(vol, levels: int, method: str = "mean") -> list:
    """Levels 1..levels-1 of a device (Z, Y, X) volume, each of the input's dtype, on its device; the input is only read.

    ``levels`` counts level 0 (``levels=4`` returns three tensors).  One launch writes up to three levels from one read of its
    source; deeper pyramids chain launches from the last level written.  Stream-ordered on torch's current stream."""
    import torch

    from .device import empty, get_context, ptr, resolve_device

    check_args(vol.dtype, levels, method)
    if not isinstance(vol, torch.Tensor) or vol.dim() != 3:
        raise ValueError("downsample_pyramid expects a (Z, Y, X) torch tensor")
    dev = resolve_device(vol.device)
    if levels == 1:
        return []
    src = vol.contiguous()
    shapes = level_shapes(src.shape, levels)
    outs = [empty(s, src.dtype, dev) for s in shapes[1:]]
    ctx = get_context(dev)
    arr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    code = {torch.uint8: _lib.DT_U8, torch.uint16: _lib.DT_U16, torch.int16: _lib.DT_I16, torch.float32: _lib.DT_F32,
            torch.float16: _lib.DT_F16, torch.uint32: _lib.DT_U32}[src.dtype]
    Z, Y, X = shapes[0]
    _lib.check(ctx.lib.bh_pyramid_downsample(ctx.handle, ptr(src), code, Z, Y, X, _METHOD_CODE[method], len(outs), arr))
    return outs


def pyramid(fov_path: Path, levels: int, method: str) -> None:
    """Create pyramid levels for one field of view (biahub/pyramid.py:19-40): arrays "1".."levels-1", each reduced from the one
    before it, and the matching ``multiscales`` datasets."""
    from .io import open_ome_zarr

    click.echo(f"Computing pyramid for FOV: {fov_path}")
    with open_ome_zarr(fov_path, mode="r+") as dataset:
        dataset.compute_pyramid(levels=levels, method=method)


__all__ = ["METHODS", "downsample_pyramid", "level_shapes", "pyramid"]
