"""Bleaching curves on MI355X — mirror of ``biahub/estimate_bleaching.py``: the mean and standard deviation of every (t, c)
volume of a position, an exponential fit per channel, one plot per position.

The reference computes ``np.mean`` and ``np.std`` of each volume through dask on host cores.  Here a volume comes into HBM
through the store's device read path and ``bh_volume_moments`` (csrc/moments.hip) reduces it in one pass to one
record per z-slice: NaN and zero counts, min, max, and two sums — exact integers for uint8 / uint16 / int16, float64 sums of
``x - centre`` and ``(x - centre)^2`` for float32.  ``mean_std`` turns the records into the two numbers: for the integer dtypes
the correctly rounded value of the exact rational, for float32 a two-pass variance in float64.

``device="cpu"`` (or ``BH_BLEACHING_DEVICE=cpu`` for the command line) computes the same records with numpy on the host: what a
box without a GPU runs.  It is a choice of the caller, never a fall-back: with ``device="cuda"`` and no GPU the call raises.
"""

from __future__ import annotations

import ctypes as C
import math
import os
import warnings
from pathlib import Path

import numpy as np

MSECS_PER_MINUTE = 60000

# bh_moments of include/bhcore.h, member for member
MOMENTS_DTYPE = np.dtype([("n_nan", np.uint64), ("n_zero", np.uint64), ("min", np.float64), ("max", np.float64),
                          ("isum", np.int64), ("isumsq", np.uint64), ("fsum", np.float64), ("fsumsq", np.float64)])
SUPPORTED_DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.int16), np.dtype(np.float32))
_EXACT_IN_FLOAT32 = (np.dtype(np.bool_), np.dtype(np.float16))
MAX_VOXELS = 1 << 32  # per bh_volume_moments call: the exact sum of squares of 16-bit data stays below 2^64


def _is_cpu(device) -> bool:
    return str(device).startswith("cpu")


def moments_plan(Y: int, X: int, block_rows: int = 0):
    """``(rows, blocks, wg_per_cu)`` of ``bh_volume_moments_plan``: rows per item, items per slice, and the cap of the reduction's
    grid in workgroups per compute unit (host only)."""
    from . import _lib

    rows, blocks, cap = C.c_int64(), C.c_int64(), C.c_int()
    _lib.check(_lib.load().bh_volume_moments_plan(int(Y), int(X), int(block_rows), C.byref(rows), C.byref(blocks), C.byref(cap)))
    return int(rows.value), int(blocks.value), int(cap.value)


def _moments_host(v: np.ndarray, centre: float) -> np.ndarray:
    """The records from numpy: int64 / Python-int sums for the integer dtypes, plain float64 numpy sums for float32."""
    Z = v.shape[0]
    out = np.zeros(Z, dtype=MOMENTS_DTYPE)
    flat = v.reshape(Z, -1)
    for z in range(Z):
        s = flat[z]
        r = out[z]
        r["n_zero"] = int(np.count_nonzero(s == 0))
        if v.dtype.kind == "f":
            nan = np.isnan(s)
            r["n_nan"] = int(np.count_nonzero(nan))
            ok = s[~nan]
            r["min"], r["max"] = (float(ok.min()), float(ok.max())) if ok.size else (np.inf, -np.inf)
            d = s.astype(np.float64) - np.float64(centre)
            r["fsum"], r["fsumsq"] = np.sum(d), np.sum(d * d)
        else:
            r["min"], r["max"] = float(s.min()), float(s.max())
            w = s.astype(np.int64)
            r["isum"] = int(np.sum(w, dtype=np.int64))
            r["isumsq"] = int(np.sum((w * w).astype(np.uint64), dtype=np.uint64))
    return out


def _host_volume(zyx) -> np.ndarray:
    """A host array in a dtype the reduction reads: bool and float16 widen to float32 exactly, anything else is refused."""
    v = np.asarray(zyx)
    if v.dtype in _EXACT_IN_FLOAT32:
        v = v.astype(np.float32)
    if v.dtype not in SUPPORTED_DTYPES:
        raise ValueError(f"volume_moments reads uint8, uint16, int16 and float32 volumes; {v.dtype} is not exactly representable in float32")
    return v


def volume_moments(zyx, device="cuda", centre: float = 0.0, block_rows: int = 0) -> np.ndarray:
    """Per-slice records (``MOMENTS_DTYPE``, one per z) of a 3-D volume: a numpy array (uploaded) or a device tensor, which may be
    a strided view of a larger volume (read in place when x has unit stride and rows and planes do not overlap).  ``centre``
    matters for float32 only.  ``block_rows`` > 0 fixes the rows per item of the reduction (``moments_plan``).  bool and float16
    widen to float32 (exact); any other dtype outside uint8 / uint16 / int16 / float32 raises ``ValueError``."""
    import torch

    if len(zyx.shape) != 3:
        raise ValueError(f"expected a 3-D (Z, Y, X) array, got shape {tuple(zyx.shape)}")
    Z, Y, X = (int(n) for n in zyx.shape)
    if min(Z, Y, X) < 1:
        raise ValueError(f"empty volume {(Z, Y, X)}")
    if _is_cpu(device) and not (isinstance(zyx, torch.Tensor) and zyx.is_cuda):
        return _moments_host(_host_volume(zyx.numpy() if isinstance(zyx, torch.Tensor) else zyx), centre)
    from . import _lib
    from .device import _TORCH_TO_DT, get_context, ptr
    from .focus import _device_window

    if isinstance(zyx, torch.Tensor):
        if zyx.dtype in (torch.bool, torch.float16):
            zyx = zyx.to(torch.float32)
        if zyx.dtype not in _TORCH_TO_DT:
            raise ValueError(f"volume_moments reads uint8, uint16, int16 and float32 volumes; {zyx.dtype} is not exactly representable in float32")
    else:
        zyx = _host_volume(zyx)
    if Z * Y * X > MAX_VOXELS:  # split along z: the records are per slice
        step = max(1, MAX_VOXELS // (Y * X))
        return np.concatenate([volume_moments(zyx[z0:z0 + step], device, centre, block_rows) for z0 in range(0, Z, step)])
    t, code, dev = _device_window(zyx, device)
    sz, sy, _ = t.stride()
    if Y == 1:  # torch leaves the stride of an axis of length 1 arbitrary
        sy = max(sy, X)
    if Z == 1:
        sz = max(sz, (Y - 1) * sy + X)
    ctx = get_context(dev)
    out = np.zeros(Z, dtype=MOMENTS_DTYPE)
    with torch.cuda.device(dev):
        _lib.check(ctx.lib.bh_volume_moments(ctx.handle, ptr(t), code, Z, Y, X, int(sz), int(sy), float(centre), int(block_rows),
                                             out.ctypes.data_as(C.c_void_p)))
    return out


def mean_std_from_moments(records_of_centre, n_voxels: int, is_float: bool):
    """``(mean, std)`` from the records.  Integer dtypes: ``records_of_centre`` is the records; float32: a callable ``centre ->
    records`` (called with 0, then with the mean)."""
    N = int(n_voxels)
    if not is_float:
        rec = records_of_centre
        S = sum(int(v) for v in rec["isum"])
        Q = sum(int(v) for v in rec["isumsq"])
        return S / N, math.sqrt((N * Q - S * S) / (N * N))  # int / int: correctly rounded, each once
    total = 0.0
    for v in records_of_centre(0.0)["fsum"]:  # z order
        total += float(v)
    mean = total / N
    if not math.isfinite(mean):  # a NaN or an infinity in the volume: np.mean and np.std give the same
        return mean, float("nan")
    sd, sq = 0.0, 0.0
    for r in records_of_centre(mean):
        sd += float(r["fsum"])
        sq += float(r["fsumsq"])
    var = (sq - sd * sd / N) / N
    return mean, math.sqrt(max(var, 0.0))


def mean_std(zyx, device="cuda"):
    """``(np.mean(v), np.std(v))`` (ddof 0) of a volume as Python floats.  Integer dtypes: one reduction, exact sums, the mean
    ``S / N`` and the variance ``(N Q - S^2) / N^2`` each rounded once from the exact rational.  float32: one reduction about 0
    for the mean, a second about the mean for ``var = (sum d^2 - (sum d)^2 / N) / N``, everything in float64, the slices added
    in z order."""
    import torch

    if not isinstance(zyx, torch.Tensor):
        zyx = _host_volume(zyx)
    N = int(np.prod(zyx.shape))
    if isinstance(zyx, torch.Tensor) and zyx.is_cuda and not _is_cpu(device):
        from .focus import _device_window

        zyx = _device_window(zyx, device)[0]  # one conversion for both passes
        is_float = zyx.dtype.is_floating_point
    elif isinstance(zyx, torch.Tensor):
        is_float = zyx.dtype.is_floating_point or zyx.dtype == torch.bool
    else:
        is_float = zyx.dtype.kind == "f"
        if not _is_cpu(device):
            from .device import resolve_device, upload

            zyx = upload(zyx, resolve_device(device))[0]  # one upload for both passes
    if is_float:
        return mean_std_from_moments(lambda c: volume_moments(zyx, device, centre=c), N, True)
    return mean_std_from_moments(volume_moments(zyx, device), N, False)


def bleaching_curves(position, device="cuda"):
    """``(means[T, C], stds[T, C])`` in float64 of array "0" of an open position.  The next volume is read on an I/O thread
    (``stage_volume``: files and entropy decoding) while this thread runs the device half (``upload_staged``: lz4 / zstd blocks,
    un-shuffle) and the reduction; a layout without a device read path is read on the host and uploaded."""
    from concurrent.futures import ThreadPoolExecutor

    arr = position["0"]
    T, Cn = (int(n) for n in arr.shape[:2])
    if np.dtype(arr.dtype) not in SUPPORTED_DTYPES + _EXACT_IN_FLOAT32:
        raise ValueError(f"estimate-bleaching reads uint8, uint16, int16 and float32 stores; {np.dtype(arr.dtype)} is not exactly "
                         "representable in float32")
    cpu = _is_cpu(device)
    if not cpu:
        from .device import resolve_device

        dev = resolve_device(device)
    units = [(t, c) for t in range(T) for c in range(Cn)]

    def load(u):
        staged = None if cpu else arr.stage_volume(*u)
        return ("staged", staged) if staged is not None else ("host", arr.read_volume(*u))

    means, stds = np.zeros((T, Cn), dtype=np.float64), np.zeros((T, Cn), dtype=np.float64)
    with ThreadPoolExecutor(1, thread_name_prefix="bh-bleach-r") as reader:
        nxt = reader.submit(load, units[0]) if units else None
        for i, (t, c) in enumerate(units):
            kind, vol = nxt.result()
            nxt = reader.submit(load, units[i + 1]) if i + 1 < len(units) else None
            if kind == "staged":
                vol = arr.upload_staged(vol, dev)
            means[t, c], stds[t, c] = mean_std(vol, device)
            del vol
    return means, stds


def _model(x, a, b, c):
    return a * np.exp(-x / b) + c


def fit_bleaching(times, means, stds):
    """``a exp(-t / b) + c`` fitted to one channel exactly as the reference does (estimate_bleaching.py:60-71): ``curve_fit``
    with ``sigma = stds``, ``p0 = (max - min, 100, min)``, ``maxfev = 5000``.  Returns ``(popt, None)``, or ``(None, exception)``
    when the fit failed — any exception, as in the reference, which then plots the points only.

    One more failure than the reference has: weighted residuals that are not finite at the result (a standard deviation of 0,
    as for a constant volume, or a NaN mean).  MINPACK then stops at once and hands ``p0`` back without an error, and the
    reference labels the channel with ``p0``'s "100 minutes"; here that is "fit failed"."""
    from scipy.optimize import curve_fit

    xdata, ydata, yerr = np.asarray(times), np.asarray(means), np.asarray(stds)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # OptimizeWarning: covariance could not be estimated (the reference shows it)
            popt, _ = curve_fit(_model, xdata, ydata, sigma=yerr, p0=(np.max(ydata) - np.min(ydata), 100, np.min(ydata)), maxfev=5000)
            if not np.all(np.isfinite((_model(xdata, *popt) - ydata) / yerr)):
                raise ValueError("Residuals are not finite: a standard deviation is 0, or a mean is not finite")
        return popt, None
    except Exception as e:  # noqa: BLE001 - "fit failed" is a result
        return None, e


def plot_bleaching_curves(times, means, stds, channel_names, output_file, title="", channel_colors=None, echo=print):
    """The reference's figure (estimate_bleaching.py:48-102) from the statistics: 4 x 4 in, per channel the fitted curve at
    alpha 0.5 and the means as markers, legend ``"<channel> - <b:0.0f> minutes"``, no top / right spines, saved with
    ``bbox_inches="tight"`` (SVG by the file name).  The reference's second argument is the raw (T, C, Z, Y, X) data, reduced
    inside; here the reduction has run on the GPU (``bleaching_curves``) and its results come in.  ``channel_colors``: one
    matplotlib colour or ``None`` (the colour cycle) per channel.  Returns the fits: one ``(popt or None)`` per channel."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    means, stds = np.asarray(means, dtype=np.float64), np.asarray(stds, dtype=np.float64)
    fig = Figure(figsize=(4, 4))
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    fits = []
    for ci, name in enumerate(channel_names):
        color = channel_colors[ci] if channel_colors and channel_colors[ci] is not None else f"C{ci % 10}"
        xdata, ydata = np.asarray(times), means[:, ci]
        popt, err = fit_bleaching(xdata, ydata, stds[:, ci])
        if popt is not None:
            xx = np.linspace(0, np.max(xdata), 100)
            ax.plot(xx, _model(xx, *popt), color=color, alpha=0.5)
            label = name + f" - {popt[1]:0.0f} minutes"
            echo("Curve fit successful!")
            echo(label)
        else:
            echo(str(err))
            label = name
            echo("Curve fit failed!")
        fits.append(popt)
        ax.plot(xdata, ydata, label=label, marker="o", markeredgewidth=0, linewidth=0, color=color)
    ax.set_title(title, {"fontsize": 8})
    ax.set_xlabel("Time (minutes)")
    ax.set_ylabel("Mean Intensity (AU)")
    ax.legend(frameon=False, markerfirst=False)
    ax.spines["right"].set_visible(False)
    ax.spines["top"].set_visible(False)
    fig.savefig(output_file, bbox_inches="tight")
    return fits


def plate_zattrs(position_path):
    """Attributes of the plate three levels above a position, or ``None`` with the reference's warning when there is none."""
    from .io import _read_group_attrs

    try:
        return _read_group_attrs(Path(*Path(position_path).parts[:-3]))
    except Exception as e:  # noqa: BLE001 - the reference prints and warns (estimate_bleaching.py:114-123)
        print(e)
        warnings.warn("WARNING: this position has no plate metadata, so the time metadata will be missing.", stacklevel=2)
        return None


def time_axis(T: int, zattrs, well_name: str = "") -> np.ndarray:
    """Acquisition times in minutes: ``np.arange(T) * float(dt)`` with ``dt = np.float32(Summary.Interval_ms / 60000)`` of the
    plate's attributes, or ``dt = 1`` with the reference's warning when the plate or the key is missing.

    Deliberate deviation: the reference's ``np.arange(0, T * dt, step=dt)`` (estimate_bleaching.py:142) can return T + 1 samples
    when ``T * dt / dt`` rounds up, and then fails in ``ax.plot`` against T means; this axis always has T samples."""
    try:
        dt = np.float32(zattrs["Summary"]["Interval_ms"] / MSECS_PER_MINUTE)
    except Exception as e:  # noqa: BLE001 - as the reference (estimate_bleaching.py:135-140)
        print(e)
        warnings.warn(f"WARNING: missing time metadata for p={well_name}", stacklevel=2)
        dt = 1
    return np.arange(int(T)) * float(dt)


def _channel_colors(position, n):
    chans = position.zattrs.get("omero", {}).get("channels", [])
    out = []
    for i in range(n):
        col = chans[i].get("color") if i < len(chans) and isinstance(chans[i], dict) else None
        try:
            import matplotlib.colors

            out.append(matplotlib.colors.to_rgb("#" + str(col)) if col else None)
        except ValueError:
            out.append(None)
    if len({c for c in out if c is not None}) < len([c for c in out if c is not None]):
        return [None] * n  # every channel the same stored colour (this package writes FFFFFF): tell them apart by the cycle
    return out


def estimate_bleaching_position(position_path, output_dirpath, zattrs=None, device=None, echo=print) -> float:
    """One position: the curves, ``<out>/<row>/<col>/<fov>/bleaching.svg`` as the reference writes it, and next to it
    ``bleaching.csv`` (t, time_minutes, channel, mean, std) and ``bleaching_fit.csv`` (channel, a, lifetime_minutes, c, fit_ok),
    floats with ``repr`` precision.  ``device`` None: ``BH_BLEACHING_DEVICE`` or "cuda".  Returns the voxels read."""
    from .io import open_ome_zarr

    device = device or os.environ.get("BH_BLEACHING_DEVICE", "cuda")
    position_path = Path(position_path)
    well_name = "/".join(position_path.parts[-3:])
    echo(f"Generating bleaching curves for position {well_name}")
    with open_ome_zarr(position_path) as reader:
        names = list(reader.channel_names)
        shape = tuple(int(n) for n in reader["0"].shape)
        means, stds = bleaching_curves(reader, device)
        colors = _channel_colors(reader, shape[1])
    names = names if len(names) == shape[1] else [f"channel_{i}" for i in range(shape[1])]
    times = time_axis(shape[0], zattrs, well_name)
    out = Path(output_dirpath).joinpath(*position_path.parts[-3:])
    out.mkdir(parents=True, exist_ok=True)
    title = str(position_path) + f" - position = {well_name}"
    fits = plot_bleaching_curves(times, means, stds, names, out / "bleaching.svg", title, colors, echo=echo)
    import csv

    with open(out / "bleaching.csv", "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["t", "time_minutes", "channel", "mean", "std"])
        for t in range(shape[0]):
            for c, name in enumerate(names):
                w.writerow([t, repr(float(times[t])), name, repr(float(means[t, c])), repr(float(stds[t, c]))])
    with open(out / "bleaching_fit.csv", "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["channel", "a", "lifetime_minutes", "c", "fit_ok"])
        for name, popt in zip(names, fits):
            w.writerow([name, "nan", "nan", "nan", 0] if popt is None else [name, *(repr(float(p)) for p in popt), 1])
    return float(np.prod(shape))
