"""Focus finding by mid-band power on MI355X — waveorder's ``focus.compute_midband_power`` and
``focus_from_transverse_band`` as the reference calls them (``biahub/estimate_stabilization.py:948``, ``track.py:310``,
``estimate_registration.py:114-138``).

waveorder is not a dependency of this package: the definition is restated from waveorder 3.0.5 with the defaults those callers
leave untouched.  Per z-slice of the window: 2-D FFT, ``|F|``, summed over the annulus
``cutoff * lo < |f| < cutoff * hi`` with ``cutoff = 2 NA_det / lambda_ill``; the slice with the largest (``mode="max"``) or
smallest sum is the focus.  ``bh_focus_band_power`` (csrc/focus.hip) reads the window in place from a device volume, transforms
in float32 like the reference and sums in float64.  Windows with an odd extent (no reference caller cuts one) are evaluated on
the host in float64, with a warning.
"""

from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib
from .device import _TORCH_TO_DT, get_context, ptr, resolve_device, upload, volume_pool

MIDBAND_FRACTIONS = (0.125, 0.25)


def band_table(Y: int, X: int, pixel_size: float, NA_det: float, lambda_ill: float, midband_fractions=MIDBAND_FRACTIONS):
    """``(kx_lo int32[Y], kx_hi int32[Y], n_bins)``: per row of the half spectrum the band's columns ``[kx_lo, kx_hi)``, and
    the band's bins in the full plane (``bh_focus_band_table``; host only)."""
    lo, hi, n = (C.c_int32 * int(Y))(), (C.c_int32 * int(Y))(), C.c_int64()
    _lib.check(_lib.load().bh_focus_band_table(int(Y), int(X), float(pixel_size), float(NA_det), float(lambda_ill),
                                               float(midband_fractions[0]), float(midband_fractions[1]), lo, hi, C.byref(n)))
    return np.array(lo, dtype=np.int32), np.array(hi, dtype=np.int32), int(n.value)


def _midband_power_host(zyx, NA_det, lambda_ill, pixel_size, midband_fractions):
    """The definition in float64 numpy, for extents the device call refuses (odd Y or X: no half-bin convention to pin)."""
    v = np.asarray(zyx).astype(np.float64)
    _, Y, X = v.shape

    def freq(n):
        k = np.arange(n)
        return np.where(k < n / 2, k, k - n) / n / pixel_size

    frr = np.sqrt(freq(Y)[:, None] ** 2 + freq(X)[None, :] ** 2)
    cutoff = 2 * NA_det / lambda_ill
    mask = (frr > cutoff * midband_fractions[0]) & (frr < cutoff * midband_fractions[1])
    return np.array([np.abs(np.fft.fft2(s))[mask].sum() for s in v], dtype=np.float64)


def _device_window(zyx, device):
    """A device tensor the kernel can read in place: a supported dtype, unit stride along x, rows and planes that do not
    overlap.  Anything else (and every host array) becomes a contiguous device copy."""
    if isinstance(zyx, torch.Tensor):
        dev = resolve_device(zyx.device if zyx.is_cuda else device)
        t = zyx
        if not t.is_cuda or t.dtype not in _TORCH_TO_DT:
            with volume_pool(dev):
                t = t.to(dev)
                if t.dtype not in _TORCH_TO_DT:
                    t = t.to(torch.float32)
        Z, Y, X = t.shape
        sz, sy, sx = t.stride()
        if not (sx == 1 and sy >= X and (Z == 1 or sz >= (Y - 1) * sy + X)):
            t = t.contiguous()
        return t, _TORCH_TO_DT[t.dtype], dev
    dev = resolve_device(device)
    t, code = upload(np.asarray(zyx), dev)
    return t, code, dev


def midband_power_and_sum(zyx, NA_det, lambda_ill, pixel_size, midband_fractions=MIDBAND_FRACTIONS, device="cuda", max_batch: int = 0):
    """``(power float64[Z], sum float)`` of a 3-D window: a numpy array (uploaded) or a device tensor, which may be a strided
    view of a larger volume (read in place).  ``sum`` is the float64 sum of the window, exact for the integer dtypes."""
    if len(zyx.shape) != 3:
        raise ValueError(f"expected a 3-D (Z, Y, X) array, got shape {tuple(zyx.shape)}")
    Z, Y, X = (int(n) for n in zyx.shape)
    if Y % 2 or X % 2:
        warnings.warn(f"focus: window ({Y}, {X}) has an odd extent; evaluated on the host in float64", stacklevel=2)
        host = zyx.cpu().numpy() if isinstance(zyx, torch.Tensor) else np.asarray(zyx)
        return _midband_power_host(host, NA_det, lambda_ill, pixel_size, midband_fractions), float(host.sum(dtype=np.float64))
    t, code, dev = _device_window(zyx, device)
    sz, sy, _ = t.stride()
    if Z == 1:
        sz = max(sz, (Y - 1) * sy + X)
    ctx = get_context(dev)
    power, total = (C.c_double * Z)(), C.c_double()
    with torch.cuda.device(dev):
        _lib.check(ctx.lib.bh_focus_band_power(ctx.handle, ptr(t), code, Z, Y, X, int(sz), int(sy), float(pixel_size), float(NA_det),
                                               float(lambda_ill), float(midband_fractions[0]), float(midband_fractions[1]),
                                               int(max_batch), power, C.byref(total)))
    return np.array(power, dtype=np.float64), float(total.value)


def compute_midband_power(zyx, NA_det, lambda_ill, pixel_size, midband_fractions=MIDBAND_FRACTIONS, device="cuda"):
    """waveorder ``focus.compute_midband_power`` for a whole stack: float64 ``[Z]``."""
    return midband_power_and_sum(zyx, NA_det, lambda_ill, pixel_size, midband_fractions, device)[0]


def focus_from_power(power, mode: str = "max", threshold_FWHM: float = 0):
    """The slice index from the mid-band powers: first maximum (minimum), or ``None`` when the peak's full width at half
    maximum (``scipy.signal.peak_widths``) is below ``threshold_FWHM``."""
    from scipy.signal import peak_widths

    if mode not in ("max", "min"):
        raise ValueError("mode must be either `min` or `max`")
    power = np.asarray(power, dtype=np.float64)
    peak = int(np.argmax(power) if mode == "max" else np.argmin(power))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # PeakPropertyWarning for a peak at the stack's edge, as in waveorder
        fwhm = peak_widths(power, [peak])[0][0]
    return peak if fwhm >= threshold_FWHM else None


def focus_from_transverse_band(zyx_array, NA_det, lambda_ill, pixel_size, midband_fractions=MIDBAND_FRACTIONS, mode: str = "max",
                               polynomial_fit_order=None, plot_path=None, threshold_FWHM: float = 0,
                               enable_subpixel_precision: bool = False, device="cuda"):
    """waveorder ``focus.focus_from_transverse_band``: the in-focus slice of a ``(Z, Y, X)`` stack, or ``None`` when the
    peak is narrower than ``threshold_FWHM``.  ``Z == 1`` returns 0 without touching the device.  ``polynomial_fit_order``,
    ``plot_path`` and ``enable_subpixel_precision`` are not available (no reference caller sets them)."""
    if polynomial_fit_order is not None or plot_path is not None or enable_subpixel_precision:
        raise NotImplementedError("focus_from_transverse_band: polynomial_fit_order, plot_path and enable_subpixel_precision "
                                  "are not available in biahub_amd")
    if mode not in ("max", "min"):
        raise ValueError("mode must be either `min` or `max`")
    if len(zyx_array.shape) != 3:
        raise ValueError(f"expected a 3-D (Z, Y, X) array, got shape {tuple(zyx_array.shape)}")
    if zyx_array.shape[0] == 1:
        warnings.warn("The dataset only contained a single slice. Returning trivial slice index = 0.", stacklevel=2)
        return 0
    power = compute_midband_power(zyx_array, NA_det, lambda_ill, pixel_size, midband_fractions, device)
    return focus_from_power(power, mode, threshold_FWHM)
