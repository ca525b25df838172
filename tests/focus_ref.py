"""Float64 numpy restatement of waveorder 3.0.5 ``focus.compute_midband_power`` / ``focus_from_transverse_band`` with the
defaults the reference's callers leave untouched (estimate_stabilization.py:948, track.py:310, estimate_registration.py:114-138),
and the generator of the test windows.  Test infrastructure: what csrc/focus.hip and biahub_amd/focus.py are held to
(DESIGN.md §3.8, §7 item 6).

For a window v[Z, Y, X], pixel size p, NA_det, lambda_ill and midband fractions (lo, hi):
    fy = s_y / Y / p, fx = s_x / X / p   with signed FFT indices s (N/2 -> -N/2),   frr = sqrt(fy^2 + fx^2)
    cutoff = 2 NA_det / lambda_ill,      mask = (frr > cutoff lo) & (frr < cutoff hi)      (float64, strict)
    power[z] = sum over the mask of |fft2(v[z])|
"""

from __future__ import annotations

import numpy as np

NA_DET, LAMBDA_ILL = 1.35, 0.5
FRACTIONS = (0.125, 0.25)
NP_DTYPES = {"uint8": np.uint8, "uint16": np.uint16, "int16": np.int16, "float32": np.float32}


def signed_index(n: int) -> np.ndarray:
    k = np.arange(n)
    return np.where(k < n / 2, k, k - n).astype(np.float64)


def band_radius(Y: int, X: int, pixel_size: float) -> np.ndarray:
    fy = signed_index(Y) / Y / pixel_size
    fx = signed_index(X) / X / pixel_size
    return np.sqrt(fy[:, None] ** 2 + fx[None, :] ** 2)


def band_edges(NA_det: float = NA_DET, lambda_ill: float = LAMBDA_ILL, fractions=FRACTIONS) -> tuple[float, float]:
    cutoff = 2 * NA_det / lambda_ill
    return cutoff * fractions[0], cutoff * fractions[1]


def band_mask(Y: int, X: int, pixel_size: float, NA_det: float = NA_DET, lambda_ill: float = LAMBDA_ILL, fractions=FRACTIONS) -> np.ndarray:
    frr = band_radius(Y, X, pixel_size)
    lo, hi = band_edges(NA_det, lambda_ill, fractions)
    return (frr > lo) & (frr < hi)


def midband_power(v, pixel_size: float, NA_det: float = NA_DET, lambda_ill: float = LAMBDA_ILL, fractions=FRACTIONS) -> np.ndarray:
    """float64 [Z]."""
    v = np.asarray(v).astype(np.float64)
    mask = band_mask(v.shape[1], v.shape[2], pixel_size, NA_det, lambda_ill, fractions)
    return np.array([np.abs(np.fft.fft2(s))[mask].sum() for s in v], dtype=np.float64)


def midband_power_f32(v, pixel_size: float, NA_det: float = NA_DET, lambda_ill: float = LAMBDA_ILL, fractions=FRACTIONS, workers: int = 1) -> np.ndarray:
    """The same formula in float32 / complex64 with scipy.fft (the stand-in for the reference's complex64 torch pipeline)."""
    import scipy.fft

    v = np.asarray(v).astype(np.float32)
    mask = band_mask(v.shape[1], v.shape[2], pixel_size, NA_det, lambda_ill, fractions)
    spec = scipy.fft.fft2(v, axes=(-2, -1), workers=workers)
    assert spec.dtype == np.complex64
    return np.abs(spec)[:, mask].sum(axis=1, dtype=np.float32)


def focus_index(power, mode: str = "max") -> int:
    return int(np.argmax(power) if mode == "max" else np.argmin(power))


def make_window(shape, dtype: str, z0: int, seed: int) -> np.ndarray:
    """A random texture in focus at slice z0: Gaussian-blurred (wrap) with sigma = 0.6 |z - z0|, plus offset 100, plus noise of
    sigma 2, cast to ``dtype`` (rounded for the integer types; the values stay inside uint8)."""
    from scipy.ndimage import gaussian_filter

    Z, Y, X = shape
    rng = np.random.default_rng(seed)
    texture = rng.random((Y, X)) * 100.0
    out = np.empty(shape, dtype=np.float64)
    for z in range(Z):
        s = 0.6 * abs(z - z0)
        out[z] = (gaussian_filter(texture, s, mode="wrap") if s > 0 else texture) + 100.0 + rng.normal(0.0, 2.0, (Y, X))
    dt = NP_DTYPES[dtype]
    if np.issubdtype(dt, np.integer):
        info = np.iinfo(dt)
        out = np.clip(np.rint(out), info.min, info.max)
    return out.astype(dt)


def case_window(case: dict) -> np.ndarray:
    return make_window(tuple(case["shape"]), case["dtype"], case["z0"], case["seed"])
