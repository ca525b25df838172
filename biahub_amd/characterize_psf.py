"""Bead detection and extraction — mirror of the on-path parts of ``biahub/characterize_psf.py``.

``detect_peaks`` (characterize_psf.py:562-711) is the reference's torch approximation of ``peak_local_max``: box blur,
blocked max-pool with indices, then top-k / threshold / non-maximum suppression on at most ``max_num_peaks`` candidates.
The two pooling passes over the volume are one fused HIP kernel (``bh_block_peaks``, bit-identical to torch's CPU
pooling); the candidate filtering is the reference's logic on a few thousand points, here in NumPy.
``extract_beads`` (:173-190 + vendor BeadExtractor) recentres each point on the Gaussian-smoothed maximum of its crop
(``bh_patch_peaks``) and returns the crops.

``analyze_psf`` (:193-272) is the ``characterize-psf`` half: the reference's per-bead loop of three
``scipy.optimize.curve_fit`` calls is one batched float64 Levenberg-Marquardt solve on the device (``bh_psf_fit``,
csrc/psffit.hip) that reads the patches in place from the uploaded volume; the data-frame post-processing,
the 1-D peak widths (scipy on <= 2000 short profiles), the noise level and the report follow the reference.
"""

from __future__ import annotations

import ctypes as C
import datetime
import pickle
from pathlib import Path

import numpy as np
import torch

from . import _lib
from .device import as_device_volume, get_context, ptr, resolve_device


def block_peaks(vol: torch.Tensor, blur_kernel_size: int, block_size) -> tuple[np.ndarray, np.ndarray]:
    """(values, flat indices) of ``max_pool3d(avg_pool3d(vol))`` as ``detect_peaks`` configures them, flattened."""
    ctx = get_context(vol.device)
    blk = (C.c_int * 3)(*[int(b) for b in block_size])
    nb = (C.c_int64 * 3)()
    Z, Y, X = (int(s) for s in vol.shape)
    _lib.check(ctx.lib.bh_block_peaks(None, None, Z, Y, X, int(blur_kernel_size), blk, None, None, nb))
    n = int(nb[0]) * int(nb[1]) * int(nb[2])
    with torch.cuda.device(vol.device):
        values = torch.empty(n, dtype=torch.float32, device=vol.device)
        indices = torch.empty(n, dtype=torch.int64, device=vol.device)
    _lib.check(ctx.lib.bh_block_peaks(ctx.handle, ptr(vol), Z, Y, X, int(blur_kernel_size), blk, ptr(values), ptr(indices), nb))
    return values.cpu().numpy(), indices.cpu().numpy()


def detect_peaks(
    zyx_data: np.ndarray,
    block_size: int | tuple[int, int, int] = (8, 8, 8),
    nms_distance: int = 3,
    min_distance: int = 40,
    threshold_abs: float = 200.0,
    max_num_peaks: int = 500,
    exclude_border: tuple[int, int, int] | None = None,
    blur_kernel_size: int = 3,
    device: str = "cuda",
    verbose: bool = False,
):
    """Detect peaks with local maxima (characterize_psf.py:562-711); returns (N, 3) ZYX coordinates, brightest first."""
    if isinstance(block_size, int):
        block_size = (block_size,) * 3
    if not blur_kernel_size:
        raise ValueError("blur_kernel_size must be a positive odd number")  # the reference fails later (NameError)
    if blur_kernel_size % 2 != 1:
        raise ValueError(f"kernel_size={blur_kernel_size} must be an odd number")
    t, _, dev = as_device_volume(np.asarray(zyx_data).astype(np.float32) if not isinstance(zyx_data, torch.Tensor)
                                 else zyx_data.to(torch.float32), device)
    zyx_shape = tuple(int(s) for s in t.shape[-3:])
    peak_value, peak_idx = block_peaks(t.reshape(zyx_shape).contiguous(), blur_kernel_size, block_size)
    num_peaks = len(peak_idx)

    # top max_num_peaks brightest, brightest first (torch.topk; ties keep block order)
    order = np.argsort(-peak_value, kind="stable")[: min(max_num_peaks, num_peaks)]
    peak_value, peak_idx = peak_value[order], peak_idx[order]
    num_rejected_max_num_peaks = num_peaks - len(order)

    num_rejected_threshold_abs = 0
    if threshold_abs:
        keep = peak_value > threshold_abs
        num_rejected_threshold_abs = int((~keep).sum())
        peak_value, peak_idx = peak_value[keep], peak_idx[keep]

    coords = np.stack(np.unravel_index(peak_idx, zyx_shape), -1).astype(np.int64)
    f = coords.astype(np.float64)
    dist = np.sqrt(((f[:, None, :] - f[None, :, :]) ** 2).sum(-1)) if len(f) else np.zeros((0, 0))
    dist_mask = np.ones(len(coords), dtype=bool)
    nearby = np.argwhere(np.triu(dist < nms_distance, k=1))
    dist_mask[nearby[:, 1]] = False  # the peak in the second column is dimmer
    num_rejected_nms_distance = int((~dist_mask).sum())

    num_rejected_min_distance = 0
    if min_distance:
        close = dist < min_distance
        close[nearby[:, 0], nearby[:, 1]] = False
        dist_mask &= close.sum(1) < 2
        num_rejected_min_distance = int((~dist_mask).sum()) - num_rejected_nms_distance
    coords = coords[dist_mask]

    num_rejected_exclude_border = 0
    if exclude_border is not None:
        if not (isinstance(exclude_border, tuple) and len(exclude_border) == 3
                and all(isinstance(v, int) for v in exclude_border)):
            raise ValueError(f"invalid argument exclude_border={exclude_border}")
        for dim, size in enumerate(exclude_border):
            border_mask = (size < coords[:, dim]) & (coords[:, dim] < zyx_shape[dim] - size)
            coords = coords[border_mask]
            num_rejected_exclude_border += int((~border_mask).sum())

    if verbose:
        print(f"Number of peaks detected: {num_peaks}")
        print(f"Number of peaks rejected by max_num_peaks: {num_rejected_max_num_peaks}")
        print(f"Number of peaks rejected by threshold_abs: {num_rejected_threshold_abs}")
        print(f"Number of peaks rejected by nms_distance: {num_rejected_nms_distance}")
        print(f"Number of peaks rejected by min_distance: {num_rejected_min_distance}")
        print(f"Number of peaks rejected by exclude_border: {num_rejected_exclude_border}")
        print(f"Number of peaks returned: {len(coords)}")
    return coords


def _patch_margins(scale, patch_size):
    if patch_size is None:
        patch_size = (scale[0] * 15, scale[1] * 18, scale[2] * 18)
    return np.array(patch_size, dtype=np.float64) / np.array(scale, dtype=np.float64)


def _starts(points, margins):
    """BeadExtractor._create_slices: start = int(c - margin // 2), extent int(margin)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.array([[int(c - m // 2) for c, m in zip(pt, margins)] for pt in pts], dtype=np.int64).reshape(-1, 3)


def recentre_beads(vol: torch.Tensor, points, margins, sigma: float = 2.0) -> np.ndarray:
    """``BeadExtractor._find_closest_peak`` for every point that passes ``_in_margins``; returns the new centres."""
    shape = np.array(vol.shape, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ok = ~(np.any(pts < margins / 2, axis=1) | np.any(pts >= shape - margins / 2, axis=1))
    pts = pts[ok]
    if len(pts) == 0:
        return np.zeros((0, 3), dtype=np.int64)
    patch = [int(m) for m in margins]
    starts = _starts(pts, margins).astype(np.int32)
    ctx = get_context(vol.device)
    peaks = (C.c_int64 * len(pts))()
    _lib.check(ctx.lib.bh_patch_peaks(ctx.handle, ptr(vol), *vol.shape, np.ascontiguousarray(starts).ctypes.data_as(
        C.POINTER(C.c_int)), len(pts), (C.c_int * 3)(*patch), float(sigma), peaks))
    local = np.stack(np.unravel_index(np.array(peaks, dtype=np.int64), patch), -1)
    offset = local - np.array(patch) // 2
    return np.array([[int(p[a] + offset[i, a]) for a in range(3)] for i, p in enumerate(pts)], dtype=np.int64)


def extract_beads(zyx_data, points, scale: tuple, patch_size: tuple = None, device="cuda"):
    """``characterize_psf.extract_beads`` (:173-190): recentred crops and their offsets; empty crops are dropped."""
    a = np.asarray(zyx_data)
    t, _, dev = as_device_volume(a.astype(np.float32), device)
    margins = _patch_margins(scale, patch_size)
    centres = recentre_beads(t, points, margins)
    beads, offsets = [], []
    for c in centres:
        st = _starts(c[None], margins)[0]
        sl = tuple(slice(int(s), int(s) + int(m)) for s, m in zip(st, margins))
        crop = a[sl]  # numpy slicing semantics, as the reference: truncated at the far border, empty for negative starts
        if crop.size > 0:
            beads.append(crop)
            offsets.append(tuple(int(v) for v in (np.array(c) - np.array(crop.shape) // 2)))
    return beads, offsets


# ---------------------------------------------------------------------------------------- characterize-psf: the Gaussian fits
# the keys of PSF.get_summary_dict(), in order: ZFitRecord, YXFitRecord, ZYXFitRecord (vendor psf_analysis/records.py)
FIT_COLUMNS = (
    "z_bg", "z_amp", "z_mu", "z_sigma", "z_fwhm", "z_bg_sde", "z_amp_sde", "z_mu_sde", "z_sigma_sde",
    "yx_bg", "yx_amp", "y_mu", "x_mu", "yx_cyy", "yx_cyx", "yx_cxx", "y_fwhm", "x_fwhm", "yx_pc1_fwhm", "yx_pc2_fwhm",
    "yx_bg_sde", "yx_amp_sde", "y_mu_sde", "x_mu_sde", "yx_cyy_sde", "yx_cyx_sde", "yx_cxx_sde",
    "zyx_bg", "zyx_amp", "zyx_z_mu", "zyx_y_mu", "zyx_x_mu", "zyx_czz", "zyx_czy", "zyx_czx", "zyx_cyy", "zyx_cyx", "zyx_cxx",
    "zyx_z_fwhm", "zyx_y_fwhm", "zyx_x_fwhm", "zyx_pc1_fwhm", "zyx_pc2_fwhm", "zyx_pc3_fwhm",
    "zyx_bg_sde", "zyx_amp_sde", "zyx_z_mu_sde", "zyx_y_mu_sde", "zyx_x_mu_sde", "zyx_czz_sde", "zyx_czy_sde", "zyx_czx_sde",
    "zyx_cyy_sde", "zyx_cyx_sde", "zyx_cxx_sde",
)
assert len(FIT_COLUMNS) == _lib.PSF_NCOL
# every record field but the covariance entries is a NonNegativeFloat: a negative one fails the reference's validation, the
# bead's summary becomes {} (characterize_psf.py:241-246) and dropna() removes the bead
_SIGNED = {"yx_cyy", "yx_cyx", "yx_cxx", "zyx_czz", "zyx_czy", "zyx_czx", "zyx_cyy", "zyx_cyx", "zyx_cxx"}
_NON_NEGATIVE = [i for i, c in enumerate(FIT_COLUMNS) if c not in _SIGNED]
FIT_STATUS = ("converged", "iteration cap", "non-finite", "singular", "empty sample")
FIT_MAX_ITERATIONS = 100
PEAK_WIDTH_COLUMNS = ("1d_z_fwhm", "1d_y_fwhm", "1d_x_fwhm")
# what float32 holds exactly: the device volume is float32 and the fits need the stored integers
SUPPORTED_DTYPES = (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.int16), np.dtype(np.float32))


def bead_boxes(volume_shape, centres, margins):
    """The boxes ``extract_beads`` crops: (starts, shapes, offsets) of the non-empty ones.  NumPy slicing semantics, as the
    reference's ``data[slices]``: truncated at the far border, a negative start counts from the far end (mostly empty)."""
    starts, shapes, offsets = [], [], []
    for c in np.asarray(centres).reshape(-1, 3):
        st = _starts(c[None], margins)[0]
        lo_hi = [slice(int(s), int(s) + int(m)).indices(int(n))[:2] for s, m, n in zip(st, margins, volume_shape)]
        shape = [max(hi - lo, 0) for lo, hi in lo_hi]
        if min(shape) > 0:
            starts.append([lo for lo, _ in lo_hi])
            shapes.append(shape)
            offsets.append(tuple(int(v) for v in (np.array(c) - np.array(shape) // 2)))
    return np.array(starts, dtype=np.int32).reshape(-1, 3), np.array(shapes, dtype=np.int32).reshape(-1, 3), offsets


def locate_beads(vol: torch.Tensor, points, scale: tuple, patch_size: tuple = None):
    """``extract_beads`` without the crops, on a volume that is already on the device: (starts, shapes, offsets)."""
    margins = _patch_margins(scale, patch_size)
    return bead_boxes(vol.shape, recentre_beads(vol, points, margins), margins)


def fit_beads(vol: torch.Tensor, starts, shapes, scale, offset: float = 0.0, gain: float = 1.0, float32_math: bool = True,
              max_iterations: int = FIT_MAX_ITERATIONS):
    """``bh_psf_fit`` on a float32 device volume: (rows (n, 55) in ``FIT_COLUMNS`` order with patch-local coordinates,
    initial guesses (n, 22), status (n, 3) indexing ``FIT_STATUS``, iterations (n, 3)) for the z, yx and zyx fits."""
    if vol.dtype != torch.float32 or vol.dim() != 3 or not vol.is_contiguous():
        raise ValueError("fit_beads needs a contiguous float32 (Z, Y, X) device volume")
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.int32).reshape(-1, 3))
    shapes = np.ascontiguousarray(np.asarray(shapes, dtype=np.int32).reshape(-1, 3))
    if len(starts) != len(shapes):
        raise ValueError("starts and shapes differ in length")
    n = len(starts)
    rows, guesses = np.empty((n, _lib.PSF_NCOL)), np.empty((n, _lib.PSF_NGUESS))
    status, iterations = np.empty((n, 3), dtype=np.int32), np.empty((n, 3), dtype=np.int32)
    ctx = get_context(vol.device)
    pi, pd_ = C.POINTER(C.c_int), C.POINTER(C.c_double)
    _lib.check(ctx.lib.bh_psf_fit(ctx.handle, ptr(vol), *vol.shape, starts.ctypes.data_as(pi), shapes.ctypes.data_as(pi), n,
                                  (C.c_double * 3)(*[float(s) for s in scale]), float(offset), float(gain), int(bool(float32_math)),
                                  int(max_iterations), rows.ctypes.data_as(pd_), guesses.ctypes.data_as(pd_),
                                  status.ctypes.data_as(pi), iterations.ctypes.data_as(pi)))
    return rows, guesses, status, iterations


def _pack_patches(patches):
    """A list of (differently shaped) patches as one (sum of sz, max sy, max sx) volume with its starts and shapes."""
    patches = [np.asarray(p) for p in patches]
    dtypes = {p.dtype for p in patches}
    if len(dtypes) != 1 or next(iter(dtypes)) not in SUPPORTED_DTYPES:
        raise ValueError(f"patches must share one of the dtypes {[str(d) for d in SUPPORTED_DTYPES]}, got {sorted(map(str, dtypes))}")
    shapes = np.array([p.shape for p in patches], dtype=np.int32).reshape(-1, 3)
    z0 = np.concatenate([[0], np.cumsum(shapes[:, 0])])
    vol = np.zeros((int(z0[-1]), int(shapes[:, 1].max()), int(shapes[:, 2].max())), dtype=patches[0].dtype)
    starts = np.zeros_like(shapes)
    for i, p in enumerate(patches):
        vol[z0[i]:z0[i + 1], : p.shape[1], : p.shape[2]] = p
        starts[i, 0] = z0[i]
    return vol, starts, shapes


def analyze_psf(zyx_patches, peak_coordinates, scale: tuple, offset: float = 0.0, gain: float = 1.0, noise: float = 1.0,
                use_robust_1d_fwhm: bool = False, device="cuda", float32_math: bool | None = None):
    """``characterize_psf.analyze_psf`` (:193-272): (df_gaussian_fit, df_1d_peak_width) with the reference's columns.

    ``zyx_patches`` is the reference's list of crops, or ``(volume, starts, shapes)``: a NumPy volume or a float32 device
    tensor that is uploaded once (not at all) and read in place, box by box.  ``float32_math`` says whether
    ``(patch + offset) * gain`` is float32 arithmetic, as NumPy's is for a float32 patch; None takes it from the dtype.
    A bead whose fits do not all converge, or whose record the reference's validation refuses (a negative background,
    amplitude, centre, FWHM or error), is a row of NaN that ``dropna`` removes, as the reference's ``except`` does.
    """
    import pandas as pd

    f_1d_peak_width = calculate_robust_peak_widths if use_robust_1d_fwhm else calculate_peak_widths
    peak_coordinates = np.asarray(peak_coordinates).reshape(-1, 3)
    boxed = isinstance(zyx_patches, tuple) and len(zyx_patches) == 3 and np.ndim(zyx_patches[1]) == 2
    volume, starts, shapes = zyx_patches if boxed else (_pack_patches(zyx_patches) if len(zyx_patches) else (None, [], []))
    if len(starts) != len(peak_coordinates):
        raise ValueError("zyx_patches and peak_coordinates differ in length")  # zip(strict=True)
    if len(starts) == 0:
        empty = pd.DataFrame(columns=list(FIT_COLUMNS) + ["zyx_snr"], dtype=np.float64)
        return empty, pd.DataFrame(columns=["z_mu", "y_mu", "x_mu", *PEAK_WIDTH_COLUMNS], dtype=np.float64)
    if isinstance(volume, torch.Tensor):
        vol = volume
        host = None
    else:
        host = np.asarray(volume)
        if host.dtype not in SUPPORTED_DTYPES:
            raise ValueError(f"dtype {host.dtype} is not exactly representable in float32")
        vol = as_device_volume(host.astype(np.float32), device)[0]
    if float32_math is None:
        float32_math = host is None or host.dtype == np.float32
    starts, shapes = np.asarray(starts).reshape(-1, 3), np.asarray(shapes).reshape(-1, 3)
    rows, _, status, _ = fit_beads(vol, starts, shapes, scale, offset, gain, float32_math)
    refused = (status != _lib.PSF_CONVERGED).any(axis=1) | ~(rows[:, _NON_NEGATIVE] >= 0).all(axis=1)
    rows[refused] = np.nan

    df_gaussian_fit = pd.DataFrame(rows, columns=list(FIT_COLUMNS))
    df_gaussian_fit["z_mu"] += peak_coordinates[:, 0] * scale[0]
    df_gaussian_fit["y_mu"] += peak_coordinates[:, 1] * scale[1]
    df_gaussian_fit["x_mu"] += peak_coordinates[:, 2] * scale[2]
    df_gaussian_fit["z_amp"] /= gain  # amplitude is measured relative to the offset
    df_gaussian_fit["zyx_amp"] /= gain

    def crop(st, sh):
        sl = tuple(slice(int(s), int(s) + int(n)) for s, n in zip(st, sh))
        return host[sl] if host is not None else vol[sl].cpu().numpy()

    df_1d_peak_width = pd.DataFrame([f_1d_peak_width(crop(st, sh), scale) for st, sh in zip(starts, shapes)],
                                    columns=list(PEAK_WIDTH_COLUMNS))
    df_1d_peak_width = pd.concat((df_gaussian_fit[["z_mu", "y_mu", "x_mu"]], df_1d_peak_width), axis=1)

    df_gaussian_fit = df_gaussian_fit.dropna()
    zero_width = (df_1d_peak_width[list(PEAK_WIDTH_COLUMNS)] == 0).any(axis=1)
    df_1d_peak_width = df_1d_peak_width.dropna()
    df_1d_peak_width = df_1d_peak_width.loc[~zero_width[df_1d_peak_width.index]]
    df_gaussian_fit["zyx_snr"] = df_gaussian_fit["zyx_amp"] / noise
    return df_gaussian_fit, df_1d_peak_width


def compute_noise_level(zyx_data, peak_coordinates, patch_size_pix, device="cuda") -> float:
    """``characterize_psf.compute_noise_level`` (:275-292): standard deviation (ddof 0) of the voxels outside the beads' boxes
    [c - size // 2, c + size // 2 + 1), on the device in float64: a bool mask cleared box by box, then mean and squared
    deviations in two masked passes."""
    if isinstance(zyx_data, torch.Tensor):
        x = zyx_data.to(resolve_device(zyx_data.device if zyx_data.is_cuda else device), torch.float64)
    else:
        x = torch.from_numpy(np.ascontiguousarray(zyx_data, dtype=np.float64)).to(resolve_device(device))
    mask = torch.ones(x.shape, dtype=torch.bool, device=x.device)
    half = [int(size) // 2 for size in patch_size_pix]
    for zyx in peak_coordinates:
        mask[tuple(slice(max(0, int(c) - h), min(n, int(c) + h + 1)) for c, h, n in zip(zyx, half, x.shape))] = False
    n = mask.sum()
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    mean = torch.where(mask, x, zero).sum() / n
    dev = torch.where(mask, x - mean, zero)
    return float(torch.sqrt((dev * dev).sum() / n))


def calculate_robust_peak_widths(zyx_data, zyx_scale: tuple):
    """``characterize_psf.calculate_robust_peak_widths`` (:295-332): per axis, the profile through the patch centre, its peak
    from a parabola through the samples around the maximum, and the width between the two linearly interpolated crossings
    of half that peak; 0.0 for an axis on which any of it fails."""
    from scipy.interpolate import interp1d

    nz, ny, nx = zyx_data.shape
    profiles = (zyx_data[:, ny // 2, nx // 2], zyx_data[nz // 2, :, nx // 2], zyx_data[nz // 2, ny // 2, :])
    fwhm = []
    for y, step in zip(profiles, zyx_scale, strict=True):
        try:
            x = np.arange(y.size)
            top = np.argmax(y)
            near = slice(max(0, top - 2), min(top + 2, y.size))
            p = np.polyfit(x[near], y[near], 2)
            vertex = -p[1] / (2 * p[0])
            half_max = np.polyval(p, vertex) / 2
            x = x * step
            above = np.where(y >= half_max / 2)[0]  # the reference keeps samples down to a quarter of the peak
            left, right = above[above < vertex], above[above > vertex]
            x_left = interp1d(y[left], x[left], kind="linear", fill_value="extrapolate")(half_max)
            x_right = interp1d(y[right], x[right], kind="linear", fill_value="extrapolate")(half_max)
            fwhm.append(x_right - x_left)
        except Exception:
            fwhm.append(0.0)
    return fwhm


def calculate_peak_widths(zyx_data, zyx_scale: tuple):
    """``characterize_psf.calculate_peak_widths`` (:335-346): scipy.signal.peak_widths at half height of the three profiles
    through the patch centre, the centre index taken as the peak; all three are 0.0 if any raises."""
    from scipy.signal import peak_widths

    nz, ny, nx = zyx_data.shape
    try:
        z_fwhm = peak_widths(zyx_data[:, ny // 2, nx // 2], [nz // 2])[0][0]
        y_fwhm = peak_widths(zyx_data[nz // 2, :, nx // 2], [ny // 2])[0][0]
        x_fwhm = peak_widths(zyx_data[nz // 2, ny // 2, :], [nx // 2])[0][0]
    except Exception:
        z_fwhm, y_fwhm, x_fwhm = (0.0, 0.0, 0.0)
    return z_fwhm * zyx_scale[0], y_fwhm * zyx_scale[1], x_fwhm * zyx_scale[2]


# ------------------------------------------------------------------------------------------------------------- the report
def _figure(*grid, **kw):
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    fig = Figure(**kw)
    FigureCanvasAgg(fig)
    return fig, fig.subplots(*grid, squeeze=False)


def plot_psf_slices(plots_dir: Path, beads: list, zyx_scale: tuple, axis_labels: tuple, bead_numbers: list) -> Path:
    """``beads_psf_slices.png``: the centre yx, zx and zy planes of the chosen beads, one column per bead."""
    sz, sy, sx = zyx_scale
    fig, ax = _figure(3, len(beads), figsize=(8, 8 * 3 / max(len(beads), 3) + 1))
    for col, (bead, number) in enumerate(zip(beads, bead_numbers, strict=True)):
        nz, ny, nx = bead.shape
        planes = ((bead[nz // 2], sy / sx, -1, -2), (bead[:, ny // 2], sz / sx, -1, -3), (bead[:, :, nx // 2], sz / sy, -2, -3))
        for row, (plane, aspect, across, up) in enumerate(planes):
            a = ax[row, col]
            a.imshow(plane, cmap="viridis", origin="lower", aspect=aspect)
            a.set_xlabel(axis_labels[across])
            a.set_ylabel(axis_labels[up])
            a.set_xticks([])
            a.set_yticks([])
        ax[0, col].set_title(f"Bead: {number}")
    fig.tight_layout()
    path = Path(plots_dir) / "beads_psf_slices.png"
    fig.savefig(path)
    return path


def plot_fwhm_vs_acq_axes(plots_dir: Path, x, y, z, fwhm_x, fwhm_y, fwhm_z, axis_labels: tuple) -> list[Path]:
    """``fwhm_vs_<axis>.png`` per axis: the lateral FWHMs on the left scale, the axial one on the right."""
    paths = [Path(plots_dir) / f"fwhm_vs_{axis}.png" for axis in axis_labels]
    for path, position, label in zip(paths, (z, y, x), axis_labels, strict=True):
        fig, ax = _figure(1, 1)
        ax = ax[0, 0]
        lateral = ax.plot(position, fwhm_x, "o", position, fwhm_y, "o")
        ax.set_xlabel(f"{label} position (um)")
        ax.set_ylabel(f"{axis_labels[2]} and {axis_labels[1]} FWHM (um)")
        right = ax.twinx()
        axial = right.plot(position, fwhm_z, "o", color="green")
        right.set_ylabel(f"{axis_labels[0]} FWHM (um)", color="green")
        right.tick_params(axis="y", labelcolor="green")
        right.legend(lateral + axial, axis_labels[::-1])
        fig.savefig(path)
    return paths


def plot_psf_amp(plots_dir: Path, x, y, z, amp, axis_labels: tuple) -> tuple[Path, Path]:
    """``psf_amp_xy.png`` (amplitude as colour over x, y) and ``psf_amp_z.png`` (amplitude against z)."""
    xy_path, z_path = Path(plots_dir) / "psf_amp_xy.png", Path(plots_dir) / "psf_amp_z.png"
    fig, ax = _figure(1, 1)
    sc = ax[0, 0].scatter(x, y, c=amp, vmin=np.quantile(amp, 0.01), vmax=np.quantile(amp, 0.99), cmap="summer")
    ax[0, 0].set_aspect("equal")
    ax[0, 0].set_xlabel(f"{axis_labels[-1]} (um)")
    ax[0, 0].set_ylabel(f"{axis_labels[-2]} (um)")
    fig.colorbar(sc, label="Amplitude (a.u.)")
    fig.savefig(xy_path)
    fig, ax = _figure(1, 1)
    ax[0, 0].scatter(z, amp)
    ax[0, 0].set_xlabel(f"{axis_labels[-3]} (um)")
    ax[0, 0].set_ylabel("Amplitude (a.u.)")
    fig.savefig(z_path)
    return xy_path, z_path


def _make_plots(output_path: Path, beads: list, df_gaussian_fit, df_1d_peak_width, scale: tuple, axis_labels: tuple,
                fwhm_plot_type: str):
    plots_dir = Path(output_path) / "plots"
    plots_dir.mkdir(parents=True, exist_ok=True)
    # the reference draws exactly 5 and fails on a slide with fewer beads
    chosen = sorted(int(i) for i in np.random.choice(len(beads), min(5, len(beads)), replace=False))
    slices_path = plot_psf_slices(plots_dir, [beads[i] for i in chosen], scale, axis_labels, chosen)
    if fwhm_plot_type == "1D":
        df, widths = df_1d_peak_width, ("1d_x_fwhm", "1d_y_fwhm", "1d_z_fwhm")
    elif fwhm_plot_type == "3D":
        df, widths = df_gaussian_fit, ("zyx_x_fwhm", "zyx_y_fwhm", "zyx_z_fwhm")
    else:
        raise ValueError(f"Invalid fwhm_plot_type: {fwhm_plot_type}")
    fwhm_paths = plot_fwhm_vs_acq_axes(plots_dir, *[df[c].values for c in ("x_mu", "y_mu", "z_mu")], *[df[c].values for c in widths],
                                       axis_labels)
    amp_paths = plot_psf_amp(plots_dir, *[df_gaussian_fit[c].values for c in ("x_mu", "y_mu", "z_mu", "zyx_amp")], axis_labels)
    return slices_path, fwhm_paths, amp_paths


_REPORT_STYLE = "<style>body { max-width: 60em; margin: 2em auto; font-family: sans-serif; } img { max-width: 100%; }</style>"


def _report_markdown(dataset, data_dir, scale, counts, df_gaussian_fit, df_1d_peak_width, plot_paths, axis_labels, fwhm_plot_type):
    def stats(df, cols):
        return [(df[c].mean(), df[c].std()) for c in cols]

    slices_path, fwhm_paths, amp_paths = plot_paths
    fit3d = stats(df_gaussian_fit, ("zyx_x_fwhm", "zyx_y_fwhm", "zyx_z_fwhm"))
    prof = stats(df_1d_peak_width, ("1d_x_fwhm", "1d_y_fwhm", "1d_z_fwhm"))
    pcs = [df_gaussian_fit[c].mean() for c in ("zyx_pc3_fwhm", "zyx_pc2_fwhm", "zyx_pc1_fwhm")]
    snr = df_gaussian_fit["zyx_snr"]
    labels = axis_labels[::-1]  # x, y, z
    lines = ["# PSF Analysis", "", "## Overview", "", "### Dataset", "", f"* Name: `{dataset}`", f"* Path: `{data_dir}`",
             f"* Scale (z, y, x): {tuple(float(v) for v in np.round(scale, 3))} um",
             f"* Date analyzed: {datetime.datetime.now().strftime('%Y-%m-%d %H:%M:%S')}", "", "### Number of beads", "",
             f"* Detected: {counts[0]}", f"* Analyzed: {counts[1]}", f"* Skipped: {counts[2]}",
             f"* Signal-to-noise ratio: {snr.mean():.0f} ± {snr.std():.0f}", "", "### FWHM", "", "* **3D Gaussian fit**"]
    lines += [f"    - {lab}: {m:.3f} ± {s:.3f} um" for lab, (m, s) in zip(labels, fit3d)]
    lines += ["* 1D profile"] + [f"    - {lab}: {m:.3f} ± {s:.3f} um" for lab, (m, s) in zip(labels, prof)]
    lines += ["* 3D principal components", "    - " + ", ".join(f"{v:.3f} um" for v in pcs), "",
              "## Representative bead PSF images", f"![beads psf slices]({slices_path})", ""]
    for lab, path in zip(axis_labels, fwhm_paths):
        lines += [f"## {fwhm_plot_type} FWHM versus {lab} position", f"![fwhm vs {lab}]({path})", ""]
    lines += [f"## PSF amplitude versus {axis_labels[-1]}-{axis_labels[-2]} position", f"![psf amp xy]({amp_paths[0]})", "",
              f"## PSF amplitude versus {axis_labels[-3]} position", f"![psf amp z]({amp_paths[1]})", ""]
    return "\n".join(lines)


def generate_report(output_path: Path, data_dir: Path, dataset: str, beads: list, peaks, df_gaussian_fit, df_1d_peak_width,
                    scale: tuple, axis_labels: tuple, fwhm_plot_type: str) -> None:
    """``characterize_psf.generate_report`` (:87-170): ``psf_gaussian_fit.csv``, ``psf_1d_peak_width.csv``, ``peaks.pkl``,
    ``plots/`` and ``psf_analysis_report.md``; ``psf_analysis_report.html`` as well where the ``markdown`` package imports.
    Unlike the reference it ships no stylesheet file and never opens a browser; the per-axis standard deviations are
    printed next to their own axis (the reference pairs x's mean with z's deviation)."""
    output_path = Path(output_path)
    output_path.mkdir(exist_ok=True)
    plots = _make_plots(output_path, beads, df_gaussian_fit, df_1d_peak_width, scale, axis_labels, fwhm_plot_type)
    rel = (plots[0].relative_to(output_path).as_posix(), [p.relative_to(output_path).as_posix() for p in plots[1]],
           [p.relative_to(output_path).as_posix() for p in plots[2]])
    counts = (len(beads), len(df_gaussian_fit), len(beads) - len(df_gaussian_fit))
    report = _report_markdown(dataset, data_dir, scale, counts, df_gaussian_fit, df_1d_peak_width, rel, axis_labels, fwhm_plot_type)
    with open(output_path / "peaks.pkl", "wb") as file:
        pickle.dump(peaks, file)
    df_gaussian_fit.to_csv(output_path / "psf_gaussian_fit.csv", index=False)
    df_1d_peak_width.to_csv(output_path / "psf_1d_peak_width.csv", index=False)
    (output_path / "psf_analysis_report.md").write_text(report)
    try:
        import markdown
    except ImportError:
        return
    (output_path / "psf_analysis_report.html").write_text(
        f"<head><title>PSF Analysis: {dataset}</title>{_REPORT_STYLE}</head>\n<article>\n{markdown.markdown(report)}\n</article>\n")


def characterize_psf(zyx_data: np.ndarray, zyx_scale: tuple, settings, output_report_path, input_dataset_path,
                     input_dataset_name: str, echo=print):
    """``characterize_psf._characterize_psf`` (:713-788): detect, recentre, fit and report; returns the detected peaks.  The
    volume is uploaded once; detection, recentring, the noise level and the fits read that copy."""
    import time
    import warnings

    zyx_data = np.asarray(zyx_data)
    if zyx_data.dtype not in SUPPORTED_DTYPES:
        raise ValueError(f"characterize-psf reads uint8, uint16, int16 and float32 stores; {zyx_data.dtype} is not exactly "
                         "representable in float32")
    zyx_scale = tuple(float(s) for s in zyx_scale)
    cfg = settings.model_dump()
    patch_size, axis_labels = cfg.pop("patch_size"), cfg.pop("axis_labels")
    offset, gain = cfg.pop("offset"), cfg.pop("gain")
    use_robust_1d_fwhm, fwhm_plot_type = cfg.pop("use_robust_1d_fwhm"), cfg.pop("fwhm_plot_type")
    cfg["block_size"], cfg["exclude_border"] = tuple(cfg["block_size"]), tuple(cfg["exclude_border"])
    if patch_size is None:  # extract_beads' default; the reference's noise mask needs a patch size and fails on None
        patch_size = (zyx_scale[0] * 15, zyx_scale[1] * 18, zyx_scale[2] * 18)

    echo("Detecting peaks...")
    t1 = time.time()
    vol, _, dev = as_device_volume(zyx_data.astype(np.float32), cfg.pop("device"))
    peaks = detect_peaks(vol, **cfg, device=dev, verbose=True)
    echo(f"Time to detect peaks: {time.time() - t1}")

    t1 = time.time()
    starts, shapes, peak_coordinates = locate_beads(vol, peaks, zyx_scale, patch_size)
    if len(starts) == 0:
        raise RuntimeError("No beads were detected.")
    beads = [zyx_data[tuple(slice(int(s), int(s) + int(n)) for s, n in zip(st, sh))] for st, sh in zip(starts, shapes)]
    patch_size_pix = np.ceil(np.array(patch_size) / np.array(zyx_scale)).astype(int)
    noise = compute_noise_level(vol, peak_coordinates, patch_size_pix)
    echo("Analyzing PSFs...")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        df_gaussian_fit, df_1d_peak_width = analyze_psf((vol, starts, shapes), peak_coordinates, zyx_scale, offset=offset, gain=gain,
                                                        noise=noise, use_robust_1d_fwhm=use_robust_1d_fwhm,
                                                        float32_math=zyx_data.dtype == np.float32)
    echo(f"Time to analyze PSFs: {time.time() - t1}")
    generate_report(Path(output_report_path), input_dataset_path, input_dataset_name, beads, peaks, df_gaussian_fit,
                    df_1d_peak_width, zyx_scale, axis_labels, fwhm_plot_type)
    return peaks
