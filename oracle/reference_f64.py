"""Float64 restatement of the FFT deconvolutions: the yardstick for the float32 FFT engine.

``oracle_np`` computes Richardson-Lucy and Tikhonov with complex64 FFTs on float32 arrays, so a float32 GPU result compared
with it is judged by another float32 computation.  The functions here follow the same definitions in float64 throughout and
are written in torch, so the same code runs on the CPU and, for volumes too large for the host, on the GPU (torch's FFTs
there are the vendor library's double-precision transforms, independent of the project's kernels).

Richardson-Lucy (the project's definition, the C3 comment in ``oracle_np.py``):
    h    = psf / sum(psf), zero-padded and rolled so its centre voxel sits at 0 (``oracle_np.rl_otf`` / ``pad_psf``:
           tap k of an axis of extent K sits at offset k - K // 2)
    e0   = max(d, 0)
    e   <- max(e * corr_h(d / max(conv_h(e), eps)), 0)        circular convolution / correlation
Tikhonov (``oracle_np.tikhonov_zyx``):  real(ifftn(fftn(x) * conj(H) / (|H|^2 + reg)))
Inverse filter (``oracle_np.wo_apply_inverse_transfer_function``):  crop_z(real(ifftn(fftn(pad_z(n(x))) * conj(H) / (|H|^2 + reg))))
for any H, with n(x) = x / mean(x) - 1; and the same with the filter stored as bfloat16 pairs, rounded as the staging kernel does.
Phase cross-correlation (``oracle_np.phase_cross_corr``):  |irfftn(F1 conj(F2) / norm)|, fftshifted, and the signed position of its
first maximum; norm = 1, max(|F1 conj(F2)|, eps) or |F1| |F2|.
Smooth + shrink (``oracle_np.smooth_shrink``):  per axis out[i] = sum_k w[k] in[clamp(f i + o + k - R)], the weights rounded to
float32 as ``bh_smooth_shrink`` stages them, every sum in float64.
Deskew (``oracle_np.fast_deskew_zyx``):  (1/N) sum_k (v0 w0 + v1 w1) at the float32 sample positions of ``oracle_np.deskew_coords``
with their float32 weights, every tap, product and sum in float64, and the magnitude sum beside it; then the reference's fill.
Overhang fill (``oracle_np.fill_overhang`` / ``fill_overhang_with_mean``):  mask = (vol == 0) dilated by the 3x3x3 cube or the cross,
the float64 mean of the rest, and the magnitude per valid voxel that a sum(all) - sum(masked) evaluation carries.
Affine warp (``oracle_np.affine_pull``, orders 0 and 1):  the inside rule on the float64 coordinate; linear with an edge clamp at
the operator's Q32.32 sample positions (exact integers), every tap, weight and sum in float64; ZEROS and nearest at the float64
positions; and the largest tap magnitude beside it.
Cubic B-spline warp (``oracle_np.spline_prefilter`` / ``spline_affine_pull``, SciPy order 3, mode "constant"):  the coefficients by
SciPy's recursion with its exact mirror initialisation, the 4^n taps mirrored about the edge samples with SciPy's float64 weight
polynomials, and beside the value the local scale M = sum_i w_i A[tap_i], A the samples' magnitudes under the absolute value of
the prefilter's impulse response.

Inputs may be numpy arrays or torch tensors; results are float64 torch tensors on the input's device (or ``device``).
Nothing here imports the product package.
"""

from __future__ import annotations

import numpy as np
import torch

F64 = torch.float64


def _tensor(x, device=None, dtype=None) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if device is not None:
        t = t.to(device)
    return t if dtype is None else t.to(dtype)


def psf_is_point_symmetric(psf) -> bool:
    """Odd extents and equal to its point mirror: the transfer function is real (exactly, in exact arithmetic)."""
    p = _tensor(psf)
    return all(k % 2 for k in p.shape) and bool(torch.equal(p, p.flip((0, 1, 2))))


def centred_kernel(psf, shape, device=None) -> torch.Tensor:
    """h = psf / sum(psf) in float64 on a zero box of ``shape``, tap k of each axis at offset k - K // 2 (mod N)."""
    h = _tensor(psf, device, F64)
    if h.ndim != 3 or any(k > n for k, n in zip(h.shape, shape)):
        raise ValueError(f"psf {tuple(h.shape)} does not fit the box {tuple(shape)}")
    h = h / h.sum()
    box = torch.zeros(tuple(int(n) for n in shape), dtype=F64, device=h.device)
    box[: h.shape[0], : h.shape[1], : h.shape[2]] = h
    return torch.roll(box, tuple(-(k // 2) for k in h.shape), dims=(0, 1, 2))


def rl_otf_f64(psf, shape, device=None, real=None) -> torch.Tensor:
    """Half spectrum rfftn(h) of the centred kernel (complex128), or its real part (float64) when ``real`` — by default when
    the PSF is point-symmetric, whose transfer function is real: the imaginary part is float64 rounding and dropping it
    halves the memory."""
    otf = torch.fft.rfftn(centred_kernel(psf, shape, device))
    if real is None:
        real = psf_is_point_symmetric(psf)
    return otf.real.contiguous() if real else otf


def conv_f64(x: torch.Tensor, otf: torch.Tensor) -> torch.Tensor:
    """Circular convolution with the kernel whose half spectrum is ``otf``."""
    s = torch.fft.rfftn(x)
    s.mul_(otf)
    return torch.fft.irfftn(s, s=x.shape)


def corr_f64(x: torch.Tensor, otf: torch.Tensor) -> torch.Tensor:
    """Circular correlation with that kernel (convolution with its point mirror: conj(otf))."""
    s = torch.fft.rfftn(x)
    s.mul_(otf.conj() if otf.is_complex() else otf)
    return torch.fft.irfftn(s, s=x.shape)


def rl_step_f64(est: torch.Tensor, d: torch.Tensor, otf: torch.Tensor, eps: float) -> torch.Tensor:
    """One update in place: est <- max(est * corr(d / max(conv(est), eps)), 0).  ``d`` may stay float32 (the division
    promotes); at most one volume-sized temporary and one half spectrum live besides ``est``."""
    blur = conv_f64(est, otf)
    blur.clamp_(min=eps)
    torch.div(d, blur, out=blur)        # the ratio, in place of the blur
    corr = corr_f64(blur, otf)
    del blur
    return est.mul_(corr).clamp_(min=0.0)


def richardson_lucy_f64_checkpoints(zyx, psf, checkpoints=(1, 2, 5, 10), eps: float = 1e-6, device=None):
    """One float64 run that yields ``(k, est)`` at every iteration count in ``checkpoints`` (ascending; 0 allowed).  ``est`` is
    the live state: read it before advancing the generator, and do not modify it."""
    d = _tensor(zyx, device)
    if d.dtype not in (torch.float32, F64):
        d = d.to(F64)
    otf = rl_otf_f64(psf, d.shape, d.device)
    est = d.to(F64, copy=True).clamp_(min=0.0)
    done = 0
    for k in sorted(int(c) for c in checkpoints):
        while done < k:
            rl_step_f64(est, d, otf, eps)
            done += 1
        yield k, est


def richardson_lucy_f64(zyx, psf, iterations: int = 10, eps: float = 1e-6, device=None) -> torch.Tensor:
    """Richardson-Lucy in float64, ``iterations`` updates."""
    for _, est in richardson_lucy_f64_checkpoints(zyx, psf, (iterations,), eps, device):
        return est


def tikhonov_f64(zyx, transfer_function, regularization_strength: float = 1e-3, device=None) -> torch.Tensor:
    """real(ifftn(fftn(x) * conj(H) / (|H|^2 + reg))) on full complex128 spectra; H as given (real or complex)."""
    x = _tensor(zyx, device, F64)
    H = _tensor(transfer_function, x.device)
    H = H.to(torch.complex128) if H.is_complex() else H.to(F64)
    filt = H.conj() / (H.abs() ** 2 + float(regularization_strength))
    return torch.fft.ifftn(torch.fft.fftn(x) * filt).real.contiguous()


# ----------------------------------------------------------------------------- the inverse filter (apply-inv-tf)
def normalize_pad_f64(zyx, z_padding: int = 0, normalize: bool = False, device=None, mirror: bool = True) -> torch.Tensor:
    """pad_z(n(x)) in float64: n(x) = x / mean(x) - 1 when ``normalize``; ``z_padding`` planes on either side of z, as
    ``oracle_np.wo_apply_inverse_transfer_function`` defines them — the volume's own edge planes mirrored (plane pad - 1 - z
    below, plane Z - 1 - k for the k-th plane above) when ``z_padding < Z``, zeros otherwise (or when ``mirror`` is off)."""
    x = _tensor(zyx, device, F64)
    if normalize:
        x = x / x.mean() - 1.0
    pad = int(z_padding)
    if not pad:
        return x
    Z = x.shape[0]
    xp = torch.zeros((Z + 2 * pad,) + tuple(x.shape[1:]), dtype=F64, device=x.device)
    xp[pad:pad + Z] = x
    if mirror and pad < Z:
        xp[:pad] = x[:pad].flip(0)
        xp[pad + Z:] = x[Z - pad:].flip(0)
    return xp


def _apply_filter_f64(xp: torch.Tensor, filt: torch.Tensor, z_padding: int) -> torch.Tensor:
    out = torch.fft.ifftn(torch.fft.fftn(xp) * filt).real
    pad = int(z_padding)
    return (out[pad:out.shape[0] - pad] if pad else out).contiguous()


def inverse_filter_f64(zyx, transfer_function, z_padding: int = 0, regularization_strength: float = 1e-3,
                       normalize: bool = False, device=None, mirror: bool = True) -> torch.Tensor:
    """crop_z(Re ifftn(fftn(pad_z(n(x))) * conj(H) / (|H|^2 + reg))) on full complex128 spectra; H of the padded shape in natural
    FFT order, real or complex, with or without any symmetry (the real part keeps only the filter's Hermitian part)."""
    xp = normalize_pad_f64(zyx, z_padding, normalize, device, mirror)
    H = _tensor(transfer_function, xp.device)
    if tuple(H.shape) != tuple(xp.shape):
        raise ValueError(f"transfer function shape {tuple(H.shape)} != padded data shape {tuple(xp.shape)}")
    H = H.to(torch.complex128) if H.is_complex() else H.to(F64)
    return _apply_filter_f64(xp, H.conj() / (H.abs() ** 2 + float(regularization_strength)), z_padding)


def minus_k(H: torch.Tensor) -> torch.Tensor:
    """H(-k): every axis reversed about bin 0 (bin 0 and, on even axes, the Nyquist bin map to themselves)."""
    dims = tuple(range(H.ndim))
    return torch.roll(H.flip(dims), (1,) * H.ndim, dims)


def staged_filter_f32(transfer_function, regularization_strength: float, scale: float, one_division: bool = False):
    """The value ``inverse_filter_rows_kernel`` (csrc/fftconv.hip) stages per bin, formed in float32 from a complex64 / float32
    H on the full spectrum:  F_h(k) * scale,  F_h(k) = (conj(H(k)) q(k) + H(-k) q(-k)) / 2,  q = 1 / (|H|^2 + reg) — the
    Hermitian part of conj(H) / (|H|^2 + reg), which is all that acts on a real volume.  Returns (re, im) float32.
    ``one_division``: the same value with h / (|h|^2 + reg) as one division instead of reciprocal-then-multiply (a second
    float32 formulation; the distance between the two is the float32 uncertainty of the staged value)."""
    H = _tensor(transfer_function)
    H = H.to(torch.complex64) if H.is_complex() else H.to(torch.float32)
    hr, hi = (H.real, H.imag) if H.is_complex() else (H, torch.zeros_like(H))
    reg = torch.tensor(float(regularization_strength), dtype=torch.float32, device=H.device)
    s = torch.tensor(float(scale), dtype=torch.float32, device=H.device)
    den = hr * hr + hi * hi + reg
    if one_division:
        fr, fi = hr / den, hi / den
    else:
        q = 1.0 / den
        fr, fi = hr * q, hi * q
    return 0.5 * (fr + minus_k(fr)) * s, 0.5 * (-fi + minus_k(fi)) * s


def bf16_round(t: torch.Tensor, truncate: bool = False) -> torch.Tensor:
    """float32 -> bfloat16 -> float32: round to nearest even (``truncate``: drop the low 16 bits instead — a planted defect)."""
    if truncate:
        return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return t.to(torch.bfloat16).to(torch.float32)


def inverse_filter_bf16_f64(zyx, transfer_function, z_padding: int = 0, regularization_strength: float = 1e-3,
                            normalize: bool = False, device=None, mirror: bool = True, truncate: bool = False,
                            one_division: bool = False) -> torch.Tensor:
    """The inverse filter with the staged filter kept as bfloat16 pairs, transforms in float64.  The staged value is what the
    kernel documents: F_h(k) formed in float32, multiplied by float32(2 / V) (V the padded volume's voxel count — what the
    engine's unnormalised transforms need), THEN each component rounded to bfloat16 (round to nearest even) and widened; the
    2 / V is divided back out in float64.  The scale belongs inside the rounding: V is no power of two on 3 * 2^k and
    5 * 2^k boxes, so rounding F_h itself lands on other bfloat16 values."""
    xp = normalize_pad_f64(zyx, z_padding, normalize, device, mirror)
    H = _tensor(transfer_function, xp.device)
    if tuple(H.shape) != tuple(xp.shape):
        raise ValueError(f"transfer function shape {tuple(H.shape)} != padded data shape {tuple(xp.shape)}")
    scale = 2.0 / float(xp.numel())
    fr, fi = staged_filter_f32(H, regularization_strength, scale, one_division)
    filt = torch.complex(bf16_round(fr, truncate).to(F64), bf16_round(fi, truncate).to(F64)) / scale
    return _apply_filter_f64(xp, filt, z_padding)


# ----------------------------------------------------------------------------- phase cross-correlation
PCC_EPS = 1.1920929e-07   # the operator's constant (np.finfo(complex64).eps), whatever the working precision


def rfftn_by_axis(x: torch.Tensor) -> torch.Tensor:
    """rfftn of a 3-D tensor, one axis per call.  The same transform; the CPU back-end of torch 2.10.0 (threaded pocketfft)
    corrupts the heap in a multi-axis transform over the leading axes of a half spectrum (a loop of rfftn / irfftn at e.g.
    (4, 512, 33) ends in a segmentation fault), one axis at a time it does not.  With a torch that no longer does, these two
    helpers can give way to rfftn / irfftn."""
    return torch.fft.fft(torch.fft.fft(torch.fft.rfft(x, dim=2), dim=1), dim=0)


def irfftn_by_axis(spec: torch.Tensor) -> torch.Tensor:
    """irfftn WITHOUT a shape, one axis per call (see ``rfftn_by_axis``): the last axis comes back with 2 (m - 1) columns."""
    return torch.fft.irfft(torch.fft.ifft(torch.fft.ifft(spec, dim=0), dim=1), dim=2)


def phase_cross_corr_f64(ref, mov, normalization=None, device=None):
    """``oracle_np.phase_cross_corr`` in float64 / complex128: ``(shift, corr_shifted)``.  corr = irfftn(F1 conj(F2) / norm)
    WITHOUT a shape, so an odd last axis comes back one shorter; norm is 1 (``None``), max(|F1 conj(F2)|, eps) (``"magnitude"``)
    or |F1| |F2| (``"classic"``; a zero bin gives NaN, as it does in the definition).  ``corr_shifted`` = fftshift(|corr|), a
    float64 tensor; ``shift`` a float64 numpy array, the first occurrence of the maximum of |corr| with every component
    greater than fix(n / 2) wrapped negative."""
    a, b = _tensor(ref, device, F64), _tensor(mov, device, F64)
    if a.ndim != 3 or a.shape != b.shape:
        raise ValueError(f"expected two 3-D images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    F1, F2 = rfftn_by_axis(a), rfftn_by_axis(b)
    prod = F1 * F2.conj()
    if normalization == "magnitude":
        prod = prod / prod.abs().clamp(min=PCC_EPS)
    elif normalization == "classic":
        prod = prod / (F1.abs() * F2.abs())
    elif normalization is not None:
        raise ValueError(f"unknown normalization {normalization!r}")
    del F1, F2
    mag = irfftn_by_axis(prod).abs_()
    first = int(torch.argmax(mag))   # the first of equal maxima (a NaN counts as one, as in numpy)
    shift = np.array(np.unravel_index(first, tuple(mag.shape)), dtype=np.float64)
    n = np.array(mag.shape, dtype=np.float64)
    wrap = shift > np.fix(n / 2)
    shift[wrap] -= n[wrap]
    return shift, torch.fft.fftshift(mag)


# ----------------------------------------------------------------------------- smooth + shrink (registration pyramid)
def smooth_shrink_f64(vol, sigma, factor):
    """``oracle_np.smooth_shrink`` with float64 sums: x, then y, then z; per axis No = max(1, N // f) outputs at
    f i + o, o = ((N - 1) - f (No - 1)) // 2, an edge-clamped sampled Gaussian of radius R = ceil(4 sigma) (R = 0: the identity).
    The weights are the operator's own constants — exp(-k^2 / (2 sigma^2)) normalised in float64, THEN rounded to float32, as
    the kernel receives them — so they enter as given; products and sums are float64.  Returns (float64 tensor, offsets)."""
    out = np.asarray(vol.cpu() if isinstance(vol, torch.Tensor) else vol, dtype=np.float64)
    if out.ndim != 3:
        raise ValueError(f"expected a 3-D volume, got {out.shape}")
    offsets = [0, 0, 0]
    for a in (2, 1, 0):
        N, f, s = out.shape[a], int(factor[a]), float(sigma[a])
        if f < 1 or s < 0.0:
            raise ValueError("shrink factor must be >= 1 and sigma >= 0")
        No = max(1, N // f)
        o = ((N - 1) - f * (No - 1)) // 2
        offsets[a] = o
        R = int(np.ceil(4.0 * s))
        k = np.arange(-R, R + 1)
        w = np.exp(-0.5 * k.astype(np.float64) ** 2 / (s * s)) if R else np.ones(1)
        w = (w / w.sum()).astype(np.float32).astype(np.float64)
        centres = f * np.arange(No) + o
        acc = np.zeros(out.shape[:a] + (No,) + out.shape[a + 1:], dtype=np.float64)
        for kk, wk in zip(k, w):
            acc += wk * np.take(out, np.clip(centres + kk, 0, N - 1), axis=a)
        out = acc
    return torch.from_numpy(out), tuple(offsets)


# ----------------------------------------------------------------------------- deskew
def dilate_mask(mask: torch.Tensor, iterations: int = 3) -> torch.Tensor:
    """``oracle_np.dilate_zero_mask`` on a torch bool tensor (any device): ``iterations`` 3x3x3 dilations, nothing entering from
    outside the array.  Separable: one or-of-neighbours per axis and iteration."""
    m = mask.clone()
    for _ in range(int(iterations)):
        for axis in range(3):
            lo, hi = m.narrow(axis, 0, m.shape[axis] - 1), m.narrow(axis, 1, m.shape[axis] - 1)
            grown = m.clone()
            grown.narrow(axis, 1, m.shape[axis] - 1).logical_or_(lo)
            grown.narrow(axis, 0, m.shape[axis] - 1).logical_or_(hi)
            m = grown
    return m


def dilate_mask_cross(mask: torch.Tensor, iterations: int = 3) -> torch.Tensor:
    """The 6-connected counterpart of ``dilate_mask`` (SciPy ``binary_dilation``'s default structure, border value 0):
    ``iterations`` steps of m | (m shifted by +-1 along each axis), every shift of a step taken from the previous step's m, nothing
    entering from outside the array — the L1 ball of radius ``iterations``."""
    m = mask.clone()
    for _ in range(int(iterations)):
        grown = m.clone()
        for axis in range(3):
            n = m.shape[axis]
            if n > 1:
                grown.narrow(axis, 1, n - 1).logical_or_(m.narrow(axis, 0, n - 1))
                grown.narrow(axis, 0, n - 1).logical_or_(m.narrow(axis, 1, n - 1))
        m = grown
    return m


def fill_overhang_f64(vol, fill_value=None, iterations: int = 3, connectivity: int = 26, device=None):
    """``oracle_np.fill_overhang`` (connectivity 26) / ``fill_overhang_with_mean`` (6) with the mean in float64: ``(mask, fill, kappa)``.

      mask   ``vol == 0`` (so -0.0 too; a subnormal is not zero) dilated ``iterations`` times by the 3x3x3 cube or the cross;
      fill   the float64 mean of ``vol[~mask]`` (NaN when nothing is outside the mask), or ``fill_value`` as a float;
      kappa  (sum |vol| + sum |vol[mask]|) / count(~mask): the magnitude that the two float64 sums of csrc/fill.hip — over all
             voxels and over the masked ones — carry per valid voxel; the rounding bound of tests/fill_cases.py scales with it
             (infinite when nothing is outside the mask).
    The filled volume is ``torch.where(mask, fill, vol)``."""
    if isinstance(vol, np.ndarray) and not vol.flags.writeable:
        vol = vol.copy()
    x = _tensor(vol, device)
    if x.ndim != 3:
        raise ValueError(f"vol must be 3-D (Z, Y, X), got {tuple(x.shape)}")
    if connectivity not in (6, 26):
        raise ValueError(f"connectivity must be 6 or 26, got {connectivity}")
    mask = (dilate_mask if connectivity == 26 else dilate_mask_cross)(x == 0, iterations)
    nvalid = x.numel() - int(mask.sum())
    x64 = x.to(F64)
    if fill_value is None:
        fill = float(x64[~mask].sum()) / nvalid if nvalid else float("nan")
    else:
        fill = float(fill_value)
    mag = float(x64.abs().sum()) + float(x64[mask].abs().sum())
    return mask, fill, (mag / nvalid if nvalid else float("inf"))


def deskew_f64(raw, ls_angle_deg, px_to_scan_ratio, keep_overhang, average_n_slices=1, overhang_fill=0, device=None):
    """``oracle_np.fast_deskew_zyx`` with float64 arithmetic at the float32 sample positions.  The positions are the contract
    (``oracle_np.deskew_coords``: the reference's float32 operation order, which the kernels reproduce bit for bit), and so are
    the float32 weights w1 = ix - floor(ix), w0 = (floor(ix) + 1) - ix; the taps (zero outside the scanned range), the products,
    the sum over the N averaged slices and the division by N are float64.  Integer input is widened exactly.

    Returns ``(V, M, mask, fill)``:
      V     the deskewed volume before the fill, float64 ``(ceil(Y / N), X, Xp)``;
      M     (1/N) sum_k (|v0| w0 + |v1| w1), the magnitude a float32 evaluation's rounding error scales with (M == 0: every tap
            outside the scanned range or zero, V is an exact zero in any precision);
      mask  with a fill (``keep_overhang`` and ``overhang_fill`` "mean" or non-zero): V == 0 dilated three times by 3x3x3, else None;
      fill  the float64 mean of V outside ``mask`` (NaN when nothing is outside) or the constant as a float, else None.
    The filled volume is ``torch.where(mask, fill, V)``."""
    from . import oracle_np as O

    x = _tensor(raw, device)
    if x.ndim != 3:
        raise ValueError(f"raw must be 3-D (Z, Y, X), got {tuple(x.shape)}")
    Z, Y, X = (int(s) for s in x.shape)
    N = int(average_n_slices)
    (_, _, Xp), _ = O.get_deskewed_data_shape((Z, Y, X), ls_angle_deg, px_to_scan_ratio, keep_overhang)
    Za = -(-Y // N)
    V = torch.zeros((Za, X, Xp), dtype=F64, device=x.device)
    M = torch.zeros_like(V)
    for a in range(Za):
        for k in range(N):
            zo = a * N + k
            plane = x[:, Y - 1 - min(zo, Y - 1), :].to(F64).flip(1)            # (Z, X'), the output's y' axis
            ix = O.deskew_coords(Z, Y, Xp, ls_angle_deg, px_to_scan_ratio, zo)  # float32
            fl = np.floor(ix)
            w1 = (ix - fl).astype(np.float32)
            w0 = ((fl + np.float32(1.0)) - ix).astype(np.float32)
            i0 = fl.astype(np.int64)
            for i, w in ((i0, w0), (i0 + 1, w1)):
                inside = torch.from_numpy(((i >= 0) & (i < Z)).astype(np.float64) * w.astype(np.float64)).to(x.device)
                tap = plane[torch.from_numpy(np.clip(i, 0, Z - 1)).to(x.device)].T  # (X', Xp)
                V[a] += tap * inside
                M[a] += tap.abs() * inside
    if N > 1:
        V /= N
        M /= N
    if not (keep_overhang and (overhang_fill == "mean" or overhang_fill != 0)):
        return V, M, None, None
    mask = dilate_mask(V == 0, 3)
    if overhang_fill == "mean":
        valid = V[~mask]
        fill = float(valid.mean()) if valid.numel() else float("nan")
    else:
        fill = float(overhang_fill)
    return V, M, mask, fill


# ----------------------------------------------------------------------------- affine warp
def llround_q32(matrix) -> np.ndarray:
    """``llround(m * 2^32)`` of every entry as int64: round half AWAY from zero (C's llround; ``np.rint`` rounds half to even).
    ``m * 2^32`` is exact in float64 (a power of two), so is floor(|.| + 0.5) below 2^52; entries are below 2^30 in magnitude."""
    m = np.asarray(matrix, dtype=np.float64) * 4294967296.0
    if not (np.abs(m) < 2.0 ** 62).all():
        raise ValueError("matrix entry out of the Q32.32 range")
    a = np.abs(m)
    fl = np.floor(a)
    r = np.where(a - fl >= 0.5, fl + 1.0, fl)      # a - fl is exact
    return (np.sign(m) * r).astype(np.int64)


def warp_f64(vol, matrix, output_shape, crop_lo=(0, 0, 0), interpolation="linear", boundary=0, cval=0.0, device=None):
    """``out(p) = in(M p)`` for p = crop_lo + (z, y, x) over ``output_shape``, in float64: the pull-resample of ``oracle_np.affine_pull``
    (orders 0 and 1; boundary 0 ITK, 1 SciPy "constant", 2 zeros / grid-constant) as the operator defines it.

    * The input is cleaned first (``nan_to_num(nan=0)`` in its own type: NaN -> 0, +-inf -> +-FLT_MAX), then widened exactly.
    * ``inside`` is decided on the float64 coordinate in numpy's association, ((m0 z + m1 y) + m2 x) + m3, by affine_pull's rule
      per boundary (ZEROS: everywhere); outside it V is ``cval`` (rounded to float32 once, as the operator receives it).
    * Linear with ITK / SCIPY_CONSTANT: the sample position is the Q32.32 coordinate cq = mq0 z + mq1 y + mq2 x + mq3 in exact
      int64 arithmetic, mq = llround(m 2^32): taps at cq >> 32 and + 1 clamped to the volume, fractions (cq & 0xffffffff) / 2^32
      (exact in float64), the trilinear blend in float64.  The position grid is part of the operator.
    * Linear with ZEROS, and nearest: float64 positions, floor(c) / floor(c + 0.5), as affine_pull.

    Returns ``(V, M, inside)``: V float64; M the largest |tap| among the (clamped, cleaned) taps of the voxel — with ZEROS also
    |cval| —, the scale a float32 evaluation's rounding error is measured in (``cval``'s magnitude outside); inside bool."""
    if isinstance(vol, np.ndarray) and not vol.flags.writeable:
        vol = vol.copy()        # torch does not wrap read-only arrays quietly
    x = _tensor(vol, device)
    if x.ndim != 3:
        raise ValueError(f"vol must be 3-D (Z, Y, X), got {tuple(x.shape)}")
    if interpolation not in ("linear", "nearestneighbor"):
        raise ValueError(f"unknown interpolation {interpolation!r}")
    dev = x.device
    if x.dtype == torch.uint16:
        x = x.to(torch.int32)
    if x.is_floating_point():
        x = torch.nan_to_num(x, nan=0.0)
    x = x.to(F64)
    dims = tuple(int(n) for n in x.shape)
    m = np.asarray(matrix, dtype=np.float64)[:3, :4]
    cv = float(np.float32(cval))
    grids = [torch.arange(int(lo), int(lo) + int(n), device=dev, dtype=torch.int64) for lo, n in zip(crop_lo, output_shape)]
    gz, gy, gx = grids[0][:, None, None], grids[1][None, :, None], grids[2][None, None, :]
    fz, fy, fx = gz.to(F64), gy.to(F64), gx.to(F64)
    c = [((float(m[a, 0]) * fz + float(m[a, 1]) * fy) + float(m[a, 2]) * fx) + float(m[a, 3]) for a in range(3)]
    inside = torch.ones(tuple(int(n) for n in output_shape), dtype=torch.bool, device=dev)
    for ca, n in zip(c, dims):
        if boundary == 0:
            inside &= (ca >= -0.5) & (ca < n - 0.5)
        elif boundary == 1:
            inside &= (ca >= 0.0) & (ca <= n - 1)
    flat = x.reshape(-1)

    def tap(iz, iy, ix):
        return flat[(iz.clamp(0, dims[0] - 1) * dims[1] + iy.clamp(0, dims[1] - 1)) * dims[2] + ix.clamp(0, dims[2] - 1)]

    cvt = torch.full((), cv, dtype=F64, device=dev)
    if interpolation == "nearestneighbor":
        idx = [torch.floor(ca + 0.5).to(torch.int64) for ca in c]
        val = tap(*idx)
        if boundary != 0:
            ok = torch.ones_like(inside)
            for i, n in zip(idx, dims):
                ok &= (i >= 0) & (i < n)
            val = torch.where(ok, val, cvt)
        V = torch.where(inside, val, cvt)
        return V, V.abs(), inside
    if boundary == 2:
        base = [torch.floor(ca) for ca in c]
        frac = [ca - b for ca, b in zip(c, base)]
        base = [b.to(torch.int64) for b in base]
    else:
        mq = llround_q32(m)
        cq = [(int(mq[a, 0]) * gz + int(mq[a, 1]) * gy) + int(mq[a, 2]) * gx + int(mq[a, 3]) for a in range(3)]
        base = [q >> 32 for q in cq]
        frac = [(q & 0xFFFFFFFF).to(F64) / 4294967296.0 for q in cq]
    V = torch.zeros(inside.shape, dtype=F64, device=dev)
    M = torch.zeros_like(V)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (frac[0] if dz else 1 - frac[0]) * (frac[1] if dy else 1 - frac[1]) * (frac[2] if dx else 1 - frac[2])
                iz, iy, ix = base[0] + dz, base[1] + dy, base[2] + dx
                v = tap(iz, iy, ix)
                if boundary == 2:
                    ok = (iz >= 0) & (iz < dims[0]) & (iy >= 0) & (iy < dims[1]) & (ix >= 0) & (ix < dims[2])
                    v = torch.where(ok, v, cvt)
                V += w * v
                M = torch.maximum(M, v.abs())
    if boundary == 2:
        M = torch.maximum(M, cvt.abs())
    V = torch.where(inside, V, cvt)
    M = torch.where(inside, M, cvt.abs())
    return V, M, inside


# ----------------------------------------------------------------------------- cubic B-spline warp
SPLINE_POLE = float(np.sqrt(3.0) - 2.0)
SPLINE_REACH = 128      # |k| <= 128 of the impulse response: |z|^128 = 6e-74 of a sample, beyond what any kernel block can see


def _clean_f64(vol, device=None) -> torch.Tensor:
    """``nan_to_num(nan=0)`` in the input's own type (NaN -> 0, +-inf -> +-FLT_MAX for float32), widened exactly."""
    if isinstance(vol, np.ndarray) and not vol.flags.writeable:
        vol = vol.copy()
    x = _tensor(vol, device)
    if x.dtype == torch.uint16:
        x = x.to(torch.int32)
    if x.is_floating_point():
        x = torch.nan_to_num(x, nan=0.0)
    return x.to(F64)


def mirror_index(i: torch.Tensor, n: int) -> torch.Tensor:
    """Whole-sample symmetric extension of 0 .. n - 1 to any integer i (n == 1: always 0)."""
    if n <= 1:
        return torch.zeros_like(i)
    s2 = 2 * n - 2
    i = torch.remainder(i, s2)
    return torch.where(i >= n, s2 - i, i)


def spline_coef_f64(vol, device=None) -> torch.Tensor:
    """float64 cubic B-spline coefficients of an n-D array, axis by axis as SciPy computes them (ni_splines.c): c = 6 s; the causal
    start value c[0] = (sum_{i=0}^{n-2} z^i (c[i] + z^(n-1) c[n-1-i])) / (1 - z^(2n-2)) — the exact sum over the mirror extension,
    no run-in —; c[i] += z c[i-1]; c[n-1] = z (z c[n-2] + c[n-1]) / (z^2 - 1); c[i] = z (c[i+1] - c[i]).  Axes of length 1 are left
    alone.  The input is cleaned first (``nan_to_num(nan=0)``)."""
    c = _clean_f64(vol, device)
    z = SPLINE_POLE
    for ax in range(c.ndim):
        n = int(c.shape[ax])
        if n <= 1:
            continue
        c = (c.movedim(ax, 0) * ((1.0 - z) * (1.0 - 1.0 / z))).contiguous()
        zn1 = z ** (n - 1)
        shape = (-1,) + (1,) * (c.ndim - 1)
        zi = torch.from_numpy(z ** np.arange(n - 1, dtype=np.float64)).to(c.device).reshape(shape)      # z^0 .. z^(n-2)
        c0 = (zi * c[: n - 1]).sum(0) + zn1 * c[n - 1]
        if n > 2:
            c0 = c0 + zn1 * (zi[1:] * c[1: n - 1].flip(0)).sum(0)      # i = 1 .. n-2: z^i z^(n-1) c[n-1-i]
        c[0] = c0 / (1.0 - zn1 * zn1)
        for i in range(1, n):
            c[i] += z * c[i - 1]
        c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
        for i in range(n - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
        c = c.movedim(0, ax)
    return c.contiguous()


def spline_scale_f64(vol, device=None, weight=None) -> torch.Tensor:
    """A: the mirror-extended |sample| convolved per axis (length > 1) with ``sqrt(3) |z|^|k|``, the absolute value of the
    prefilter's impulse response (row sum 3): |coefficient| <= A everywhere, and A is local — a sample k voxels away along an axis
    counts with 0.268^|k|.  ``weight(k, axis)`` (an array over k = -REACH .. REACH) replaces the kernel on the axes it returns
    something for: tests/cubic_cases.py convolves with its rounding-error kernels that way."""
    a = _clean_f64(vol, device).abs()
    K = SPLINE_REACH
    k = np.arange(-K, K + 1)
    for ax in range(a.ndim):
        n = int(a.shape[ax])
        if n <= 1:
            continue
        h = None if weight is None else weight(k, ax)
        if h is None:
            h = np.sqrt(3.0) * np.abs(SPLINE_POLE) ** np.abs(k)
        idx = mirror_index(torch.arange(-K, n + K, device=a.device), n)
        ext = a.index_select(ax, idx)
        out = torch.zeros_like(a)
        for j, hj in enumerate(h):
            if hj != 0.0:
                out += float(hj) * ext.narrow(ax, j, n)
        a = out
    return a


def spline3_weights_f64(x: torch.Tensor):
    """SciPy's four cubic B-spline weights of the taps floor(c) - 1 .. floor(c) + 2 at the fraction x = c - floor(c), in float64."""
    z = 1.0 - x
    w1 = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return [w0, w1, w2, 1.0 - w0 - w1 - w2]


def cubic_geometry_f64(in_shape, matrix, output_shape, crop_lo=None, device=None):
    """(inside, idx, wts, frac) of the cubic warp: ``inside`` on the float64 coordinate in the association
    ((m0 p0 + m1 p1) + m2 p2) + m3, p the integer output index plus crop_lo (SciPy "constant": 0 <= c <= n - 1 on every axis);
    per axis the four mirrored tap indices (int64), SciPy's float64 weights and the fraction, each broadcastable to the output."""
    nd = len(in_shape)
    m = np.asarray(matrix, dtype=np.float64)[:nd, : nd + 1]
    lo = (0,) * nd if crop_lo is None else crop_lo
    g = []
    for a in range(nd):
        view = [1] * nd
        view[a] = -1
        g.append(torch.arange(int(lo[a]), int(lo[a]) + int(output_shape[a]), device=device, dtype=torch.int64).to(F64).reshape(view))
    inside = torch.ones(tuple(int(n) for n in output_shape), dtype=torch.bool, device=device)
    coords = []
    for a in range(nd):
        c = float(m[a, 0]) * g[0]
        for b in range(1, nd):
            c = c + float(m[a, b]) * g[b]
        c = c + float(m[a, nd])
        coords.append(c)
        inside = inside & (c >= 0.0) & (c <= float(in_shape[a] - 1))
    idx, wts, frac = [], [], []
    for c, n in zip(coords, in_shape):
        c = torch.where(inside, c, torch.zeros((), dtype=F64, device=device))
        fl = torch.floor(c)
        x = c - fl
        base = fl.to(torch.int64) - 1
        idx.append([mirror_index(base + k, int(n)) for k in range(4)])
        wts.append(spline3_weights_f64(x))
        frac.append(x)
    return inside, idx, wts, frac


def cubic_sum_f64(fields, idx, wts, weight_sets=None):
    """sum over the 4^n taps of (prod_a wts[a][k_a]) field[idx[0][k_0], ...] in float64, for every field of the list (one tensor:
    one result).  ``weight_sets``: further weight lists like ``wts`` — the result is then a list per weight set (wts first)."""
    single = isinstance(fields, torch.Tensor)
    fields = [fields] if single else list(fields)
    sets = [wts] + list(weight_sets or [])
    nd = fields[0].ndim
    flats = [f.reshape(-1) for f in fields]
    strides = [int(np.prod(fields[0].shape[a + 1:], dtype=np.int64)) for a in range(nd)]
    offs = [[idx[a][k] * strides[a] for k in range(4)] for a in range(nd)]
    acc = [[None] * len(fields) for _ in sets]
    for taps in np.ndindex(*([4] * nd)):
        off = offs[0][taps[0]]
        for a in range(1, nd):
            off = off + offs[a][taps[a]]
        vals = [f[off] for f in flats]
        for s, ws in enumerate(sets):
            w = ws[0][taps[0]]
            for a in range(1, nd):
                w = w * ws[a][taps[a]]
            for j, v in enumerate(vals):
                acc[s][j] = w * v if acc[s][j] is None else acc[s][j] + w * v
    out = [a[0] if single else a for a in acc]
    return out[0] if weight_sets is None else out


def cubic_warp_f64(vol, matrix, output_shape, crop_lo=None, cval=0.0, device=None):
    """``scipy.ndimage.affine_transform(vol, matrix, output_shape=..., order=3, mode="constant", cval=cval)`` in float64, on the
    sub-box starting at ``crop_lo`` of the output grid; n-D (2-D images, 3-D volumes).

    * The input is cleaned first (``nan_to_num(nan=0)``), the coefficients are ``spline_coef_f64``.
    * ``inside`` on the float64 coordinate (``cubic_geometry_f64``); outside it V is ``cval`` (rounded to float32 once).
    * SciPy's float64 weight polynomials, taps mirrored about the edge samples, the float64 sum.

    Returns ``(V, M, inside)``: M = sum_i w_i A[tap_i] with A = ``spline_scale_f64`` — the scale a float32 evaluation's rounding
    error is measured in (``|cval|`` outside): local, unlike the volume's maximum."""
    x = _clean_f64(vol, device)
    dev = x.device
    inside, idx, wts, _ = cubic_geometry_f64(tuple(x.shape), matrix, output_shape, crop_lo, dev)
    V, M = cubic_sum_f64([spline_coef_f64(x), spline_scale_f64(x)], idx, wts)
    cv = torch.full((), float(np.float32(cval)), dtype=F64, device=dev)
    return torch.where(inside, V, cv), torch.where(inside, M, cv.abs()), inside
