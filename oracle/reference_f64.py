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
