"""Inputs of the transfer-function tests (tests/test_tf_reference.py on the CPU, tests/test_gpu_tf_f64.py on the GPU): the case
tables of compute-tf's two models, the pupil ties, and a float32 / complex64 restatement of both functions with its planted
defects.

The float64 reference is ``oracle_np.wo_phase_transfer_function_3d`` / ``wo_fluorescence_transfer_function_3d``; it is computed
once per case (``phase_reference`` / ``fluorescence_reference``) and shared, read-only, by every test that needs it.
"""

import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import oracle_np as O

PhaseCase = namedtuple("PhaseCase", "name shape pad invert yx dz lamb index na_ill na_det")
FluorCase = namedtuple("FluorCase", "name shape pad yx dz lamb index na_det")


def phase_case(name, shape, pad, invert, yx=0.1, dz=0.25, lamb=0.45, index=1.3, na_ill=0.5, na_det=1.2):
    return PhaseCase(name, tuple(shape), pad, invert, yx, dz, lamb, index, na_ill, na_det)


def fluor_case(name, shape, pad, yx=0.1, dz=0.25, lamb=0.507, index=1.3, na_det=1.2):
    return FluorCase(name, tuple(shape), pad, yx, dz, lamb, index, na_det)


def phase_args(c):
    """The positional arguments of ``phase_transfer_function_3d`` and of ``oracle_np.wo_phase_transfer_function_3d``."""
    return (c.shape, c.yx, c.dz, c.lamb, c.pad, c.index, c.na_ill, c.na_det, c.invert)


def fluor_args(c):
    return (c.shape, c.yx, c.dz, c.lamb, c.pad, c.index, c.na_det)


# Every kernel of compute-tf is a grid-stride loop of 256-thread blocks over a grid that csrc/invtf.hip's grid_for caps at
# num_cus * 16 blocks: 256 CUs * 16 * 256 = 1 048 576 threads on an MI355X (fewer CUs only wrap sooner).
#   (35, 150, 202):    1 060 500 bins = 1 048 576 + 11 924: every volume loop takes a second, ragged trip (202 = 2 * 101 and
#                      150 = 2 * 3 * 5^2, so no power-of-two stride lines up with a row or a plane).
#   (3, 730, 727):     a plane of 530 710 bins, the widest case below the cap: pupil_count_kernel's plane loop does not wrap, the
#                      volume loops (1 592 130 bins) do with a ragged tail of 543 554.
#   (4, 1030, 1027):   a plane of 1 057 810 = 1 048 576 + 9 234 bins: pupil_count_kernel's plane loop wraps with a ragged tail,
#                      and 4 231 240 bins = 4 * 1 048 576 + 36 936: a fifth, ragged trip of every volume loop.  Four planes, not
#                      three: at Zt <= 3 the window keeps the plane z = 0 alone and the real potential vanishes (below).
GRID_CAP_THREADS = 256 * 16 * 256
WRAP_VOLUME = (35, 150, 202)
WRAP_PLANE_BELOW = (3, 730, 727)
WRAP_PLANE = (4, 1030, 1027)
assert GRID_CAP_THREADS < math.prod(WRAP_VOLUME) < 2 * GRID_CAP_THREADS
assert WRAP_PLANE_BELOW[1] * WRAP_PLANE_BELOW[2] < GRID_CAP_THREADS < math.prod(WRAP_PLANE_BELOW)
assert GRID_CAP_THREADS < WRAP_PLANE[1] * WRAP_PLANE[2] and 4 * GRID_CAP_THREADS < math.prod(WRAP_PLANE) < 5 * GRID_CAP_THREADS

# The depth of BASELINE config 5 on a small plane: the phases 2 pi z ob reach 2 pi * 64 * 2.9 = 1.2e3 rad, where forming them in
# float32 costs 7e-5 rad.  The error of that slip grows with the depth; below some 160 planes it stays inside the bounds.
DEEP = (512, 12, 14)

PHASE_CASES = [
    phase_case("native", (8, 16, 20), 0, False),
    phase_case("padded inverted even Zt", (6, 12, 10), 2, True),
    phase_case("factors 2 and 2", (5, 10, 12), 1, False, yx=0.16, dz=0.3),
    phase_case("all odd inverted", (7, 15, 21), 0, True),
    phase_case("odd Zt padded inverted", (5, 9, 14), 1, True),
    phase_case("Zt 1", (1, 16, 20), 0, False),
    phase_case("Zt 3", (1, 12, 10), 1, False),
    phase_case("factors 3 and 3", (4, 10, 12), 1, False, yx=0.3, dz=0.6),   # refined box (14, 30, 36) cut back to (6, 10, 12)
    phase_case("long rows", (3, 6, 64), 0, False),
    phase_case("long columns", (3, 64, 6), 0, False),
    phase_case("volume loops wrap", WRAP_VOLUME, 0, False),
    phase_case("widest plane below the cap", WRAP_PLANE_BELOW, 0, False),
    phase_case("plane loop wraps", WRAP_PLANE, 0, False),
    phase_case("512 planes", DEEP, 0, False),
]
FLUOR_CASES = [
    fluor_case("native", (8, 16, 20), 0),
    fluor_case("factors 2 and 2", (6, 12, 10), 2, yx=0.15, dz=0.4),
    fluor_case("all odd", (7, 15, 21), 1),
    fluor_case("Zt 1", (1, 16, 20), 0),
    fluor_case("volume loops wrap", WRAP_VOLUME, 0),
    fluor_case("512 planes", DEEP, 0),
]

# ----------------------------------------------------------------------------- pupil ties
# A 30 x 30 plane at yx 0.1 and wavelength 0.5: NA = 0.5 * cut makes NA / wavelength == cut exactly (a halving and a doubling),
# and nothing is refined.  The cut-offs are radial frequencies of the plane itself, so one bin (and its mirror images) sits on
# ``frr < cut`` — outside, as the oracle forms frr; an implementation that forms it an ulp lower takes the bin in.
TIE_PLANE, TIE_Z, TIE_LAMB, TIE_YX = 30, 4, 0.5, 0.1
TIE1_K = 7          # k / (n d) and k * (1 / (n d)) differ here (and at 5, 10, 14)
TIE2_BIN = (2, 4)   # the fused and the unfused fy^2 + fx^2 differ here
TIE1_CUT = max(TIE1_K / (TIE_PLANE * TIE_YX), TIE1_K * (1.0 / (TIE_PLANE * TIE_YX)))
TIE2_CUT = float(O.wo_radial_frequencies((TIE_PLANE, TIE_PLANE), TIE_YX)[TIE2_BIN])
_TIE_SHAPE = (TIE_Z, TIE_PLANE, TIE_PLANE)
PHASE_TIES = [
    phase_case("T1 detection cut on fftfreq", _TIE_SHAPE, 0, False, lamb=TIE_LAMB, yx=TIE_YX, na_det=0.5 * TIE1_CUT),
    phase_case("T2 detection cut on frr", _TIE_SHAPE, 0, False, lamb=TIE_LAMB, yx=TIE_YX, na_det=0.5 * TIE2_CUT),
    phase_case("T3 illumination cut on frr", _TIE_SHAPE, 0, False, lamb=TIE_LAMB, yx=TIE_YX, na_ill=0.5 * TIE2_CUT),
]
FLUOR_TIES = [fluor_case("T2 detection cut on frr", _TIE_SHAPE, 0, lamb=TIE_LAMB, yx=TIE_YX, na_det=0.5 * TIE2_CUT)]


def case_id(c):
    return f"{c.name} {c.shape}+{c.pad}"


def total_planes(c):
    """Zt of the returned functions: Z + 2 z_padding."""
    return c.shape[0] + 2 * c.pad


def real_potential_vanishes(c):
    """With at most three planes in all, ifftshift(hann(Zt)) is (1,), or (1, 0, 0): only the plane z = 0 is kept.  There the
    propagation kernel is the real pupil and the Green's function purely imaginary, so H1 = -H2 and the real-potential function
    is zero but for rounding (1e-16 of the imaginary one in float64): relative metrics mean nothing, and it is held to
    ``fft_metrics.TF_ZERO_RE_RATIO_TOL`` of the imaginary one instead.  Such a case must not be refined along z."""
    return total_planes(c) <= 3


@functools.lru_cache(maxsize=None)
def phase_reference(c):
    """(real, imaginary) potential transfer functions of a case in complex128, read-only."""
    out = O.wo_phase_transfer_function_3d(*phase_args(c))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fluorescence_reference(c):
    out = O.wo_fluorescence_transfer_function_3d(*fluor_args(c))
    out.setflags(write=False)
    return out


def as_real(a):
    """A complex array or tensor as a real one of shape (Z, Y, X, 2): the metrics of fft_metrics weigh real numbers."""
    if isinstance(a, torch.Tensor):
        return torch.view_as_real(a.contiguous())
    a = np.ascontiguousarray(a)
    return a.view(a.real.dtype).reshape(a.shape + (2,))


# ----------------------------------------------------------------------------- the float32 / complex64 restatement
def refinement(yx, dz, lamb, index, na_sum, na_det):
    """(yx factor, z factor) of waveorder's Nyquist rule; ``na_sum`` is NA_det + NA_ill (2 NA_det for fluorescence)."""
    tn = lamb / (2 * na_sum)
    nl = index / lamb
    an = 1.0 / (2 * (nl - np.sqrt(nl**2 - (na_det / lamb) ** 2)))
    return int(np.ceil(yx / tn)), int(np.ceil(dz / an))


def central_cuboid_c64(a, shape, split_floor=False):
    """nd_fourier_central_cuboid on a tensor.  ``split_floor``: a planted defect, the low block ends at n // 2."""
    for ax, n in enumerate(shape):
        N = a.shape[ax]
        lo = n // 2 if split_floor else (n + 1) // 2
        idx = torch.cat([torch.arange(lo), torch.arange(N - (n - lo), N)])
        a = a.index_select(ax, idx)
    return a.contiguous()


def _z_positions(zt, pz, invert, invert_after_shift):
    if invert and invert_after_shift:
        return np.fft.ifftshift(((np.arange(zt) - zt // 2) * pz)[::-1])
    return O.wo_z_positions(zt, pz, invert)


def _pupil(frr, cut, le, flip):
    p = (frr <= cut) if le else (frr < cut)
    if flip is not None:
        p = p.copy()
        p[flip] = ~p[flip]
    return p.astype(np.float64)


def _planes(frr, det, lamb, z, green, phases_f32):
    """det * exp(i 2 pi z ob), or with ``green`` the Green's function, formed in float64 and rounded to complex64 — as the
    kernel documents (the phases reach hundreds of radians).  ``phases_f32``: a planted defect, the phase formed in float32."""
    ob = O._wo_oblique(frr, det, lamb)
    zz = np.abs(z) if green else z
    if phases_f32:
        ph = (np.float32(2 * np.pi) * zz.astype(np.float32))[:, None, None] * ob.astype(np.float32)[None]
        e = (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex128)
    else:
        e = np.exp(2j * np.pi * zz[:, None, None] * ob[None])
    v = det[None] * e
    if green:
        v = -1j / (4 * np.pi) * v / (ob[None] + 1e-15)
    return torch.from_numpy(v.astype(np.complex64))


def window_f32(zt, periodic=False, shifted=True):
    """ifftshift(hann(zt)) in float32 arithmetic.  ``periodic`` and ``shifted=False``: planted defects."""
    if zt == 1:
        return torch.ones(1, dtype=torch.float32)
    k = np.arange(zt, dtype=np.float32)
    w = np.float32(0.5) - np.float32(0.5) * np.cos(np.float32(2 * np.pi) * k / np.float32(zt if periodic else zt - 1))
    assert w.dtype == np.float32
    return torch.from_numpy(np.fft.ifftshift(w) if shifted else w)


def phase_c64(c, phases_f32=False, pupil_le=False, periodic_window=False, unshifted_window=False, invert_after_shift=False,
              flip_det=None, cuboid_split_floor=False):
    """``phase_thick_3d.calculate_transfer_function`` restated in float32 / complex64 on the CPU (torch's FFTs): the pupils,
    the phases 2 pi z ob and the Green's function in float64 and rounded to float32, everything after that — the plane
    transforms, the products, the window, the z transform and the z_px / count factor — in complex64 and float32.  What a float32
    implementation of the definition gives: the yardstick of the bounds.  The keyword switches are planted defects."""
    Z, Y, X = c.shape
    yf, zf = refinement(c.yx, c.dz, c.lamb, c.index, c.na_det + c.na_ill, c.na_det)
    fz, fy, fx = Z * zf, Y * yf, X * yf
    px, pz = c.yx / yf, c.dz / zf
    frr = O.wo_radial_frequencies((fy, fx), px)
    zt = fz + 2 * c.pad
    z = _z_positions(zt, pz, c.invert, invert_after_shift)
    ill = _pupil(frr, c.na_ill / c.lamb, pupil_le, None)
    det = _pupil(frr, c.na_det / c.lamb, pupil_le, flip_det)
    lamb = c.lamb / c.index
    a = _planes(frr, det, lamb, z, False, phases_f32) * torch.from_numpy(ill.astype(np.float32))[None]
    b = _planes(frr, det, lamb, z, True, phases_f32) * torch.from_numpy(det.astype(np.float32))[None]
    assert a.dtype == b.dtype == torch.complex64
    sphz, pg = torch.fft.fft2(a), torch.fft.fft2(b)
    w = window_f32(zt, periodic_window, not unshifted_window)[:, None, None]
    h1 = torch.fft.fft(torch.fft.ifft2(sphz.conj() * pg) * w, dim=0)
    h2 = torch.fft.fft(torch.fft.ifft2(sphz * pg.conj()) * w, dim=0)
    count = float(np.sum(ill * ill * det * det))
    f = np.float32(pz) / np.float32(count)
    re, im = (h1 + h2) * f, 1j * ((h1 - h2) * f)
    assert re.dtype == im.dtype == torch.complex64
    out = (Z + 2 * c.pad, Y, X)
    return central_cuboid_c64(re, out, cuboid_split_floor), central_cuboid_c64(im, out, cuboid_split_floor)


def fluorescence_c64(c, phases_f32=False, pupil_le=False, flip_det=None):
    """``isotropic_fluorescent_thick_3d.calculate_transfer_function`` restated the same way: pupil and phases in float64,
    rounded; the plane transform, |.|^2, the 3-D transform and the division by the maximum in complex64 / float32."""
    Z, Y, X = c.shape
    yf, zf = refinement(c.yx, c.dz, c.lamb, c.index, 2 * c.na_det, c.na_det)
    fz, fy, fx = Z * zf, Y * yf, X * yf
    frr = O.wo_radial_frequencies((fy, fx), c.yx / yf)
    zt = fz + 2 * c.pad
    z = O.wo_z_positions(zt, c.dz / zf)
    det = _pupil(frr, c.na_det / c.lamb, pupil_le, flip_det)
    a = _planes(frr, det, c.lamb / c.index, z, False, phases_f32)
    psf = torch.fft.ifft2(a).abs() ** 2
    assert psf.dtype == torch.float32
    otf = torch.fft.fftn(psf.to(torch.complex64))
    otf = otf / otf.abs().max()
    assert otf.dtype == torch.complex64
    return central_cuboid_c64(otf, (Z + 2 * c.pad, Y, X))


def edge_bin(c):
    """The bin of the detection pupil nearest its cut-off from inside (the first in index order): flipping it is the
    smallest change one bin can make."""
    yf, _ = refinement(c.yx, c.dz, c.lamb, c.index, c.na_det + getattr(c, "na_ill", c.na_det), c.na_det)
    frr = O.wo_radial_frequencies((c.shape[1] * yf, c.shape[2] * yf), c.yx / yf)
    inside = np.where(frr < c.na_det / c.lamb, frr, -1.0)
    return tuple(int(i) for i in np.unravel_index(int(inside.argmax()), frr.shape))
