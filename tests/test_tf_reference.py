"""CPU: the float64 reference of compute-tf's transfer functions (oracle/oracle_np.py: wo_phase_transfer_function_3d,
wo_fluorescence_transfer_function_3d, wo_central_cuboid) and the bounds the GPU is held to in tests/test_gpu_tf_f64.py.

The oracle is held to what must be true of it; the pupil ties of tests/tf_cases.py are shown to be ties; the float32 / complex64
restatement of both functions is shown to sit inside a tenth of the bounds at every case of the GPU tests; and every planted
defect of the restatement is shown to fail them, with the factor by which it does (``-s`` shows the figures).
"""

import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from fft_metrics import RMS_TOL, TF_RMS_TOL, TF_VOXEL_TOL, TF_ZERO_RE_RATIO_TOL, assert_fft_close, fft_errors
from oracle import oracle_np as O
from tf_cases import (FLUOR_CASES, FLUOR_TIES, PHASE_CASES, PHASE_TIES, TIE1_CUT, TIE1_K, TIE2_BIN, TIE2_CUT, TIE_PLANE, TIE_YX,
                      as_real, case_id, central_cuboid_c64, edge_bin, fluorescence_c64, fluorescence_reference, phase_args,
                      phase_c64, phase_reference, real_potential_vanishes, refinement, total_planes)

SMALL = 200_000   # bins: the cases the property tests of the oracle run on

BY_NAME = {c.name: c for c in PHASE_CASES + PHASE_TIES}
FLUOR_BY_NAME = {c.name: c for c in FLUOR_CASES + FLUOR_TIES}


def small(cases):
    return [c for c in cases if math.prod(c.shape) <= SMALL]


def minus_k(a):
    """a(-k) in FFT order: every axis reversed about its bin 0."""
    for ax in range(a.ndim):
        a = np.roll(np.flip(a, ax), 1, ax)
    return a


def off_nyquist(shape):
    """Mask of the bins off the Nyquist planes of the even axes.  A central cuboid cut from a finer grid keeps, at index n / 2 of
    an even axis, the source's frequency -n / 2 alone, so that plane has no partner to be Hermitian with."""
    m = np.ones(shape, bool)
    for ax, n in enumerate(shape):
        if n % 2 == 0:
            idx = [slice(None)] * len(shape)
            idx[ax] = n // 2
            m[tuple(idx)] = False
    return m


def hermitian_defect(h, refined):
    d = np.abs(minus_k(h) - np.conj(h))
    if refined:
        d = d[off_nyquist(h.shape)]
    return float(d.max() / np.abs(h).max())


def phase_refined(c):
    return refinement(c.yx, c.dz, c.lamb, c.index, c.na_det + c.na_ill, c.na_det) != (1, 1)


def fluor_refined(c):
    return refinement(c.yx, c.dz, c.lamb, c.index, 2 * c.na_det, c.na_det) != (1, 1)


# ----------------------------------------------------------------------------- the oracle is what it must be
@pytest.mark.parametrize("c", small(FLUOR_CASES + FLUOR_TIES), ids=case_id)
def test_fluorescence_otf_is_one_at_dc_and_hermitian(c):
    """The PSF is real and non-negative: its spectrum is Hermitian and largest at DC, where the normalisation makes it 1."""
    h = fluorescence_reference(c)
    assert h.shape == (total_planes(c),) + c.shape[1:] and h.dtype == np.complex128
    assert abs(h[0, 0, 0] - 1.0) <= 1e-15
    assert np.abs(h).max() <= 1.0 + 1e-15
    assert hermitian_defect(h, fluor_refined(c)) <= 1e-14


@pytest.mark.parametrize("c", small(PHASE_CASES + PHASE_TIES), ids=case_id)
def test_phase_transfer_functions_are_hermitian(c):
    """Both potential transfer functions are spectra of real kernels: H(-k) = conj(H(k)) (off the Nyquist planes of a cut)."""
    re, im = phase_reference(c)
    assert re.shape == im.shape == (total_planes(c),) + c.shape[1:]
    scale = np.abs(im).max()
    for h in (re, im):
        assert hermitian_defect(h, phase_refined(c)) * np.abs(h).max() / scale <= 1e-14


@pytest.mark.parametrize("c", [c for c in PHASE_CASES + PHASE_TIES], ids=case_id)
def test_real_potential_vanishes_exactly_where_the_window_keeps_one_plane(c):
    """``real_potential_vanishes`` names the cases whose real-potential reference is rounding alone — Zt = 1, and Zt = 3, whose
    symmetric Hann window is (0, 1, 0) — and only those: everywhere else the two functions are of one order."""
    re, im = phase_reference(c)
    ratio = np.abs(re).max() / np.abs(im).max()
    if real_potential_vanishes(c):
        assert refinement(c.yx, c.dz, c.lamb, c.index, c.na_det + c.na_ill, c.na_det)[1] == 1
        assert ratio <= 1e-14, ratio
    else:
        assert ratio >= 0.1, ratio


def test_zt_two_has_no_reference():
    """Why no case has Zt = 2: its Hann window is identically zero, so both functions are."""
    re, im = O.wo_phase_transfer_function_3d((2, 8, 10), 0.1, 0.25, 0.45, 0, 1.3, 0.5, 1.2)
    assert not re.any() and not im.any()


@pytest.mark.parametrize("name", ["padded inverted even Zt", "all odd inverted", "odd Zt padded inverted", "native"])
def test_invert_phase_contrast_reverses_the_planes(monkeypatch, name):
    """``invert_phase_contrast`` reverses the array of z positions, so plane i of the stack before the z transform is plane
    Zt - 1 - i of the upright one — on odd and even Zt alike.  Without the window (which stays centred on index 0 and so does not
    move with the planes) that is, after the z transform, H_inv(kz) = exp(2 pi i kz / Zt) H(-kz): the non-DC planes reversed and
    the one-plane offset of a reversal about (Zt - 1) / 2 as a linear phase.  No relation without that phase holds: the
    inverted functions are neither the upright ones reversed nor their conjugates."""
    c = BY_NAME[name]
    zt = total_planes(c)
    inv, up = c._replace(invert=True), c._replace(invert=False)
    with_window = [O.wo_phase_transfer_function_3d(*phase_args(k)) for k in (inv, up)]
    monkeypatch.setattr(np, "hanning", lambda n: np.ones(n))
    (ire, iim), (ure, uim) = [O.wo_phase_transfer_function_3d(*phase_args(k)) for k in (inv, up)]
    monkeypatch.undo()
    ramp = np.exp(2j * np.pi * np.fft.fftfreq(zt))[:, None, None]   # fftfreq(zt) = kz / zt with kz signed: the ramp is exact at -kz too
    for got, upright in ((ire, ure), (iim, uim)):
        want = ramp * np.roll(upright[::-1], 1, 0)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    for (got, upright) in zip(*with_window):
        s = np.abs(upright).max()
        assert np.abs(got - np.roll(upright[::-1], 1, 0)).max() > 0.1 * s and np.abs(got - np.conj(upright)).max() > 0.1 * s


@pytest.mark.parametrize("name", ["native", "all odd inverted", "Zt 1"])
def test_refined_and_cut_is_direct_at_factor_one(name):
    """Where both factors are 1 the result is the construction itself: the cuboid of an array to its own shape is the array, and
    the functions equal the same construction written out without the refinement."""
    c = BY_NAME[name]
    assert not phase_refined(c)
    re, im = phase_reference(c)
    a = np.random.default_rng(3).standard_normal(re.shape)
    assert np.array_equal(O.wo_central_cuboid(a, a.shape), a)
    Z, Y, X = c.shape
    zt = Z + 2 * c.pad
    frr = O.wo_radial_frequencies((Y, X), c.yx)
    z = O.wo_z_positions(zt, c.dz, c.invert)
    ill, det = O.wo_pupil(frr, c.na_ill, c.lamb), O.wo_pupil(frr, c.na_det, c.lamb)
    s = np.fft.fft2(ill[None] * O.wo_propagation_kernel(frr, det, c.lamb / c.index, z), axes=(1, 2))
    p = np.fft.fft2(det[None] * O.wo_greens_function_z(frr, det, c.lamb / c.index, z), axes=(1, 2))
    w = np.fft.ifftshift(np.hanning(zt))[:, None, None] if zt > 1 else np.ones((1, 1, 1))
    h1 = np.fft.fft(np.fft.ifft2(np.conj(s) * p, axes=(1, 2)) * w, axis=0)
    h2 = np.fft.fft(np.fft.ifft2(s * np.conj(p), axes=(1, 2)) * w, axis=0)
    f = c.dz / np.sum(ill * det)
    scale = np.abs(im).max()
    assert np.abs(re - (h1 + h2) * f).max() <= 1e-14 * scale
    assert np.abs(im - 1j * (h1 - h2) * f).max() <= 1e-14 * scale


def test_central_cuboid_keeps_the_low_frequencies():
    """``wo_central_cuboid`` against its definition on frequencies: bin i of the target holds the source's bin of the same signed
    frequency, the odd target's extra bin on the positive side, the even target's Nyquist bin from the negative one."""
    src = np.arange(11 * 12).reshape(11, 12).astype(float)
    for shape in ((5, 7), (4, 6), (11, 12), (1, 1)):
        got = O.wo_central_cuboid(src, shape)
        assert got.shape == shape
        ky = [int(round(f * shape[0])) % 11 for f in np.fft.fftfreq(shape[0])]
        kx = [int(round(f * shape[1])) % 12 for f in np.fft.fftfreq(shape[1])]
        assert np.array_equal(got, src[np.ix_(ky, kx)])
        assert np.array_equal(central_cuboid_c64(torch.from_numpy(src), shape).numpy(), got)


# ----------------------------------------------------------------------------- the ties are ties
def test_tie_cases_sit_on_the_cut_off():
    """T1: the two fftfreq formulas differ at its bin, and the cut-off is the larger value: the bin is inside for one formula and
    outside for the other.  T2 / T3: the cut-off is the oracle's own frr at the bin — outside under ``<`` — while a fused
    multiply-add (exact product plus rounded product, rounded once: emulated in exact rationals) gives a sum whose root is
    below it: inside.  NA / wavelength reproduces the cut-off exactly, and nothing is refined."""
    nd = TIE_PLANE * TIE_YX
    a, b = TIE1_K / nd, TIE1_K * (1.0 / nd)
    assert a != b and TIE1_CUT == max(a, b)
    assert np.fft.fftfreq(TIE_PLANE, TIE_YX)[TIE1_K] == b == float(torch.fft.fftfreq(TIE_PLANE, TIE_YX, dtype=torch.float64)[TIE1_K])
    assert (min(a, b) < TIE1_CUT) and not (max(a, b) < TIE1_CUT)

    f = np.fft.fftfreq(TIE_PLANE, TIE_YX)
    fy, fx = float(f[TIE2_BIN[0]]), float(f[TIE2_BIN[1]])
    unfused = fx * fx + fy * fy
    assert math.sqrt(unfused) == TIE2_CUT == O.wo_radial_frequencies((TIE_PLANE, TIE_PLANE), TIE_YX)[TIE2_BIN]
    fused = [float(Fraction(p) ** 2 + Fraction(q * q)) for p, q in ((fx, fy), (fy, fx))]   # fma(p, p, q * q), either operand order
    print(f"tie T2: unfused {unfused!r} -> frr {math.sqrt(unfused)!r}; fused {fused[0]!r}, {fused[1]!r} -> frr "
          f"{math.sqrt(fused[0])!r}, {math.sqrt(fused[1])!r}")
    assert all(v != unfused for v in fused)
    assert all(math.sqrt(v) < TIE2_CUT for v in fused)

    for c in PHASE_TIES + FLUOR_TIES:
        assert c.na_det / c.lamb in (TIE1_CUT, TIE2_CUT) or c.na_ill / c.lamb == TIE2_CUT
        refined = phase_refined(c) if hasattr(c, "na_ill") else fluor_refined(c)
        assert not refined
    # the bin on the cut-off changes the pupil count: what scales every bin of the result
    frr = O.wo_radial_frequencies((TIE_PLANE, TIE_PLANE), TIE_YX)
    assert int((frr <= TIE2_CUT).sum()) - int((frr < TIE2_CUT).sum()) == 8


# ----------------------------------------------------------------------------- float32 is not the limit
def report(name, errs, extra=""):
    print(f"C64 {name}: rms_rel {errs[0]:.2e} voxel_rel {errs[1]:.2e} maxnorm {errs[2]:.2e} {extra}".rstrip())


@pytest.mark.parametrize("c", PHASE_CASES + PHASE_TIES, ids=case_id)
def test_phase_restatement_within_a_tenth_of_the_gpu_bounds(c):
    """The phase model in float32 / complex64 on the CPU against float64 at every case of the GPU tests: inside a tenth of the
    bounds the GPU is held to, each function on its own scale.  (Measured when written, over all cases: rms_rel
    8.7e-8 .. 3.9e-7, voxel_rel 1.8e-5 .. 3.0e-4; max|re| / max|im| where the real potential vanishes 0 .. 2.2e-7.)"""
    wre, wim = phase_reference(c)
    re, im = phase_c64(c)
    assert re.dtype == im.dtype == torch.complex64 and tuple(re.shape) == wre.shape
    report(f"tf phase imag {case_id(c)}", fft_errors(as_real(im), as_real(wim)))
    assert_fft_close(as_real(im), as_real(wim), TF_RMS_TOL / 10, TF_VOXEL_TOL / 10, "imaginary potential")
    if real_potential_vanishes(c):
        ratio = float(re.abs().max() / im.abs().max())
        print(f"C64 tf phase real {case_id(c)}: max|re| / max|im| {ratio:.2e}")
        assert ratio <= TF_ZERO_RE_RATIO_TOL / 10
    else:
        report(f"tf phase real {case_id(c)}", fft_errors(as_real(re), as_real(wre)))
        assert_fft_close(as_real(re), as_real(wre), TF_RMS_TOL / 10, TF_VOXEL_TOL / 10, "real potential")


@pytest.mark.parametrize("c", FLUOR_CASES + FLUOR_TIES, ids=case_id)
def test_fluorescence_restatement_within_a_tenth_of_the_gpu_bounds(c):
    """The fluorescence model the same way.  (Measured when written: rms_rel 1.0e-7 .. 2.3e-7, voxel_rel 4.3e-5 .. 5.3e-4.)"""
    want = fluorescence_reference(c)
    got = fluorescence_c64(c)
    assert got.dtype == torch.complex64 and tuple(got.shape) == want.shape
    report(f"tf fluorescence {case_id(c)}", fft_errors(as_real(got), as_real(want)))
    assert_fft_close(as_real(got), as_real(want), TF_RMS_TOL / 10, TF_VOXEL_TOL / 10, "fluorescence")
    assert abs(complex(got[0, 0, 0]) - 1.0) <= TF_VOXEL_TOL / 10
    assert float(got.abs().max()) <= 1.0 + 2.0 ** -23


# ----------------------------------------------------------------------------- planted defects
def factor_over_bounds(got, want):
    """By how much a result misses the GPU bounds: max over its functions of rms_rel / bound and voxel_rel / bound."""
    worst = 0.0
    for g, w in zip(got, want):
        rms, voxel, _ = fft_errors(as_real(g), as_real(w))
        worst = max(worst, rms / TF_RMS_TOL, voxel / TF_VOXEL_TOL)
    return worst


PHASE_DEFECTS = [
    ("phases_f32", {"phases_f32": True}, ["512 planes"]),
    ("pupil <=", {"pupil_le": True}, ["T2 detection cut on frr", "T3 illumination cut on frr"]),
    ("periodic window", {"periodic_window": True}, ["native", "odd Zt padded inverted", "volume loops wrap"]),
    ("window not shifted", {"unshifted_window": True}, ["native", "odd Zt padded inverted"]),
    ("inverted after the shift", {"invert_after_shift": True}, ["all odd inverted", "odd Zt padded inverted"]),
    ("one pupil bin flipped", "edge", ["native", "all odd inverted", "volume loops wrap"]),
    ("cuboid split at n // 2", {"cuboid_split_floor": True}, ["factors 2 and 2"]),
]
FLUOR_DEFECTS = [
    ("phases_f32", {"phases_f32": True}, ["512 planes"]),
    ("pupil <=", {"pupil_le": True}, ["T2 detection cut on frr"]),
    ("one pupil bin flipped", "edge", ["native", "volume loops wrap"]),
]


def _params(table):
    return [pytest.param(what, kw, name, id=f"{what} @ {name}") for what, kw, names in table for name in names]


@pytest.mark.parametrize("what,kw,name", _params(PHASE_DEFECTS))
def test_planted_phase_defect_fails_the_bounds(what, kw, name):
    """Each switch of the restatement is a slip a kernel could make; each misses the bounds the GPU is held to, and the
    restatement without it meets them ten times over (above).  The factor printed is miss / bound; the least, per defect,
    when written: float32 phases 6.9x at 512 planes (at the 35 planes of (35, 150, 202) that slip stays inside the bounds, 0.1x:
    its error grows with the depth, which is what the 512-plane case is for); ``<=`` in the pupil 2.9e4x; periodic window
    4.8e3x; unshifted window 2.6e5x; inversion after the shift 3.3e5x; one edge bin of the detection pupil flipped 423x at
    (35, 150, 202) (2e4x at the small shapes); cuboid split at n // 2 1.3e5x."""
    c = BY_NAME[name]
    if what == "inverted after the shift":
        assert c.invert and total_planes(c) % 2 == 1
    if what == "cuboid split at n // 2":
        assert phase_refined(c) and total_planes(c) % 2 == 1
    kw = {"flip_det": edge_bin(c)} if kw == "edge" else kw
    want = phase_reference(c)
    factor = factor_over_bounds(phase_c64(c, **kw), want)
    print(f"planted {what} @ {case_id(c)}: {factor:.3g}x the bounds")
    assert factor > 1.0


def test_inversion_and_shift_commute_on_an_even_zt():
    """Reversing the plane index before or after the half-length shift gives the same z positions when Zt is even (the shift is
    its own inverse and maps the reversal onto itself), so that slip can only show on an odd Zt — where it is planted above —
    and where Zt // 2 and (Zt + 1) // 2 differ.  The even inverted case guards the rest of the inversion."""
    from tf_cases import _z_positions

    for zt in (2, 4, 10):
        assert np.array_equal(_z_positions(zt, 0.25, True, True), _z_positions(zt, 0.25, True, False))
    for zt in (3, 5, 7):
        assert not np.array_equal(_z_positions(zt, 0.25, True, True), _z_positions(zt, 0.25, True, False))
    assert float(np.abs(np.subtract(*[np.asarray(phase_c64(BY_NAME["padded inverted even Zt"], invert_after_shift=s)[0])
                                      for s in (False, True)])).max()) == 0.0


@pytest.mark.parametrize("what,kw,name", _params(FLUOR_DEFECTS))
def test_planted_fluorescence_defect_fails_the_bounds(what, kw, name):
    """The same for the fluorescence model.  Least factors when written: float32 phases 3.5x (512 planes), ``<=`` 2.4e4x, one edge
    bin 385x at (35, 150, 202)."""
    c = FLUOR_BY_NAME[name]
    kw = {"flip_det": edge_bin(c)} if kw == "edge" else kw
    factor = factor_over_bounds([fluorescence_c64(c, **kw)], [fluorescence_reference(c)])
    print(f"planted {what} @ {case_id(c)}: {factor:.3g}x the bounds")
    assert factor > 1.0
