"""CPU: the float64 reference of phase cross-correlation (oracle/reference_f64.py: phase_cross_corr_f64) and the bounds the GPU
paths are held to in tests/test_gpu_pcc_f64.py.

The reference is held to the numpy definition; every input of the GPU tests is shown to have one peak no float32 path can
miss and spectra without an empty bin; a complex64 restatement of the operator is shown to sit inside a tenth of the bounds at
every one of them; and planted defects show what the assertions of test_gpu_parity.py (equal shift, ``rel_err <= 1e-4``) let
through and the new bounds do not.
"""

import numpy as np
import pytest
import torch

import pcc_cases as P
from conftest import rel_err
from fft_metrics import PCC_NORM_RMS_TOL, assert_fft_close, fft_errors, pcc_bounds
from oracle import oracle_np as O
from oracle import reference_f64 as R

FFT_TOL = 1e-4    # the max-normalised bound of tests/test_gpu_parity.py
PEAK_GAP = 1e-2   # condition 1: the runner-up voxel lies at least this fraction of the peak below the peak
# condition 3: pcc_cases.weak_bin of a pair that runs normalised.  A bin of magnitude m carries a rounding error of about
# eps x median |F| (eps = 6e-8), relative eps x median / m; normalised to unit weight it adds eps x median / (m sqrt(n)) =
# eps / weak_bin to rms_rel.  At 0.03 that is 2e-6, what all the other bins together give (8e-7 .. 2.6e-6): below it one bin
# sets the error, above it none does.  (Measured: 0.040 at the least.)
WEAK_BIN = 0.03


# ----------------------------------------------------------------------------- the reference is the definition
@pytest.mark.parametrize("norm", P.NORMS)
@pytest.mark.parametrize("shape", [(5, 7, 9), (6, 8, 10), (4, 6, 11), (7, 5, 8), (2, 3, 2)])
def test_reference_equals_the_numpy_definition(shape, norm):
    """Tiny odd and even shapes, odd X included (the volume comes back one column short), three normalisations:
    ``phase_cross_corr_f64`` (torch, one axis per transform) is ``oracle_np.phase_cross_corr_f64`` (numpy's pocketfft, rfftn /
    irfftn) to float64 rounding, shifts equal — among them shifts of exactly n // 2, which the sign rule leaves positive on an
    even axis and wraps on an odd one.  The complex64 restatement is the float32 oracle to float32 rounding."""
    rng = np.random.default_rng(sum(shape))
    ref = rng.random(shape) * 50 + 100
    for roll in ((0, 0, 0), tuple(n // 2 for n in shape), (1, -2, 1)):
        mov = np.roll(ref, roll, axis=(0, 1, 2)) + 0.5 * rng.random(shape)
        want_shift, want = O.phase_cross_corr_f64(ref, mov, norm)
        got_shift, got = R.phase_cross_corr_f64(ref, mov, norm)
        assert got.dtype == torch.float64 and tuple(got.shape) == want.shape == shape[:2] + (shape[2] - (shape[2] & 1),)
        assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max(), (roll, np.abs(got.numpy() - want).max())
        assert np.array_equal(got_shift, want_shift), (roll, got_shift, want_shift)
        if norm == "magnitude" and not shape[2] & 1:
            peak = [(-r) % n for r, n in zip(roll, shape)]
            assert np.array_equal(got_shift, [i - n if i > n // 2 else i for i, n in zip(peak, shape)]), (roll, got_shift)
        s32, c32 = P.phase_cross_corr_c64(ref, mov, norm)
        o32, oc32 = O.phase_cross_corr(ref, mov, norm)
        assert np.array_equal(s32, o32) and rel_err(c32.numpy(), oc32) <= 1e-5


def test_reference_on_an_all_zero_pair_and_bad_arguments():
    """Zeros: shift (0, 0, 0); exact zeros for None and magnitude (0 / eps), NaN for classic (0 / 0) — as the definition."""
    z = np.zeros((4, 6, 8), np.float32)
    for norm in P.NORMS:
        with np.errstate(invalid="ignore", divide="ignore"):
            want_shift, want = O.phase_cross_corr(z, z, norm)
        shift, corr = R.phase_cross_corr_f64(z, z, norm)
        assert np.array_equal(shift, want_shift) and np.array_equal(shift, [0, 0, 0])
        assert np.array_equal(corr.numpy(), want, equal_nan=True)
        assert bool(torch.isnan(corr).all()) == (norm == "classic")
    assert R.PCC_EPS == 1.1920929e-07 and np.float32(R.PCC_EPS) == np.finfo(np.complex64).eps
    with pytest.raises(ValueError):
        R.phase_cross_corr_f64(z, z[:-1], None)
    with pytest.raises(ValueError):
        R.phase_cross_corr_f64(z, z, "l2")


# ----------------------------------------------------------------------------- the inputs, and float32 is not the limit
SHAPES = P.all_shapes()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_inputs_are_well_posed_and_the_restatement_is_within_a_tenth_of_the_bounds(shape):
    """Every input the GPU tests run at ``shape`` — one float64 and one complex64 evaluation each:
      1. the float64 correlation's runner-up voxel lies at least 1e-2 of the peak below the peak, so no float32 path can
         legitimately return another shift (the restatement returns the same one);
      2. where "classic" runs, no bin of either spectrum is zero, so it is finite;
      3. where a normalised mode runs, the weakest bin is not far below an ordinary one (``pcc_cases.weak_bin``);
    and the restatement lies within a tenth of the bounds of tests/fft_metrics.py.
    (Measured when written, over all inputs: gap 1.95e-2 at the least — (9, 14, 31), half shift, None; >= 4.6e-2 on the engine
    shapes for None with the offset, 0.62 mean-removed, 0.97 normalised.  Errors: the derivation in tests/fft_metrics.py.)"""
    for name, ref, mov, classes in P.cpu_inputs(shape):
        if any(norm is not None for norm, _ in classes):
            F1, F2 = (R.rfftn_by_axis(torch.from_numpy(x).double()) for x in (ref, mov))
            assert float(torch.minimum(F1.abs().min(), F2.abs().min())) > 0.0, name
            assert P.weak_bin(F1, F2) >= WEAK_BIN, (name, P.weak_bin(F1, F2))
            del F1, F2
        for norm, removed in classes:
            a, b = P.class_inputs(ref, mov, removed)
            shift, corr = R.phase_cross_corr_f64(a, b, norm)
            top = torch.topk(corr.reshape(-1), 2).values
            gap = float((top[0] - top[1]) / top[0])
            assert bool(torch.isfinite(corr).all()) and gap >= PEAK_GAP, (name, norm, removed, gap)
            shift32, corr32 = P.phase_cross_corr_c64(a, b, norm)
            assert np.array_equal(shift32, shift), (name, norm, removed, shift32, shift)
            zero_mean = removed or not name.startswith("shift") and not name.startswith("chain")
            rms, voxel = pcc_bounds(norm, zero_mean)
            assert_fft_close(corr32, corr, rms / 10, voxel / 10, f"complex64 restatement, {name} {norm} removed {removed}")


def test_restatement_at_the_inputs_of_the_older_gpu_tests():
    """The pairs whose volumes test_gpu_parity.py's three phase cross-correlation tests now hold to the reference (uniform
    random volumes and the goldens): the restatement within a tenth of ``pcc_bounds(norm, white=True)``, finite everywhere.
    Where the two images are related the peak stands 0.2 (None) to 0.99 (normalised) above the runner-up; the first two
    volumes of the handle test are unrelated, their correlation has no peak, and there only the volumes are compared."""
    for name, ref, mov in P.parity_inputs():
        related = name not in ("prepared 0-1", "prepared 1-2")
        for norm in P.NORMS:
            shift, corr = R.phase_cross_corr_f64(ref, mov, norm)
            shift32, corr32 = P.phase_cross_corr_c64(ref, mov, norm)
            assert bool(torch.isfinite(corr).all())
            if related:
                top = torch.topk(corr.reshape(-1), 2).values
                assert float((top[0] - top[1]) / top[0]) >= PEAK_GAP and np.array_equal(shift32, shift), (name, norm)
            rms, voxel = pcc_bounds(norm, white=True)
            assert_fft_close(corr32, corr, rms / 10, voxel / 10, f"complex64 restatement, {name} {ref.shape} {norm}")


# ----------------------------------------------------------------------------- planted defects
def _planted(shape, k, norm, removed, defect):
    a, b = P.class_inputs(*P.pair(shape, k), removed)
    shift, corr = R.phase_cross_corr_f64(a, b, norm)
    bad_shift, bad = P.phase_cross_corr_c64(a, b, norm, defect)
    errs = fft_errors(bad, corr)
    rms, voxel = pcc_bounds(norm, removed)
    print(f"planted {defect} {shape} shift {k} {norm} removed {int(removed)}: rms {errs[0]:.2e} ({errs[0] / rms:.1f}x) "
          f"voxel {errs[1]:.2e} ({errs[1] / voxel:.1f}x) maxnorm {errs[2]:.2e}")
    return shift, corr, bad_shift, bad, errs, (rms, voxel)


def _passes_old_fails_new(shape, k, norm, removed, defect, factor):
    """The old assertion (equal shift, rel_err <= 1e-4) passes; the new bounds fail, rms or voxel by at least ``factor``."""
    shift, corr, bad_shift, bad, errs, (rms, voxel) = _planted(shape, k, norm, removed, defect)
    assert np.array_equal(bad_shift, shift) and rel_err(bad.numpy(), corr.numpy()) <= FFT_TOL
    with pytest.raises(AssertionError, match="worst voxel"):
        assert_fft_close(bad, corr, rms, voxel, defect)
    assert max(errs[0] / rms, errs[1] / voxel) >= factor, errs


@pytest.mark.parametrize("shape", [(8, 64, 512), (24, 96, 192)])
def test_planted_column_without_the_conjugate(shape):
    """One (y, kx) column of the spectrum — what one thread column of the Z pass holds — multiplied as F1 F2.  With magnitude
    normalisation and on the mean-removed None pair it passes the old assertion (maxnorm 3.6e-5 .. 8.3e-5) and fails the rms
    bound 320x at the least (None: 1000x).  On the None pair WITH its camera offset it passes the new bounds too (0.3x .. 0.8x):
    the DC term hides one column among 10^5 from any metric, which is why every None case also runs mean-removed."""
    for k in (0, 2):
        _passes_old_fails_new(shape, k, "magnitude", False, "column_no_conj", 300)
        _passes_old_fails_new(shape, k, None, True, "column_no_conj", 1000)
        _, corr, _, bad, _, bounds = _planted(shape, k, None, False, "column_no_conj")
        assert_fft_close(bad, corr, *bounds, "hidden under DC")


def test_planted_dropped_nyquist_column():
    """The last column of the half spectrum left out, None on the camera pair at (8, 64, 512): maxnorm 7.8e-5 passes the old
    assertion; the new bounds fail it 1.9x (rms) and 4.2x (voxel) — not the 10x one would like: one column in 257 of a
    spectrum that DC dominates.  The mean-removed pair of the same images fails 4800x (and the old assertion too, at 1e-3)."""
    _passes_old_fails_new((8, 64, 512), 0, None, False, "drop_nyquist", 4)
    _passes_old_fails_new((8, 64, 512), 2, None, False, "drop_nyquist", 4)
    _, _, _, _, errs, (rms, _) = _planted((8, 64, 512), 2, None, True, "drop_nyquist")
    assert errs[0] >= 1000 * rms


@pytest.mark.parametrize("norm,removed", P.CLASSES)
def test_planted_swap_on_the_wrong_factor(norm, removed):
    """conj(F1) F2 instead of F1 conj(F2) (``pcc_swap`` inverted): the volume is mirrored about the origin.  With the mixed
    shift the shift comes back negated and the shift check catches it; with no shift the peak stays at the origin, the shift
    check cannot see it, and the volume bounds do (6x on the camera None pair, 10^4 x elsewhere)."""
    shape = (8, 64, 512)
    shift, corr, bad_shift, bad, errs, (rms, voxel) = _planted(shape, 2, norm, removed, "swap")
    assert bool(shift.any()) and np.array_equal(bad_shift, -shift) and not np.array_equal(bad_shift, shift)
    shift, corr, bad_shift, bad, errs, (rms, voxel) = _planted(shape, 0, norm, removed, "swap")
    assert np.array_equal(bad_shift, shift)
    with pytest.raises(AssertionError, match="worst voxel"):
        assert_fft_close(bad, corr, rms, voxel, "swap, no shift")
    assert max(errs[0] / rms, errs[1] / voxel) >= 6


@pytest.mark.parametrize("norm", ["magnitude", "classic"])
@pytest.mark.parametrize("shape", [(8, 64, 512), (16, 32, 320), (24, 96, 192)])
def test_planted_normalisation_good_to_1e_4(shape, norm):
    """Every bin's normalisation off by up to 1e-4, relative (uniform): maxnorm 5e-7 .. 8e-7, two hundred times inside the old
    assertion; rms_rel 5.8e-5 at every shape, 1.9x the rms bound — not 10x: the bound is ten times what float32 itself does
    with the weak bins (2.6e-6), and a defect of 5.8e-5 per bin is only 22x that.  voxel_rel 1.6e-2 .. 2.1e-2 stays inside its
    bound (0.3x)."""
    shift, corr, bad_shift, bad, errs, (rms, voxel) = _planted(shape, 2, norm, False, "norm_1e-4")
    assert np.array_equal(bad_shift, shift) and rel_err(bad.numpy(), corr.numpy()) <= FFT_TOL / 100
    with pytest.raises(AssertionError, match="worst voxel"):
        assert_fft_close(bad, corr, rms, voxel, "normalisation to 1e-4")
    assert rms == PCC_NORM_RMS_TOL and errs[0] >= 1.8 * rms
