"""CPU: the float64 reference of the inverse filter (oracle/reference_f64.py: inverse_filter_f64, inverse_filter_bf16_f64) and
the bounds the GPU engine is held to in tests/test_gpu_invtf_f64.py.

The reference is held to the numpy oracle and to the Tikhonov reference; a float32 restatement of the operator is shown to
sit inside a tenth of the float32 bounds at every input of the GPU tests, and two float32 formulations of the staged bfloat16
filter inside a tenth of the bfloat16 bounds' own share; and planted defects show what the assertions of test_gpu_parity.py let
through and the new bounds do not.
"""

import numpy as np
import pytest
import torch

from conftest import rel_err
from fft_metrics import (INVTF_BF16_RMS_TOL, INVTF_BF16_VOXEL_TOL, INVTF_VOXEL_TOL, RMS_TOL, assert_fft_close, fft_errors)
from invtf_cases import (BF16_CASE, CASES, bf16_inputs, case_transfer_function, case_volume, float32_inputs,
                         inverse_filter_c64, transfer_function)
from oracle import oracle_np as O
from oracle import reference_f64 as R

FFT_TOL = 1e-4   # the max-normalised bound of tests/test_gpu_parity.py


def _padded(shape, pad):
    return (shape[0] + 2 * pad,) + tuple(shape[1:])


# ----------------------------------------------------------------------------- the reference is the definition
@pytest.mark.parametrize("kind", ["complex", "real", "real_even"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape,pad", [((5, 7, 9), 0), ((6, 8, 10), 0), ((5, 7, 9), 2), ((6, 8, 11), 3), ((4, 6, 9), 4),
                                       ((3, 7, 8), 5)])
def test_reference_equals_the_numpy_oracle(shape, pad, normalize, kind):
    """Odd and even shapes, pad 0, pad < Z (mirrored edge planes) and pad >= Z (zero planes), with and without normalisation, a
    complex H without symmetry, a real H without symmetry and a real even H: ``inverse_filter_f64`` (torch) is
    ``oracle_np.wo_apply_inverse_transfer_function`` before its float32 cast (numpy's pocketfft) to float64 rounding."""
    rng = np.random.default_rng(sum(shape) + pad)
    vol = rng.random(shape) * 50 + 100
    H = transfer_function(kind, _padded(shape, pad), 3).astype(np.float64 if kind != "complex" else np.complex128)
    for reg in (1e-2, 1e-3):
        want = O.wo_apply_inverse_transfer_function_f64(vol, H, pad, reg, normalize)
        got = R.inverse_filter_f64(vol, H, pad, reg, normalize).numpy()
        assert got.shape == want.shape == shape
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (reg, np.abs(got - want).max())
    zeros = R.inverse_filter_f64(vol, H, pad, 1e-3, normalize, mirror=False).numpy()
    assert np.array_equal(zeros, got) == (pad == 0 or pad >= shape[0])   # zero planes: what pad >= Z gives anyway


def test_minus_k_and_the_staged_filter():
    """``minus_k`` against explicit indices on odd and even axes; the staged value is Hermitian (F_h(-k) = conj(F_h(k))), is the
    Hermitian part of conj(H) / (|H|^2 + reg) to float32 rounding, and both float32 formulations agree to a few ulp."""
    shape = (4, 5, 6)
    H = torch.from_numpy(transfer_function("complex_offset", shape, 11))
    m = R.minus_k(H)
    for k in np.ndindex(*shape):
        assert m[k] == H[tuple((-i) % n for i, n in zip(k, shape))]
    fr, fi = R.staged_filter_f32(H, 1e-3, 0.25)
    assert fr.dtype == fi.dtype == torch.float32
    assert torch.equal(R.minus_k(fr), fr) and torch.equal(R.minus_k(fi), -fi)
    F = H.to(torch.complex128).conj() / (H.to(torch.complex128).abs() ** 2 + 1e-3)
    Fh = 0.5 * (F + R.minus_k(F).conj()) * 0.25
    assert float((torch.complex(fr.double(), fi.double()) - Fh).abs().max()) <= 4 * 2.0 ** -24 * float(Fh.abs().max())
    gr, gi = R.staged_filter_f32(H, 1e-3, 0.25, one_division=True)
    assert float((gr - fr).abs().max()) <= 4 * 2.0 ** -24 * float(fr.abs().max())
    assert float((gi - fi).abs().max()) <= 4 * 2.0 ** -24 * float(fi.abs().max())
    # a real H: the same through the float32 branch
    fr, fi = R.staged_filter_f32(torch.from_numpy(transfer_function("real", shape, 12)), 1e-3, 1.0)
    assert torch.equal(R.minus_k(fr), fr) and not bool(fi.any())


@pytest.mark.parametrize("shape,pshape", [((9, 12, 10), (3, 5, 4)), ((8, 7, 15), (4, 3, 5))])
def test_reference_with_a_hermitian_transfer_function_is_tikhonov(shape, pshape):
    """H = fftn of a real asymmetric PSF is Hermitian: the whole filter acts, and ``inverse_filter_f64`` is ``tikhonov_f64``."""
    rng = np.random.default_rng(21)
    vol = rng.random(shape) * 50 + 100
    psf = rng.random(pshape) + 0.1
    H = np.fft.fftn(psf / psf.sum(), shape, axes=(0, 1, 2))
    assert np.abs(H.imag).max() > 1e-2
    want = R.tikhonov_f64(vol, H, 1e-3)
    got = R.inverse_filter_f64(vol, H, 0, 1e-3, False)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_bf16_reference_rounds_the_scaled_value():
    """The bfloat16 reference differs from the exact filter by bfloat16's 8-bit mantissa; and the 2 / V scale belongs inside the
    rounding: on a box whose V is no power of two, rounding the unscaled F_h gives other values, on a power-of-two box
    it is the same rounding."""
    kind, reg, _ = BF16_CASE
    for shape, scale_matters in (((8, 32, 64), False), ((12, 48, 96), True)):
        vol, H = case_volume(shape), case_transfer_function(kind, shape)
        rms = fft_errors(R.inverse_filter_bf16_f64(vol, H, 0, reg), R.inverse_filter_f64(vol, H, 0, reg))[0]
        assert 2.0 ** -12 < rms < 2.0 ** -8, rms
        s = 2.0 / np.prod(shape)
        scaled = R.bf16_round(R.staged_filter_f32(H, reg, s)[0]).double() / s
        unscaled = R.bf16_round(R.staged_filter_f32(H, reg, 1.0)[0]).double()
        differ = float((scaled != unscaled).double().mean())
        assert (differ > 0.1) == scale_matters, (shape, differ)
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7 - 2.0 ** -20, -(1.0 + 3 * 2.0 ** -8)])
    assert R.bf16_round(t).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -6)]          # ties to even
    assert R.bf16_round(t, truncate=True).tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0, -(1.0 + 2.0 ** -7)]        # toward zero


# ----------------------------------------------------------------------------- float32 is not the limit
F32_INPUTS = float32_inputs()


@pytest.mark.parametrize("shape,pad", list(F32_INPUTS), ids=[f"{s}+{p}" for s, p in F32_INPUTS])
def test_float32_restatement_within_a_tenth_of_the_gpu_bounds(shape, pad):
    """The operator in float32 / complex64 on the CPU against float64 at every input the GPU tests run in float32 storage: inside
    a tenth of the bounds the engine is held to.  (Measured when written, over all inputs: rms_rel 1.0e-7 .. 3.2e-7, voxel_rel up
    to 5.4e-4 — (30, 160, 320) + pad 5, 1 + 0.3 (N + iN), normalised; maxnorm <= 3.9e-7.)"""
    vol = case_volume(shape)
    for kind, reg, normalize in F32_INPUTS[(shape, pad)]:
        H = case_transfer_function(kind, _padded(shape, pad))
        ref = R.inverse_filter_f64(vol, H, pad, reg, normalize)
        got = inverse_filter_c64(vol, H, pad, reg, normalize)
        assert got.dtype == torch.float32
        assert_fft_close(got, ref, RMS_TOL / 10, INVTF_VOXEL_TOL / 10, f"float32 restatement {kind} reg {reg} norm {normalize}")


BF16_INPUTS = bf16_inputs()


@pytest.mark.parametrize("shape,pad,normalize", BF16_INPUTS, ids=[f"{s}+{p} norm {int(n)}" for s, p, n in BF16_INPUTS])
def test_bf16_staging_formulations_within_a_tenth_of_the_bf16_share(shape, pad, normalize):
    """What the bfloat16 bounds add to the float32 ones is 10x the distance between two float32 formulations of the staged value
    (reciprocal-then-multiply, as the kernel, against one division), each rounded to bfloat16: the bins that fall on the other
    side of a rounding boundary.  (Measured when written: rms_rel 4e-11 .. 2.1e-5, voxel_rel up to 5.7e-3.)"""
    kind, reg, _ = BF16_CASE
    vol, H = case_volume(shape), case_transfer_function(kind, _padded(shape, pad))
    a = R.inverse_filter_bf16_f64(vol, H, pad, reg, normalize)
    b = R.inverse_filter_bf16_f64(vol, H, pad, reg, normalize, one_division=True)
    assert_fft_close(b, a, (INVTF_BF16_RMS_TOL - RMS_TOL) / 10, (INVTF_BF16_VOXEL_TOL - INVTF_VOXEL_TOL) / 10, "two formulations")


# ----------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize("shape,pad", [((16, 32, 64), 0), ((8, 64, 1024), 0), ((24, 96, 192), 0), ((40, 160, 320), 0),
                                       ((20, 96, 192), 2)])
def test_planted_bf16_truncation_passes_the_old_assertion_and_fails_the_bounds(shape, pad):
    """bfloat16 by truncation instead of round-to-nearest-even, planted in the reference itself.  It passes what
    test_apply_inverse_transfer_function_vs_oracle asserted of the bfloat16 path, ``1e-7 < rel_err(vs exact) <= 1e-2``, and
    fails the bounds against ``inverse_filter_bf16_f64``; the defect-free rounding passes them exactly.
    (Measured when written, rms / voxel / maxnorm against the bf16 reference, then the old metric against the exact filter:
    (16, 32, 64) 3.0e-3 / 4.6e-1 / 2.7e-3, 2.7e-3; (8, 64, 1024) 1.3e-3 / 7.8e-3 / 2.7e-3, 2.7e-3; (24, 96, 192)
    1.0e-3 / 5.2e-3 / 2.8e-3, 2.9e-3; (40, 160, 320) 8.4e-4 / 4.1e-3 / 2.7e-3, 2.7e-3; (20, 96, 192) + pad 2 9.7e-4 / 4.9e-3 / 2.8e-3,
    2.9e-3; over every bfloat16 input of the GPU tests rms_rel 8.4e-4 .. 7.1e-3 — at least 3.8x the rms bound —
    and the old metric 2.7e-3 .. 3.0e-3.)"""
    kind, reg, normalize = BF16_CASE
    vol, H = case_volume(shape), case_transfer_function(kind, _padded(shape, pad))
    exact = R.inverse_filter_f64(vol, H, pad, reg, normalize)
    ref16 = R.inverse_filter_bf16_f64(vol, H, pad, reg, normalize)
    bad = R.inverse_filter_bf16_f64(vol, H, pad, reg, normalize, truncate=True)
    print(f"planted truncation {shape}+{pad}: " + " / ".join(f"{e:.1e}" for e in fft_errors(bad, ref16))
          + f"; old metric {rel_err(bad.numpy(), exact.numpy()):.1e}")
    assert 1e-7 < rel_err(bad.numpy(), exact.numpy()) <= 1e-2
    assert 1e-7 < rel_err(ref16.numpy(), exact.numpy()) <= 1e-2      # the old assertion cannot tell the two apart
    with pytest.raises(AssertionError, match="worst voxel"):
        assert_fft_close(bad, ref16, INVTF_BF16_RMS_TOL, INVTF_BF16_VOXEL_TOL, "truncation")
    assert fft_errors(bad, ref16)[0] > 3 * INVTF_BF16_RMS_TOL


@pytest.mark.parametrize("shape", [(8, 32, 1536), (24, 96, 192), (8, 64, 512)])
def test_planted_running_sum_mean_passes_rel_err_and_fails_the_bounds(shape):
    """The mean of ``x / mean - 1`` from a sequential float32 sum (what a one-thread-per-row accumulation without a float64
    or pairwise finish gives), planted in the float32 restatement: it shifts every voxel by the bias of the mean times the
    filter's gain at frequency 0.  It passes ``rel_err <= 1e-4`` (test_apply_inverse_transfer_function_vs_oracle) and fails
    the new bounds, which the same restatement with a float64 mean meets ten times over.
    (Measured when written, rms / voxel / maxnorm: (8, 32, 1536) 1.9e-5 / 1.7e-3 / 1.3e-5; (24, 96, 192) 5.8e-5 / 5.7e-3 / 2.2e-5;
    (8, 64, 512) 1.8e-5 / 1.7e-3 / 1.0e-5.)"""
    kind, reg, normalize = CASES["complex"]
    assert normalize
    vol, H = case_volume(shape), case_transfer_function(kind, shape)
    ref = R.inverse_filter_f64(vol, H, 0, reg, True)
    bad = inverse_filter_c64(vol, H, 0, reg, True, mean_f32_running_sum=True)
    print(f"planted running-sum mean {shape}: " + " / ".join(f"{e:.1e}" for e in fft_errors(bad, ref)))
    assert rel_err(bad.numpy(), ref.numpy()) <= FFT_TOL
    with pytest.raises(AssertionError, match="worst voxel"):
        assert_fft_close(bad, ref, RMS_TOL, INVTF_VOXEL_TOL, "running-sum mean")
    assert_fft_close(inverse_filter_c64(vol, H, 0, reg, True), ref, RMS_TOL / 10, INVTF_VOXEL_TOL / 10, "float64 mean")
