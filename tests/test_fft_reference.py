"""CPU: the float64 FFT reference (oracle/reference_f64.py) and the per-voxel metrics (tests/fft_metrics.py) the GPU FFT
engine is judged by in tests/test_gpu_f64_parity.py.

The reference is held to the definition (a spatial-domain restatement, no FFT) and to a numpy restatement; the float32 oracle is
shown not to be the limiting factor; and planted defects show what the max-normalised ``rel_err <= 1e-4`` of the older tests
lets through and the new bounds do not.
"""

import numpy as np
import pytest
import torch

from conftest import rel_err
from fft_metrics import RMS_TOL, TIK_VOXEL_TOL, VOXEL_TOL, assert_fft_close, fft_errors
from oracle import oracle_np as O
from oracle import reference_f64 as R

FFT_TOL = 1e-4   # the max-normalised bound of tests/test_gpu_parity.py


def bench_like(shape, seed=1, n_beads=64, z_margin=10):
    """Camera-like volume as bench.synthetic_position makes it (offset 110 + N(0, 4) noise + 7-voxel beads of 200..4000
    counts, rounded), on the host; beads stay ``z_margin`` planes away from the z faces."""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    v = rng.normal(110.0, 4.0, shape)
    zz, yy, xx = rng.integers(z_margin, Z - z_margin, n_beads), rng.integers(2, Y - 2, n_beads), rng.integers(2, X - 2, n_beads)
    amp = rng.random(n_beads) * 3800 + 200
    for dz, dy, dx, w in ((0, 0, 0, 1.0), (1, 0, 0, 0.6), (-1, 0, 0, 0.6), (0, 1, 0, 0.6), (0, -1, 0, 0.6), (0, 0, 1, 0.6),
                          (0, 0, -1, 0.6)):
        np.add.at(v, (zz + dz, yy + dy, xx + dx), amp * w)
    return np.clip(np.round(v), 0, 65535).astype(np.float32)


BENCH_PSF = O.gaussian_psf((33, 17, 17), (3.0, 1.5, 1.5))


@pytest.fixture(scope="module")
def bench_case():
    d = bench_like((64, 128, 128))
    return d, R.richardson_lucy_f64(d, BENCH_PSF, 10, 1e-6)


def _spatial_rl(d, psf, iterations, eps):
    """The definition with circular convolution / correlation as sums of rolled copies (tap k at offset k - K // 2)."""
    h = psf / psf.sum()

    def conv(x, flip):
        out = np.zeros_like(x)
        for k in np.ndindex(*psf.shape):
            off = tuple(ki - K // 2 for ki, K in zip(k, psf.shape))
            out += h[k] * np.roll(x, tuple(-o if flip else o for o in off), axis=(0, 1, 2))
        return out

    est = np.maximum(d, 0.0)
    for _ in range(iterations):
        est = np.maximum(est * conv(d / np.maximum(conv(est, False), eps), True), 0.0)
    return est


@pytest.mark.parametrize("shape,pshape", [((6, 7, 9), (3, 3, 5)), ((5, 8, 6), (2, 4, 3)), ((4, 4, 4), (3, 1, 2)),
                                          ((7, 6, 10), (1, 3, 1)), ((6, 8, 9), (1, 4, 3)),
                                          ((8, 9, 8), (4, 5, 6))])
def test_reference_equals_spatial_restatement(shape, pshape):
    """Odd, even and unit PSF extents: the FFT reference is the circular R-L of the definition to float64 rounding, including
    the centre convention and the e0 clamp of negative data."""
    rng = np.random.default_rng(sum(shape) + sum(pshape))
    d = rng.random(shape) * 50 + 5
    d[0, 0, 0] = -3.0
    psf = rng.random(pshape) + 0.1
    want = _spatial_rl(d, psf, 4, 1e-6)
    got = R.richardson_lucy_f64(d, psf, 4, 1e-6).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (shape, pshape, np.abs(got - want).max())
    ck = dict(R.richardson_lucy_f64_checkpoints(d, psf, (0, 1, 4), 1e-6))   # the checkpoint form is the same run
    assert np.array_equal(ck[4].numpy(), got)


def test_reference_torch_equals_numpy():
    """The torch reference on the CPU against a numpy float64 restatement (numpy's pocketfft, not torch's): R-L with a complex
    and with a real transfer function, and Tikhonov with a real transfer function."""
    rng = np.random.default_rng(7)
    d = (rng.random((12, 20, 18)) * 200 + 10).astype(np.float32)
    d[3, 4, 5] = -1.0
    for psf in (O.gaussian_psf((5, 7, 3), (1.0, 1.5, 0.8)), O.gaussian_psf((4, 7, 3), (1.0, 1.5, 0.8))):
        psf = psf.copy()
        if psf.shape[0] == 5:
            psf[0, 0, 0] += 0.01   # asymmetric: complex transfer function
        h = psf.astype(np.float64) / psf.astype(np.float64).sum()
        padded, before = O.pad_psf(h, d.shape)
        otf = np.fft.rfftn(np.roll(padded, [-(b + k // 2) for b, k in zip(before, psf.shape)], axis=(0, 1, 2)))
        dd = d.astype(np.float64)
        est = np.maximum(dd, 0.0)
        for _ in range(6):
            blur = np.fft.irfftn(otf * np.fft.rfftn(est), s=d.shape, axes=(0, 1, 2))
            est = np.maximum(est * np.fft.irfftn(np.conj(otf) * np.fft.rfftn(dd / np.maximum(blur, 1e-6)), s=d.shape, axes=(0, 1, 2)), 0.0)
        got = R.richardson_lucy_f64(d, psf, 6, 1e-6).numpy()
        assert np.abs(got - est).max() <= 1e-12 * np.abs(est).max()
    sym = O.gaussian_psf((5, 7, 3), (1.0, 1.5, 0.8))
    assert R.psf_is_point_symmetric(sym) and not R.rl_otf_f64(sym, d.shape).is_complex()
    assert np.abs(R.richardson_lucy_f64(d, sym, 6).numpy()
                  - R.richardson_lucy_f64(d, sym, 6, device="cpu").numpy()).max() == 0.0
    H = O.compute_transfer_function(sym, d.shape)
    want = np.real(np.fft.ifftn(np.fft.fftn(d.astype(np.float64)) * np.conj(H.astype(np.float64)) / (H.astype(np.float64) ** 2 + 1e-3)))
    got = R.tikhonov_f64(d, H, 1e-3).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_float32_oracle_within_a_tenth_of_the_gpu_bounds(bench_case):
    """The float32 oracle (complex64 scipy FFTs) against float64, R-L 10 iterations on a bench-like volume with the bench PSF,
    and Tikhonov: inside a tenth of the bounds the GPU engine is held to, so the oracle is not what limits the older tests.
    (Measured when written, rms / voxel / maxnorm: R-L 3.4e-7 / 1.7e-6 / 5.5e-7; Tikhonov reg 1e-3 2.2e-7 / 8.7e-5 / 1.9e-7,
    reg 1e-2 1.4e-7 / 4.4e-5 / 1.7e-7 — the inverse filter rings through zero, hence its own voxel bound.)"""
    d, ref = bench_case
    o = O.richardson_lucy_zyx(d, BENCH_PSF, 10, 1e-6)
    assert_fft_close(o, ref, RMS_TOL / 10, VOXEL_TOL / 10, "float32 oracle, R-L")
    H = O.compute_transfer_function(BENCH_PSF, d.shape)
    for reg in (1e-3, 1e-2):
        assert_fft_close(O.tikhonov_zyx(d, H, reg), R.tikhonov_f64(d, H, reg), RMS_TOL / 10, TIK_VOXEL_TOL / 10,
                         f"float32 oracle, Tikhonov {reg}")


def _rl_planted(d, psf, iterations, defect):
    """The float64 reference with one planted defect (the kind a kernel could carry without the max-normalised metric noticing)."""
    d = torch.from_numpy(d)
    otf = R.rl_otf_f64(psf, d.shape, real=False)
    est = d.double().clamp(min=0.0)
    Z = d.shape[0]
    for _ in range(iterations):
        blur = R.conv_f64(est, otf)
        if defect == "wrap_face":
            # the convolution's circular wrap along z reads plane Z-2 where it should read the face plane Z-1: output planes of
            # the lower half reach plane Z-1 only across the wrap (the PSF is shorter than Z / 2)
            e2 = est.clone()
            e2[-1] = e2[-2]
            blur[: Z // 2] = R.conv_f64(e2, otf)[: Z // 2]
        ratio = d / blur.clamp(min=1e-6)
        if defect == "dim_ratio_bias":
            ratio = torch.where(d < 200, ratio * (1 + 1e-4), ratio)   # e.g. an approximate reciprocal on one kernel family
        corr = R.conv_f64(ratio, otf) if defect == "otf_not_conj" else R.corr_f64(ratio, otf)
        est = (est * corr).clamp(min=0.0)
    return est


@pytest.mark.parametrize("defect", ["dim_ratio_bias", "wrap_face", "otf_not_conj"])
def test_planted_defect_passes_rel_err_and_fails_the_bounds(defect, bench_case):
    """The record of the gap: each defect, applied to the float64 reference itself, passes ``rel_err <= 1e-4`` (what every R-L
    test of test_gpu_parity.py asserts) and fails ``assert_fft_close`` at the bounds test_gpu_f64_parity.py uses.
    (Measured when written, rms / voxel / maxnorm: dim_ratio_bias 8.4e-5 / 1.7e-4 / 1.6e-5; wrap_face 3.0e-4 / 6.1e-3 / 6.8e-5;
    otf_not_conj 7.0e-5 / 4.9e-3 / 5.5e-5.)"""
    d, ref = bench_case
    psf = BENCH_PSF
    if defect == "otf_not_conj":
        psf = BENCH_PSF.copy()
        psf[0, 0, 0] += 0.005 * psf.max()   # slightly asymmetric: conj(otf) != otf
        ref = R.richardson_lucy_f64(d, psf, 10, 1e-6)
    bad = _rl_planted(d, psf, 10, defect)
    assert rel_err(bad.numpy(), ref.numpy()) <= FFT_TOL
    with pytest.raises(AssertionError, match="worst voxel"):
        assert_fft_close(bad, ref, RMS_TOL, VOXEL_TOL, defect)
    # and the defect-free run of the same code passes them with room
    rms, vox, _ = fft_errors(_rl_planted(d, psf, 10, None), ref)
    assert rms <= 1e-12 and vox <= 1e-12


def test_fft_errors_metrics():
    """The three numbers on a hand-made case, a 2-D plane, and the message of a failure."""
    ref = np.full((2, 3, 4), 100.0)
    ref[0, 0, 0] = 1000.0
    ref[1, 2, 3] = 0.0
    got = ref.copy()
    got[1, 1, 1] += 0.5
    got[1, 2, 3] = 0.25
    rms_ref = np.sqrt((ref ** 2).mean())
    rms_rel, voxel_rel, maxnorm = fft_errors(torch.from_numpy(got).float(), torch.from_numpy(ref))
    assert rms_rel == pytest.approx(np.sqrt(0.5 ** 2 + 0.25 ** 2) / np.linalg.norm(ref), rel=1e-12)
    assert voxel_rel == pytest.approx(0.25 / (0.01 * rms_ref), rel=1e-12)   # the zero voxel, against the floor
    assert maxnorm == pytest.approx(0.5 / 1000.0, rel=1e-12)
    assert fft_errors(got[0], ref[0]) == (0.0, 0.0, 0.0)
    with pytest.raises(AssertionError, match=r"worst voxel \(1, 2, 3\): got 0.25, float64 reference 0.0"):
        assert_fft_close(got, ref, 1.0, 1e-3, "hand-made")
    bad = got.copy()
    bad[0, 1, 1] = np.nan
    with pytest.raises(AssertionError):
        assert_fft_close(bad, ref, 1.0, 1.0)
