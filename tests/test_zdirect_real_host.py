"""CPU: which PSFs have a real Q, in float64 numpy.

Q(t; ky, kx) is the centred PSF transformed along y and x only; the direct Z pass of Richardson-Lucy convolves every
(ky, kx) column with it along z.  The real-tap kernels drop Im Q, so the inputs of tests/test_gpu_zdirect_real.py that take
them must have an imaginary part that is round-off (<= 1e-12 max|Q|), and the counter-examples that keep the complex taps
must not (> 1e-6 max|Q|): otherwise the GPU tests would not tell a wrong decision from a right one.  The numpy predicate those
tests expect the handle's decision from is checked against the same four.
"""

import numpy as np
import pytest

from oracle import reference_f64 as R
from test_gpu_zdirect_real import psf_kind, slices_symmetric

BOX_YX = (32, 64)
PSHAPES = [(33, 3, 5), (33, 5, 5), (9, 5, 5), (7, 5, 9), (3, 3, 5)]


def q_of(psf):
    """FFT over (y, x) of h = psf / sum(psf) on a zero plane, tap k of each axis at offset k - K // 2 (mod N)."""
    pz, py, px = psf.shape
    h = np.zeros((pz,) + BOX_YX, dtype=np.float64)
    h[:, :py, :px] = psf.astype(np.float64) / psf.astype(np.float64).sum()
    h = np.roll(h, (-(py // 2), -(px // 2)), axis=(1, 2))
    return np.fft.fft2(h, axes=(1, 2))


def imag_share(psf):
    q = q_of(psf)
    return float(np.abs(q.imag).max() / np.abs(q).max())


@pytest.mark.parametrize("pshape", PSHAPES)
@pytest.mark.parametrize("kind", ["mirror", "aberrated"])
def test_real_q_inputs_have_round_off_imaginary_parts(kind, pshape):
    psf = psf_kind(pshape, kind)
    assert slices_symmetric(psf)
    assert R.psf_is_point_symmetric(psf) == (kind == "mirror")
    assert imag_share(psf) <= 1e-12


@pytest.mark.parametrize("pshape", PSHAPES)
@pytest.mark.parametrize("kind", ["sheared", "complex"])
def test_counter_examples_have_a_complex_q(kind, pshape):
    psf = psf_kind(pshape, kind)
    assert not slices_symmetric(psf)
    assert R.psf_is_point_symmetric(psf) == (kind == "sheared")
    assert imag_share(psf) > 1e-6


def test_near_miss_and_even_extents_fail_the_predicate():
    assert not slices_symmetric(psf_kind((33, 3, 5), "near miss"))
    for pshape in [(33, 4, 5), (33, 3, 4)]:
        psf = psf_kind(pshape, "mirror")
        assert not slices_symmetric(psf)
        assert imag_share(psf) > 1e-6  # the centre tap K // 2 of an even extent is no centre of symmetry
    assert slices_symmetric(psf_kind((32, 3, 5), "mirror"))  # an even z-extent does not matter


def test_aberrated_stack_is_asymmetric_along_z():
    """Convolution and correlation differ: q(t) != q(-t) by far more than rounding."""
    q = q_of(psf_kind((33, 3, 5), "aberrated")).real
    assert np.abs(q - q[::-1]).max() > 1e-3 * np.abs(q).max()
