"""GPU: the four registration kernels (csrc/regmetric.hip: bh_mattes_mi, bh_smooth_shrink, bh_sobel, bh_image_stats) against
float64, where their loops wrap and at the edges of their arguments.

Every kernel there is a capped grid with a grid-stride loop, and test_registration_kernels_vs_oracle's one shape fits inside
every cap.  The wrap cases here send each kernel through its outer loop a second time — for ``mi_hist_kernel`` that is the
re-zeroed LDS histogram, the flush behind a barrier and the running ``nvalid``, for ``mi_grad_kernel`` twelve doubles carried
across chunks — and each asserts against the card's own compute-unit count that it does.  The other cases: a chunk histogram
at 67 % of 2^32, ``bins`` from 6 to 64, planar volumes, samples on the last index, pulls that leave few samples or none
inside, volumes of different shapes, one-sample strides and offsets, a range narrower than the data, the smoothing radius
from 0 to 32 with axes shorter than radius or factor, Sobel on axes of 1 and 2, statistics with their extremes in the first
and the last voxel.  Inputs, float32 restatements and bounds: tests/regmetric_cases.py (10x the restatement's own error against
float64, measured on the CPU by tests/test_regmetric_reference.py; none from the kernels).  ``-s`` shows one ``REG gpu`` line
per case; DESIGN.md §3.5 keeps the table.
"""

import ctypes

import numpy as np
import pytest
import torch

import regmetric_cases as C
from fft_metrics import assert_fft_close
from oracle import oracle_np as O
from oracle import reference_f64 as R

pytestmark = pytest.mark.gpu


def _thresholds(gpu):
    return C.thresholds(torch.cuda.get_device_properties(gpu).multi_processor_count)


def _samples(case):
    return -(-(case.fixed.size - case.offset) // case.stride)


def _dev(a, gpu):
    return torch.from_numpy(np.array(a, copy=True)).to(gpu)   # the case arrays are read-only: upload a copy


def _run_mi(case, gpu):
    from biahub_amd.registration import metric

    return metric.mattes_mi(_dev(case.fixed, gpu), _dev(case.moving, gpu), case.P, case.rng, case.bins, case.stride, case.offset)


def _hold_mi(what, got, ref, tols):
    (v, g, n), (wv, wg, wn) = got, ref
    errs = C.mi_errors(v, g, wv, wg)
    print(f"REG gpu mi {what}: n {n} value {v:.9f} errors " + " ".join(f"{e:.2e}" for e in errs))
    assert n == wn, f"{what}: nvalid {n}, float64 reference {wn}"
    assert all(e <= t for e, t in zip(errs, tols)), (
        f"{what}: value / gradient / entry errors {errs} against bounds {tols}; value {v!r} reference {wv!r}; gradient\n{g}\n"
        f"reference\n{np.asarray(wg)}")
    return errs


NAMED_TOLS = (C.MI_VALUE_TOL, C.MI_GRAD_TOL, C.MI_GRAD_ENTRY_TOL)
SWEEP_TOLS = (C.MI_SWEEP_VALUE_TOL, C.MI_SWEEP_GRAD_TOL, C.MI_SWEEP_GRAD_ENTRY_TOL)


# ----------------------------------------------------------------------------- bh_mattes_mi
def test_mattes_wrap_vs_float64(gpu):
    """The slow case: 9.1 M samples at stride 1, 2 224 chunks on 8 x 256 workgroups, so 176 workgroups take a second chunk
    (the float64 reference of 8.5 M samples inside takes seconds and gigabytes on the host; built once per module).  Then the
    same volumes at stride 5, offset 3 in a single pass: a fault in the index arithmetic shows in both, a fault in the wrap
    only in the first.  Value, twelve gradient entries, nvalid; and bit-reproducible."""
    t = _thresholds(gpu)
    case = C.mi_case("wrap")
    assert _samples(case) > t["samples"] and -(-_samples(case) // C.MI_CHUNK) > t["samples"] // C.MI_CHUNK, (
        f"{_samples(case)} samples do not wrap a grid of {t['samples'] // C.MI_CHUNK} workgroups: size the case for this card")
    got = _run_mi(case, gpu)
    _hold_mi("wrap", got, C.mi_reference("wrap"), NAMED_TOLS)
    again = _run_mi(case, gpu)
    assert again[0] == got[0] and again[2] == got[2] and np.array_equal(again[1], got[1])
    single = C.mi_case("wrap stride 5")
    assert _samples(single) <= t["samples"]
    _hold_mi("wrap stride 5", _run_mi(single, gpu), C.mi_reference("wrap stride 5"), NAMED_TOLS)


def test_mattes_flat_background_fills_a_chunk_bin(gpu):
    """Whole chunks of 4096 samples on one Parzen coordinate: the 32-bit chunk histogram holds 4096 x 699 051 = 67 % of 2^32
    in one bin.  The float64 reference (its closed form: tests/test_regmetric_reference.py) and nvalid = every voxel."""
    case = C.mi_case("flat")
    got = _run_mi(case, gpu)
    _hold_mi("flat", got, C.mi_reference("flat"), NAMED_TOLS)
    assert got[2] == case.fixed.size == 16 * C.MI_CHUNK


@pytest.mark.parametrize("name", [n for n in C.MI_CASES if n not in ("wrap", "wrap stride 5", "flat", "none inside")])
def test_mattes_case_vs_float64(gpu, name):
    """bins 6, 7, 33 and 64; planar volumes and a moving axis of length 1 in each position; a face of samples on c = N - 1;
    a tenth of the samples inside; volumes of different shapes; one sample at the last voxel, one at the first, stride 64
    down one column; the range of the 5th to 95th percentile."""
    _hold_mi(name, _run_mi(C.mi_case(name), gpu), C.mi_reference(name), NAMED_TOLS)


def test_mattes_no_sample_inside(gpu):
    """A pull that leaves nothing inside: value 0.0, a gradient of exactly zero, n = 0."""
    v, g, n = _run_mi(C.mi_case("none inside"), gpu)
    assert n == 0 and v == 0.0 and g.shape == (3, 4) and not g.any()
    assert C.mi_reference("none inside")[2] == 0


def test_mattes_rejects_bins_outside_6_to_64(gpu):
    case = C.mi_case("bins 6")
    for bins in (5, 65):
        with pytest.raises(ValueError, match="bins"):
            _run_mi(case._replace(bins=bins), gpu)


def test_fuzz_regmetric(gpu):
    """The seeded sweep: 40 draws, axes of 1 to 48, random pulls (a fifth partly outside), bins 6 to 64, stride 1 to 9, any
    offset, against float64 at the sweep's bounds."""
    for what, case in C.fuzz_cases():
        _hold_mi(what, _run_mi(case, gpu), C.mattes_f64(case), SWEEP_TOLS)


# ----------------------------------------------------------------------------- bh_smooth_shrink
@pytest.mark.parametrize("shape,sigma,factor,wraps,note", C.SMOOTH_CASES, ids=[c[4] for c in C.SMOOTH_CASES])
def test_smooth_shrink_vs_float64(gpu, shape, sigma, factor, wraps, note):
    """Each voxel against ``smooth_shrink_f64``; shape and offset equal.  The wrap cases assert which passes wrap."""
    from biahub_amd.registration import metric

    if wraps:
        t = _thresholds(gpu)
        assert tuple(v > t["voxels"] for v in C.smooth_pass_voxels(shape, factor)) == wraps, (
            f"{note}: passes of {C.smooth_pass_voxels(shape, factor)} voxels against a grid of {t['voxels']}")
    vol = C.camera(shape)
    got, off = metric.smooth_shrink(_dev(vol, gpu), sigma, factor)
    ref, woff = R.smooth_shrink_f64(vol, sigma, factor)
    assert tuple(got.shape) == tuple(ref.shape) and tuple(off) == woff
    assert metric.smooth_shrink_geometry(shape, factor) == (tuple(ref.shape), woff)
    errs = assert_fft_close(got, ref, C.SMOOTH_RMS_TOL, C.SMOOTH_VOXEL_TOL, f"smooth {shape} sigma {sigma} factor {factor}")
    print(f"REG gpu smooth {shape} sigma {sigma} factor {factor}: rms_rel {errs[0]:.2e} voxel_rel {errs[1]:.2e}")


def test_smooth_shrink_rejects_sigma_above_8_and_factor_0(gpu):
    from biahub_amd.registration import metric

    t = _dev(C.camera((5, 70, 9)), gpu)
    for sigma, factor in C.SMOOTH_RAISES:
        with pytest.raises(ValueError):
            metric.smooth_shrink(t, sigma, factor)


# ----------------------------------------------------------------------------- bh_sobel
@pytest.mark.parametrize("shape", C.SOBEL_WRAP + C.SOBEL_EDGES)
def test_sobel_vs_float64(gpu, shape):
    """Each voxel against ``oracle_np.sobel`` in float64, unrounded: the wrap shape, and axes of length 1 and 2."""
    from biahub_amd.registration import metric

    if shape in C.SOBEL_WRAP:
        assert int(np.prod(shape)) > _thresholds(gpu)["voxels"], f"{shape} does not wrap the Sobel grid of this card"
    vol = C.camera(shape)
    errs = assert_fft_close(metric.sobel(_dev(vol, gpu)), O.sobel(vol, dtype=np.float64), C.SOBEL_RMS_TOL, C.SOBEL_VOXEL_TOL, f"sobel {shape}")
    print(f"REG gpu sobel {shape}: rms_rel {errs[0]:.2e} voxel_rel {errs[1]:.2e}")


def test_sobel_constant_and_impulse(gpu):
    """A constant volume gives exactly 0; one voxel of 1024 on zeros gives its 26 neighbours their closed-form values, each to
    the voxel bound of its own magnitude, and exactly 0 everywhere else."""
    from biahub_amd.registration import metric

    assert not metric.sobel(torch.full((9, 33, 70), 173.0, device=gpu)).any()
    vol = np.zeros(C.IMPULSE_SHAPE, np.float32)
    vol[C.IMPULSE_AT] = C.IMPULSE
    got = metric.sobel(_dev(vol, gpu)).cpu().numpy().astype(np.float64)
    want = C.sobel_impulse(C.IMPULSE_SHAPE, C.IMPULSE_AT, C.IMPULSE)
    near = want > 0
    assert int(near.sum()) == 26 and not got[~near].any()
    assert (np.abs(got[near] - want[near]) <= C.SOBEL_VOXEL_TOL * want[near]).all(), (got[near], want[near])


# ----------------------------------------------------------------------------- bh_image_stats
def _raw_stats(t):
    """The six doubles of bh_image_stats as the ABI returns them (the wrapper divides the moments by the sum)."""
    from biahub_amd import _lib
    from biahub_amd.device import get_context, ptr

    out = (ctypes.c_double * 6)()
    ctx = get_context(t.device)
    _lib.check(ctx.lib.bh_image_stats(ctx.handle, ptr(t), *t.shape, out))
    return [float(v) for v in out]


@pytest.mark.parametrize("shape", C.STATS_WRAP + C.STATS_EDGES)
def test_image_stats_vs_fsum(gpu, shape):
    """Minimum in the very first voxel, maximum in the very last (read in a wrapped iteration on the wrap shapes), a negative
    background: min and max exact; the sum and the three first moments equal to math.fsum of the float64 products —
    integer counts, so float64 accumulation is exact in any order (regmetric_cases.STATS_TOL)."""
    from biahub_amd.registration import metric

    if shape in C.STATS_WRAP:
        assert shape[0] * shape[1] > _thresholds(gpu)["rows"], f"{shape} does not wrap the statistics grid of this card"
    vol = C.stats_volume(shape)
    mn, mx, sums, sums_abs = C.stats_fsum(vol)
    t = _dev(vol, gpu)
    got = _raw_stats(t)
    err = C.stats_errors(got[2:], sums, sums_abs)
    print(f"REG gpu stats {shape}: min {got[0]} max {got[1]} sums error {err:.2e}")
    assert got[0] == mn and got[1] == mx
    assert err <= C.STATS_TOL, (got[2:], sums)
    st = metric.image_stats(t)
    assert st["min"] == mn and st["max"] == mx and st["sum"] == sums[0]
    assert np.array_equal(st["center_of_mass"], np.array(sums[1:]) / sums[0])
