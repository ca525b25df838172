"""CPU: the float64 references of the registration metric kernels (csrc/regmetric.hip), the float32 restatements the bounds of
tests/test_gpu_regmetric.py are measured from, and the preconditions its case list states.

Every input the GPU tests use is built here too (tests/regmetric_cases.py): the restatement is held to a tenth of each bound,
the wrap cases are shown to exceed their loop thresholds at 256 compute units, the flat case to put whole chunks on one
histogram bin, the geometry cases to leave the samples inside that they are meant to, and three planted defects to be caught.
``-s`` shows the measured figures (lines starting ``REG``).
"""

import math

import numpy as np
import pytest

import regmetric_cases as C
from fft_metrics import assert_fft_close, fft_errors
from oracle import oracle_np as O
from oracle import reference_f64 as R


def _fmt(errs):
    return " ".join(f"{e:.2e}" for e in errs)


def _samples(case):
    return -(-(case.fixed.size - case.offset) // case.stride)


# ----------------------------------------------------------------------------- preconditions of the case list
def test_wrap_cases_exceed_their_thresholds_at_256_compute_units():
    """Each wrap case is 1.08x or more of the work at which its kernel's grid-stride loop takes a second trip; the cases
    meant to stay inside one trip do."""
    t = C.thresholds(C.CUS)
    assert t == {"rows": 8192, "voxels": 1048576, "samples": 8388608}
    assert C.WRAP_SHAPE == (139, 256, 256)
    assert int(np.prod(C.WRAP_SHAPE)) >= C.WRAP_MARGIN * t["samples"] > int(np.prod((138, 256, 256)))
    for name in C.MI_CASES:
        n = _samples(C.mi_case(name))
        assert (n >= C.WRAP_MARGIN * t["samples"]) == (name in C.MI_WRAP_CASES), (name, n)
        assert name in C.MI_WRAP_CASES or n <= t["samples"]
    case = C.mi_case("wrap stride 5")
    assert case.fixed is C.mi_case("wrap").fixed and (case.stride, case.offset) == (5, 3) and _samples(case) < t["samples"] // 4
    for shape, sigma, factor, wraps, note in C.SMOOTH_CASES:
        vox = C.smooth_pass_voxels(shape, factor)
        for v, w in zip(vox, wraps or (False,) * 3):
            assert v >= C.WRAP_MARGIN * t["voxels"] if w else v <= t["voxels"], (note, vox)
    assert C.SMOOTH_CASES[0][3] == (True, True, True) and C.SMOOTH_CASES[1][3] == (True, True, False)
    assert all(np.prod(s) >= C.WRAP_MARGIN * t["voxels"] for s in C.SOBEL_WRAP)
    assert all(np.prod(s) <= t["voxels"] for s in C.SOBEL_EDGES)
    assert all(s[0] * s[1] >= C.WRAP_MARGIN * t["rows"] for s in C.STATS_WRAP) and all(s[0] * s[1] <= t["rows"] for s in C.STATS_EDGES)
    assert C.STATS_WRAP[0][2] < 64 and C.STATS_WRAP[1][2] == 65


def test_flat_case_puts_whole_chunks_on_one_bin():
    """100 sits on the integer moving Parzen coordinate 16 (float32 and float64 alike), so every sample of a background
    chunk gives bin 16 the weight floor(2/3 2^20 + 0.5): 4096 of them 2 863 312 896, 67 % of 2^32.  The histogram follows
    from the voxel counts in closed form; the float64 reference and the restatement both give its mutual information."""
    case = C.mi_case("flat")
    assert case.fixed.shape == case.moving.shape == C.FLAT_SHAPE and case.fixed.size == 16 * C.MI_CHUNK and case.bins == 32
    mbin = (case.rng[3] - case.rng[2]) / 28
    mscale, mnmin = np.float32(1 / mbin), np.float32(case.rng[2] / mbin - 2)
    assert np.float32(100) * mscale - mnmin == np.float32(16) and 100 / mbin - (case.rng[2] / mbin - 2) == 16.0
    n200 = int((case.fixed == 200).sum())
    n100 = case.fixed.size - n200
    assert n200 == 64 and set(np.unique(case.fixed)) == {100.0, 200.0}
    # B3 at -1, 0, 1 (and 0 at 2) for the background; at -1.5, -0.5, 0.5, 1.5 for the block (coordinate 28.5)
    hist = np.zeros((32, 32))
    hist[16, 15:18] = n100 * np.array([1, 4, 1]) / 6
    hist[28, 27:31] = n200 * np.array([1, 23, 23, 1]) / 48
    p = hist / hist.sum()
    pF, pM = p.sum(axis=1), p.sum(axis=0)
    nz = p > 0
    want = float((p[nz] * np.log(p[nz] / (pF[:, None] * pM[None, :])[nz])).sum())
    value, grad, n = C.mi_reference("flat")
    assert n == case.fixed.size and abs(value - want) <= 1e-13
    v32, g32, n32, info = C.mattes_f32(case)
    q = lambda w: math.floor(w * C.MI_FIX + 0.5)   # noqa: E731
    assert q(2 / 3) == 699051 and info["chunk_max"] == 4096 * 699051 == 2863312896 < 2 ** 32
    assert n32 == n and info["hist"][16, 16] == n100 * 699051 and info["hist"][16, 15] == info["hist"][16, 17] == n100 * q(1 / 6)
    assert info["hist"][28, 27:31].tolist() == [n200 * q(1 / 48), n200 * q(23 / 48), n200 * q(23 / 48), n200 * q(1 / 48)]
    assert info["hist"].sum() == info["hist"][16, 15:18].sum() + info["hist"][28, 27:31].sum()
    print(f"REG flat: value {value:.12f} closed form {want:.12f} chunk bin {info['chunk_max']} = {info['chunk_max'] / 2 ** 32:.3f} of 2^32")


def test_geometry_and_sampling_cases_are_what_they_claim():
    """nvalid of each case, trivial or not as intended, from the float64 reference."""
    def n_of(name):
        return C.mi_reference(name)[2]

    case = C.mi_case("face")                     # z + 2 <= 23, y - 3 >= 0, x + 5 <= 55: the face x = 50 lands on c = 55
    assert np.array_equal(case.P, np.hstack([np.eye(3), [[2.0], [-3.0], [5.0]]]))
    assert n_of("face") == 22 * 37 * 51 and case.moving.shape[2] - 1 == 50 + 5
    frac = n_of("tenth inside") / C.mi_case("tenth inside").fixed.size
    assert 0.05 < frac < 0.2, frac
    value, grad, n = C.mi_reference("none inside")
    assert n == 0 and value == 0.0 and not np.asarray(grad).any()
    v32, g32, n32, _ = C.mattes_f32(C.mi_case("none inside"))
    assert n32 == 0 and v32 == 0.0 and not g32.any()
    case = C.mi_case("shapes differ")
    assert case.fixed.shape == C.GEOMETRY_SHAPE and case.moving.shape == C.OTHER_SHAPE
    assert 0.5 * case.fixed.size < n_of("shapes differ") < case.fixed.size       # some samples leave the moving volume
    for name in ("last voxel", "stride past the end"):
        case = C.mi_case(name)
        assert _samples(case) == 1 and n_of(name) == 1
    assert C.mi_case("last voxel").offset == C.mi_case("last voxel").fixed.size - 1
    assert C.mi_case("stride past the end").stride == C.mi_case("stride past the end").fixed.size + 7
    case = C.mi_case("stride 64")
    assert case.fixed.shape[2] == 64 and case.stride == 64 and 100 < n_of("stride 64") < _samples(case) == 960
    case = C.mi_case("planar")
    assert case.fixed.shape == case.moving.shape == (1, 96, 130) and tuple(case.P[0]) == (1, 0, 0, 0)
    assert 0.8 * case.fixed.size < n_of("planar") < case.fixed.size
    for name, mshape in C.MOVING_PLANES.items():
        case = C.mi_case(name)
        a = mshape.index(1)
        assert case.moving.shape == mshape and not case.P[a].any() and n_of(name) == case.fixed.size
        assert all(case.P[b].any() for b in range(3) if b != a)
    for b in C.BINS:
        assert C.mi_case(f"bins {b}").bins == b and C.mi_case(f"bins {b}").fixed.shape == C.BINS_SHAPE


def test_narrow_range_clamps_both_ends_and_loses_samples():
    """5th to 95th percentile: samples below and above the range on both images, and samples inside the moving volume whose
    four B-spline weights all vanish — the histogram's mass is well below nvalid, which is why the two must not be confused."""
    case = C.mi_case("narrow range")
    assert (case.moving < case.rng[2]).mean() > 0.02 and (case.moving > case.rng[3]).mean() > 0.02
    assert (case.fixed > case.rng[1]).mean() > 0.02     # its 5th percentile is the 0 outside the pulled volume
    _, _, n, info = C.mattes_f32(case)
    assert n == C.mi_reference("narrow range")[2] and info["total"] < 0.97 * n
    print(f"REG narrow range: nvalid {n}, histogram mass {info['total']:.1f}")


# ----------------------------------------------------------------------------- the restatement against float64
def _hold_mi(what, case, ref, tols):
    worst = [0.0, 0.0, 0.0]
    wv, wg, wn = ref
    for contract in (False, True):
        v, g, n, info = C.mattes_f32(case, contract=contract)
        errs = C.mi_errors(v, g, wv, wg)
        print(f"REG mi {what} contract {int(contract)}: n {n} of {_samples(case)} flips {info['flips']} value {wv:.6f} max|grad| "
              f"{np.abs(wg).max():.3e} errors {_fmt(errs)}")
        assert n == wn, what
        assert info["chunk_max"] < 2 ** 32
        assert all(e <= t / 10 for e, t in zip(errs, tols)), (what, contract, errs)
        worst = [max(a, b) for a, b in zip(worst, errs)]
    return worst


@pytest.mark.parametrize("name", C.MI_CASES)
def test_metric_restatement_within_a_tenth_of_the_bounds(name):
    """``mattes_mi_f32`` (the kernel's documented arithmetic, with and without contraction of the Parzen coordinates) against
    ``oracle_np.mattes_mi`` at every named case: inside a tenth of the bounds, nvalid equal.  The wrap case is the slow one
    (9.1 M samples: seconds per evaluation)."""
    _hold_mi(name, C.mi_case(name), C.mi_reference(name), (C.MI_VALUE_TOL, C.MI_GRAD_TOL, C.MI_GRAD_ENTRY_TOL))


def test_sweep_restatement_within_a_tenth_of_the_sweep_bounds():
    """The same at the 40 draws of the seeded sweep, against the sweep's own bounds; a fifth of the draws reach outside the
    moving volume, and the sweep covers bins 6 to 64, strides 1 to 9 and degenerate axes."""
    worst, partly, planes = [0.0, 0.0, 0.0], 0, 0
    for what, case in C.fuzz_cases():
        ref = C.mattes_f64(case)
        w = _hold_mi(what, case, ref, (C.MI_SWEEP_VALUE_TOL, C.MI_SWEEP_GRAD_TOL, C.MI_SWEEP_GRAD_ENTRY_TOL))
        worst = [max(a, b) for a, b in zip(worst, w)]
        partly += 0 < ref[2] < _samples(case)
        planes += 1 in case.moving.shape or 1 in case.fixed.shape
    print(f"REG mi sweep worst {_fmt(worst)}; {partly} draws partly outside, {planes} with an axis of length 1")
    assert len(C.fuzz_cases()) == 40 and partly >= 6 and planes >= 2   # 8 draws reach outside; 2 of them keep no sample at all
    assert min(c.bins for _, c in C.fuzz_cases()) <= 8 and max(c.bins for _, c in C.fuzz_cases()) >= 62 and {c.stride for _, c in C.fuzz_cases()} == set(range(1, 10))


@pytest.mark.parametrize("shape,sigma,factor,wraps,note", C.SMOOTH_CASES, ids=[c[4] for c in C.SMOOTH_CASES])
def test_smooth_shrink_restatement_within_a_tenth_of_the_bounds(shape, sigma, factor, wraps, note):
    """``oracle_np.smooth_shrink`` (float32 products and sums) against ``smooth_shrink_f64`` (the same float32 weights, float64
    sums): shape and offset equal, the volume inside a tenth of the bounds."""
    vol = C.camera(shape)
    ref, off = R.smooth_shrink_f64(vol, sigma, factor)
    got, goff = O.smooth_shrink(vol, sigma, factor)
    assert tuple(ref.shape) == got.shape == tuple(max(1, n // f) for n, f in zip(shape, factor)) and off == goff
    print(f"REG smooth {shape} sigma {sigma} factor {factor}: {_fmt(fft_errors(got, ref))}")
    assert_fft_close(got, ref, C.SMOOTH_RMS_TOL / 10, C.SMOOTH_VOXEL_TOL / 10, note)


def test_smooth_shrink_f64_is_the_definition():
    """Against a direct triple loop on a small volume, and the identity at sigma 0, factor 1."""
    rng = np.random.default_rng(5)
    vol = (rng.random((4, 5, 7)) * 100).astype(np.float32)
    ref, off = R.smooth_shrink_f64(vol, (0.5, 0, 1.0), (2, 1, 3))
    assert tuple(ref.shape) == (2, 5, 2) and off == (0, 0, 1)
    wz = np.exp(-0.5 * np.arange(-2, 3) ** 2 / 0.25)
    wx = np.exp(-0.5 * np.arange(-4, 5) ** 2 / 1.0)
    wz, wx = (wz / wz.sum()).astype(np.float32).astype(np.float64), (wx / wx.sum()).astype(np.float32).astype(np.float64)
    for z, y, x in np.ndindex(2, 5, 2):
        want = sum(wz[a + 2] * wx[b + 4] * float(vol[min(max(2 * z + a, 0), 3), y, min(max(3 * x + 1 + b, 0), 6)])
                   for a in range(-2, 3) for b in range(-4, 5))
        assert abs(float(ref[z, y, x]) - want) <= 1e-12 * want
    same, off = R.smooth_shrink_f64(vol, (0, 0, 0), (1, 1, 1))
    assert off == (0, 0, 0) and np.array_equal(same.numpy(), vol.astype(np.float64))


@pytest.mark.parametrize("shape", C.SOBEL_WRAP + C.SOBEL_EDGES)
def test_sobel_restatement_within_a_tenth_of_the_bounds(shape):
    vol = C.camera(shape)
    ref = O.sobel(vol, dtype=np.float64)
    assert ref.dtype == np.float64 and np.array_equal(ref.astype(np.float32), O.sobel(vol))
    got = C.sobel_f32(vol)
    print(f"REG sobel {shape}: {_fmt(fft_errors(got, ref))}")
    assert_fft_close(got, ref, C.SOBEL_RMS_TOL / 10, C.SOBEL_VOXEL_TOL / 10, str(shape))


def test_sobel_constant_and_impulse():
    """A constant volume gives exactly 0; one voxel of 1024 gives its 26 neighbours their closed-form values (and itself 0)."""
    assert not O.sobel(np.full((4, 5, 6), 173.0, np.float32), dtype=np.float64).any()
    assert not C.sobel_f32(np.full((4, 5, 6), 173.0, np.float32)).any()
    vol = np.zeros(C.IMPULSE_SHAPE, np.float32)
    vol[C.IMPULSE_AT] = C.IMPULSE
    want = C.sobel_impulse(C.IMPULSE_SHAPE, C.IMPULSE_AT, C.IMPULSE)
    assert int((want > 0).sum()) == 26 and want[C.IMPULSE_AT] == 0.0
    assert np.abs(O.sobel(vol, dtype=np.float64) - want).max() <= 1e-12 * C.IMPULSE
    assert np.abs(C.sobel_f32(vol) - want).max() <= C.SOBEL_VOXEL_TOL / 10 * want[want > 0].min()


@pytest.mark.parametrize("shape", C.STATS_WRAP + C.STATS_EDGES)
def test_stats_volumes_and_their_float64_sums(shape):
    """The minimum sits in the first voxel and the maximum in the last, the background is negative; the counts are integers,
    so every product and every partial sum is an integer far below 2^53 and float64 accumulation is exact in ANY order: the
    running sum, numpy's pairwise sum and math.fsum agree to the last bit, and the kernel is held to equality."""
    v = C.stats_volume(shape)
    mn, mx, sums, sums_abs = C.stats_fsum(v)
    flat = v.reshape(-1)
    if v.size > 1:
        assert flat[0] == mn < flat[1:].min() and flat[-1] == mx > flat[:-1].max() and mn < 0
        assert shape not in C.STATS_WRAP or (v < 0).mean() > 0.1
    assert np.array_equal(v, np.rint(v)) and max(sums_abs) < 2.0 ** 53
    assert C.stats_running_f64(v) == sums and list(O.image_stats(v)[2:]) == sums and tuple(O.image_stats(v)[:2]) == (mn, mx)
    assert C.STATS_TOL == 0.0
    print(f"REG stats {shape}: min {mn} max {mx} sums {sums}")


# ----------------------------------------------------------------------------- planted defects
def _ratios(errs):
    return [e / t for e, t in zip(errs, (C.MI_VALUE_TOL, C.MI_GRAD_TOL, C.MI_GRAD_ENTRY_TOL))]


def test_planted_defects_fail_the_bounds():
    """Planted in the restatement, each on the case meant to show it:

    (1) the LDS histogram not cleared before a workgroup's second chunk (wrap case, 2 048 workgroups: the first 176 chunks
        are flushed twice): value / gradient / per entry at 1.2e3 / 3.7e3 / 93 times their bounds;
    (2) the gradient divided by nvalid instead of the histogram's mass (narrow range): gradient 2.2e3x, per entry 56x (the
        value does not depend on it);
    (3) the moving Parzen coordinate of every sample biased by 1e-4 bins (wrap case) is NOT caught: 0.42 / 0.032 / 0.0038 of
        the bounds.  Mutual information does not change when every moving intensity shifts by the same amount, except through
        the position of the bin edges, so a uniform bias is the one defect of the coordinate the metric itself forgives: the
        value crosses its bound at 1e-3 bins (3.6x; 36x at 1e-2), the gradient at 1e-2 (2.3x), the per-entry figure not even
        at 0.1 bins (0.44).  What is asserted is what holds: the value catches 1e-3 bins by 3x."""
    case, (wv, wg, wn) = C.mi_case("wrap"), C.mi_reference("wrap")
    v, g, n, _ = C.mattes_f32(case, defect="no rezero")
    r = _ratios(C.mi_errors(v, g, wv, wg))
    print(f"REG defect no rezero (wrap): value / grad / entry at {_fmt(r)} of their bounds")
    assert n == wn and min(r) >= 3.0
    for bias in (1e-4, 1e-3):
        v, g, n, _ = C.mattes_f32(case, defect=bias)
        r = _ratios(C.mi_errors(v, g, wv, wg))
        print(f"REG defect Parzen bias {bias:g} bins (wrap): value / grad / entry at {_fmt(r)} of their bounds")
    assert r[0] >= 3.0
    case, (wv, wg, wn) = C.mi_case("narrow range"), C.mi_reference("narrow range")
    v, g, n, _ = C.mattes_f32(case, defect="nvalid")
    r = _ratios(C.mi_errors(v, g, wv, wg))
    print(f"REG defect nvalid normalisation (narrow range): value / grad / entry at {_fmt(r)} of their bounds")
    assert r[0] <= 0.1 and min(r[1:]) >= 3.0     # the value does not depend on the normalisation
