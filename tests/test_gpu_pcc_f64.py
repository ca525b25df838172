"""GPU: phase cross-correlation (bh_phase_cross_corr, bh_phase_cross_corr_create / _apply) on every path against the float64
reference (oracle/reference_f64.py: phase_cross_corr_f64), per voxel.

The operator has code of its own that no other test holds to an independent reference: the Z-pass mode COL_PCC
(``colz::colz_kernel<COL_PCC>`` at Z = 512, ``col_pass_kernel<COL_PCC, R, RDX>`` at radix 1, 3 and 5), the hand-written product
``pcc_bin`` whose "magnitude" branch normalises with frexp / ldexp / rsq, ``pcc_swap`` (which factor is conjugated), ``roll`` (the
Z pass overwrites the stored spectrum), ``xw::INV_ARGMAX`` (an inverse X pass that never stores the volume), and the unfused /
library route with ``pcc_product_kernel`` and an odd last axis that comes back one column short.  Here each of them is named by
a case and its correlation volume is held to ``rms_rel`` / ``voxel_rel`` (tests/fft_metrics.py: ``pcc_bounds``; bounds from a
complex64 restatement on the CPU, tests/test_pcc_reference.py), its shift to the reference's — which no float32 path may miss:
tests/test_pcc_reference.py asserts that at every input here the runner-up voxel lies 1e-2 of the peak below it.

Inputs: tests/pcc_cases.py.  Every case prints one ``F64 pcc ...`` line (``-s`` shows them; DESIGN.md §3.2 keeps the table).
"""

import functools

import numpy as np
import pytest
import torch

import pcc_cases as P
from fft_metrics import assert_fft_close, fft_errors, pcc_bounds
from invtf_cases import ENGINE
from oracle import oracle_np as O
from oracle import reference_f64 as R
from test_gpu_f64_parity import report

pytestmark = pytest.mark.gpu

CLASS_IDS = ["None", "None, mean removed", "magnitude", "classic"]


def is_engine(shape):
    """The predicate bh_phase_cross_corr itself uses, read through the Richardson-Lucy plan (no C ABI of its own)."""
    from biahub_amd.deconvolve import richardson_lucy_plan

    return richardson_lucy_plan((3, 3, 3), tuple(shape))[1] == "engine"


@functools.lru_cache(maxsize=8)
def _pair(shape, k, removed):
    return tuple(torch.from_numpy(x).cuda() for x in P.class_inputs(*P.pair(shape, k), removed))


@functools.lru_cache(maxsize=2)
def _chain(shape, removed):
    return tuple(torch.from_numpy(P.mean_removed(x) if removed else x).cuda() for x in P.chain(shape))


def check(name, got_shift, got_corr, a, b, norm, removed, bounds=None):
    """One result against the float64 reference of its own pair: the shift equal, the volume (when there is one) inside the bounds."""
    want_shift, want_corr = R.phase_cross_corr_f64(a, b, norm)
    assert got_shift.dtype == np.float32
    if got_corr is not None:
        assert tuple(got_corr.shape) == tuple(want_corr.shape) == (a.shape[0], a.shape[1], a.shape[2] - (a.shape[2] & 1))
        report(f"pcc {name} {tuple(a.shape)} {norm}{' mean removed' if removed else ''}", fft_errors(got_corr, want_corr),
               f"shift {got_shift.tolist()}")
    assert np.array_equal(got_shift, want_shift), (name, norm, got_shift, want_shift)
    if got_corr is not None:
        assert_fft_close(got_corr, want_corr, *(bounds or pcc_bounds(norm, removed)), f"{name} {norm}")


def one_shot(name, a, b, norm, removed, bounds=None):
    """The one-shot call with the volume (held to the reference) and without it (the same shift, no volume)."""
    from biahub_amd.estimate_stabilization import phase_cross_corr_device

    shift, corr = phase_cross_corr_device(a, b, norm, want_corr=True)
    check(name, shift, corr, a, b, norm, removed, bounds)
    peak, none = phase_cross_corr_device(a, b, norm, want_corr=False)
    assert none is None and np.array_equal(peak, shift), (name, norm, peak, shift)
    return shift, corr


def _family_id(f):
    return f"{f[2]} [{P.z_pass(f[0], f[1])}] {f[1] or ''}".strip()


# ----------------------------------------------------------------------------- every engine family
@pytest.mark.parametrize("norm,removed", P.CLASSES, ids=CLASS_IDS)
@pytest.mark.parametrize("shape,env,what", ENGINE, ids=[_family_id(f) for f in ENGINE])
def test_pcc_family_vs_float64(gpu, shape, env, what, norm, removed, monkeypatch):
    """Every engine family (its Z-pass kernel in the id) at the three shifts: none, exactly n // 2 on all axes, mixed sign."""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    assert is_engine(shape)
    for k, s in enumerate(P.shifts(shape)):
        one_shot(f"{_family_id((shape, env, what))} shift {s}", *_pair(shape, k, removed), norm, removed)


@pytest.mark.parametrize("norm,removed", P.CLASSES, ids=CLASS_IDS)
@pytest.mark.parametrize("switch", ["BH_PCC_UNFUSED", "BH_PCC_NO_FUSED_PEAK"])
@pytest.mark.parametrize("shape", P.SWITCH_SHAPES)
def test_pcc_switches_vs_float64(gpu, shape, switch, norm, removed, monkeypatch):
    """BH_PCC_UNFUSED=1: the engine's forward / pcc_product_kernel / inverse route (the register-stage Z passes at 256 among
    them); BH_PCC_NO_FUSED_PEAK=1: the stored volume and the search pass where INV_ARGMAX would run.  Same bounds, same shifts."""
    monkeypatch.setenv(switch, "1")
    assert is_engine(shape)
    for k, s in enumerate(P.shifts(shape)):
        one_shot(f"{switch} shift {s}", *_pair(shape, k, removed), norm, removed)


# ----------------------------------------------------------------------------- the prepared handle
@pytest.mark.parametrize("norm,removed", P.CLASSES, ids=CLASS_IDS)
@pytest.mark.parametrize("shape,env,what", P.PREPARED, ids=[f"{p[2]} {p[0]}" for p in P.PREPARED])
def test_pcc_prepared_handle_vs_float64(gpu, shape, env, what, norm, removed, monkeypatch):
    """The handle against the reference (not against the one-shot call, which runs the same kernels), one shape per Z-pass
    kernel: the stored image as first and as second factor (``pcc_swap``), and a ``roll`` chain of three calls, in which the
    spectrum the Z pass wrote during a call is the stored one of the next and is itself replaced in the one after.  Each call
    is compared with the reference of its own pair; ``want_corr`` alternates, and the alternation flips with ``fixed_is_second``."""
    from biahub_amd.estimate_stabilization import PreparedPhaseCrossCorr

    for k, val in env.items():
        monkeypatch.setenv(k, val)
    assert is_engine(shape) == (not what.startswith("library"))
    imgs = _chain(shape, removed)
    for second in (False, True):
        with PreparedPhaseCrossCorr(imgs[0], fixed_is_second=second, device=gpu) as h:
            for k in range(3):
                mov = _pair(shape, k, removed)[1]
                a, b = (mov, imgs[0]) if second else (imgs[0], mov)
                shift, corr = h(mov, norm, want_corr=(k % 2 == int(second)))
                check(f"handle {what} second {int(second)} shift {k}", shift, corr, a, b, norm, removed)
        with PreparedPhaseCrossCorr(imgs[0], fixed_is_second=second, device=gpu) as h:
            for k in range(1, len(imgs)):
                a, b = (imgs[k], imgs[k - 1]) if second else (imgs[k - 1], imgs[k])
                shift, corr = h(imgs[k], norm, want_corr=(k % 2 != int(second)), roll=True)
                check(f"handle {what} second {int(second)} roll {k}", shift, corr, a, b, norm, removed)


# ----------------------------------------------------------------------------- the library route
@pytest.mark.parametrize("norm,removed", P.CLASSES, ids=CLASS_IDS)
@pytest.mark.parametrize("shape,env", [(s, {}) for s in P.LIBRARY_SHAPES] + [P.HIPFFT], ids=str)
def test_pcc_library_route_vs_float64(gpu, shape, env, norm, removed, monkeypatch):
    """hipFFT R2C -> pcc_product_kernel -> C2R of (Z, Y, X - (X & 1)): odd X (Z and Y odd too — the fftshift of odd axes), an
    even shape the engine does not take, and an engine shape sent there by BH_FFT_BACKEND=hipfft."""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    assert not is_engine(shape)
    for k, s in enumerate(P.shifts(shape)):
        _, corr = one_shot(f"library {env or ''} shift {s}", *_pair(shape, k, removed), norm, removed)
        assert corr.shape[2] == shape[2] - (shape[2] & 1)


# ----------------------------------------------------------------------------- edges
@pytest.mark.parametrize("shape", P.EDGE_SHAPES)
def test_pcc_impulses(gpu, shape):
    """A single impulse in each image, at (0, 0, 0) and at the far corner: the correlation is one spike (on an odd X, whose
    volume is one column short, a spike with a tail along x), None and magnitude; the volume against the reference, and the
    spike's position against the shift."""
    assert is_engine(shape) == (shape == (8, 64, 512))
    for pa, pb, a, b in P.impulse_pairs(shape):
        a, b = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
        for norm in (None, "magnitude"):
            shift, corr = one_shot(f"impulses {pa} {pb}", a, b, norm, False, pcc_bounds(norm, True))
            cshape = tuple(corr.shape)
            peak = np.unravel_index(int(torch.argmax(corr)), cshape)
            assert [(p - n // 2) % n for p, n in zip(peak, cshape)] == [int(s) % n for s, n in zip(shift, cshape)]
            if not shape[2] & 1:
                want = [(i - j) % n for i, j, n in zip(pa, pb, shape)]
                assert [int(s) % n for s, n in zip(shift, shape)] == want, (pa, pb, shift)
                top = float(corr.max())
                assert abs(top - (1000.0 * 700.0 if norm is None else 1.0)) <= 1e-5 * top
                assert int((corr > 1e-4 * top).sum()) == 1


@pytest.mark.parametrize("shape", P.EDGE_SHAPES)
def test_pcc_beads_of_65535_counts(gpu, shape):
    """Beads of 65535 counts on a zero background, no noise, ``None`` only: the products reach 4e9 V.  (Normalising a
    noiseless spectrum divides rounding noise by itself wherever the spectrum is empty; no precision reproduces that, so the
    normalised modes are not run here.)"""
    a, b = (torch.from_numpy(x).to(gpu) for x in P.bead_pair(shape))
    one_shot("beads 65535", a, b, None, False, pcc_bounds(None, True))


@pytest.mark.parametrize("shape", P.EDGE_SHAPES)
def test_pcc_all_zero_pair(gpu, shape):
    """Two all-zero images: whatever ``oracle_np.phase_cross_corr`` gives — shift (0, 0, 0), a volume of exact zeros for None
    and magnitude (0 / eps), NaN everywhere for classic (0 / 0) — from the stored, the peak-only and the handle's routes."""
    from biahub_amd.estimate_stabilization import PreparedPhaseCrossCorr, phase_cross_corr_device

    zeros = np.zeros(shape, np.float32)
    z = torch.from_numpy(zeros).to(gpu)
    for norm in P.NORMS:
        with np.errstate(invalid="ignore", divide="ignore"):
            want_shift, want_corr = O.phase_cross_corr(zeros, zeros, norm)
        assert np.array_equal(want_shift, [0, 0, 0])
        assert bool(np.isnan(want_corr).all()) if norm == "classic" else not want_corr.any()
        results = [phase_cross_corr_device(z, z, norm, want_corr=True), phase_cross_corr_device(z, z, norm, want_corr=False)]
        with PreparedPhaseCrossCorr(z, device=gpu) as h:
            results += [h(z, norm, want_corr=True), h(z, norm, want_corr=False), h(z, norm, want_corr=True, roll=True)]
        for shift, corr in results:
            assert np.array_equal(shift, want_shift), (norm, shift)
            if corr is not None:
                assert np.array_equal(corr.cpu().numpy(), want_corr, equal_nan=True), norm
