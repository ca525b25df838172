"""GPU: compute-tf's transfer functions (bh_phase_transfer_function_3d, bh_fluorescence_transfer_function_3d,
bh_fourier_central_cuboid; csrc/invtf.hip) against the float64 oracle (oracle/oracle_np.py: wo_*), per frequency bin.

Their result is the H that apply-inv-tf turns into conj(H) / (|H|^2 + reg): at reg = 1e-3 a bin at a thousandth of the peak
weighs as much as the peak, and a max-norm cannot see it.  So every case of tests/tf_cases.py — odd and even extents, padding,
inverted contrast on odd and even Zt, one and three planes, refinement factors 2 and 3, elongated planes, 512 planes (phases of
a thousand radians), volumes and planes past the grid cap of the kernels' grid-stride loops, and cut-offs that land exactly on a
bin's radial frequency — is held to rms_rel and voxel_rel, each complex array weighed as a real one of shape (Z, Y, X, 2) and each
function on its own scale.

Every case prints one ``F64 tf ...`` line with its errors and their share of the bounds (``-s`` shows them).  Bounds:
tests/fft_metrics.py; their yardstick: tests/test_tf_reference.py.
"""

import numpy as np
import pytest
import torch

from fft_metrics import TF_RMS_TOL, TF_VOXEL_TOL, TF_ZERO_RE_RATIO_TOL, assert_fft_close, fft_errors
from oracle import oracle_np as O
from test_gpu_f64_parity import report
from tf_cases import (FLUOR_CASES, FLUOR_TIES, PHASE_CASES, PHASE_TIES, as_real, case_id, fluor_args, fluorescence_reference,
                      phase_args, phase_reference, real_potential_vanishes, total_planes)

pytestmark = pytest.mark.gpu


def _phase(c):
    from biahub_amd.compute_transfer_function import phase_transfer_function_3d

    return phase_transfer_function_3d(*phase_args(c))


def _fluorescence(c):
    from biahub_amd.compute_transfer_function import fluorescence_transfer_function_3d

    return fluorescence_transfer_function_3d(*fluor_args(c))


def _well_formed(t, c, gpu):
    assert tuple(t.shape) == (total_planes(c),) + c.shape[1:]
    assert t.dtype == torch.complex64 and t.device.type == "cuda" and t.device.index == gpu.index
    assert bool(torch.isfinite(torch.view_as_real(t)).all())


def _held(name, got, want):
    errs = fft_errors(as_real(got), as_real(want))
    share = max(errs[0] / TF_RMS_TOL, errs[1] / TF_VOXEL_TOL)
    report(f"tf {name}", errs, f"{share:.2f} of the bounds")
    assert_fft_close(as_real(got), as_real(want), TF_RMS_TOL, TF_VOXEL_TOL, name)


def check_phase(gpu, c):
    re, im = _phase(c)
    wre, wim = phase_reference(c)
    for t in (re, im):
        _well_formed(t, c, gpu)
    _held(f"phase imag {case_id(c)}", im, wim)
    if real_potential_vanishes(c):
        ratio = float(re.abs().max() / im.abs().max())
        print(f"F64 tf phase real {case_id(c)}: max|re| / max|im| {ratio:.2e} {ratio / TF_ZERO_RE_RATIO_TOL:.2f} of the bound")
        assert ratio <= TF_ZERO_RE_RATIO_TOL
    else:
        _held(f"phase real {case_id(c)}", re, wre)


def check_fluorescence(gpu, c):
    h = _fluorescence(c)
    _well_formed(h, c, gpu)
    _held(f"fluorescence {case_id(c)}", h, fluorescence_reference(c))
    dc, peak = complex(h[0, 0, 0].cpu()), float(h.abs().max())
    print(f"F64 tf fluorescence {case_id(c)}: |H(0) - 1| {abs(dc - 1.0):.2e} max|H| - 1 {peak - 1.0:.2e}")
    assert abs(dc - 1.0) <= TF_VOXEL_TOL
    assert peak <= 1.0 + 2.0 ** -23


@pytest.mark.parametrize("c", PHASE_CASES, ids=case_id)
def test_phase_transfer_function_vs_float64(gpu, c):
    check_phase(gpu, c)


@pytest.mark.parametrize("c", PHASE_TIES, ids=case_id)
def test_phase_transfer_function_on_a_pupil_tie(gpu, c):
    """A cut-off that equals a bin's radial frequency as the oracle forms it: the bin is outside.  A kernel that forms fftfreq
    as k / (n d), or the sum of squares with a fused multiply-add, takes it in, and the pupil count with it — every bin of the
    result is then off by 1 / count, percent-level at this size."""
    check_phase(gpu, c)


@pytest.mark.parametrize("c", FLUOR_CASES, ids=case_id)
def test_fluorescence_transfer_function_vs_float64(gpu, c):
    check_fluorescence(gpu, c)


@pytest.mark.parametrize("c", FLUOR_TIES, ids=case_id)
def test_fluorescence_transfer_function_on_a_pupil_tie(gpu, c):
    check_fluorescence(gpu, c)


# ----------------------------------------------------------------------------- the central cuboid, called directly
def _cuboid(src, shape):
    from biahub_amd import _lib
    from biahub_amd.device import get_context, ptr

    ctx = get_context(src.device)
    dst = torch.full(tuple(shape), complex(np.nan, np.nan), dtype=torch.complex64, device=src.device)
    _lib.check(ctx.lib.bh_fourier_central_cuboid(ctx.handle, ptr(src), *(int(n) for n in src.shape), ptr(dst),
                                                 *(int(n) for n in shape)))
    return dst


@pytest.mark.parametrize("N,n", [
    ((7, 9, 10), (3, 4, 5)),                # odd and even sources to odd and even targets
    ((6, 8, 9), (5, 8, 1)),                 # one axis kept whole, one cut to a single bin
    ((4, 4, 4), (4, 4, 4)),                 # equal shapes: compute_transfer_function._central_cuboid never sends these
    ((14, 30, 36), (6, 10, 12)),            # the refined box of the factor-3 case
    ((40, 150, 202), (39, 149, 201)),       # 1 170 819 target bins: past the grid cap, the loop wraps
])
def test_central_cuboid_bit_for_bit(gpu, N, n):
    rng = np.random.default_rng(sum(N))
    host = (rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)
    src = torch.from_numpy(host).to(gpu)
    got = _cuboid(src, n).cpu().numpy()
    want = O.wo_central_cuboid(host, n)
    assert got.shape == want.shape == n and got.dtype == np.complex64
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(src.cpu().numpy().view(np.uint32), host.view(np.uint32))   # the source is only read


def test_central_cuboid_refuses_a_target_outside_the_source(gpu):
    src = torch.zeros((4, 6, 8), dtype=torch.complex64, device=gpu)
    for n in ((5, 6, 8), (4, 7, 8), (4, 6, 9)):
        with pytest.raises(ValueError, match="the target must fit inside the source"):
            _cuboid(src, n)


# ----------------------------------------------------------------------------- scratch reuse
def test_second_calls_are_bit_identical(gpu):
    """Both functions keep their planes and their one counter word (the pupil count of the phase model, the maximum of the
    fluorescence model: the same scratch) in the context: interleaved calls, at two shapes each, give the same bits again."""
    by_name = {c.name: c for c in PHASE_CASES + PHASE_TIES}
    fby_name = {c.name: c for c in FLUOR_CASES}
    calls = [(_phase, by_name["native"]), (_fluorescence, fby_name["all odd"]), (_phase, by_name["factors 3 and 3"]),
             (_fluorescence, fby_name["factors 2 and 2"]), (_phase, by_name["T2 detection cut on frr"])]
    first = [f(c) for f, c in calls]
    for (f, c), a in zip(calls, first):
        b = f(c)
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert torch.equal(torch.view_as_real(x).view(torch.int32), torch.view_as_real(y).view(torch.int32)), (f.__name__, case_id(c))
