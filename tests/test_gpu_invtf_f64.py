"""GPU: the inverse filter (bh_inverse_filter, csrc/invtf.hip) on every family of the FFT engine against the float64
reference (oracle/reference_f64.py), per voxel, with transfer functions that have no symmetry.

The inverse filter is the one spectral operator that writes a caller's transfer function straight into the engine's scrambled
half-spectrum layout: ``inverse_filter_rows_kernel`` computes stored position -> natural frequency -> mirror bin -k by
formula, per axis, for power-of-two, 3 * 2^k and 5 * 2^k lengths and for the column order of the wave-private rows.  Nothing
cancels as it does in Richardson-Lucy (whose transfer function goes through the engine's own forward passes), and with a real
even H (every Tikhonov and ``deconvolve`` test) the mirror arithmetic and the sign of the imaginary part are invisible.  So
each family of test_gpu_f64_parity.FAMILIES the engine takes, and two boxes with an odd radix on all three axes, runs it
with a complex asymmetric H, a real asymmetric H and the bfloat16 filter — the last against ``inverse_filter_bf16_f64``, which
rounds the staged value exactly as the kernel documents, so that the bfloat16 path is held as tightly as the float32 one.

Every case prints one ``F64 invtf ...`` line (``-s`` shows them; DESIGN.md §3.2 keeps the table).  Bounds: tests/fft_metrics.py.
"""

import functools

import numpy as np
import pytest
import torch

from fft_metrics import INVTF_BF16_RMS_TOL, INVTF_BF16_VOXEL_TOL, INVTF_VOXEL_TOL, RMS_TOL, assert_fft_close, fft_errors
from invtf_cases import BF16_CASE, CASES, ENGINE, LIBRARY, NO_REG, PADDED, WAVE_PRIVATE, WAVE_PRIVATE_X, case_transfer_function, case_volume
from oracle import reference_f64 as R
from test_gpu_f64_parity import camera_volume, report

pytestmark = pytest.mark.gpu


assert len(WAVE_PRIVATE) == len(WAVE_PRIVATE_X)   # FAMILIES has one family per wave-private row length


def _id(f):
    return f"{f[2]} {f[1] or ''}".strip()


@functools.lru_cache(maxsize=2)
def _volume(shape):
    return torch.from_numpy(case_volume(shape)).cuda()


@functools.lru_cache(maxsize=4)
def _tf(kind, tshape):
    return torch.from_numpy(case_transfer_function(kind, tshape)).cuda()


def _padded(shape, pad):
    return (shape[0] + 2 * pad,) + tuple(shape[1:])


def run_f32(name, shape, kind, reg, normalize, pad=0, mirror=True):
    """The one-shot call (bench.py's ``apply_inv_tf``; its staged filter lives in the context's scratch) against float64."""
    from biahub_amd.apply_inverse_transfer_function import apply_inverse_transfer_function_zyx

    v, H = _volume(shape), _tf(kind, _padded(shape, pad))
    got = apply_inverse_transfer_function_zyx(v, H, pad, reg, normalize)
    ref = R.inverse_filter_f64(v, H, pad, reg, normalize, mirror=mirror)
    report(f"invtf {name} {shape} pad {pad} {kind} reg {reg:g} norm {int(normalize)} f32", fft_errors(got, ref))
    assert_fft_close(got, ref, RMS_TOL, INVTF_VOXEL_TOL, f"{name} {kind} f32")
    return got


def run_bf16(name, shape, kind, reg, normalize, pad=0):
    """A bfloat16 handle — accepted exactly on engine shapes, so creating it asserts the back-end — against the float64
    reference that rounds the staged filter as the kernel does."""
    from biahub_amd.apply_inverse_transfer_function import PreparedInverseFilter

    v, H = _volume(shape), _tf(kind, _padded(shape, pad))
    h = PreparedInverseFilter(H, shape, pad, reg, "bf16", v.device)
    got = h(v, normalize)
    h.close()
    ref = R.inverse_filter_bf16_f64(v, H, pad, reg, normalize)
    report(f"invtf {name} {shape} pad {pad} {kind} reg {reg:g} norm {int(normalize)} bf16", fft_errors(got, ref))
    assert_fft_close(got, ref, INVTF_BF16_RMS_TOL, INVTF_BF16_VOXEL_TOL, f"{name} {kind} bf16")
    return got


def assert_engine(shape, pad=0):
    from biahub_amd.apply_inverse_transfer_function import PreparedInverseFilter

    PreparedInverseFilter(_tf("real", _padded(shape, pad)), shape, pad, 1e-3, "bf16", "cuda").close()


def assert_library(shape, pad=0):
    from biahub_amd.apply_inverse_transfer_function import PreparedInverseFilter

    with pytest.raises(ValueError, match="bfloat16"):
        PreparedInverseFilter(_tf("real", _padded(shape, pad)), shape, pad, 1e-3, "bf16", "cuda")


# ----------------------------------------------------------------------------- every engine family
@pytest.mark.parametrize("case", list(CASES) + ["bf16"])
@pytest.mark.parametrize("shape,env,what", ENGINE, ids=[_id(f) for f in ENGINE])
def test_inverse_filter_family_vs_float64(gpu, shape, env, what, case, monkeypatch):
    """complex: 0.3 (N + iN), reg 1e-2, normalised (on wave-private rows the fused x / mean - 1 load of the forward X pass);
    complex_offset: 1 + 0.3 (N + iN), reg 1e-3; real: 0.5 N, reg 1e-3; bf16: complex_offset with the bfloat16 filter."""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    assert_engine(shape)
    name = f"{what} {env or ''}".strip()
    if case == "bf16":
        run_bf16(name, shape, *BF16_CASE)
    else:
        run_f32(name, shape, *CASES[case])


@pytest.mark.parametrize("shape,env,what", WAVE_PRIVATE, ids=[_id(f) for f in WAVE_PRIVATE])
def test_inverse_filter_staged_normalisation(gpu, shape, env, what, monkeypatch):
    """The rows whose normalisation rides in the forward X pass, once more on the tile X passes (BH_FC_XW=0): normalize_pad_kernel
    stages x / mean - 1 (the fused form of the same rows runs in test_inverse_filter_family_vs_float64)."""
    monkeypatch.setenv("BH_FC_XW", "0")
    assert_engine(shape)
    for case in ("complex", "complex_offset"):
        kind, reg, _ = CASES[case]
        run_f32(f"{what} staged norm", shape, kind, reg, True)


# ----------------------------------------------------------------------------- z padding on the engine
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("shape,pad,bf16,note", PADDED, ids=[p[3] for p in PADDED])
def test_inverse_filter_z_padding_on_the_engine(gpu, shape, pad, bf16, note, normalize):
    """The staged-input path: mirrored (or, pad >= Z, zero) pad planes written by normalize_pad_kernel, the transforms in
    place on the padded buffer, the crop — at padded Z of 3 * 2^k and 5 * 2^k too."""
    assert_engine(shape, pad)
    kind, reg, _ = CASES["complex_offset"]
    run_f32(note, shape, kind, reg, normalize, pad)
    if bf16:
        run_bf16(note, shape, kind, reg, normalize, pad)


def test_inverse_filter_zero_pad_planes(gpu, monkeypatch):
    """BH_INVTF_ZPAD=zeros: constant-zero pad planes, against the reference with zero planes."""
    monkeypatch.setenv("BH_INVTF_ZPAD", "zeros")
    kind, reg, _ = CASES["complex_offset"]
    got = run_f32("zero pad planes", (20, 96, 192), kind, reg, True, 2, mirror=False)
    mirrored = R.inverse_filter_f64(_volume((20, 96, 192)), _tf(kind, (24, 96, 192)), 2, reg, True)
    assert fft_errors(got, mirrored)[0] > 1e-2   # and the switch did change the planes


# ----------------------------------------------------------------------------- the library path
@pytest.mark.parametrize("shape,pad,env", LIBRARY)
def test_inverse_filter_library_path_vs_float64(gpu, shape, pad, env, monkeypatch):
    """hipFFT R2C -> one pointwise kernel -> C2R: odd X and the X / 2 + 1 mirror column, with and without z padding, and an
    engine shape sent there by BH_FFT_BACKEND=hipfft."""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    assert_library(shape, pad)
    for case in CASES:
        kind, reg, normalize = CASES[case]
        run_f32("library", shape, kind, reg, normalize, pad)


@pytest.mark.parametrize("shape", NO_REG)
def test_inverse_filter_without_regularisation(gpu, shape):
    """reg = 0 with |H| in [0.5, 1.5] and a random phase: the filter is the exact inverse 1 / H (its Hermitian part)."""
    run_f32("reg 0", shape, "unit", 0.0, False)
    run_f32("reg 0", shape, "unit", 0.0, True)


# ----------------------------------------------------------------------------- handles and scratch
def test_prepared_filter_equals_one_shot_and_reuses_the_pooled_block(gpu):
    """A handle applied to three volumes is bit-equal to the one-shot call on each; destroyed, its block goes to the pool and the
    next handle of that size — another H — receives it and must match its own one-shot call bit for bit."""
    from biahub_amd.apply_inverse_transfer_function import PreparedInverseFilter, apply_inverse_transfer_function_zyx

    shape = (24, 96, 192)
    vols = [torch.from_numpy(camera_volume(shape, seed=s)).to(gpu) for s in (1, 2, 3)]
    Ha, Hb = _tf("complex_offset", shape), _tf("complex", shape)
    for H, reg, normalize in ((Ha, 1e-3, False), (Hb, 1e-2, True)):
        h = PreparedInverseFilter(H, shape, 0, reg, "f32", gpu)
        for v in vols:
            assert torch.equal(h(v, normalize), apply_inverse_transfer_function_zyx(v, H, 0, reg, normalize))
        h.close()
    ref = R.inverse_filter_f64(vols[0], Hb, 0, 1e-2, True)
    assert_fft_close(apply_inverse_transfer_function_zyx(vols[0], Hb, 0, 1e-2, True), ref, RMS_TOL, INVTF_VOXEL_TOL, "second handle")


def test_one_shot_scratch_shared_between_f32_and_bf16(gpu):
    """The one-shot form keeps its staged filter in the context's grow-only ``itf_filter`` scratch: float32 (8 B per bin) and
    bfloat16 (4 B per bin) calls alternate in it at one shape and every result stays what it was."""
    from biahub_amd.apply_inverse_transfer_function import apply_inverse_transfer_function_zyx

    shape = (16, 32, 320)
    v, H = _volume(shape), _tf("complex_offset", shape)
    first = {}
    for rep in range(3):
        for storage in ("bf16", "f32"):
            got = apply_inverse_transfer_function_zyx(v, H, 0, 1e-3, False, storage)
            assert torch.equal(got, first.setdefault(storage, got)), (rep, storage)
    assert not torch.equal(first["f32"], first["bf16"])
    assert_fft_close(first["f32"], R.inverse_filter_f64(v, H, 0, 1e-3, False), RMS_TOL, INVTF_VOXEL_TOL, "f32 after bf16")
    assert_fft_close(first["bf16"], R.inverse_filter_bf16_f64(v, H, 0, 1e-3, False), INVTF_BF16_RMS_TOL, INVTF_BF16_VOXEL_TOL,
                     "bf16 before f32")


def test_deconvolve_equals_the_handle(gpu):
    """``deconvolve(czyx, transfer_function=real H)`` at a radix-3 shape is the prepared inverse filter: equal to the handle's
    result, and both to float64 (a real H without symmetry: the mirror bins matter here too)."""
    from biahub_amd.apply_inverse_transfer_function import PreparedInverseFilter
    from biahub_amd.deconvolve import deconvolve

    shape = (24, 96, 192)
    v, H = _volume(shape), _tf("real", shape)
    got = deconvolve(v.cpu().numpy()[None], transfer_function=H.cpu().numpy(), regularization_strength=1e-3)[0]
    h = PreparedInverseFilter(H, shape, 0, 1e-3, "f32", gpu)
    want = h(v, False)
    h.close()
    assert np.array_equal(got, want.cpu().numpy())
    assert_fft_close(got, R.inverse_filter_f64(v, H, 0, 1e-3, False), RMS_TOL, INVTF_VOXEL_TOL, "deconvolve, real H")
