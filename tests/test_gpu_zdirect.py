"""GPU: the direct Z pass of Richardson-Lucy (compact z taps, fftconv_zdirect.inc) against the float64 reference.

When a PSF's z-extent fits the compiled taps (R = pz // 2 <= 16, columns longer than 2R), a prepared handle keeps R + 1
Hermitian or 2R + 1 general taps per (ky, kx) column instead of the full transfer function, and its Z passes convolve along z
directly (``PreparedRichardsonLucy.z_pass == "direct"``).  Each case here asserts the path and holds 10 iterations to the same
bounds as test_gpu_f64_parity.py.  The FFT Z kernels keep their coverage: their families re-run with ``BH_RL_ZDIRECT=0``.
"""

import numpy as np
import pytest
import torch

from fft_metrics import RMS_TOL, VOXEL_TOL, assert_fft_close, fft_errors
from oracle import reference_f64 as R
from test_gpu_f64_parity import EPS, FAMILIES, ITS, camera_volume, psf_of, report

pytestmark = pytest.mark.gpu


def run_rl_zpass(gpu, vol, psf, backend, z_pass, z_taps=None):
    """The prepared handle (back-end and Z pass asserted) and the float64 reference, both on the GPU."""
    from biahub_amd.deconvolve import PreparedRichardsonLucy, richardson_lucy_plan

    shape = tuple(vol.shape)
    assert richardson_lucy_plan(psf.shape, shape)[1] == backend
    v = torch.from_numpy(vol).to(gpu)
    with PreparedRichardsonLucy(psf, shape, gpu) as h:
        assert h.backend == backend
        assert h.otf_is_real == (backend != "library" and R.psf_is_point_symmetric(psf))
        assert h.z_pass == z_pass, (shape, psf.shape, h.z_pass)
        if z_taps is not None:
            assert h.z_taps == z_taps, (shape, psf.shape, h.z_taps)
        got = h(v, ITS, EPS)
        torch.cuda.synchronize(gpu)
    ref = R.richardson_lucy_f64(v, psf, ITS, EPS)
    return got, ref


def check(gpu, name, vol, psf, backend, z_pass, z_taps=None):
    got, ref = run_rl_zpass(gpu, vol, psf, backend, z_pass, z_taps)
    errs = fft_errors(got, ref)
    report(f"zdirect {name} {tuple(vol.shape)} psf {tuple(psf.shape)} {z_pass}", errs)
    assert_fft_close(got, ref, RMS_TOL, VOXEL_TOL, name)


# (shape, pshape, back-end, what): the column lengths the engine's Z passes exist for
ZLENGTHS = [
    ((512, 32, 64), (7, 3, 5), "engine", "Z of 512"),
    ((384, 32, 64), (7, 3, 5), "engine", "Z of 384"),
    ((256, 64, 128), (9, 5, 5), "engine", "Z of 256"),
    ((768, 32, 64), (5, 5, 3), "engine", "Z of 768"),
    ((384, 64, 160), (9, 5, 5), "engine-padded", "Z of 384 at a padded box"),
    ((21, 64, 1500), (7, 5, 9), "engine-padded", "wrap-padded box (32, 64, 1536)"),
    ((21, 64, 150), (7, 5, 9), "engine-padded", "padded box (32, 64, 256), fold path"),
]


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("shape,pshape,backend,what", ZLENGTHS, ids=[f[3] for f in ZLENGTHS])
def test_direct_z_lengths(gpu, shape, pshape, backend, what, kind):
    vol = camera_volume(shape, seed=sum(shape) + 7)
    check(gpu, f"{what} {kind}", vol, psf_of(pshape, kind), backend, "direct")


# z-extents: 1 and 3 (radius 4 taps), 32 and 33 (the largest radius, 16: an even extent leaves tap +16 zero)
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("pz,taps", [(1, 9), (3, 9), (9, 9), (10, 33), (32, 33), (33, 33)])
def test_direct_z_extents(gpu, pz, taps, kind):
    shape = (64, 32, 64)
    vol = camera_volume(shape, seed=pz + 3)
    check(gpu, f"z-extent {pz} {kind}", vol, psf_of((pz, 3, 5), kind), "engine", "direct", taps)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("Z", [64, 512])
def test_direct_z_wrap_impulses(gpu, Z, kind):
    """Bright voxels on the first two and the last two planes: their blur wraps round z through the held-back rows."""
    shape = (Z, 32, 64)
    vol = camera_volume(shape, seed=Z, n_beads=4)
    rng = np.random.default_rng(Z + 1)
    for z in (0, 1, Z - 2, Z - 1):
        for _ in range(3):
            vol[z, rng.integers(0, shape[1]), rng.integers(0, shape[2])] = rng.uniform(2000.0, 9000.0)
    check(gpu, f"wrap impulses {kind}", vol, psf_of((33, 3, 5), kind), "engine", "direct", 33)


@pytest.mark.parametrize("shape", [(64, 32, 128), (64, 32, 2048)], ids=["pitch 80", "pitch 1040"])
def test_direct_z_strips_straddle_rows(gpu, shape):
    """A wavefront's 64 columns are flattened (y, kx): with a row pitch that is no multiple of 64 (80, and the bench's 1040)
    strips straddle two spectrum rows, pad columns included."""
    vol = camera_volume(shape, seed=sum(shape))
    check(gpu, "straddling strips", vol, psf_of((33, 5, 5), "real"), "engine", "direct", 33)


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("shape,pz", [((64, 32, 64), 35), ((32, 32, 64), 32)], ids=["too tall", "column too short"])
def test_fft_z_fallback(gpu, shape, pz, kind):
    """A PSF taller than the largest taps (R 17), or columns no longer than 2R: the full transfer function and the FFT Z pass."""
    vol = camera_volume(shape, seed=pz)
    check(gpu, f"fallback {kind}", vol, psf_of((pz, 3, 5), kind), "engine", "fft", 0)


def test_bench_shape_reports_direct(gpu):
    """bench.py's volume and PSF run the direct Z pass, and the handle keeps 17 Hermitian tap planes."""
    from biahub_amd.deconvolve import PreparedRichardsonLucy

    shape, pshape, sigma = (512, 2048, 2048), (33, 17, 17), (3.0, 1.5, 1.5)
    ax = [torch.arange(n, dtype=torch.float64, device=gpu) - (n - 1) / 2 for n in pshape]
    g = [torch.exp(-0.5 * (a / s) ** 2) for a, s in zip(ax, sigma)]
    psf = g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    psf = (psf / psf.sum()).to(torch.float32)
    with PreparedRichardsonLucy(psf, shape, gpu) as h:
        assert h.backend == "engine" and h.otf_is_real
        assert (h.z_pass, h.z_taps) == ("direct", 33)
        assert h.otf_bytes == 17 * 2048 * (2048 // 2 + 16) * 8


# the FFT Z kernels' own families (colz, colz3, the radix-4 and LDS Z passes) with the direct pass switched off
FFT_Z = [f for f in FAMILIES if any(k in f[4] for k in ("colz", "radix-4 Z", "LDS Z", "Z of 256", "Z of 1024"))]


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("shape,pshape,env,backend,what", FFT_Z, ids=[f[4] for f in FFT_Z])
def test_fft_z_families_with_zdirect_off(gpu, shape, pshape, env, backend, what, kind, monkeypatch):
    for k, val in {**env, "BH_RL_ZDIRECT": "0"}.items():
        monkeypatch.setenv(k, val)
    vol = camera_volume(shape, seed=sum(shape) + len(what))
    check(gpu, f"{what} {kind} {env}", vol, psf_of(pshape, kind), backend, "fft", 0)
