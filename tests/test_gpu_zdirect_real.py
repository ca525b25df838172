"""GPU: the real-tap kernels of the direct Z pass (fftconv_zdirect.inc, REALQ) against the float64 reference.

Q(t; ky, kx), the PSF transformed along x and y only, is real when the y and x extents are odd and every z-slice equals its
own 180-degree rotation in (y, x).  A prepared handle decides that once, bit for bit (``PreparedRichardsonLucy.z_taps_real``),
writes the imaginary halves of its compact z taps as zero and runs kernels that never read them:

* point-symmetric as well (``mirror``): R + 1 real, even taps, one packed add and one packed FMA per tap pair;
* slice-symmetric only (``aberrated``: asymmetric along z): 2R + 1 real taps, convolution and correlation still differ;
* point-symmetric with slices that are not symmetric (``sheared``), a near miss, even y / x extents and the two switches keep
  the complex-tap kernels, which keeps the Hermitian kernel covered now that the Gaussian cases of test_gpu_zdirect.py moved.

Every case asserts the path the handle reports and holds 10 iterations to the bounds of test_gpu_f64_parity.py.

Walk lengths.  A wave's walk is unrolled by P = 2R + 1 + D rows and runs whole chunks while z0 + P - 1 + R + D < Z, then a
tail.  Radius 16: the real, even kernel keeps D = 12 rows in flight (P = 45, whole chunks from Z > 72: 80 and 96 are the first
such lengths, 40 / 48 / 64 run the tail alone); the real general kernel D = 6 (P = 39, whole chunks from Z > 60: 64 and 80;
40 / 48 tail only).  Radius 4 keeps D = 8 in every kernel (P = 17, whole chunks from Z > 28).  Recompute these if a D changes.
"""

import numpy as np
import pytest
import torch

from fft_metrics import RMS_TOL, VOXEL_TOL, assert_fft_close, fft_errors
from oracle import reference_f64 as R
from test_gpu_f64_parity import EPS, ITS, camera_volume, psf_of, report
from test_gpu_zdirect import ZLENGTHS

pytestmark = pytest.mark.gpu


# ---- PSFs and the predicate (host side, numpy; also imported by test_zdirect_real_host.py) ----
def slices_symmetric(psf) -> bool:
    """Odd y and x extents and every z-slice equal to its own 180-degree rotation, bit for bit: Q is real."""
    p = np.ascontiguousarray(psf, dtype=np.float32).view(np.uint32)
    return bool(p.shape[1] % 2 and p.shape[2] % 2 and np.array_equal(p, p[:, ::-1, ::-1]))


def _axes(pshape):
    return [np.arange(n, dtype=np.float64) - (n - 1) / 2 for n in pshape]


def aberrated_psf(pshape):
    """a(z) G_sigma(z)(y, x), a and sigma growing with z: every slice symmetric, the stack asymmetric along z."""
    az, ay, ax = _axes(pshape)
    zn = (np.arange(pshape[0]) + 0.5) / pshape[0]
    a = 1.0 + zn
    sy = max(pshape[1] / 4.0, 0.8) * (0.75 + 0.5 * zn)
    sx = max(pshape[2] / 4.0, 0.8) * (0.75 + 0.5 * zn)
    p = a[:, None, None] * np.exp(-0.5 * (ay[None, :, None] / sy[:, None, None]) ** 2) * np.exp(-0.5 * (ax[None, None, :] / sx[:, None, None]) ** 2)
    return (p / p.sum()).astype(np.float32)


def sheared_psf(pshape):
    """A Gaussian whose y-centre moves by half a pixel per plane, made point-symmetric bit for bit: the transfer function is
    real, the slices are not symmetric, Q is complex."""
    az, ay, ax = _axes(pshape)
    s = [max(n / 4.0, 0.8) for n in pshape]
    p = (np.exp(-0.5 * (az / s[0]) ** 2)[:, None, None] * np.exp(-0.5 * ((ay[None, :, None] - 0.5 * az[:, None, None]) / s[1]) ** 2)
         * np.exp(-0.5 * (ax / s[2]) ** 2)[None, None, :])
    p = (p + p[::-1, ::-1, ::-1]) / 2
    return (p / p.sum()).astype(np.float32)


def near_miss_psf(pshape):
    """The mirror PSF with one voxel moved to the next float32."""
    p = psf_of(pshape, "real").copy()
    i = (pshape[0] // 2, 0, pshape[2] - 1)
    p[i] = np.nextafter(p[i], np.float32(1.0))
    return p


def psf_kind(pshape, kind):
    if kind == "mirror":
        return psf_of(pshape, "real")
    if kind == "complex":
        return psf_of(pshape, "complex")
    return {"aberrated": aberrated_psf, "sheared": sheared_psf, "near miss": near_miss_psf}[kind](pshape)


# ---- the check ----
def check_real(gpu, name, vol, psf, backend, z_taps, *, otf_is_real=None, z_taps_real=None):
    """test_gpu_zdirect.check with the path asserted in full: back-end, direct pass, tap count, real transfer function, real
    taps (by default what the PSF's symmetries say).  Bounds: RMS_TOL / VOXEL_TOL against the float64 reference."""
    from biahub_amd.deconvolve import PreparedRichardsonLucy, richardson_lucy_plan

    shape = tuple(vol.shape)
    assert richardson_lucy_plan(psf.shape, shape)[1] == backend
    want_otf = R.psf_is_point_symmetric(psf) if otf_is_real is None else otf_is_real
    want_taps = slices_symmetric(psf) if z_taps_real is None else z_taps_real
    v = torch.from_numpy(vol).to(gpu)
    with PreparedRichardsonLucy(psf, shape, gpu) as h:
        got_path = (h.backend, h.z_pass, h.z_taps, h.otf_is_real, h.z_taps_real)
        assert got_path == (backend, "direct", z_taps, want_otf, want_taps), (name, shape, psf.shape, got_path)
        got = h(v, ITS, EPS)
        torch.cuda.synchronize(gpu)
    ref = R.richardson_lucy_f64(v, psf, ITS, EPS)
    errs = fft_errors(got, ref)
    report(f"zdirect-real {name} {shape} psf {tuple(psf.shape)} real taps {want_taps}", errs)
    assert_fft_close(got, ref, RMS_TOL, VOXEL_TOL, name)


REAL_KINDS = ["mirror", "aberrated"]


@pytest.mark.parametrize("kind", REAL_KINDS)
@pytest.mark.parametrize("Z", [40, 48, 64, 80, 96, 512])
def test_real_taps_z_lengths(gpu, Z, kind):
    """Tail-only walks, the first lengths with a whole unrolled chunk (module docstring), and the bench's column length."""
    shape, pshape = (Z, 32, 64), (33, 3, 5)
    psf = psf_kind(pshape, kind)
    assert slices_symmetric(psf) and R.psf_is_point_symmetric(psf) == (kind == "mirror")
    check_real(gpu, f"Z {Z} {kind}", camera_volume(shape, seed=Z + 11), psf, "engine", 33)


@pytest.mark.parametrize("kind", REAL_KINDS)
@pytest.mark.parametrize("Z", [16, 24, 32])
def test_real_taps_radius_4_lengths(gpu, Z, kind):
    """Radius 4 keeps D = 8 (P = 17): whole chunks from Z > 28, so 16 and 24 run the tail alone and 32 one whole chunk."""
    shape = (Z, 32, 64)
    check_real(gpu, f"R 4 Z {Z} {kind}", camera_volume(shape, seed=Z + 13), psf_kind((9, 3, 5), kind), "engine", 9)


# radius 4 (9 taps) and radius 16 (33 taps; an even extent leaves tap +16 zero and is never point-symmetric)
@pytest.mark.parametrize("kind", REAL_KINDS)
@pytest.mark.parametrize("pz,taps", [(1, 9), (3, 9), (9, 9), (10, 33), (32, 33), (33, 33)])
def test_real_taps_z_extents(gpu, pz, taps, kind):
    shape = (64, 32, 64)
    check_real(gpu, f"z-extent {pz} {kind}", camera_volume(shape, seed=pz + 5), psf_kind((pz, 3, 5), kind), "engine", taps)


@pytest.mark.parametrize("kind", REAL_KINDS)
@pytest.mark.parametrize("Z", [64, 80])
def test_real_taps_wrap_impulses(gpu, Z, kind):
    """Bright voxels on the first two and the last two planes: their blur wraps round z through the stash of rows 0 .. R - 1."""
    shape = (Z, 32, 64)
    vol = camera_volume(shape, seed=Z, n_beads=4)
    rng = np.random.default_rng(Z + 1)
    for z in (0, 1, Z - 2, Z - 1):
        for _ in range(3):
            vol[z, rng.integers(0, shape[1]), rng.integers(0, shape[2])] = rng.uniform(2000.0, 9000.0)
    check_real(gpu, f"wrap impulses {kind}", vol, psf_kind((33, 3, 5), kind), "engine", 33)


@pytest.mark.parametrize("kind", REAL_KINDS)
@pytest.mark.parametrize("shape", [(64, 32, 128), (64, 32, 2048)], ids=["pitch 80", "pitch 1040"])
def test_real_taps_strips_straddle_rows(gpu, shape, kind):
    """Row pitches that are no multiple of 64 (80, and the bench's 1040): strips straddle two spectrum rows, pad columns included."""
    check_real(gpu, f"straddling strips {kind}", camera_volume(shape, seed=sum(shape)), psf_kind((33, 5, 5), kind), "engine", 33)


PADDED = [z for z in ZLENGTHS if z[3] in ("wrap-padded box (32, 64, 1536)", "padded box (32, 64, 256), fold path")]


@pytest.mark.parametrize("kind", REAL_KINDS)
@pytest.mark.parametrize("shape,pshape,backend,what", PADDED, ids=[z[3] for z in PADDED])
def test_real_taps_padded_boxes(gpu, shape, pshape, backend, what, kind):
    assert len(PADDED) == 2
    check_real(gpu, f"{what} {kind}", camera_volume(shape, seed=sum(shape) + 7), psf_kind(pshape, kind), backend, 9)


@pytest.mark.parametrize("pshape,taps", [((9, 5, 5), 9), ((33, 5, 5), 33)])
def test_sheared_psf_keeps_the_hermitian_complex_taps(gpu, pshape, taps):
    """Point-symmetric, slices not symmetric: a real transfer function and complex taps (zdirect_kernel<R, COL_FILTER, false>)."""
    shape = (80, 32, 64)
    psf = sheared_psf(pshape)
    assert R.psf_is_point_symmetric(psf) and not slices_symmetric(psf)
    check_real(gpu, "sheared", camera_volume(shape, seed=taps), psf, "engine", taps, otf_is_real=True, z_taps_real=False)


def test_near_miss_keeps_the_complex_taps(gpu):
    shape, pshape = (64, 32, 64), (33, 3, 5)
    psf = near_miss_psf(pshape)
    assert slices_symmetric(psf_of(pshape, "real")) and not slices_symmetric(psf)
    check_real(gpu, "near miss", camera_volume(shape, seed=3), psf, "engine", 33, otf_is_real=False, z_taps_real=False)


@pytest.mark.parametrize("pshape", [(33, 4, 5), (33, 3, 4)], ids=["even y", "even x"])
def test_even_y_or_x_extent_keeps_the_complex_taps(gpu, pshape):
    shape = (64, 32, 64)
    check_real(gpu, "even extent", camera_volume(shape, seed=sum(pshape)), psf_of(pshape, "real"), "engine", 33, otf_is_real=False,
               z_taps_real=False)


@pytest.mark.parametrize("env,otf_is_real", [("BH_RL_ZREAL=0", True), ("BH_RL_COMPLEX_OTF=1", False)])
def test_switches_keep_the_complex_taps(gpu, env, otf_is_real, monkeypatch):
    """Both are read when the handle is created."""
    monkeypatch.setenv(*env.split("="))
    shape = (64, 32, 64)
    check_real(gpu, env, camera_volume(shape, seed=9), psf_of((33, 3, 5), "real"), "engine", 33, otf_is_real=otf_is_real, z_taps_real=False)
