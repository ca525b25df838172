"""GPU: every family of the FFT engine against the float64 reference (oracle/reference_f64.py), per voxel, at 10 iterations.

test_gpu_parity.py holds the engine to the float32 oracle with the max-normalised ``rel_err <= 1e-4``, which lets through
defects that touch only the dim voxels (tests/test_fft_reference.py plants three).  Here each code path — named by its shape
and A/B switch, its back-end asserted — runs Richardson-Lucy (10 iterations; a real and a complex transfer function) and,
where the engine has it, Tikhonov, and is held to ``rms_rel`` / ``voxel_rel`` (tests/fft_metrics.py).  The reference runs in
float64 on the GPU through torch's FFTs (the vendor library), independent of the project's kernels.

Every case prints one ``F64 ...`` line with its measured errors (``-s`` shows them; DESIGN.md §3.2 keeps the table).
"""

import time

import numpy as np
import pytest
import torch

from fft_metrics import RMS_TOL, TIK_VOXEL_TOL, VOXEL_TOL, assert_fft_close, fft_errors
from oracle import oracle_np as O
from oracle import reference_f64 as R

pytestmark = pytest.mark.gpu

ITS = 10
EPS = 1e-6


def camera_volume(shape, seed, n_beads=None, background=110.0, noise=4.0, amp=(200.0, 4000.0)):
    """bench.synthetic_position's kind of volume on the host: offset + Gaussian noise + 7-voxel beads (wrapped at the faces,
    so beads sit on them too), rounded to counts."""
    rng = np.random.default_rng(seed)
    v = rng.normal(background, noise, shape) if noise else np.full(shape, background)
    n = n_beads if n_beads is not None else max(16, int(np.prod(shape)) // 2**14)
    c = [rng.integers(0, s, n) for s in shape]
    a = rng.uniform(amp[0], amp[1], n)
    for dz, dy, dx, w in ((0, 0, 0, 1.0), (1, 0, 0, 0.6), (-1, 0, 0, 0.6), (0, 1, 0, 0.6), (0, -1, 0, 0.6), (0, 0, 1, 0.6),
                          (0, 0, -1, 0.6)):
        np.add.at(v, ((c[0] + dz) % shape[0], (c[1] + dy) % shape[1], (c[2] + dx) % shape[2]), a * w)
    return np.clip(np.round(v), 0, 65535).astype(np.float32)


def psf_of(pshape, kind):
    psf = O.gaussian_psf(pshape, tuple(max(p / 4.0, 0.8) for p in pshape))
    if kind == "complex":
        psf = psf.copy()
        psf[0, 0, 0] += 0.02   # asymmetric: conv and corr differ, the transfer function is complex
    return psf


def report(name, errs, extra=""):
    print(f"F64 {name}: rms_rel {errs[0]:.2e} voxel_rel {errs[1]:.2e} maxnorm {errs[2]:.2e} {extra}".rstrip())


def run_rl(gpu, vol, psf, backend, its=ITS, box=None):
    """The engine through the prepared handle (its back-end asserted) and the float64 reference, both on the GPU."""
    from biahub_amd.deconvolve import PreparedRichardsonLucy, richardson_lucy_plan

    shape = tuple(vol.shape)
    plan_box, plan_backend = richardson_lucy_plan(psf.shape, shape)
    assert plan_backend == backend, (shape, psf.shape, plan_backend)
    if box is not None:
        assert plan_box == box, (shape, plan_box)
    v = torch.from_numpy(vol).to(gpu)
    with PreparedRichardsonLucy(psf, shape, gpu) as h:
        assert h.backend == backend
        assert h.otf_is_real == (backend != "library" and R.psf_is_point_symmetric(psf))
        got = h(v, its, EPS)
        torch.cuda.synchronize(gpu)
    ref = R.richardson_lucy_f64(v, psf, its, EPS)
    return got, ref


# (shape, pshape, switches, back-end, what runs) — one case per code path of the engine
FAMILIES = [
    ((8, 64, 512), (3, 5, 7), {}, "engine", "xw rows of 512 (4 pairs / wave)"),
    ((4, 64, 1024), (3, 7, 7), {}, "engine", "xw rows of 1024"),
    ((8, 32, 2048), (5, 5, 9), {}, "engine", "xw rows of 2048"),
    ((8, 32, 1536), (3, 5, 9), {}, "engine", "x3 rows of 1536"),
    ((4, 64, 3072), (3, 3, 11), {}, "engine", "x3 rows of 3072"),
    ((8, 64, 512), (3, 5, 7), {"BH_FC_XW": "0"}, "engine", "tile X passes, rows of 512"),
    ((8, 32, 1536), (3, 5, 9), {"BH_FC_XW": "0"}, "engine", "tile X passes, rows of 1536"),
    ((16, 32, 320), (3, 3, 5), {}, "engine", "tile X passes, rows of 5 * 64"),
    ((8, 32, 2560), (3, 3, 3), {}, "engine", "tile X passes, rows of 5 * 512"),
    ((40, 160, 64), (5, 5, 3), {}, "engine", "radix-5 columns"),
    ((256, 64, 128), (9, 5, 5), {}, "engine", "colw Z of 256"),
    ((1024, 32, 64), (11, 3, 3), {"BH_FC_COLW": "1"}, "engine", "colw Z of 1024"),
    ((4, 512, 64), (3, 9, 5), {}, "engine", "colw Y of 256"),
    ((8, 1024, 128), (3, 7, 5), {}, "engine", "colw Y of 512"),
    ((4, 2048, 64), (3, 11, 3), {}, "engine", "colw Y of 1024"),
    ((256, 64, 128), (9, 5, 5), {"BH_FC_COLW": "0"}, "engine", "LDS columns, Z of 256"),
    ((8, 1024, 128), (3, 7, 5), {"BH_FC_COLW": "0"}, "engine", "LDS columns, Y of 512"),
    ((512, 32, 64), (7, 3, 5), {}, "engine", "colz radix-8 Z of 512"),
    ((512, 64, 192), (9, 5, 5), {}, "engine", "colz, ragged column tile"),
    ((512, 32, 64), (7, 3, 5), {"BH_FC_COLZ": "0"}, "engine", "radix-4 Z of 512"),
    ((384, 32, 64), (7, 3, 5), {}, "engine", "colz3 Z of 384"),
    ((384, 64, 160), (9, 5, 5), {}, "engine-padded", "colz3 Z of 384 at a padded box, ragged column tile"),
    ((768, 32, 64), (5, 5, 3), {}, "engine", "colz3 Z of 768"),
    ((384, 32, 64), (7, 3, 5), {"BH_FC_COLZ3": "0"}, "engine", "LDS Z of 384"),
    ((768, 32, 64), (5, 5, 3), {"BH_FC_COLZ3": "0"}, "engine", "LDS Z of 768"),
    ((21, 64, 1500), (7, 5, 9), {}, "engine-padded", "wrap-padded box (32, 64, 1536)"),
    ((12, 32, 500), (5, 3, 7), {}, "engine-padded", "wrap-padded box, rows of 512"),
    ((21, 64, 1500), (7, 5, 9), {"BH_RL_NOWRAP": "1"}, "engine-padded", "padded box, fold path"),
    ((21, 64, 150), (7, 5, 9), {}, "engine-padded", "padded box (32, 64, 256), fold path"),
    ((15, 21, 25), (5, 3, 3), {}, "library", "hipFFT at an awkward shape"),
    ((37, 53, 71), (7, 5, 9), {"BH_RL_ENGINE_PAD": "0"}, "library", "hipFFT pad-and-fold box"),
    ((32, 64, 128), (4, 5, 5), {}, "engine", "even PSF extent along z"),
    ((32, 64, 128), (5, 6, 5), {}, "engine", "even PSF extent along y"),
    ((32, 64, 128), (5, 5, 8), {}, "engine", "even PSF extent along x"),
    ((10, 32, 3000), (3, 3, 8), {}, "engine-padded", "even x extent, wrap margins differ"),
]


@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("shape,pshape,env,backend,what", FAMILIES, ids=[f[4] for f in FAMILIES])
def test_richardson_lucy_family_vs_float64(gpu, shape, pshape, env, backend, what, kind, monkeypatch):
    """Richardson-Lucy, 10 iterations, on a camera-like volume (beads on the faces too) against float64, per voxel."""
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    vol = camera_volume(shape, seed=sum(shape) + len(what))
    psf = psf_of(pshape, kind)
    got, ref = run_rl(gpu, vol, psf, backend)
    errs = fft_errors(got, ref)
    report(f"rl {what} {shape} psf {pshape} {kind} {env or ''}", errs)
    assert_fft_close(got, ref, RMS_TOL, VOXEL_TOL, f"{what} {kind}")


TIKHONOV = [f for f in FAMILIES if f[3] == "engine" and all(p % 2 for p in f[1])]


@pytest.mark.parametrize("shape,pshape,env,backend,what", TIKHONOV, ids=[f[4] for f in TIKHONOV])
def test_tikhonov_family_vs_float64(gpu, shape, pshape, env, backend, what, monkeypatch):
    """The Tikhonov filter (bh_tikhonov) with the reference's transfer function at reg 1e-3 against float64."""
    from biahub_amd.deconvolve import tikhonov_zyx

    for k, val in env.items():
        monkeypatch.setenv(k, val)
    vol = camera_volume(shape, seed=sum(shape) + 1)
    H = O.compute_transfer_function(psf_of(pshape, "real"), shape)
    v = torch.from_numpy(vol).to(gpu)
    got = tikhonov_zyx(v, torch.from_numpy(H).to(gpu), 1e-3)
    ref = R.tikhonov_f64(v, H, 1e-3, device=gpu)
    errs = fft_errors(got, ref)
    report(f"tikhonov {what} {shape} {env or ''}", errs)
    assert_fft_close(got, ref, RMS_TOL, TIK_VOXEL_TOL, f"tikhonov {what}")


# ----------------------------------------------------------------------------- edge inputs
EDGE_PATHS = [((8, 64, 512), (5, 5, 7), "engine"), ((12, 32, 500), (5, 3, 7), "engine-padded"), ((21, 64, 150), (7, 5, 9), "engine-padded"),
              ((15, 21, 25), (5, 3, 3), "library")]


@pytest.mark.parametrize("shape,pshape,backend", EDGE_PATHS)
def test_richardson_lucy_corner_impulses(gpu, shape, pshape, backend):
    """A single bright voxel at (0, 0, 0), then at (Z-1, Y-1, X-1), on a flat background: all of the blur around it comes
    across the wrap on three faces at once (complex transfer function: convolution and correlation wrap opposite ways)."""
    psf = psf_of(pshape, "complex")
    for corner in ((0, 0, 0), tuple(s - 1 for s in shape)):
        vol = np.full(shape, 100.0, np.float32)
        vol[corner] = 5000.0
        got, ref = run_rl(gpu, vol, psf, backend)
        report(f"impulse {corner} {backend} {shape}", fft_errors(got, ref))
        assert_fft_close(got, ref, RMS_TOL, VOXEL_TOL, f"impulse at {corner}, {backend}")


@pytest.mark.parametrize("shape,pshape,backend", EDGE_PATHS)
def test_richardson_lucy_dynamic_range_and_exact_zeros(gpu, shape, pshape, backend):
    """65535-count beads on a zero background (the blur spans 0 .. 6e4 and meets the eps floor), and a volume with exact-zero
    regions and negative voxels: wherever d <= 0 the estimate is EXACTLY 0 after any number of iterations (e0 = max(d, 0) = 0
    and every update multiplies), a per-voxel check of the clamp."""
    psf = psf_of(pshape, "complex")
    beads = camera_volume(shape, seed=5, n_beads=24, background=0.0, noise=0.0, amp=(65535.0, 65535.0))
    got, ref = run_rl(gpu, beads, psf, backend)
    report(f"beads 65535 {backend} {shape}", fft_errors(got, ref))
    assert_fft_close(got, ref, RMS_TOL, VOXEL_TOL, f"65535 beads, {backend}")
    assert bool((got[torch.from_numpy(beads).to(gpu) == 0] == 0).all())

    vol = camera_volume(shape, seed=6)
    rng = np.random.default_rng(7)
    vol[: shape[0] // 3, : shape[1] // 2] = 0.0                          # an exact-zero block against a face
    vol[rng.random(shape) < 0.02] *= -1.0                                # scattered negative voxels
    vol[-1, -1, :] = -50.0                                               # a negative row on the far edge
    dz = torch.from_numpy(vol <= 0).to(gpu)
    for its in (1, 3, ITS):
        got, ref = run_rl(gpu, vol, psf, backend, its)
        assert bool((got[dz] == 0).all()), (its, int((got[dz] != 0).sum()))
        assert bool((ref[dz] == 0).all())
        report(f"zeros/negatives {backend} {shape} it {its}", fft_errors(got, ref))
        assert_fft_close(got, ref, RMS_TOL, VOXEL_TOL, f"zero / negative voxels, {backend}, {its} iterations")


def test_richardson_lucy_of_a_deskewed_volume(gpu):
    """BASELINE config 4 in its literal order, deskew -> deconvolve: the deskewed volume with overhang_fill=0 has exact-zero
    wedges, where the blur falls to the eps floor at their borders; those voxels stay exactly 0 and the rest agrees with float64."""
    from biahub_amd.deconvolve import richardson_lucy_plan
    from biahub_amd.deskew import fast_deskew_zyx

    raw = torch.from_numpy(camera_volume((48, 64, 160), seed=8)).to(gpu)
    dk = fast_deskew_zyx(raw, ls_angle_deg=36.17, px_to_scan_ratio=0.371, keep_overhang=True, average_n_slices=3,
                         overhang_fill=0).contiguous()
    vol = dk.cpu().numpy()
    assert (vol == 0).mean() > 0.1
    psf = psf_of((9, 5, 5), "complex")
    backend = richardson_lucy_plan(psf.shape, vol.shape)[1]
    got, ref = run_rl(gpu, vol, psf, backend)
    assert bool((got[dk == 0] == 0).all())
    report(f"deskewed {vol.shape} {backend}", fft_errors(got, ref))
    assert_fft_close(got, ref, RMS_TOL, VOXEL_TOL, f"deskewed volume {vol.shape}, {backend}")


# ----------------------------------------------------------------------------- the bench's own call at full size
def test_bench_call_full_size_10_iterations(gpu):
    """bench.py's inputs and call — ``PreparedRichardsonLucy(psf, shape)(vol, k, 1e-6, row_sums=rs)`` on its (512, 2048, 2048)
    position — for k = 1, 2, 5, 10 against ONE float64 run on the GPU that stops at those checkpoints: the bounds at every
    checkpoint, bounded growth rms_rel(10) <= 5 rms_rel(2) (the float32 oracle grows 2.5x on the CPU), the row sums of the last
    update pass against est.double().sum(-1), and the deskew that takes them against the standalone deskew.

    Memory: the float64 state, its half spectrum and one spectrum temporary live on the card with the bench volume, the engine
    handle and one engine result at a time (the transfer function is real: the bench PSF is symmetric); each result is compared
    and freed before the reference moves on."""
    import bench
    from biahub_amd.deconvolve import PreparedRichardsonLucy
    from biahub_amd.deskew import fast_deskew_zyx

    shape = (512, 2048, 2048)
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(gpu)
    need = 150 << 30
    assert free >= need, f"the full-size float64 check needs ~{need >> 30} GiB free on the card, {free / 2**30:.1f} GiB are"
    t0 = time.perf_counter()
    psf = bench.gaussian_psf(bench.PSF_SHAPE, bench.PSF_SIGMA, gpu)
    vol = bench.synthetic_position(shape, 0xB1A0 + 1, gpu)
    rs = torch.empty(shape[:2], dtype=torch.float64, device=gpu)
    h = PreparedRichardsonLucy(psf, shape)
    assert h.backend == "engine" and h.otf_is_real
    low = [free]
    errs, rs_err, deskew_diff = {}, None, None
    for k, ref in R.richardson_lucy_f64_checkpoints(vol, psf, (1, 2, 5, 10), EPS):
        low.append(torch.cuda.mem_get_info(gpu)[0])
        est, got_rs = h(vol, k, 1e-6, row_sums=rs)
        low.append(torch.cuda.mem_get_info(gpu)[0])
        assert got_rs is rs
        errs[k] = fft_errors(est, ref)
        report(f"bench call {shape} it {k}", errs[k])
        if k == 10:
            want = est.double().sum(-1)
            rs_err = float(((got_rs - want).abs() / want.abs().clamp(min=1e-300)).max())
            a = fast_deskew_zyx(est, row_sums=got_rs, **bench.DESKEW)
            b = fast_deskew_zyx(est, **bench.DESKEW)
            deskew_diff = float((a - b).abs().max())
            fill_ulp = float(torch.finfo(torch.float32).eps) * float(a[-1, 0, 0].abs())   # a[-1, 0, 0]: deep in the overhang wedge
            del a, b, want
        del est
    h.close()
    elapsed = time.perf_counter() - t0
    print(f"F64 bench call: row_sums rel {rs_err:.2e}, deskew with / without row sums max diff {deskew_diff:.3e} "
          f"(fill ulp {fill_ulp:.3e}), peak device memory {(total - min(low)) / 2**30:.1f} GiB, {elapsed:.1f} s")
    for k, e in errs.items():
        assert e[0] <= RMS_TOL and e[1] <= VOXEL_TOL, (k, e)
    assert errs[10][0] <= 5 * errs[2][0], errs
    assert rs_err <= 1e-12, rs_err
    assert deskew_diff == 0.0, deskew_diff
