"""Inputs of the phase cross-correlation tests (tests/test_pcc_reference.py on the CPU, tests/test_gpu_pcc_f64.py on the GPU):
the image pairs of each case, the shapes, and a float32 / complex64 restatement of the operator that derives the bounds
(tests/fft_metrics.py) and carries planted defects.

Pairs are camera-like: ``ref`` is ``camera_volume``, ``mov`` is ``ref`` rolled by the case's shift plus fresh Gaussian noise of
sigma 4, rounded and clipped to counts.  Without normalisation the correlation of two images with a camera offset is one DC
term under every voxel, which hides everything else, so ``None`` also runs on the mean-removed pair (``x - mean(x)``).
"""

import functools

import numpy as np
import torch

from invtf_cases import ENGINE
from oracle.reference_f64 import PCC_EPS, irfftn_by_axis, rfftn_by_axis
from test_gpu_f64_parity import camera_volume

NORMS = (None, "magnitude", "classic")
# (normalisation, mean removed): the four runs of every pair
CLASSES = [(None, False), (None, True), ("magnitude", False), ("classic", False)]

LIBRARY_SHAPES = [(15, 21, 25), (9, 14, 31), (10, 20, 50)]       # odd X (Z and Y odd too), and an even X no engine plan takes
HIPFFT = ((24, 96, 192), {"BH_FFT_BACKEND": "hipfft"})
SWITCH_SHAPES = [(8, 64, 512), (256, 64, 128), (512, 64, 192)]   # BH_PCC_UNFUSED / BH_PCC_NO_FUSED_PEAK
EDGE_SHAPES = [(8, 64, 512), (12, 32, 500), (15, 21, 25)]        # fused peak; a shape the library takes; odd X

# (shape, switches, the Z pass that takes COL_PCC there) — launch_col's dispatch; the register-stage colw never takes COL_PCC
PREPARED = [
    ((512, 64, 192), {}, "colz, ragged column tile"),
    ((512, 32, 64), {"BH_FC_COLZ": "0"}, "LDS radix 1, Z 512"),
    ((384, 32, 64), {}, "LDS radix 3, Z 384"),
    ((40, 160, 64), {}, "LDS radix 5, Z 40"),
    ((256, 64, 128), {}, "LDS radix 1, Z 256"),
    ((1024, 32, 64), {}, "LDS radix 1, Z 1024"),
    ((8, 64, 512), {}, "LDS radix 1, Z 8, fused peak"),
    ((15, 21, 25), {}, "library, odd X"),
    ((9, 14, 31), {}, "library, odd X"),
]


def z_pass(shape, env):
    """The kernel launch_col gives COL_PCC along z at this shape under these switches."""
    Z = shape[0]
    if Z == 512 and env.get("BH_FC_COLZ") != "0":
        return "colz"
    radix = 3 if Z % 3 == 0 else 5 if Z % 5 == 0 else 1
    return f"LDS radix {radix} Z {Z}"


def shifts(shape):
    """No shift; exactly n // 2 on every axis (the boundary of the sign rule); one shift of mixed sign."""
    Z, Y, X = shape
    return [(0, 0, 0), (Z // 2, Y // 2, X // 2), (max(1, Z // 3), -max(1, Y // 5), X // 4 + 1)]


# Seeds of the shapes of a few thousand bins.  There one near-empty bin of a spectrum — 2.4 against a median of 10000 at
# (15, 21, 25) with the default seed and the mixed shift — is normalised to unit weight like every other and carries its own
# float32 rounding, thousands of times the usual relative error, into all voxels: the complex64 restatement stood at 8.6e-6
# rms there, 4x any other input (1.3e-6 .. 9.1e-6 over six seeds per shape).  That is float32 at that input, not an
# implementation's doing, and it would set the bound of every case; so these shapes use a seed at which the restatement sits
# where it does at the large shapes, and tests/test_pcc_reference.py screens every input with ``weak_bin`` (condition 3).
SEED_OFFSET = {(15, 21, 25): 100, (9, 14, 31): 100, (10, 20, 50): 500}


def _seed(shape):
    return sum(shape) + SEED_OFFSET.get(tuple(shape), 0)


def weak_bin(F1, F2):
    """min |F| over both spectra x sqrt(number of bins) / median |F1|: how far the weakest bin lies below an ordinary one,
    scaled by how little one bin among many weighs in the rms."""
    n = F1.numel()
    return float(torch.minimum(F1.abs().min(), F2.abs().min())) * n ** 0.5 / float(F1.abs().median())


@functools.lru_cache(maxsize=2)
def ref_volume(shape):
    return camera_volume(shape, seed=_seed(shape))


def moved(img, shift, seed):
    """``img`` rolled by ``shift`` plus fresh Gaussian noise of sigma 4, rounded and clipped to counts."""
    rng = np.random.default_rng(seed)
    v = np.roll(img, shift, axis=(0, 1, 2)) + rng.normal(0.0, 4.0, img.shape)
    return np.clip(np.round(v), 0, 65535).astype(np.float32)


def pair(shape, k):
    """(ref, mov) of the k-th shift of ``shifts(shape)``."""
    ref = ref_volume(tuple(shape))
    return ref, moved(ref, shifts(shape)[k], 2000 + _seed(shape) + k)


def chain(shape):
    """Four images, each the one before it moved by one of the shape's shifts (mixed, half, none) and re-noised: the ``roll``
    chain of the prepared handle.  chain[0], chain[1] is ``pair(shape, 2)``."""
    imgs = [ref_volume(tuple(shape))]
    for k in (2, 1, 0):
        imgs.append(moved(imgs[-1], shifts(shape)[k], (2000 if k == 2 else 3000) + _seed(shape) + k))
    return imgs


def mean_removed(x):
    return (x - x.mean(dtype=np.float64)).astype(np.float32)


def impulse_pairs(shape):
    """A single impulse in each image: both at (0, 0, 0); ref at (0, 0, 0) and mov at the far corner; and the reverse."""
    far = tuple(n - 1 for n in shape)
    out = []
    for pa, pb in (((0, 0, 0), (0, 0, 0)), ((0, 0, 0), far), (far, (0, 0, 0))):
        a, b = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        a[pa], b[pb] = 1000.0, 700.0
        out.append((pa, pb, a, b))
    return out


def bead_pair(shape):
    """Beads of 65535 counts on a zero background, no noise; mov is ref rolled by the mixed shift."""
    a = camera_volume(shape, seed=5, n_beads=24, background=0.0, noise=0.0, amp=(65535.0, 65535.0))
    return a, np.roll(a, shifts(shape)[2], axis=(0, 1, 2)).copy()


def all_shapes():
    """Every shape of the GPU tests' camera pairs."""
    return list(dict.fromkeys([f[0] for f in ENGINE] + LIBRARY_SHAPES + [HIPFFT[0]] + [p[0] for p in PREPARED] + EDGE_SHAPES))


def cpu_inputs(shape):
    """Every (name, ref, mov, classes) the GPU tests run at ``shape``, one by one: the three shifted pairs in all four classes,
    the later pairs of the roll chain where a handle runs it, and the impulses and beads of the edge shapes.  (A handle with
    ``fixed_is_second`` correlates the same pairs in the other order: the mirrored volume, the same values.)"""
    shape = tuple(shape)
    for k, s in enumerate(shifts(shape)):
        yield (f"shift {s}",) + pair(shape, k) + (CLASSES,)
    if shape in [p[0] for p in PREPARED]:
        imgs = chain(shape)
        for k in (2, 3):
            yield (f"chain {k - 1}-{k}", imgs[k - 1], imgs[k], CLASSES)
    if shape in EDGE_SHAPES:
        a, b = bead_pair(shape)
        yield ("beads", a, b, [(None, False)])
        for pa, pb, a, b in impulse_pairs(shape):
            yield (f"impulses {pa} {pb}", a, b, [(None, False), ("magnitude", False)])


def class_inputs(ref, mov, removed):
    return (mean_removed(ref), mean_removed(mov)) if removed else (ref, mov)


# The uniform random volumes of test_gpu_parity.py's three phase cross-correlation tests.  Those tests iterate over these
# generators and ``parity_inputs`` (the CPU side, which derives their bounds) does too, so both see the same draws.
PARITY_ORACLE = (((32, 64, 128), ((0, 0, 0), (5, -20, 33), (-16, 32, -64))),
                 # z / y of 3 * 2^k and 5 * 2^k: the engine's column passes start with a radix-3 / radix-5 step
                 ((48, 96, 64), ((0, 0, 0), (7, -40, 21), (-24, 48, -32))), ((16, 32, 192), ((3, -9, 77), (-8, 16, -96))),
                 ((40, 160, 320), ((-20, 80, 160), (9, -70, 33))))
PARITY_PEAK_ONLY = (((16, 32, 512), ((0, 0, 0), (5, -11, 200), (-8, 16, -256))), ((8, 16, 1024), ((3, 7, -500),)),
                    ((4, 16, 2048), ((-2, 8, 1023),)), ((256, 128, 512), ((100, -50, 17),)))
PARITY_PREPARED = ((16, 32, 512), (32, 64, 128), (512, 16, 64), (48, 32, 64), (20, 30, 50), (9, 14, 31))


def parity_library_volume(rng):
    """The noiseless (32, 48, 40) volume of test_phase_cross_corr_golden_and_oracle: the first draw of its stream."""
    return rng.random((32, 48, 40), dtype=np.float32)


def _rolled_pairs(rng, cases):
    for shape, rolls in cases:
        ref = rng.random(shape, dtype=np.float32)
        for roll in rolls:
            yield shape, roll, ref, np.roll(ref, roll, axis=(0, 1, 2)) + 0.05 * rng.random(shape, dtype=np.float32)


def parity_oracle_pairs(rng):
    """(shape, roll, ref, mov) of test_phase_cross_corr_golden_and_oracle's engine volumes, from ``rng`` after
    ``parity_library_volume``: mov = ref rolled + 0.05 uniform noise."""
    return _rolled_pairs(rng, PARITY_ORACLE)


def parity_peak_only_pairs():
    """(shape, roll, ref, mov) of test_phase_cross_corr_peak_only, one at a time."""
    return _rolled_pairs(np.random.default_rng(21), PARITY_PEAK_ONLY)


def parity_prepared_volumes():
    """(shape, vols) of test_prepared_phase_cross_corr: two unrelated volumes, the first moved and re-noised, that one moved."""
    rng = np.random.default_rng(33)
    for shape in PARITY_PREPARED:
        vols = [rng.random(shape, dtype=np.float32) for _ in range(2)]
        vols.append(np.roll(vols[0], (3, -5, 7), axis=(0, 1, 2)) + 0.05 * rng.random(shape, dtype=np.float32))
        vols.append(np.roll(vols[2], (-2, 4, 9), axis=(0, 1, 2)))
        yield shape, vols


def parity_inputs():
    """(name, ref, mov) of every pair whose correlation volume test_gpu_parity.py's three phase cross-correlation tests hold to
    the float64 reference — the goldens and their uniform random volumes, from the generators those tests draw from.  They
    are white: no beads, a mean of 1/2, noise of 0.05 or none at all."""
    from conftest import GOLDEN

    z = np.load(GOLDEN / "phase_cross_corr.npz")
    for j in range(3):
        yield f"golden {j}", z[f"ref{j}"], z[f"mov{j}"]
    rng = np.random.default_rng(1)
    parity_library_volume(rng)
    for shape, roll, ref, mov in parity_oracle_pairs(rng):
        yield f"oracle {roll}", ref, mov
    for shape, roll, ref, mov in parity_peak_only_pairs():
        if shape[0] > 16:   # the case that test holds to the float64 reference; the others meet the complex64 oracle
            yield "peak only", ref, mov
    # every pair a handle correlates (the first two volumes of a shape are unrelated)
    for shape, vols in parity_prepared_volumes():
        for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (2, 3)):
            yield f"prepared {i}-{j}", vols[i], vols[j]


DEFECTS = ("column_no_conj", "drop_nyquist", "swap", "norm_1e-4")


def phase_cross_corr_c64(ref, mov, normalization=None, defect=None):
    """The operator restated in float32 / complex64 on the CPU (torch's FFTs): ``(shift, corr_shifted)``, what a float32
    implementation of the definition gives.  ``defect`` plants one of
      column_no_conj  one (y, kx) column of the spectrum — what one thread column of the Z pass holds — multiplied as F1 F2
      drop_nyquist    the last column of the half spectrum left out
      swap            the conjugate on the wrong factor (``pcc_swap`` inverted): conj(F1) F2
      norm_1e-4       every bin's normalisation off by up to 1e-4, relative."""
    assert defect is None or defect in DEFECTS
    a = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float32))
    b = torch.from_numpy(np.ascontiguousarray(mov, dtype=np.float32))
    F1, F2 = rfftn_by_axis(a), rfftn_by_axis(b)
    assert F1.dtype == torch.complex64
    prod = F1.conj() * F2 if defect == "swap" else F1 * F2.conj()
    if defect == "column_no_conj":
        y, kx = F1.shape[1] // 3, F1.shape[2] // 3
        prod[:, y, kx] = F1[:, y, kx] * F2[:, y, kx]
    if normalization is not None:
        norm = prod.abs().clamp(min=np.float32(PCC_EPS)) if normalization == "magnitude" else F1.abs() * F2.abs()
        if defect == "norm_1e-4":
            g = torch.Generator().manual_seed(7)
            norm = norm * (1.0 + 1e-4 * (2.0 * torch.rand(norm.shape, generator=g) - 1.0))
        prod = prod / norm
    if defect == "drop_nyquist":
        prod[..., -1] = 0
    mag = irfftn_by_axis(prod).abs_()
    assert mag.dtype == torch.float32
    shift = np.array(np.unravel_index(int(torch.argmax(mag)), tuple(mag.shape)), dtype=np.float64)
    n = np.array(mag.shape, dtype=np.float64)
    wrap = shift > np.fix(n / 2)
    shift[wrap] -= n[wrap]
    return shift, torch.fft.fftshift(mag)
