"""Error metrics of an FFT result against its float64 reference (``oracle/reference_f64.py``).

``conftest.rel_err`` is max|a - b| / max|b|: on camera-like data the beads set the maximum and the background, where almost
every voxel sits, can be wrong by a large fraction of a count without it noticing.  These metrics weigh every voxel:

    rms_rel   = ||got - ref||_2 / ||ref||_2
    voxel_rel = max |got - ref| / (|ref| + 0.01 rms(ref))     each voxel against its own magnitude (floored near zero)
    maxnorm   = max |got - ref| / max |ref|                   the old metric, for comparison

They run over slabs of whole planes (two passes: the floor needs rms(ref) first), so a volume of 2^31 voxels needs no
temporary of its size; ``got`` and ``ref`` may be numpy arrays or torch tensors on any device (planes are moved to ``ref``'s device).
"""

from __future__ import annotations

import math

import numpy as np
import torch

# Bounds of a float32 FFT result against float64: 10x the float32 oracle's own error on a bench-like volume (R-L, 10
# iterations, bench PSF); a ratio biased by 1e-4 on the dim voxels still fails them 20x (rms) and 8x (voxel)
# (tests/test_fft_reference.py).  The Tikhonov inverse filter rings through zero, where the per-voxel quotient measures the
# float32 rounding of the volume's scale: its voxel bound is 10x the oracle's own there (8.7e-5 at reg 1e-3).
RMS_TOL = 4e-6
VOXEL_TOL = 2e-5
TIK_VOXEL_TOL = 1e-3

# The inverse filter of a general transfer function (bh_inverse_filter; tests/test_gpu_invtf_f64.py).  Same rule: 10x the error
# of a float32 / complex64 restatement of the operator against float64, measured on the CPU at the very inputs the GPU tests
# use (tests/invtf_cases.py: float32_inputs; tests/test_invtf_reference.py holds the restatement to a tenth of these bounds),
# never from the engine's output.
#   rms_rel:   the restatement sits at 1.0e-7 .. 3.2e-7 (worst: (24, 96, 192), 0.3 (N + iN), normalised): RMS_TOL stands.
#   voxel_rel: a normalised volume filtered by an H without symmetry is noise about zero, so the quotient is in effect
#              max error / (0.01 rms); the restatement reaches 5.4e-4 ((30, 160, 320) + pad 5, 1 + 0.3 (N + iN), reg 1e-3,
#              normalised; 2.0e-4 .. 5.4e-4 wherever that H meets normalize=True, <= 1.2e-4 elsewhere): 10x, rounded up.
INVTF_VOXEL_TOL = 6e-3
# The bfloat16 filter against inverse_filter_bf16_f64, which rounds the staged value as the kernel documents: the only error
# on top of the float32 path is a bin whose float32 value falls on the other side of a bfloat16 rounding boundary, and that
# depends on how the float32 value was formed.  Measured on the CPU as the distance between two float32 formulations of the
# staged value (reciprocal-then-multiply, as the kernel, against one division) at the GPU tests' bfloat16 inputs: a handful
# of bins flip, rms_rel 4e-11 .. 2.1e-5, voxel_rel up to 5.7e-3 (both worst at (30, 160, 320) + pad 5, normalised; without
# normalisation 1.3e-5 / 5.4e-4).  Bound = 10x that + the float32 bound.  A truncating conversion gives rms_rel
# 8.4e-4 .. 7.1e-3 at the same inputs, so it fails the rms bound everywhere — by 3.8x at the least, not by the 10x one would
# like: the flips are few and heavy-tailed, and the bound is not to be tightened below what float32 can reproduce.
INVTF_BF16_RMS_TOL = 2.2e-4
INVTF_BF16_VOXEL_TOL = 6.3e-2

# Phase cross-correlation (bh_phase_cross_corr*; tests/test_gpu_pcc_f64.py): fftshift(|corr|) against phase_cross_corr_f64.
# Same rule: 10x the error of the complex64 restatement (tests/pcc_cases.py: phase_cross_corr_c64) against float64, measured on
# the CPU at every input of the GPU tests (pcc_cases.cpu_inputs: 24 shapes, three shifts each, the roll chains, beads, impulses;
# tests/test_pcc_reference.py holds the restatement to a tenth of these bounds), never from the engine's output.  By class:
#   None, camera pairs with their offset: the DC term sits under every voxel.  Restatement rms_rel 8.4e-8 .. 2.3e-7, voxel_rel
#       3.3e-7 .. 7.2e-7: RMS_TOL and VOXEL_TOL stand.
#   None about zero (mean-removed pairs, 65535-count beads and impulses on a zero background): rms_rel 1.7e-7 .. 3.0e-7:
#       RMS_TOL stands.  voxel_rel is max error / (0.01 rms) off the peak, and float32 carries the peak's own rounding, 6e-8 of
#       its height, along the three axis lines through it, where the volume is ordinary noise a thousand times smaller:
#       2e-5 .. 1.9e-3 on camera pairs, 1.4e-3 beads, 3.4e-3 two impulses at (12, 32, 500).  10x, rounded up.
#   magnitude and classic (the two agree to the digits given): every bin has unit weight, so each carries its own relative
#       rounding, the weak ones most: rms_rel 8.2e-7 .. 2.6e-6 (worst (24, 96, 192), no shift), voxel_rel 2.2e-4 .. 5.5e-3
#       (worst (1024, 32, 64), third link of the roll chain; the same axis lines); impulses 1.8e-7 / 2.1e-3.  10x, rounded up.
#   the uniform random volumes of test_gpu_parity.py's three phase cross-correlation tests (pcc_cases.parity_inputs: white, a
#       mean of 1/2): None 8e-8 .. 2.8e-7 / 3.5e-7 .. 8.3e-7: RMS_TOL and VOXEL_TOL stand.  Normalised, a white spectrum has
#       nothing but weak bins to weigh: rms_rel 3.7e-7 .. 4.2e-6 (worst (40, 160, 320)), a bound of its own; voxel_rel up to
#       4.4e-3: PCC_NORM_VOXEL_TOL stands.
PCC_NONE_VOXEL_TOL = 4e-2
PCC_NORM_RMS_TOL = 3e-5
PCC_NORM_VOXEL_TOL = 6e-2
PCC_NORM_RMS_TOL_WHITE = 5e-5

# The transfer functions of compute-tf (bh_phase_transfer_function_3d, bh_fluorescence_transfer_function_3d;
# tests/test_gpu_tf_f64.py) against oracle_np.wo_*_transfer_function_3d in complex128, each complex array weighed as a real one of
# shape (Z, Y, X, 2), the real- and the imaginary-potential function each on its own scale.  Same rule: 10x the error of the
# float32 / complex64 restatement (tests/tf_cases.py: phase_c64, fluorescence_c64 — pupils, phases and Green's function formed in
# float64 and rounded, as the kernel documents, everything after that in complex64) against float64, measured on the CPU at
# every case of the GPU tests, the pupil ties among them (tests/test_tf_reference.py holds the restatement to a tenth of these
# bounds), never from the GPU's output.
#   rms_rel:   phase 8.7e-8 .. 3.9e-7 (worst: the imaginary potential at (4, 1030, 1027); 3.7e-7 at (3, 730, 727), <= 2.5e-7
#              below 10^6 bins), fluorescence 1.0e-7 .. 2.3e-7: RMS_TOL stands for both.
#   voxel_rel: a transfer function falls to nothing towards the edge of its support, so the quotient is in effect
#              max error / (0.01 rms) on the weak bins, and grows with the number of planes the rms is spread over.  Phase
#              1.8e-5 .. 3.0e-4 (worst: (512, 12, 14), imaginary potential; 2.0e-4 at (4, 1030, 1027), 1.7e-4 at (35, 150, 202),
#              <= 1.3e-4 elsewhere); fluorescence 4.3e-5 .. 5.3e-4 (worst: (35, 150, 202); 2.6e-4 at (512, 12, 14), <= 1.2e-4
#              elsewhere).  The two models differ 1.8x, less than a factor of two: one bound, 10x the worst, rounded up.
TF_RMS_TOL = RMS_TOL
TF_VOXEL_TOL = 6e-3
# With at most three planes in all (Zt = 1, or Zt = 3 whose window is (1, 0, 0)) only the plane z = 0 is kept, H1 = -H2 and the
# real-potential function is zero but for rounding: 1e-16 of the imaginary one in float64, so no relative metric applies.  It is
# held to max|re| / max|im| instead.  The restatement's cancellation leaves 0 .. 2.2e-7 (0 at (1, 12, 10) + pad 1, 4.9e-8 .. 9.8e-8
# on planes up to 64 wide, worst at (3, 730, 727): the residue grows with the length of the plane transforms): 10x, rounded up.
TF_ZERO_RE_RATIO_TOL = 3e-6


# (rms, voxel) by class — the four derivations above, in their order
PCC_BOUNDS = {
    "none_offset": (RMS_TOL, VOXEL_TOL),
    "none_zero_mean": (RMS_TOL, PCC_NONE_VOXEL_TOL),
    "normalised": (PCC_NORM_RMS_TOL, PCC_NORM_VOXEL_TOL),
    "normalised_white": (PCC_NORM_RMS_TOL_WHITE, PCC_NORM_VOXEL_TOL),
}


def pcc_class(normalization, mean_removed=False, white=False):
    """The class of ``PCC_BOUNDS`` a phase cross-correlation volume belongs to.  Only two of the three arguments matter to any
    one class: without normalisation, whether the images carry an offset (``mean_removed`` False; the white volumes, whose mean
    is 1/2, among them, so ``white`` changes nothing there) or stand about zero (mean removed, or beads or impulses on a zero
    background); normalised, whether the images are camera-like or ``white`` (the uniform random volumes of
    test_gpu_parity.py) — the normalisation divides any offset out with every other amplitude, so ``mean_removed`` changes
    nothing there."""
    if normalization is None:
        return "none_zero_mean" if mean_removed else "none_offset"
    return "normalised_white" if white else "normalised"


def pcc_bounds(normalization, mean_removed=False, white=False):
    """(rms, voxel) bounds of a phase cross-correlation volume: ``PCC_BOUNDS[pcc_class(...)]``."""
    return PCC_BOUNDS[pcc_class(normalization, mean_removed, white)]


SLAB_VOXELS = 1 << 24   # planes are taken in slabs of at most this many voxels (at least one plane)


def _slab(a, z0, z1, device):
    p = a[z0:z1] if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a[z0:z1]))
    return p.to(device=device, dtype=torch.float64)


def _scan(got, ref):
    if tuple(got.shape) != tuple(ref.shape):
        raise ValueError(f"shape {tuple(got.shape)} != reference shape {tuple(ref.shape)}")
    dev = ref.device if isinstance(ref, torch.Tensor) else torch.device("cpu")
    if len(ref.shape) < 3:
        got, ref = got[None], ref[None]
    Z = int(ref.shape[0])
    step = max(1, SLAB_VOXELS // max(1, math.prod(int(s) for s in ref.shape[1:])))
    ss_ref = ss_err = 0.0
    max_ref = max_err = 0.0
    for z0 in range(0, Z, step):
        r, g = _slab(ref, z0, z0 + step, dev), _slab(got, z0, z0 + step, dev)
        e = g - r
        ss_ref += float((r * r).sum())
        ss_err += float((e * e).sum())
        max_ref = max(max_ref, float(r.abs().max()))
        max_err = max(max_err, float(e.abs().max()))
    n = math.prod(int(s) for s in ref.shape)
    floor = max(0.01 * math.sqrt(ss_ref / n), 1e-300)
    worst = (-1.0, None, 0.0, 0.0)
    for z0 in range(0, Z, step):
        r, g = _slab(ref, z0, z0 + step, dev), _slab(got, z0, z0 + step, dev)
        q = (g - r).abs_().div_(r.abs().add_(floor))
        i = int(q.reshape(-1).nan_to_num(nan=math.inf).argmax())
        v = float(q.reshape(-1)[i])
        if not v <= worst[0]:   # NaN wins
            idx = tuple(int(k) for k in np.unravel_index(i, tuple(q.shape)))
            worst = (v, (z0 + idx[0],) + idx[1:], float(g.reshape(-1)[i]), float(r.reshape(-1)[i]))
    rms_rel = math.sqrt(ss_err) / max(math.sqrt(ss_ref), 1e-300)
    return rms_rel, worst[0], max_err / max(max_ref, 1e-300), worst[1:]


def fft_errors(got, ref64):
    """(rms_rel, voxel_rel, maxnorm) of ``got`` against the float64 reference ``ref64``."""
    rms_rel, voxel_rel, maxnorm, _ = _scan(got, ref64)
    return rms_rel, voxel_rel, maxnorm


def assert_fft_close(got, ref64, rms: float, voxel: float, what: str = ""):
    """Fail unless rms_rel <= rms and voxel_rel <= voxel (NaN fails); the message names the worst voxel.  Returns the errors."""
    rms_rel, voxel_rel, maxnorm, (idx, g, r) = _scan(got, ref64)
    ok = rms_rel <= rms and voxel_rel <= voxel
    assert ok, (f"{what}: rms_rel {rms_rel:.3e} (bound {rms:.1e}), voxel_rel {voxel_rel:.3e} (bound {voxel:.1e}), "
                f"maxnorm {maxnorm:.3e}; worst voxel {idx}: got {g!r}, float64 reference {r!r}")
    return rms_rel, voxel_rel, maxnorm
