"""Inputs of the registration-metric tests (tests/test_regmetric_reference.py on the CPU, tests/test_gpu_regmetric.py on the
GPU): the case lists of ``bh_mattes_mi``, ``bh_smooth_shrink``, ``bh_sobel`` and ``bh_image_stats`` (csrc/regmetric.hip), seeded
builders of their inputs, a float32 restatement of each operator in the kernel's documented arithmetic, and the bounds.

Every kernel of regmetric.hip is a capped grid with a grid-stride loop; the "wrap" cases are the ones whose work exceeds the
cap, so that a workgroup runs its outer loop a second time (``thresholds``).  The case shapes are fixed for 256 compute units
(MI355X); the GPU tests assert against the card they run on that each wrap case does wrap.
"""

import functools
import math
from collections import namedtuple

import numpy as np

from oracle import oracle_np as O

f32 = np.float32

CUS = 256                       # compute units the wrap shapes are sized for
MI_CHUNK, MI_FIX, MI_PAD = 4096, 2 ** 20, 2
WRAP_MARGIN = 1.08              # every wrap case exceeds its threshold by this factor at CUS


def thresholds(cus):
    """Work above which a workgroup of each kernel takes a second trip through its grid-stride loop: rows of the statistics
    (8 cus workgroups x 4 rows), output voxels of a smoothing pass or of Sobel (16 cus x 256), samples of the metric (8 cus
    chunks of 4096)."""
    return {"rows": 32 * cus, "voxels": 4096 * cus, "samples": 32768 * cus}


# =============================================================================================== bounds
# Every bound is 10x the error of the float32 restatement below against float64, measured on the CPU at the very inputs of
# the GPU tests (tests/test_regmetric_reference.py prints the figures with -s and holds the restatement to a tenth of each
# bound); none comes from the kernels' output.  The 10x covers what a float32 kernel may do differently from the
# restatement (FMA contraction, association order); for the Parzen coordinates, where contraction decides on which side of
# a bin edge a sample falls, the restatement is measured both ways (``contract``) and the worse figure counts.
#
# bh_mattes_mi against oracle_np.mattes_mi; nvalid equal.  Classes:
#   value            |v - ref| / max(1, |ref|)
#   gradient         max_i |g_i - ref_i| / max |ref|
#   gradient entry   max_i |g_i - ref_i| / max(|ref_i|, 1e-3 max |ref|)      each entry against its own magnitude
# The restatement ``mattes_mi_f32`` over the 19 named cases, with and without contraction: value <= 9.2e-8 (face), gradient
# <= 1.8e-6 and entry <= 8.0e-5 (both stride 64: 522 samples, one column); next moving y1 1.2e-5, face 3.7e-6, wrap 2.5e-6; the
# wrap case at 9.1 M samples 5.9e-8 / 5.3e-7 / 2.5e-6.  What carries the gradient's error is the float32 log-ratio table
# (2^-24 of |log p|) under B-spline derivatives that sum to zero, and the float32 product w dM/dc, in sums whose terms
# largely cancel: the fewer the samples, the larger the share.
# Fixed-image bin flips (the box window: a sample whose float32 Parzen coordinate rounds across a bin edge moves a whole
# count; such samples are part of the figures above, none is excluded).  Per case: wrap 1 without contraction and 0 with it
# (the figures above are the flipped run's; 2.1e-9 / 9.1e-8 / 9.5e-8 with none), every other named case and every draw of
# the sweep 0 either way.  The fixed images are interpolated (pulled) volumes or smoothed levels, not integers, so no value
# sits on an edge by construction; with integer counts and (max - min) (bins - 4) sharing a factor, whole populations do, the
# float64 reference decides such a tie by its own last bit, and one flipped sample among 8 640 moved the value by 5.7e-5.
# The metric is evaluated a little off the matrix that made the fixed image (``OFF_OPTIMUM``): at the optimum the gradient is
# the residue of a cancellation, 100 times smaller, and one flip in 8.7 M samples moved its entries by 9e-4.
# The existing test_registration_kernels_vs_oracle asserts 2e-5 and 2e-3 at the optimum and on integer counts, flips and
# cancellation included; the bounds here are tighter, hold for these inputs only, and that test stays as it is.
MI_VALUE_TOL = 1e-6
MI_GRAD_TOL = 2e-5
MI_GRAD_ENTRY_TOL = 8e-4
# The seeded sweep (``fuzz_cases``: 40 draws of 0 to 22 681 samples inside, in up to 64^2 bins) has bounds of its own: a
# gradient of a few hundred terms of either sign keeps less of its terms' size, and its small entries sit at the 1e-3 floor.
# Restatement over the 40 draws, both ways: value <= 3.9e-7 (draw 10, 17 samples), gradient <= 6.1e-5 and entry <= 1.9e-2
# (both draw 27, 541 samples; next 1.8e-3).  Held to the named cases' bounds the sweep would test float32, not the kernel.
MI_SWEEP_VALUE_TOL = 4e-6
MI_SWEEP_GRAD_TOL = 6.1e-4
MI_SWEEP_GRAD_ENTRY_TOL = 0.19
MI_ENTRY_FLOOR = 1e-3           # of max |grad|: the floor of an entry's own magnitude

# bh_smooth_shrink against reference_f64.smooth_shrink_f64 (fft_metrics: rms_rel, voxel_rel); the restatement is
# oracle_np.smooth_shrink (the same float32 weights, float32 products and running sums, tap by tap).  Over the 7 cases:
# rms_rel 4.2e-8 .. 1.7e-7, voxel_rel 1.4e-7 .. 5.8e-7 (both worst at sigma 8 on (5, 70, 9): three passes of 65 taps; the wrap
# shapes 8.0e-8 / 3.9e-7).  The volumes carry their offset of 110 counts, so every voxel is held to its own magnitude.  The
# existing test asserts 1e-6 in the max norm on a bead volume against the float32 oracle; it stays.
SMOOTH_RMS_TOL = 1.7e-6
SMOOTH_VOXEL_TOL = 5.8e-6

# bh_sobel against oracle_np.sobel in float64, unrounded; the restatement is ``sobel_f32`` (the kernel's nine-term sums).
# Over the 4 volumes: rms_rel 3.3e-8 .. 4.1e-8 ((2, 2, 2)), voxel_rel 8.2e-8 .. 1.5e-7 ((40, 160, 200)).  The differences of
# neighbouring counts are exact in float32; what is left is the rounding of the sums, the squares and the root.
SOBEL_RMS_TOL = 4.1e-7
SOBEL_VOXEL_TOL = 1.5e-6

# bh_image_stats: min and max exact; the sum and the three first moments against math.fsum of the float64 products.  The
# volumes are integer counts: every product v z, v y, v x and every partial sum is an integer below 2^53 (at most 1.3e10
# here), so float64 accumulation is exact in ANY order — one running sum (``stats_running_f64``), numpy's pairwise sum and
# math.fsum agree to the last bit (tests/test_regmetric_reference.py asserts it).  The restatement's error is 0 and so is
# ten times it: the kernel, which accumulates in float64, is held to equality.
STATS_TOL = 0.0


# =============================================================================================== volumes
def similarity(angle_deg, scale, t):
    th = np.deg2rad(angle_deg)
    return np.array([[scale, 0, 0, t[0]], [0, scale * np.cos(th), -scale * np.sin(th), t[1]],
                     [0, scale * np.sin(th), scale * np.cos(th), t[2]], [0, 0, 0, 1.0]])


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def camera(shape, seed=None):
    """Camera-like counts (oracle_np.synthetic_volume: offset 110, noise, beads), one bead per 2000 voxels."""
    n = max(12, int(np.prod(shape)) // 2000)
    return _frozen(O.synthetic_volume(tuple(shape), seed=sum(shape) if seed is None else seed, n_blobs=n))


@functools.lru_cache(maxsize=None)
def level(shape, seed=None):
    """A pyramid level of ``shape``: the camera volume of twice the shape smoothed (sigma 1) and halved; not integers."""
    return _frozen(O.smooth_shrink(camera(tuple(2 * n for n in shape), seed), (1, 1, 1), (2, 2, 2))[0])


def pulled(vol, M, shape=None):
    """fixed(p) = vol(M p) on a grid of ``shape`` (the volume's own by default), as in test_registration_kernels_vs_oracle."""
    return _frozen(O.affine_pull(vol, M, tuple(shape or vol.shape), 1, O.BOUNDARY_ITK))


# The metric is evaluated a little off the matrix that made the fixed image, where an optimiser spends its time: at the
# optimum itself the gradient is the residue of a cancellation and measures nothing but the conditioning of the input.
OFF_OPTIMUM = (0.4, 1.003, (0.2, -0.3, 0.25))


def full_range(fixed, moving):
    return (float(fixed.min()), float(fixed.max()), float(moving.min()), float(moving.max()))


def fit_pull(fshape, mshape, margin=0.04, shear=0.03):
    """A 3x4 pull that lays the fixed index box into the moving one, ``margin`` of the moving extent inside its faces
    (negative: that much outside), with a shear between neighbouring axes.  The row of a moving axis of length 1 is zero: it
    maps to exactly 0, the only coordinate such an axis can interpolate."""
    P = np.zeros((3, 4))
    for a in range(3):
        span = mshape[a] - 1
        if span == 0:
            continue
        b = (a + 1) % 3   # c_a = span (margin + (1 - 2 margin - shear) u_a + shear u_b), u = index / (N - 1) in [0, 1]
        P[a, a] = (1 - 2 * margin - shear) * span / max(fshape[a] - 1, 1)
        P[a, b] = shear * span / max(fshape[b] - 1, 1)
        P[a, 3] = margin * span
    return P


# =============================================================================================== the metric's cases
MiCase = namedtuple("MiCase", "fixed moving P rng bins stride offset")

WRAP_SHAPE = (math.ceil(WRAP_MARGIN * thresholds(CUS)["samples"] / (256 * 256)), 256, 256)   # (139, 256, 256)
FLAT_SHAPE, FLAT_RANGE = (8, 64, 128), (-12.0, 212.0, -12.0, 212.0)   # bin width 8: 100 -> 16.0, 200 -> 28.5
BINS_SHAPE, BINS = (20, 48, 64), (6, 7, 33, 64)
GEOMETRY_SHAPE, OTHER_SHAPE = (24, 40, 56), (31, 37, 70)
MOVING_PLANES_FIXED = (10, 24, 36)
MOVING_PLANES = {"moving z1": (1, 40, 50), "moving y1": (30, 1, 50), "moving x1": (30, 40, 1)}

MI_CASES = (["wrap", "wrap stride 5", "flat"] + [f"bins {b}" for b in BINS] + ["planar"] + list(MOVING_PLANES)
            + ["face", "tenth inside", "none inside", "shapes differ", "last voxel", "stride past the end", "stride 64",
               "narrow range"])
MI_WRAP_CASES = ["wrap"]


@functools.lru_cache(maxsize=None)
def _pair(shape, kind, angle=3.0, scale=1.02, t=(0.4, 1.5, -1.2)):
    """(fixed, moving, P): moving a camera volume or a level, fixed = moving pulled by a small similarity."""
    vol = camera(shape) if kind == "camera" else level(shape)
    M = similarity(angle, scale, t)
    off = similarity(*OFF_OPTIMUM)
    if shape[0] == 1:   # planar: the z row stays (1, 0, 0, 0)
        off[0] = (1, 0, 0, 0)
    return pulled(vol, M), vol, (M @ off)[:3]


@functools.lru_cache(maxsize=None)
def flat_volume():
    v = np.full(FLAT_SHAPE, 100.0, dtype=f32)
    v[2:6, 30:34, 60:64] = 200.0
    return _frozen(v)


@functools.lru_cache(maxsize=None)
def mi_case(name):
    """The inputs of one named case (built once; the arrays are read-only)."""
    if name in ("wrap", "wrap stride 5"):
        # stride 1: 9.1 M samples, 2 224 chunks on 2 048 workgroups; stride 5, offset 3: the same volumes in a single pass
        fx, mv, P = _pair(WRAP_SHAPE, "camera", 1.5, 1.01)
        return MiCase(fx, mv, P, full_range(fx, mv), 32, *((1, 0) if name == "wrap" else (5, 3)))
    if name == "flat":
        v = flat_volume()
        return MiCase(v, v, np.eye(4)[:3], FLAT_RANGE, 32, 1, 0)
    if name.startswith("bins "):
        fx, mv, P = _pair(BINS_SHAPE, "level")
        return MiCase(fx, mv, P, full_range(fx, mv), int(name.split()[1]), 1, 0)
    if name == "stride 64":   # X = 64: every sample sits in column 0
        fx, mv, P = _pair(BINS_SHAPE, "level")
        return MiCase(fx, mv, P, full_range(fx, mv), 32, 64, 0)
    if name in ("last voxel", "stride past the end"):   # one sample each: the last voxel, the first
        mv = level(BINS_SHAPE)
        size = mv.size
        return MiCase(mv, mv, np.eye(4)[:3], full_range(mv, mv), 32, *((1, size - 1) if name == "last voxel" else (size + 7, 0)))
    if name == "planar":      # the 2-D registration path: Zf = Zm = 1, an in-plane rotation and shift
        fx, mv, P = _pair((1, 96, 130), "camera", 4.0, 1.0, (0.0, 2.5, -3.25))
        return MiCase(fx, mv, P, full_range(fx, mv), 32, 1, 0)
    if name in MOVING_PLANES:
        mv = camera(MOVING_PLANES[name])
        fx = pulled(mv, fit_pull(MOVING_PLANES_FIXED, mv.shape, 0.05, 0.02), MOVING_PLANES_FIXED)
        return MiCase(fx, mv, fit_pull(fx.shape, mv.shape), full_range(fx, mv), 32, 1, 0)
    if name == "face":        # a whole-voxel translation: the samples at x = X - 6 land on c = X - 1 exactly
        mv = camera(GEOMETRY_SHAPE)
        M = np.eye(4)
        M[:3, 3] = (2, -3, 5)
        fx = pulled(mv, M)
        return MiCase(fx, mv, M[:3], full_range(fx, mv), 32, 1, 0)
    if name == "tenth inside":
        mv = camera(GEOMETRY_SHAPE)
        M = similarity(5.0, 1.0, (13.0, 21.5, 30.3))
        fx = pulled(mv, similarity(4.0, 1.0, (13.2, 21.0, 30.0)))
        return MiCase(fx, mv, M[:3], full_range(fx, mv), 32, 1, 0)
    if name == "none inside":
        mv = camera(GEOMETRY_SHAPE)
        M = np.eye(4)
        M[1, 3] = 1000.0
        return MiCase(mv, mv, M[:3], full_range(mv, mv), 32, 1, 0)
    if name == "shapes differ":
        mv = level(OTHER_SHAPE)
        fx = pulled(mv, fit_pull(GEOMETRY_SHAPE, mv.shape, -0.02, 0.02), GEOMETRY_SHAPE)
        return MiCase(fx, mv, fit_pull(fx.shape, mv.shape, margin=-0.03), full_range(fx, mv), 32, 1, 0)
    if name == "narrow range":   # 5th to 95th percentile: bins clamp at both ends, and samples lose all four weights
        fx, mv, P = _pair((37, 70, 93), "camera")
        rng = tuple(float(v) for v in (*np.percentile(fx, (5, 95)), *np.percentile(mv, (5, 95))))
        return MiCase(fx, mv, P, rng, 32, 1, 0)
    raise KeyError(name)


FUZZ_SEED, FUZZ_DRAWS = 20261018, 40


@functools.lru_cache(maxsize=None)
def fuzz_cases(seed=FUZZ_SEED, draws=FUZZ_DRAWS):
    """The seeded sweep: axes of 1 to 48 (fixed and moving drawn apart), a random pull (every fifth draw partly outside the
    moving volume), bins 6 to 64, stride 1 to 9, offset anywhere.  Returns a tuple of (description, MiCase)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(draws):
        fshape = tuple(int(v) for v in rng.integers(1, 49, 3))
        mshape = tuple(int(v) for v in rng.integers(1, 49, 3))
        margin = float(-rng.uniform(0.05, 0.3) if k % 5 == 4 else rng.uniform(0.01, 0.1))
        shear = float(rng.uniform(0.0, 0.1))
        bins, stride = int(rng.integers(6, 65)), int(rng.integers(1, 10))
        offset = int(rng.integers(0, int(np.prod(fshape))))
        mv = _frozen(O.synthetic_volume(mshape, seed=int(rng.integers(1 << 30))))
        # the fixed image: the moving one seen through a neighbouring pull (not the one evaluated), zero where that leaves it
        fx = pulled(mv, fit_pull(fshape, mshape, 0.9 * margin + 0.004, 0.8 * shear), fshape)
        # half a count beyond the data on either side: never empty, even for a volume of one voxel
        r = (float(fx.min()) - 0.5, float(fx.max()) + 0.5, float(mv.min()) - 0.5, float(mv.max()) + 0.5)
        what = (f"seed {seed} draw {k}: fixed {fshape} moving {mshape} margin {margin:.3f} shear {shear:.3f} bins {bins} "
                f"stride {stride} offset {offset}")
        out.append((what, MiCase(fx, mv, fit_pull(fshape, mshape, margin, shear), r, bins, stride, offset)))
    return tuple(out)


def mattes_f64(case):
    """oracle_np.mattes_mi of a case: (value, grad 3x4, nvalid)."""
    return O.mattes_mi(case.fixed, case.moving, case.P, case.rng, case.bins, case.stride, case.offset)


@functools.lru_cache(maxsize=None)
def mi_reference(name):
    """The float64 reference of a named case, computed once (the wrap case: seconds and gigabytes)."""
    return mattes_f64(mi_case(name))


def mi_errors(value, grad, ref_value, ref_grad):
    """(value error, gradient error against max |grad|, worst entry against its own magnitude floored at 1e-3 max |grad|).
    A reference gradient of exactly zero admits only zero."""
    g, w = np.asarray(grad, np.float64).reshape(3, 4), np.asarray(ref_grad, np.float64).reshape(3, 4)
    ev = abs(value - ref_value) / max(1.0, abs(ref_value))
    gmax = float(np.abs(w).max())
    d = np.abs(g - w)
    if gmax == 0.0:
        e = 0.0 if not d.any() else math.inf
        return ev, e, e
    return ev, float(d.max() / gmax), float((d / np.maximum(np.abs(w), MI_ENTRY_FLOOR * gmax)).max())


# =============================================================================================== float32 restatements
def _bspline3_f32(u):
    a = np.abs(u)
    b = f32(2) - a
    inner = (f32(4) - f32(6) * a * a + f32(3) * a * a * a) * f32(1.0 / 6.0)
    return np.where(a < 1, inner, np.where(a < 2, b * b * b * f32(1.0 / 6.0), f32(0)))


def _bspline3_deriv_f32(u):
    a = np.abs(u)
    b = f32(2) - a
    return np.where(a < 1, f32(-2) * u + f32(1.5) * u * a, np.where(a < 2, np.where(u < 0, f32(0.5), f32(-0.5)) * b * b, f32(0)))


def _parzen(v, scale, nmin, contract):
    """v * scale - nmin in float32; ``contract``: as one fused multiply-add (the product of two float32 is exact in float64)."""
    if contract:
        return (v.astype(np.float64) * np.float64(scale) - np.float64(nmin)).astype(f32)
    return v * scale - nmin


def mattes_mi_f32(fixed, moving, P, rng, bins=32, stride=1, offset=0, contract=False, defect=None, grid=8 * CUS):
    """``bh_mattes_mi`` restated on the CPU in the arithmetic regmetric.hip documents: sample coordinates in float64, the
    interpolation fraction, the trilinear interpolant and its gradient, the Parzen coordinates and the B-spline weights in
    float32, the histogram in integers floor(w 2^20 + 0.5), marginals and logarithms in float64, the log-ratio table
    rounded to float32, the per-sample weight in float32 and the twelve sums in float64.

    Returns (value, grad 3x4, nvalid, info); info: ``total`` (the histogram's mass in samples), ``hist`` (int64, bins x
    bins), ``chunk_max`` (the largest bin of any one chunk of 4096 samples, what the 32-bit LDS histogram must hold) and
    ``flips`` (samples whose float32 fixed bin is not the float64 one).

    ``defect`` plants one: "no rezero" — the LDS histogram is not cleared between the chunks of a workgroup, so with ``grid``
    workgroups the flush after a workgroup's j-th chunk adds the chunks before it again; "nvalid" — the gradient divided by
    the number of samples inside instead of the histogram's mass; a float — that many bins added to the moving Parzen
    coordinate."""
    F, M = np.ascontiguousarray(fixed, dtype=f32), np.ascontiguousarray(moving, dtype=f32)
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    nb = bins - 2 * MI_PAD
    fbin, mbin = (rng[1] - rng[0]) / nb, (rng[3] - rng[2]) / nb
    fscale, fnmin = f32(1.0 / fbin), f32(rng[0] / fbin - MI_PAD)
    mscale, mnmin = f32(1.0 / mbin), f32(rng[2] / mbin - MI_PAD)
    idx = np.arange(offset, F.size, stride)
    xh = np.stack(np.unravel_index(idx, F.shape)).astype(np.float64)
    c = P[:, 0:1] * xh[0] + P[:, 1:2] * xh[1] + P[:, 2:3] * xh[2] + P[:, 3:4]
    dims = np.array(M.shape)[:, None]
    ok = np.all((c >= 0) & (c <= dims - 1), axis=0)
    sample = np.nonzero(ok)[0]
    c, xh, fv = c[:, ok], xh[:, ok], F.reshape(-1)[idx[ok]]
    nvalid = int(ok.sum())
    i0 = np.minimum(c.astype(np.int64), np.maximum(dims - 2, 0))
    i1 = np.minimum(i0 + 1, dims - 1)
    fz, fy, fx = (c - i0).astype(f32)
    v = {(dz, dy, dx): M[(i1 if dz else i0)[0], (i1 if dy else i0)[1], (i1 if dx else i0)[2]]
         for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
    a00 = v[0, 0, 0] + fx * (v[0, 0, 1] - v[0, 0, 0])
    a01 = v[0, 1, 0] + fx * (v[0, 1, 1] - v[0, 1, 0])
    a10 = v[1, 0, 0] + fx * (v[1, 0, 1] - v[1, 0, 0])
    a11 = v[1, 1, 0] + fx * (v[1, 1, 1] - v[1, 1, 0])
    b0, b1 = a00 + fy * (a01 - a00), a10 + fy * (a11 - a10)
    m = b0 + fz * (b1 - b0)
    gz = b1 - b0
    gy = (a01 - a00) + fz * ((a11 - a10) - (a01 - a00))
    d00, d01 = v[0, 0, 1] - v[0, 0, 0], v[0, 1, 1] - v[0, 1, 0]
    d10, d11 = v[1, 0, 1] - v[1, 0, 0], v[1, 1, 1] - v[1, 1, 0]
    e0, e1 = d00 + fy * (d01 - d00), d10 + fy * (d11 - d10)
    gx = e0 + fz * (e1 - e0)
    assert m.dtype == gx.dtype == f32
    fterm = _parzen(fv, fscale, fnmin, contract)
    fi = np.clip(np.floor(fterm).astype(np.int64), MI_PAD, bins - MI_PAD - 1)
    fi64 = np.clip(np.floor(fv.astype(np.float64) / fbin - (rng[0] / fbin - MI_PAD)).astype(np.int64), MI_PAD, bins - MI_PAD - 1)
    mterm = _parzen(m, mscale, mnmin, contract)
    if isinstance(defect, float):
        mterm = mterm + f32(defect)
    mi = np.clip(np.floor(mterm).astype(np.int64), MI_PAD, bins - MI_PAD - 1)
    chunk = sample // MI_CHUNK
    nchunks = -(-idx.size // MI_CHUNK)
    # "no rezero": a chunk is flushed once for itself and once more with every later chunk of its workgroup
    times = ((nchunks - 1 - chunk) // grid + 1).astype(np.float64) if defect == "no rezero" else None
    nb2 = bins * bins
    hist = np.zeros(nb2, dtype=np.int64)
    per_chunk = np.zeros(nchunks * nb2, dtype=np.float64)
    for k in (-1, 0, 1, 2):
        b = mi + k
        q = np.floor(_bspline3_f32(b.astype(f32) - mterm) * f32(MI_FIX) + f32(0.5)).astype(np.float64)
        # float64 bincount of integers: exact below 2^53 (at most 4 x 2^20 x 9.2e6 = 3.8e13 here)
        hist += np.bincount(fi * bins + b, weights=q if times is None else q * times, minlength=nb2).astype(np.int64)
        per_chunk += np.bincount(chunk * nb2 + fi * bins + b, weights=q, minlength=nchunks * nb2)
    total = float(hist.sum())
    info = {"total": total / MI_FIX, "hist": hist.reshape(bins, bins), "chunk_max": int(per_chunk.max()) if per_chunk.size else 0,
            "flips": int((fi != fi64).sum())}
    if total <= 0:
        return 0.0, np.zeros((3, 4)), nvalid, info
    H = hist.reshape(bins, bins).astype(np.float64)
    pj, pM, pF = H / total, H.sum(axis=0) / total, H.sum(axis=1) / total
    with np.errstate(divide="ignore", invalid="ignore"):
        valid = (pj > 1e-16) & (pM[None, :] > 1e-16)
        L = np.where(valid, np.log(pj / pM[None, :]), 0.0).astype(f32)
        prod = pF[:, None] * pM[None, :]
        value = float(np.where(valid & (prod > 1e-16), pj * np.log(pj / prod), 0.0).sum())
    w = np.zeros_like(mterm)
    for k in (-1, 0, 1, 2):
        b = mi + k
        w = w + _bspline3_deriv_f32(b.astype(f32) - mterm) * L[fi, b]
    w = w * -mscale
    assert w.dtype == f32
    acc = np.zeros((3, 4))
    for a, ga in enumerate((gz, gy, gx)):
        ga = (w * ga).astype(np.float64)
        acc[a, :3] = (ga[None, :] * xh).sum(axis=1)
        acc[a, 3] = ga.sum()
    return value, acc / (float(nvalid) if defect == "nvalid" else total / MI_FIX), nvalid, info


def mattes_f32(case, **kw):
    return mattes_mi_f32(case.fixed, case.moving, case.P, case.rng, case.bins, case.stride, case.offset, **kw)


def sobel_f32(vol):
    """``sobel_kernel`` restated in float32: per axis sum_bc sm[b] sm[c] (v[0][b][c] - v[2][b][c]) over the edge-clamped
    3 x 3 x 3 neighbourhood, sm = (1/4, 1/2, 1/4), nine terms in the kernel's order; sqrt((gz^2 + gy^2 + gx^2) / 3)."""
    p = np.pad(np.asarray(vol, dtype=f32), 1, mode="edge")
    Z, Y, X = vol.shape

    def V(a, b, c):
        return p[a:a + Z, b:b + Y, c:c + X]

    sm = (f32(0.25), f32(0.5), f32(0.25))
    gz, gy, gx = (np.zeros(vol.shape, dtype=f32) for _ in range(3))
    for b in range(3):
        for c in range(3):
            wbc = sm[b] * sm[c]
            gz = gz + wbc * (V(0, b, c) - V(2, b, c))
            gy = gy + wbc * (V(b, 0, c) - V(b, 2, c))
            gx = gx + wbc * (V(b, c, 0) - V(b, c, 2))
    out = np.sqrt((gz * gz + gy * gy + gx * gx) * f32(1.0 / 3.0))
    assert out.dtype == f32
    return out


def sobel_impulse(shape, at, amplitude):
    """Closed form of the Sobel magnitude of one voxel of ``amplitude`` at ``at`` (interior) on zeros: the neighbour at
    offset d has, per axis a, |g_a| = amplitude |d_a| s(d_b) s(d_c), s(0) = 1/2, s(+-1) = 1/4."""
    out = np.zeros(shape)
    s = {0: 0.5, 1: 0.25, -1: 0.25}
    for d in np.ndindex(3, 3, 3):
        d = tuple(int(k) - 1 for k in d)
        g = [amplitude * abs(d[a]) * s[d[(a + 1) % 3]] * s[d[(a + 2) % 3]] for a in range(3)]
        out[tuple(p + k for p, k in zip(at, d))] = math.sqrt(sum(v * v for v in g) / 3.0)
    return out


# =============================================================================================== smoothing, Sobel, statistics
# (shape, sigma, factor, passes that wrap in x, y, z order | None, note)
SMOOTH_CASES = [
    ((40, 160, 200), (2, 2, 2), (1, 1, 1), (True, True, True), "all three passes wrap"),
    ((40, 160, 200), (1, 1, 1), (2, 1, 1), (True, True, False), "the x and y passes wrap, the z pass does not"),
    ((5, 70, 9), (8, 8, 8), (1, 1, 1), None, "radius 32, both clamps inside one window"),
    ((5, 70, 9), (1, 1, 1), (7, 3, 50), None, "axes shorter than their factor: output length 1"),
    ((5, 70, 9), (0.1, 0.25, 0), (1, 1, 1), None, "radius 1, 1 and 0"),
    ((1, 97, 131), (0, 2, 2), (1, 3, 3), None, "the planar pyramid"),
    ((37, 70, 93), (1, 1.5, 2), (3, 4, 6), None, "remainders on every axis"),
]
SMOOTH_RAISES = [((2, 2, 8.01), (1, 1, 1)), ((1, 1, 1), (1, 0, 1))]


def smooth_pass_voxels(shape, factor):
    """Output voxels of the x, y and z pass (each pass already drops what the later ones do not need)."""
    d, out = list(shape), []
    for a in (2, 1, 0):
        d[a] = max(1, d[a] // int(factor[a]))
        out.append(d[0] * d[1] * d[2])
    return out


IMPULSE_SHAPE, IMPULSE_AT, IMPULSE = (5, 6, 7), (2, 3, 3), 1024.0
SOBEL_WRAP = [(40, 160, 200)]
SOBEL_EDGES = [(1, 50, 70), (2, 2, 2), (3, 1, 300)]

STATS_WRAP = [(96, 100, 7), (130, 70, 65)]     # X below a wave / one past a wave
STATS_EDGES = [(1, 1, 1), (1, 3, 4000), (50, 1, 1)]


@functools.lru_cache(maxsize=None)
def stats_volume(shape):
    """A camera volume lowered by 120 counts (the background is negative), the minimum written into the very first voxel and
    the maximum into the very last — the one a wrapped iteration reads on the wrap shapes."""
    v = camera(shape).copy() - f32(120.0)
    if v.size > 1:
        lo, hi = float(v.min()), float(v.max())
        v.reshape(-1)[0] = lo - 1000.0
        v.reshape(-1)[-1] = hi + 1000.0
    return _frozen(v)


def _moment_products(vol):
    v = np.asarray(vol, dtype=np.float64)
    zz, yy, xx = np.ogrid[: v.shape[0], : v.shape[1], : v.shape[2]]
    return [v.reshape(-1), (v * zz).reshape(-1), (v * yy).reshape(-1), (v * xx).reshape(-1)]   # float32 x index: exact


def stats_fsum(vol):
    """(min, max, [sum, sum v z, sum v y, sum v x] by math.fsum of the float64 products, [fsum |products|])."""
    prods = _moment_products(vol)
    return float(np.min(vol)), float(np.max(vol)), [math.fsum(p.tolist()) for p in prods], [math.fsum(np.abs(p).tolist()) for p in prods]


def stats_running_f64(vol):
    """The four sums as one float64 running sum each over the whole volume."""
    return [float(np.cumsum(p)[-1]) for p in _moment_products(vol)]


def stats_errors(sums, ref_sums, ref_abs):
    return max(abs(g - r) / max(a, 1e-300) for g, r, a in zip(sums, ref_sums, ref_abs))
