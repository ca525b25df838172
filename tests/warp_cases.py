"""Inputs, matrices, the restated launch rules and the bounds of the affine-warp tests (tests/test_warp_reference.py on the CPU,
tests/test_gpu_warp_f64.py on the GPU).

THE BOUNDS — derived, not measured.  u = 2^-24; M is the largest |tap| among the eight clamped, cleaned taps of a voxel
(oracle/reference_f64.py: warp_f64 returns it beside the value V).

Linear with an edge clamp (ITK, SCIPY_CONSTANT; csrc/affine.hip: lerp8).  The sample position is the reference's own (the Q32.32
integers), so only the blend rounds.  One lerp stage is ``fma(f, b - a, a)`` with |a|, |b| <= M:
    the subtraction                          u |b - a|   <= 2 u M
    the fraction's uint32 -> float32 cast    u f |b - a| <= 2 u M     (the scaling by 2^-32 is exact)
    the fma's one rounding                   u |result|  <=   u M     (the result lies between a and b)
five units per stage.  A lerp is a convex combination: it hands the errors of its inputs on undiminished and no larger.  Three
stages (y, z, x) give 15 u M to first order; one unit for the second-order terms and the float64 reference's own rounding:
    |got - V| <= K_LERP u M,   K_LERP = 16,
``got == 0`` exactly where M == 0 (a blend of exact zeros), ``got == cval`` exactly outside, and a NaN or an infinity never
passes.  M, not the volume's maximum, is the scale: a background voxel of 110 counts beside a bead of 60 000 is held to 16 x
6.6e-6 counts where ``rel_err <= 1e-5`` let it be wrong by 0.6.

Linear with the ZEROS boundary (the generic path: axis_plan and eight weighted taps).  Here M is the largest of the eight |tap|
and |cval|.  Per axis the weights are w1 = fl32(c - floor(c)) (the float64 difference is exact) and w0 = fl32(1 - w1): each is
within u of its exact value, and |dw0| + |dw1| <= 2 u.
    the eight weight triples: sum_i |dW_i| <= 3 x 2 u (one axis' errors times the other axes' weight sums, which are <= 1)
                              + 2 u sum_i W_i (the two roundings of (wz wy) wx)                                    8 u M
    the eight products W_i tap_i              u sum_i W_i |tap_i|                                                   1 u M
    the seven roundings of the running sum (the first add is to an exact zero), each of a partial sum <= M          7 u M
    cover = (wz0 + wz1)(wy0 + wy1)(wx0 + wx1): each axis sum within 2 u, two products, 1 - cover, its product with cval
                              (3 x 2 + 2 + 1 + 1) u |cval|                                                         10 u M
    the last add                                                                                                    1 u M
27 u M to first order (a fused multiply-add in place of a product and an add only removes roundings), one unit of slack:
    |got - V| <= K_ZEROS u M,  K_ZEROS = 28.

Nearest neighbour copies one cleaned tap: K = 0, bit for bit, in every boundary.

Measured on the CPU restatements below (tests/test_warp_reference.py prints the figures, DESIGN.md §3.3 keeps them): lerp8 stays
below 3 u M and the generic accumulation below 5 u M at every input of the GPU tests, so the derived bounds cost the reference
nothing.
"""

import functools
from collections import namedtuple

import numpy as np

import deskew_cases as D
from oracle import reference_f64 as R

U = 2.0 ** -24
K_LERP, K_ZEROS = 16, 28
f32, f64, i64 = np.float32, np.float64, np.int64
ITK, SCIPY, ZEROS = 0, 1, 2
FLT_MAX = float(np.finfo(f32).max)
CVAL = -3.5      # not 0: a voxel that should hold cval and holds a blend of zeros (or the reverse) shows


def bound(interp, boundary):
    """K of ``|got - V| <= K u M`` for one launch."""
    return 0 if interp != "linear" else (K_ZEROS if boundary == ZEROS else K_LERP)


# ----------------------------------------------------------------------------- the check
def assert_warp_close(got, ref, K, name, cval=None):
    """``got`` (float32, numpy or torch, any device) against ``ref = warp_f64(...)``: ``|got - V| <= K u M`` at every voxel (so an
    exact zero where M == 0, and never a NaN or an infinity) and, with ``cval`` given, ``got == float32(cval)`` bit for bit wherever
    the reference's ``inside`` is false.  Returns the worst error in units of u M; a failure names the worst voxel."""
    import torch

    V, M, inside = ref
    g = torch.as_tensor(got).to(V.device)
    assert g.dtype == torch.float32 and tuple(g.shape) == tuple(V.shape), (name, g.dtype, tuple(g.shape), tuple(V.shape))
    err = (g.to(torch.float64) - V).abs_()
    bad = ~(err <= K * U * M)
    if cval is not None:
        bad |= ~inside & (g != float(f32(cval)))
    pos = (M > 0) & torch.isfinite(err)
    units = torch.where(pos, err / M.clamp_min(1e-300), torch.zeros_like(err)) / U
    worst = float(units.max()) if units.numel() else 0.0
    nbad = int(bad.sum())
    if nbad:
        score = torch.where(bad, torch.where(torch.isfinite(units), units, torch.full_like(units, float("inf"))) + 1.0,
                            torch.zeros_like(units))
        at = tuple(int(i) for i in np.unravel_index(int(score.argmax()), tuple(V.shape)))
        raise AssertionError(f"{name}: {nbad} voxels outside {K} u M (worst finite {worst:.2f} u M); worst at {at}: got "
                             f"{float(g[at])!r} want {float(V[at])!r} M {float(M[at])!r} inside {bool(inside[at])}")
    return worst


# ----------------------------------------------------------------------------- inputs
T200, T198, W136, W134 = (24, 40, 200), (24, 40, 198), (40, 36, 136), (40, 36, 134)
DEGENERATE = ((1, 40, 200), (24, 1, 200), (24, 40, 1))
DTYPES = ("f32", "u16", "i16", "u8", "f32s")       # deskew_cases.as_dtype; "f32s" is the signed float32 volume

# (z, y, x) of the planted non-finite values, valid in every non-degenerate shape above.  The first four sit inside an 8 x 8 x 64
# tile of a near-identity warp, the last four on the seams z = 8 / 16, y = 8 / 16 / 24 / 32, x = 64 / 128.  "pair": a +inf and a
# -inf that are neighbours, so that every voxel sampling a 2 x 2 x 2 cell that holds them has both among its eight taps: along y
# (lerp8's first stage subtracts them directly: FLT_MAX - (-FLT_MAX) overflows at every fraction) and along z (the second stage
# subtracts their y blends: it overflows where the y fractions leave both more than half their weight).
# "big": a +inf whose y neighbour is -1.25 x 2^105.  The +inf is cleaned to FLT_MAX, the blend's first difference overflows, and
# at a y fraction that widens to 1.0f the rescue's quarter-scale blend is 2^126 - 2^102 - 1.25 x 2^103 rounded to 24 bits: 2^126,
# above FLT_MAX / 4 — the rescue must clamp there, or scaling back by 4 makes the infinity it was to avoid.
BIG_PARTNER = -1.25 * 2.0 ** 105
NONFINITE = {
    "interior": dict(nan=(11, 20, 100), pinf=(13, 27, 90), ninf=(5, 12, 110), pair=((10, 5, 40), (10, 6, 40))),
    "seam": dict(nan=(16, 16, 128), pinf=(8, 24, 64), ninf=(8, 32, 127), pair=((15, 16, 64), (16, 16, 64))),
}
NONFINITE_BIG = ((20, 31, 20), (20, 30, 20))      # the +inf at y + 1 of its partner: lerp8 forms fma(fy, inf' - partner, partner)


@functools.lru_cache(maxsize=16)
def volume(shape, dtype="f32", nonfinite=False):
    """The bead volume of ``deskew_cases`` (beads of 3 000 .. 60 000 counts on a background of 110 +- 3) as ``dtype``; with
    ``nonfinite`` (float32 only) the values of ``NONFINITE`` planted.  Read-only, shared between tests."""
    vol = np.array(D.as_dtype(D.bead_volume(tuple(shape)), dtype))
    if nonfinite:
        assert vol.dtype == f32
        for where in NONFINITE.values():
            vol[where["nan"]] = np.nan
            vol[where["pinf"]] = np.inf
            vol[where["ninf"]] = -np.inf
            vol[where["pair"][0]], vol[where["pair"][1]] = np.inf, -np.inf
        vol[NONFINITE_BIG[0]], vol[NONFINITE_BIG[1]] = np.inf, f32(BIG_PARTNER)
    vol.setflags(write=False)
    return vol


# ----------------------------------------------------------------------------- matrices
def rotation(axis, deg):
    """Rodrigues: the 3 x 3 rotation by ``deg`` about ``axis`` given in (z, y, x) order."""
    ax = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def about_z(deg, scale=1.0, az=None):
    """A similarity in the y-x plane with exact zeros coupling z: the z-separable form (z scale ``az``, default ``scale``)."""
    th = np.deg2rad(deg)
    A = np.array([[scale if az is None else az, 0, 0], [0, scale * np.cos(th), -scale * np.sin(th)],
                  [0, scale * np.sin(th), scale * np.cos(th)]])
    if deg == 90.0:
        A[1, 1] = A[2, 2] = 0.0
    return A


Z_AX, Y_AX, OBL = (1.0, 0, 0), (0, 1.0, 0), (1.0, 0.4, 0.3)
TILE, BLOCKS, ZWALK, OBLIQUE, CUBIC = 0, 1, 2, 3, 4
PATH_NAMES = {TILE: "staged tiles", BLOCKS: "compact blocks", ZWALK: "z walk", OBLIQUE: "oblique walk"}

# name: (3 x 3 part, shift added to the centre-to-centre translation, input shapes (rows aligned, rows unaligned), the launch it is
# meant for at float32 / linear / ITK on the aligned shape).  The pull matrix maps the centre of the output box onto the centre of
# the input plus ``shift``: with an output box larger than the input by more than a tile in x, tiles straddle every face and the
# outermost lie wholly outside the source.
Warp = namedtuple("Warp", "A shift shapes path")
WARPS = {
    "identity": Warp(np.eye(3), (0.0, 0.0, 2.75), (T200, T198), ZWALK),          # tile 0 reaches source x 0.75: a box of one quad
    "half-voxel shift": Warp(np.eye(3), (-0.5, -0.5, -0.5), (T200, T198), ZWALK),     # the ITK tie: c == -0.5 is inside
    "similarity 2 deg 1.02": Warp(about_z(2.0, 1.02), (3.5, -12.25, 20.75), (T200, T198), ZWALK),   # BASELINE config 3
    "30 deg 0.7 about z": Warp(about_z(30.0, 0.7), (1.0, 4.0, -5.0), (T200, T198), ZWALK),
    "90 deg about z": Warp(about_z(90.0), (0.0, 0.0, 0.0), (T200, T198), ZWALK),
    "z scale 0": Warp(about_z(0.0, 1.0, az=0.0), (7.25, 0.5, -0.5), (W136, W134), ZWALK),
    "z scale 0.4": Warp(about_z(2.0, 1.0, az=0.4), (0.3, 1.5, 0.25), (W136, W134), ZWALK),
    "z scale 2.6": Warp(about_z(-5.0, 1.3, az=2.6), (-4.0, 3.0, 6.5), (W136, W134), ZWALK),
    "minified 0.6 about z": Warp(about_z(1.0, 0.6), (0.0, 0.5, 0.25), (W136, W134), ZWALK),       # one DMA per plane
    "y scale 2 about z": Warp(np.diag([1.0, 2.0, 1.0]) @ about_z(0.5), (0.0, 0.25, 0.5), (W136, W134), ZWALK),    # three
    "y scale 3 about z": Warp(np.diag([1.0, 3.0, 1.0]) @ about_z(0.25), (0.0, 0.25, 0.5), (W136, W134), ZWALK),   # four
    "z flip": Warp(np.diag([-1.0, 1.0, 1.0]), (0.25, 0.5, 0.75), (T200, T198), TILE),             # m00 = -1 leaves both walks
    "oblique 2 deg": Warp(1.02 * rotation(OBL, 2.0), (3.5, -2.25, 0.75), (W136, W134), OBLIQUE),
    "oblique 2 deg minified 0.6": Warp(0.6 * rotation(OBL, 2.0), (0.5, 0.25, 0.75), (W136, W134), OBLIQUE),
    "oblique 2 deg y scale 2": Warp(np.diag([1.0, 2.0, 1.0]) @ rotation(OBL, 2.0), (0.5, 0.25, 0.75), (W136, W134), OBLIQUE),
    "oblique 0.5 deg y scale 3": Warp(np.diag([1.0, 3.0, 1.0]) @ rotation((0.3, 1.0, 0.0), 0.5), (0.5, 0.25, 0.75), (W136, W134), OBLIQUE),
    # 2 deg about y: a tile's x extent crosses two planes (|m_zx| 63 = 2.2).  With float32 quads the box bound is 13 x 11 x 72 = 10 296
    # floats, over the 9 984 cap: compact blocks.  Without the quad rounding (T198: 13 x 11 x 67) and with 16-bit groups of 8 (13 x 11
    # x 80 under the 13 056 cap) the box fits and the tile kernel keeps the warp by its own rule — host_plan says which, per run.
    "2 deg about y": Warp(rotation(Y_AX, 2.0), (0.5, 0.25, 0.75), (T200, T198), BLOCKS),
    "20 deg about y": Warp(rotation(Y_AX, 20.0), (0.5, 0.25, 0.75), (W136, W134), BLOCKS),
    "45 deg about y": Warp(rotation(Y_AX, 45.0), (0.5, 0.25, 0.75), (W136, W134), BLOCKS),
    "30 deg oblique": Warp(rotation(OBL, 30.0), (0.5, 0.25, 0.75), (W136, W134), BLOCKS),
    "4x minifying rotation": Warp(4.0 * rotation((0.5, 1.0, 0.4), 35.0), (0.5, 0.25, 0.75), (W136, W134), BLOCKS),
    "shear": Warp(np.array([[0.5, 0.1, 0.0], [0.0, 1.5, 0.2], [0.1, 0.0, 2.0]]), (2.0, -3.0, 1.0), (T200, T198), TILE),
}

# Output boxes: ragged against 8 x 8 x 64, 16 x 4 x 32 and 16 x 8 x 32 in all three axes, larger than the input by more than 64 in x;
# the crop starts mid-tile in all three axes.  (36 x 60 x 330 = 712 800 voxels, 44 x 52 x 270 = 617 760.)
OUT = {T200: (36, 60, 330), T198: (36, 60, 330), W136: (44, 52, 270), W134: (44, 52, 270)}
CROP_LO = (3, 5, 37)


def crop_shape(out_shape):
    return tuple(n - d for n, d in zip(out_shape, (7, 9, 75)))


def pull_matrix(name, in_shape, out_shape=None):
    """4 x 4 pull matrix of a named warp for an input shape: centre of the output box -> centre of the input + shift."""
    w = WARPS[name]
    out_shape = OUT[tuple(in_shape)] if out_shape is None else out_shape
    ci = (np.asarray(in_shape, f64) - 1) / 2
    co = (np.asarray(out_shape, f64) - 1) / 2
    m = np.eye(4)
    m[:3, :3] = w.A
    t = ci + np.asarray(w.shift, f64) - w.A @ co
    m[:3, 3] = np.round(t * 1024) / 1024        # translations on a 2^-10 grid: m * 2^32 is nowhere near a half
    return m


def degenerate_matrix(in_shape, out_shape, similar):
    """Identity with a quarter-voxel shift, or the 2 deg / 1.02 similarity, centred for a degenerate input."""
    A = about_z(2.0, 1.02) if similar else np.eye(3)
    m = np.eye(4)
    m[:3, :3] = A
    m[:3, 3] = np.round(((np.asarray(in_shape, f64) - 1) / 2 + 0.25 - A @ ((np.asarray(out_shape, f64) - 1) / 2)) * 1024) / 1024
    return m


DEGENERATE_OUT = {(1, 40, 200): (5, 52, 140), (24, 1, 200): (30, 7, 140), (24, 40, 1): (30, 52, 70)}


# ----------------------------------------------------------------------------- the launch rules of csrc/affine.hip, restated
ATZ, ATY, ATX = 8, 8, 64
A_LDS_FLOATS, A_LDS_FLOATS_X8 = 9984, 13056
GEO = {0: (8, 8, 16), 1: (16, 4, 32), 2: (16, 8, 32)}       # compact-block extents (z, y, x) of BH_AFFINE_GBLOCK
RY, QMAX, NS = 4, 4, 4
SIZE = {"f32": 4, "f32s": 4, "u16": 2, "i16": 2, "u8": 1}


def ceil_div(a, b):
    return -(-int(a) // int(b))


def _span_box(m, T, quad=0):
    """The host's bound of a tile's source box in floats: prod_a (floor(sum_j |m_aj| (T_j - 1)) + 4), x rounded out to quads."""
    nb = 1.0
    for a in range(3):
        e = np.floor(sum(abs(m[a, j]) * (T[j] - 1) for j in range(3)) * (1.0 + 1e-6)) + 4.0
        if a == 2 and quad == 4:
            e = np.floor((e + 6.0) / 4.0) * 4.0
        if a == 2 and quad == 8:
            e = np.floor((e + 14.0) / 8.0) * 8.0
        nb *= e
    return nb


Plan = namedtuple("Plan", "path x4 x8 lds_floats zslot zchunk slot")


def host_plan(m, in_shape, out_shape, dtype="f32", interp="linear", boundary=ITK, aligned=True, nozwalk=False, gather=True):
    """bh_affine's dispatch: which kernel launches, with the staging capacity, the z walk's slot and the oblique walk's chunk and
    slot.  ``aligned``: the volume's first element sits on a 16-byte boundary."""
    m = np.asarray(m, f64)
    mq = R.llround_q32(m[:3])
    Zi, Yi, Xi = in_shape
    Zo, Yo, Xo = out_shape
    x4 = dtype in ("f32", "f32s") and Xi % 4 == 0 and aligned
    x8 = dtype in ("u16", "i16") and Xi % 8 == 0 and aligned
    nb = _span_box(m, (ATZ, ATY, ATX), 4 if x4 else (8 if x8 else 0))
    cap = A_LDS_FLOATS_X8 if x8 else A_LDS_FLOATS
    lds = int(nb) if nb < cap else cap
    box_fits = nb < cap or abs(m[0, 2]) * (ATX - 1) < 2.0
    zslot = 0
    if x4 or x8:
        E, size = (4.0, 4.0) if x4 else (8.0, 2.0)
        ey = np.floor((abs(m[1, 1]) * (RY - 1) + abs(m[1, 2]) * 63.0) * (1.0 + 1e-6)) + 3.0
        ex = np.floor((abs(m[2, 1]) * (RY - 1) + abs(m[2, 2]) * 63.0) * (1.0 + 1e-6)) + 3.0
        nbytes = ey * (np.floor((ex + 2.0 * (E - 1.0)) / E) * E) * size
        if nbytes <= 4096.0:
            zslot = (int(nbytes) + 15) & ~15
    separable = m[0, 1] == 0 and m[0, 2] == 0 and m[1, 0] == 0 and m[2, 0] == 0 and mq[0, 0] >= 0
    if separable and boundary != ZEROS and Xi >= 2 and not nozwalk:
        nty = ceil_div(Yo, RY * 4)
        nchunk = max(min(ceil_div(65536, ceil_div(Xo, 64) * nty * 4), ceil_div(Zo, 32)), 1)
        return Plan(ZWALK, x4, x8, lds, zslot, ceil_div(Zo, nchunk), 0)
    if (dtype in ("f32", "f32s", "u16", "i16") and not nozwalk and interp == "linear" and boundary != ZEROS and (x4 or x8)
            and mq[0, 0] > 0 and abs(m[0, 1]) * (RY - 1) + abs(m[0, 2]) * 63.0 < 0.98):
        ntx, nty = ceil_div(Xo, 64), ceil_div(Yo, RY * 4)
        nchunk = max(min(ceil_div(131072, ntx * nty * 4), ceil_div(Zo, 32)), 1)
        zchunk = ceil_div(Zo, nchunk)
        ey = np.floor((abs(m[1, 1]) * (RY - 1) + abs(m[1, 2]) * 63.0 + abs(m[1, 0]) * (zchunk - 1)) * (1.0 + 1e-6)) + 3.0
        ex = np.floor((abs(m[2, 1]) * (RY - 1) + abs(m[2, 2]) * 63.0 + abs(m[2, 0]) * (zchunk - 1)) * (1.0 + 1e-6)) + 3.0
        E, size = (4.0, 4.0) if x4 else (8.0, 2.0)
        nbytes = ey * (np.floor((ex + 2.0 * (E - 1.0)) / E) * E) * size
        if nbytes <= 1024.0 * QMAX:
            return Plan(OBLIQUE, x4, x8, lds, zslot, zchunk, (int(nbytes) + 15) & ~15)
    if not box_fits and gather and not nozwalk:
        return Plan(BLOCKS, x4, x8, lds, zslot, 0, 0)
    return Plan(TILE, x4, x8, lds, zslot, 0, 0)


def block_capacity(m, G):
    """launch_affine_gather_g: the LDS floats a compact block of geometry G may stage."""
    nb = _span_box(np.asarray(m, f64), GEO[G])
    cap = 12288.0 if G == 0 else 16384.0
    return int(nb) if nb < cap else int(cap)


def source_boxes(m, in_shape, out_shape, crop_lo, T, quad=0):
    """compute_box for every tile (or compact block) of extents T: (org, ext, interior), integer arrays [ntiles, 3]; ``quad``
    rounds the x range out to groups of 4 or 8 samples."""
    m = np.asarray(m, f64)
    n_t = [ceil_div(n, t) for n, t in zip(out_shape, T)]
    o0 = np.stack(np.meshgrid(*[np.arange(k) * t for k, t in zip(n_t, T)], indexing="ij"), -1).reshape(-1, 3)
    o1 = np.minimum(o0 + np.asarray(T), np.asarray(out_shape)) - 1
    org, ext, interior = (np.zeros(o0.shape, i64) for _ in range(3))
    for a in range(3):
        base = m[a, 0] * (o0[:, 0] + crop_lo[0]) + m[a, 1] * (o0[:, 1] + crop_lo[1]) + m[a, 2] * (o0[:, 2] + crop_lo[2]) + m[a, 3]
        e = [m[a, j] * (o1[:, j] - o0[:, j]) for j in range(3)]
        lo = base + sum(np.minimum(v, 0.0) for v in e)
        hi = base + sum(np.maximum(v, 0.0) for v in e)
        slack = 1e-9 * (np.abs(lo) + np.abs(hi) + 1.0)
        lo, hi = lo - slack, hi + slack
        n = in_shape[a]
        lcl, h = np.maximum(np.floor(lo), 0.0), np.minimum(np.floor(hi) + 1.0, n - 1.0)
        og, ex = lcl.astype(i64), np.where(h >= lcl, (h - lcl).astype(i64) + 1, 0)
        if a == 2 and quad:
            end = (og + ex + quad - 1) & ~(quad - 1)
            og = np.where(ex > 0, og & ~(quad - 1), og)
            ex = np.where(ex > 0, end - og, ex)
        org[:, a], ext[:, a] = og, ex
        interior[:, a] = (np.floor(lo) >= 0.0) & (np.floor(hi) + 1.0 <= n - 1.0)
    return org, ext, interior


def tile_forms(m, in_shape, out_shape, crop_lo, plan, interp="linear", boundary=ITK):
    """The staged-tile kernel's per-tile forms: counts of "empty" (nbox == 0), "fallback" (the box exceeds the launch's LDS: taps
    from global memory), "interior" (the branch-free loop) and "boundary" tiles, and of staged tiles whose flat-list divisions take
    the ``L == 1`` and ``dy == 1`` branches (quad and 8-sample staging only)."""
    quad = 4 if plan.x4 else (8 if plan.x8 else 0)
    org, ext, interior = source_boxes(m, in_shape, out_shape, crop_lo, (ATZ, ATY, ATX), quad)
    nbox = ext.prod(axis=1)
    staged = (nbox > 0) & (nbox <= plan.lds_floats)
    lerp = interp == "linear" and boundary != ZEROS
    inner = staged & interior.all(axis=1) & lerp
    out = {"empty": int((nbox == 0).sum()), "fallback": int((nbox > plan.lds_floats).sum()), "interior": int(inner.sum()),
           "boundary": int((staged & ~inner).sum()), "L == 1": 0, "dy == 1": 0}
    if quad:
        out["L == 1"] = int((staged & (ext[:, 2] // quad == 1)).sum())
        out["dy == 1"] = int((staged & (ext[:, 1] == 1)).sum())
    return out


def staging_form(plan, dtype):
    """Which of stage_box's four forms a launch of the tile kernel uses."""
    if SIZE[dtype] == 4:
        return "f32 quads" if plan.x4 else "f32 dwords"
    return "16-bit groups of 8" if SIZE[dtype] == 2 and plan.x8 else "per sample"


def block_forms(m, in_shape, out_shape, crop_lo, G):
    """The compact-block kernel: blocks whose box is staged, blocks whose box exceeds the capacity (taps from global memory) and
    blocks without a source voxel."""
    _, ext, _ = source_boxes(m, in_shape, out_shape, crop_lo, GEO[G])
    nbox, cap = ext.prod(axis=1), block_capacity(m, G)
    return {"staged": int(((nbox > 0) & (nbox <= cap)).sum()), "not staged": int((nbox > cap).sum()), "empty": int((nbox == 0).sum())}


def _q(mq, a, z, y, x):
    return mq[a, 0] * z + mq[a, 1] * y + mq[a, 2] * x + mq[a, 3]


def zwalk_forms(m, in_shape, out_shape, crop_lo, plan, dtype):
    """The z walk's per-wave forms (linear): waves on the "x edge" form (a lane's pair leaves the row), on the "register ring", and
    on the "lds ring" by DMA instructions per plane: {"x edge": n, "register ring": n, "lds ring": {nq: n}}."""
    mq = R.llround_q32(np.asarray(m, f64)[:3])
    Zi, Yi, Xi = in_shape
    _, Yo, Xo = out_shape
    E = 16 // SIZE[dtype]
    out = {"x edge": 0, "register ring": 0, "lds ring": {}}
    lanes = np.arange(64, dtype=i64)
    for xt in range(ceil_div(Xo, 64)):
        for oy0 in range(0, Yo, RY):
            ox = xt * 64 + lanes[None, :] + crop_lo[2]
            oy = oy0 + np.arange(RY, dtype=i64)[:, None] + crop_lo[1]
            ix = _q(mq, 2, 0, oy, ox) >> 32
            if ((ix < 0) | (ix >= Xi - 1)).any():
                out["x edge"] += 1
                continue
            ring = None
            if SIZE[dtype] in (4, 2) and plan.zslot > 0:
                cy = [int(_q(mq, 1, 0, oy0 + dy + crop_lo[1], xt * 64 + dx + crop_lo[2])) for dy in (0, RY - 1) for dx in (0, 63)]
                cx = [int(_q(mq, 2, 0, oy0 + dy + crop_lo[1], xt * 64 + dx + crop_lo[2])) for dy in (0, RY - 1) for dx in (0, 63)]
                by, y1, x0, x1 = min(cy) >> 32, (max(cy) >> 32) + 1, min(cx) >> 32, (max(cx) >> 32) + 1
                if by >= 0 and y1 <= Yi - 1 and x0 >= 0 and x1 <= Xi - 1:
                    bxq = x0 & ~(E - 1)
                    S = (y1 - by + 1) * ((((x1 + E) & ~(E - 1)) - bxq) // E)
                    if S * 16 <= plan.zslot:
                        ring = ceil_div(S, 64)
            if ring is None:
                out["register ring"] += 1
            else:
                out["lds ring"][ring] = out["lds ring"].get(ring, 0) + 1
    return out


def oblique_forms(m, in_shape, out_shape, crop_lo, plan, dtype):
    """The oblique walk's forms: "slow waves" (the chunk's box leaves the volume or a slot: every plane by slow_voxel), and for the
    others "ring planes" by DMA instructions per plane and "slow planes" (the z window leaves the volume or the ring)."""
    mq = R.llround_q32(np.asarray(m, f64)[:3])
    Zi, Yi, Xi = in_shape
    Zo, Yo, Xo = out_shape
    E = 16 // SIZE[dtype]
    cz, cy, cx = crop_lo
    out = {"slow waves": 0, "slow planes": 0, "ring planes": {}}
    for ka in range(0, Zo, plan.zchunk):
        kb = min(ka + plan.zchunk, Zo)
        for xt in range(ceil_div(Xo, 64)):
            for oy0 in range(0, Yo, RY):
                corners = [(oy0 + dy + cy, xt * 64 + dx + cx) for dy in (0, RY - 1) for dx in (0, 63)]
                ext = {a: [int(_q(mq, a, k + cz, y, x)) for k in (ka, kb - 1) for y, x in corners] for a in (1, 2)}
                by, y1 = min(ext[1]) >> 32, (max(ext[1]) >> 32) + 1
                x0, x1 = min(ext[2]) >> 32, (max(ext[2]) >> 32) + 1
                bxq = x0 & ~(E - 1)
                S = (y1 - by + 1) * ((((x1 + E) & ~(E - 1)) - bxq) // E)
                if not (by >= 0 and y1 <= Yi - 1 and x0 >= 0 and x1 <= Xi - 1 and S * 16 <= plan.slot):
                    out["slow waves"] += 1
                    continue
                nq = ceil_div(S, 64)
                for k in range(ka, kb):
                    zc = [int(_q(mq, 0, k + cz, y, x)) for y, x in corners]
                    zlo, zhi = min(zc) >> 32, max(zc) >> 32
                    if zlo >= 0 and zhi + 1 <= Zi - 1 and zhi + 2 - zlo <= NS - 1:
                        out["ring planes"][nq] = out["ring planes"].get(nq, 0) + 1
                    else:
                        out["slow planes"] += 1
    return out


# ----------------------------------------------------------------------------- float32 restatements, with planted defects
def _fma(a, b, c):
    """fl32(a b + c) of float32 arrays: the product of two float32 is exact in float64, the sum rounds there once and once more to
    float32 (the double rounding can differ from a true fma in the last bit of a rare case; the bound does not notice)."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def lerp8_f32(P, qz, qy, qx, rescue=True):
    """lerp8 of csrc/affine.hip in numpy float32: ``P[dz][dy][dx]`` float32 tap arrays, q the Q0.32 fractions (integer arrays).
    y on both x taps, then z, then x, each ``fma(f, b - a, a)``; ``rescue`` is lerp8_clean's cold branch: a non-finite blend (the
    difference of two cleaned taps overflowed) redone on the taps scaled by 1/4."""
    fz, fy, fx = ((q.astype(np.uint32).astype(f32) * f32(2.0 ** -32)) for q in (qz, qy, qx))

    def blend(S):
        A = [[_fma(fy, S[dz][1][dx] - S[dz][0][dx], S[dz][0][dx]) for dx in (0, 1)] for dz in (0, 1)]
        B = [_fma(fz, A[1][dx] - A[0][dx], A[0][dx]) for dx in (0, 1)]
        return _fma(fx, B[1] - B[0], B[0])

    with np.errstate(over="ignore", invalid="ignore"):
        r = blend(P)
        if rescue:
            bad = ~np.isfinite(r)
            if bad.any():
                quarter = [[[t * f32(0.25) for t in row] for row in pl] for pl in P]
                lim = f32(FLT_MAX / 4)
                r = np.where(bad, np.clip(blend(quarter), -lim, lim) * f32(4.0), r)
    return r


def _coords(m, out_shape, crop_lo):
    """float64 coordinates in numpy association and the integer output grids (z, y, x broadcast)."""
    g = [np.arange(lo, lo + n, dtype=i64) for lo, n in zip(crop_lo, out_shape)]
    gz, gy, gx = g[0][:, None, None], g[1][None, :, None], g[2][None, None, :]
    c = [((m[a, 0] * gz.astype(f64) + m[a, 1] * gy.astype(f64)) + m[a, 2] * gx.astype(f64)) + m[a, 3] for a in range(3)]
    return c, (gz, gy, gx)


def warp_f32(vol, matrix, out_shape, crop_lo=(0, 0, 0), interp="linear", boundary=ITK, cval=0.0, defect=None):
    """The kernels' arithmetic in numpy float32 (a restatement to hold against the bound, not the code under test): cleaned taps,
    the float64 inside rule, Q32.32 positions and lerp8 for linear with an edge clamp; float64 positions, float32 weights and the
    eight-term accumulation for ZEROS; one cleaned tap for nearest.
    ``defect`` (linear with an edge clamp):
        "bias"      voxels below 200 counts come out 1e-5 (relative) too large;
        "ytap"      in voxels below 200 counts the second y tap is taken from iy, not iy + 1;
        "frac16"    the fractions truncated to their upper 16 bits;
        "noclamp"   the clamp at the low x face dropped (index -1 wraps to the row's last sample);
        "overflow"  lerp8 without the rescue of an overflowing difference (the kernels before lerp8_clean)."""
    vol = np.asarray(vol)
    v = np.nan_to_num(vol, nan=0).astype(f32) if vol.dtype.kind == "f" else vol.astype(f32)
    m = np.asarray(matrix, f64)[:3]
    dims = v.shape
    cv = f32(cval)
    c, (gz, gy, gx) = _coords(m, out_shape, crop_lo)
    inside = np.ones(tuple(out_shape), bool)
    for ca, n in zip(c, dims):
        if boundary == ITK:
            inside &= (ca >= -0.5) & (ca < n - 0.5)
        elif boundary == SCIPY:
            inside &= (ca >= 0.0) & (ca <= n - 1)

    def tap(iz, iy, ix, wrap_x=False):
        ixc = np.where(ix < 0, dims[2] - 1, np.minimum(ix, dims[2] - 1)) if wrap_x else np.clip(ix, 0, dims[2] - 1)
        return v[np.clip(iz, 0, dims[0] - 1), np.clip(iy, 0, dims[1] - 1), ixc]

    if interp != "linear":
        idx = [np.floor(ca + 0.5).astype(i64) for ca in c]
        val = tap(*idx)
        if boundary != ITK:
            ok = np.ones_like(inside)
            for i, n in zip(idx, dims):
                ok &= (i >= 0) & (i < n)
            val = np.where(ok, val, cv)
        return np.where(inside, val, cv).astype(f32)
    if boundary == ZEROS:
        near = np.ones_like(inside)
        for ca, n in zip(c, dims):
            near &= (ca > -2.0) & (ca < n + 1.0)
        fl = [np.floor(ca) for ca in c]
        w1 = [(ca - b).astype(f32) for ca, b in zip(c, fl)]
        w0 = [f32(1.0) - w for w in w1]
        i0 = [b.astype(i64) for b in fl]
        for a, n in enumerate(dims):
            w0[a] = np.where((i0[a] < 0) | (i0[a] >= n), f32(0), w0[a])
            w1[a] = np.where((i0[a] + 1 < 0) | (i0[a] + 1 >= n), f32(0), w1[a])
        acc = np.zeros(tuple(out_shape), f32)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w = ((w1[0] if dz else w0[0]) * (w1[1] if dy else w0[1])) * (w1[2] if dx else w0[2])
                    acc = acc + w * tap(i0[0] + dz, i0[1] + dy, i0[2] + dx)
        cover = ((w0[0] + w1[0]) * (w0[1] + w1[1])) * (w0[2] + w1[2])
        acc = acc + (f32(1.0) - cover) * cv
        assert acc.dtype == f32
        return np.where(near, acc, cv).astype(f32)
    mq = R.llround_q32(m)
    cq = [(mq[a, 0] * gz + mq[a, 1] * gy) + mq[a, 2] * gx + mq[a, 3] for a in range(3)]
    i0 = [q >> 32 for q in cq]
    fr = [q & 0xFFFFFFFF for q in cq]
    if defect == "frac16":
        fr = [q & 0xFFFF0000 for q in fr]
    P = [[[tap(i0[0] + dz, i0[1] + dy, i0[2] + dx, wrap_x=defect == "noclamp") for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    r = lerp8_f32(P, *fr, rescue=defect != "overflow")
    if defect == "ytap":
        Pd = [[pl[0], pl[0]] for pl in P]
        r = np.where(np.abs(r) < 200, lerp8_f32(Pd, *fr), r)
    if defect == "bias":
        r = np.where(np.abs(r) < 200, r * f32(1.0 + 1e-5), r).astype(f32)
    return np.where(inside, r, cv).astype(f32)


# ----------------------------------------------------------------------------- the cases
# dtypes per warp beyond float32: the walks' 16-bit rings and the 8-bit register ring on every walk matrix; one further type,
# rotating, on the others.  "f32" runs everywhere.
def dtypes_of(name):
    w = WARPS[name]
    if w.path in (ZWALK, OBLIQUE):
        return ("f32", "u16", "i16", "u8") if w.path == ZWALK else ("f32", "u16", "i16")
    return ("f32", DTYPES[1 + list(WARPS).index(name) % 4])


SIGNED_WARPS = ("similarity 2 deg 1.02", "oblique 2 deg", "30 deg oblique", "shear")      # one per launch, none of them a copy


def linear_cases():
    """[(warp name, input shape, dtype, aligned rows)] of the linear / nearest launch tests: every warp on its aligned and its
    unaligned shape with its dtypes, plus the signed float32 volume on one warp of every launch."""
    cases = []
    for name, w in WARPS.items():
        for k, shape in enumerate(w.shapes):
            for d in dtypes_of(name) + (("f32s",) if name in SIGNED_WARPS and "f32s" not in dtypes_of(name) else ()):
                cases.append((name, shape, d, k == 0))
    return cases


# ZEROS: the generic path on the tile kernel and on the compact blocks (no walk takes it), every input type.
ZEROS_WARPS = ("half-voxel shift", "similarity 2 deg 1.02", "z flip", "2 deg about y", "20 deg about y", "30 deg oblique", "shear")
# non-finite taps: one warp per launch (the tile kernel also runs every one of them under BH_AFFINE_NOZWALK=1)
NONFINITE_WARPS = ("identity", "similarity 2 deg 1.02", "z scale 0.4", "oblique 2 deg", "2 deg about y", "20 deg about y", "shear")
BLOCK_WARPS = ("20 deg about y", "45 deg about y", "30 deg oblique", "4x minifying rotation")
