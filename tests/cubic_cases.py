"""Inputs, matrices, the restated launch rules and the bounds of the cubic B-spline warp tests (tests/test_cubic_reference.py on the
CPU, tests/test_gpu_cubic_f64.py on the GPU; the kernels are csrc/spline.hip).

THE BOUNDS — derived, not measured.  u = 2^-24, z = sqrt(3) - 2 (|z| = 0.268), h[k] = sqrt(3) z^|k| the prefilter's impulse response
per axis.  A = the mirror-extended |sample| under |h| on every axis (oracle/reference_f64.py: spline_scale_f64), M = sum_i w_i A[tap_i]
over the 64 taps (cubic_warp_f64 returns it beside V), S = the largest |sample| of the volume.

    |coef - C| <= K_PRE   u A + T S        the prefilter alone (bh_spline_prefilter against spline_coef_f64)
    |got  - V| <= K_CUBIC u M + T S        the warp; got == 0 exactly where M == 0, cval bit for bit outside, never a NaN or infinity

A DEPARTURE from the form the bound was asked for in, (K u + T) A and (K u + T) M: the truncation term multiplies S, the volume's maximum,
not the local scale — at a background voxel about twenty times looser than T A would be (6e-5 counts, 1 % of 32 u A there).  The reason is
below ("The truncation"): T A is not a bound.

One pass of filter_block, to first order.  Magnitudes per stage, absolute values taken stage by stage: the causal value c[j] is at most
6 P[j], P[j] = sum_{k>=0} |z|^k |s[j-k]|; the anticausal value a[j] at most sum_l |z|^(l+1) 6 P[j+l], which is A[j] exactly.
    causal step j:      GAIN s[j] rounds (u 6 |s[j]|), the fma rounds (u 6 P[j]), Zp is a float32 (u |z| 6 P[j-1]): 12 u P[j] in all,
                        and an error e in c[j] reaches output i as e |z|^(|i-j|+1) / (1 - z^2) = e (sqrt(3) / 6) |z|^|i-j|
    anticausal step j:  the difference rounds (u A[j] / |z|, then times |z|), the product rounds, Zp again: 3 u A[j],
                        and an error in a[j] reaches a[i], i <= j, as e |z|^(j-i)
Summed over j, a sample at distance d = i - m enters the error of output i with
    kappa[d] = sqrt(3) |z|^|d| (2 d + 5.39)  for d >= 0,    sqrt(3) |z|^|d| (3 |d| + 5.39)  for d < 0     (1 / (1 - z^2) = 1.077),
that is |h[d]| (5.5 + 3 |d|) with the second-order terms: the recursion hands an error on through a double pole, so a sample's rounding
error decays more slowly than the sample's own weight in A, by the factor 1 + 0.55 |d|.  No constant K makes kappa <= K |h| at every
distance; what the per-voxel bound needs is K_PRE >= E / A, E = u sum_axes (kappa on that axis, |h| on the others) applied to
|sample| — a property of the INPUT's dynamic range, not of the code under test.  rounding_field() evaluates E in float64 and
tests/test_cubic_reference.py asserts E <= K_PRE u A at every voxel of every GPU input.  A volume without contrast has E / A = 3 x (5.5 +
sqrt(3)) = 21.7 (kappa's row sum over |h|'s is 5.5 + sqrt(3) per axis, one axis at a time carries kappa); beside a 60 000-count bead on
a 110-count background the largest ratio is 29.2, so
    K_PRE = 32.
The truncation.  A block starts its causal recursion R = 20 samples before its first output from the steady-state value of a constant
line (INIT_C) and its anticausal one R samples after the last from INIT_A; along x a row shorter than a chunk and not a multiple of 16
is padded with zeros R samples past its mirrored end.  What a block does not see, and what it assumes instead, are each at most the
tail of A beyond distance R: (1 + 1 / (1 - z)) (sqrt(3) / (1 - |z|) + 3) |z|^R S < 10 |z|^R S per pass.  A pointwise T A does not hold
(a lone bead in a field of exact zeros has an A of |z|^25 bead 25 voxels away, all of it beyond the run-in), so T multiplies S: the
x pass's error passes two more filters (x 9), the y pass filters values up to 3 S (x 3 x 3), the z pass values up to 9 S:
    T = 270 |z|^20 = 9.8e-10      (6e-5 counts beside a 60 000-count bead: a third of u A at the 110-count background).

The 64 taps (weights3, blend64; blend16 after the in-place plane combination), to first order, relative to sum_i W_i |C_i| <= M:
    the coefficients' own error                         sum_i W_i E[tap_i]                       <= K_PRE u M
    the weights: x = fl32(c - floor c) is within u x, z = fl32(1 - x) within u; w0 = ((z z) z) S: 4 u w0 + u z^2 / 2, w3 = ((x x) x) S:
    7 u w3, w1 and w2 = fma(t, 0.5, 4 S), t = (x x)(x - 2): 3.5 u absolute — per axis, times the other axes' weights
    the blend: a tap passes 2 roundings in x (product, fma), 4 in y, 4 in z and the last add                 11 (+ 1) u sum W |C|
    ZUNI: 4 in z first (product, three fmas, stored as float32), then 2 + 4 + 1: the same count in the other order — on the combined
    planes, and per voxel (blend64_zfirst) everywhere else in such a launch, so that its result does not depend on the tile grid.
The first term is at most K_PRE u M and the third at most 12 u M (|C| <= A).  The weights' term has no constant of its own either (w0
is known to u z^2 / 2 absolutely, not relatively): cubic_error_field() evaluates all three in float64 per output voxel, the CPU test
asserts their sum <= K_CUBIC u M on every GPU input (it reaches 27.7 there: |C| is far below A where A is large), and
    K_CUBIC = K_PRE + 12 + 4 = 48      (4 for the weights' term, which reaches 1.6 u M on the inputs; the blend's reaches 0.8).

Measured on the float32 numpy restatements below (filter_block in the kernels' blocks, weights3, blend64, blend16 with the in-place
combination; tests/test_cubic_reference.py prints the figures, DESIGN.md §3.3 keeps them): the prefilter stays below 1.2 u A and the
warp below 0.8 u M at every input of the GPU tests.
"""

import functools
from collections import namedtuple

import numpy as np
import torch

import deskew_cases as D
import warp_cases as W
from oracle import reference_f64 as R

U = 2.0 ** -24
f32, f64, i64 = np.float32, np.float64, np.int64
ZP = float(np.sqrt(3.0) - 2.0)
RUN = 20
K_PRE, K_CUBIC = 32, 48
T = 270.0 * abs(ZP) ** RUN
CVAL = W.CVAL
T200, T198 = W.T200, W.T198


# ----------------------------------------------------------------------------- the checks
def _units(err, scale):
    pos = (scale > 0) & torch.isfinite(err)
    return torch.where(pos, err / scale.clamp_min(1e-300), torch.zeros_like(err)) / U


def assert_close(got, V, M, S, K, name, inside=None, cval=None):
    """``|got - V| <= K u M + T S`` at every voxel, ``got == 0`` exactly where M == 0, no NaN or infinity anywhere and, with ``cval``,
    ``got == float32(cval)`` bit for bit outside ``inside``.  Returns the worst error in units of u M."""
    g = torch.as_tensor(got).to(V.device)
    assert g.dtype == torch.float32 and tuple(g.shape) == tuple(V.shape), (name, g.dtype, tuple(g.shape), tuple(V.shape))
    err = (g.to(torch.float64) - V).abs_()
    bad = ~(err <= K * U * M + torch.where(M > 0, T * S, 0.0))
    if cval is not None:
        bad |= ~inside & (g != float(f32(cval)))
    units = _units(err, M)
    worst = float(units.max()) if units.numel() else 0.0
    nbad = int(bad.sum())
    if nbad:
        score = torch.where(bad, torch.where(torch.isfinite(units), units, torch.full_like(units, float("inf"))) + 1.0,
                            torch.zeros_like(units))
        at = tuple(int(i) for i in np.unravel_index(int(score.argmax()), tuple(V.shape)))
        raise AssertionError(f"{name}: {nbad} voxels outside {K} u M + T S (worst finite {worst:.2f} u M); worst at {at}: got "
                             f"{float(g[at])!r} want {float(V[at])!r} M {float(M[at])!r}")
    return worst


def sample_max(vol):
    v = np.asarray(vol)
    return float(np.abs(np.nan_to_num(v.astype(f64), nan=0.0)).max())


# ----------------------------------------------------------------------------- the first-order error fields
def _kappa(k, axis):
    return np.sqrt(3.0) * abs(ZP) ** np.abs(k) * (5.5 + 3.0 * np.abs(k))


def rounding_field(vol, device=None):
    """E / u: the prefilter's first-order rounding error per coefficient — on each axis in turn the kernel kappa, |h| on the others."""
    nd = np.asarray(vol).ndim if not isinstance(vol, torch.Tensor) else vol.ndim
    shape = tuple(vol.shape)
    E = None
    for a in range(nd):
        if shape[a] <= 1:
            continue
        e = R.spline_scale_f64(vol, device, weight=lambda k, ax, a=a: _kappa(k, ax) if ax == a else None)
        E = e if E is None else E + e
    return E if E is not None else torch.zeros(shape, dtype=torch.float64, device=device)


def error_fields(vol, device=None):
    """(E / u, |C|, A, C) of a volume: what cubic_error_field gathers, computed once per volume."""
    x = R._clean_f64(vol, device)
    coef = R.spline_coef_f64(x)
    return rounding_field(x), coef.abs(), R.spline_scale_f64(x), coef


def cubic_error_field(vol, matrix, out_shape, crop_lo, device=None, parts=False, fields=None):
    """(F, M): F / u the warp's first-order error per output voxel (the coefficients' error through the weights, the weights' error
    on |coefficient|, twelve roundings of the blend), zero outside; M the reference's scale.  ``fields``: error_fields(vol), to share
    between calls; the reference's V is then returned as a third value."""
    E, absC, A, coef = error_fields(vol, device) if fields is None else fields
    inside, idx, wts, frac = R.cubic_geometry_f64(tuple(A.shape), matrix, out_shape, crop_lo, A.device)
    dws = []
    for a in range(3):
        xx, zz = frac[a], 1.0 - frac[a]
        dw = [4.0 * wts[a][0] + 0.5 * zz * zz, torch.full_like(xx, 3.5), torch.full_like(xx, 3.5), 7.0 * wts[a][3]]
        dws.append([dw if b == a else wts[b] for b in range(3)])
    res = R.cubic_sum_f64([E, absC, A, coef], idx, wts, dws)
    F = res[0][0] + 12.0 * res[0][1] + sum(r[1] for r in res[1:])
    zero = torch.zeros((), dtype=torch.float64, device=A.device)
    if parts:
        return [torch.where(inside, t, zero) for t in (res[0][0], sum(r[1] for r in res[1:]), 12.0 * res[0][1], res[0][2])]
    F, M = torch.where(inside, F, zero), torch.where(inside, res[0][2], zero)
    return (F, M) if fields is None else (F, M, res[0][3])


# ----------------------------------------------------------------------------- inputs and matrices
DTYPES = W.DTYPES
volume = W.volume
LONG = (9, 9, 2200)      # coordinates near 2048: a float32 coordinate there resolves the fraction to 1e-4
# ... which this bound does not see at 2200 (14.7 u M of 48); on a row of 9000 the float32 coordinate carries 5e-4 of a voxel and costs
# 200 u M on a bead's flank at x = 3221 (three chunks of the x pass besides)
LONG2 = (5, 9, 9000)


@functools.lru_cache(maxsize=4)
def nan_volume(shape):
    """The bead volume with the ``nan`` positions of W.NONFINITE planted (tile interior and tile seam); +-inf is out of scope."""
    vol = np.array(W.volume(shape, "f32"))
    for where in W.NONFINITE.values():
        vol[where["nan"]] = np.nan
    vol.setflags(write=False)
    return vol


Warp = namedtuple("Warp", "A shift launch")      # launch: the gather the restated rule must choose on T200, and whether ZUNI
G8, G4, GLOBAL = 2, 4, 1
WARPS = {
    "identity": Warp(np.eye(3), (0.0, 0.0, 2.75), (G8, True)),
    "integer shift": Warp(np.eye(3), (1.0, -2.0, 3.0), (G8, True)),
    "half-voxel shift": Warp(np.eye(3), (-0.5, -0.5, -0.5), (G8, True)),
    "similarity 2 deg 1.02": Warp(W.about_z(2.0, 1.02), (3.5, -12.25, 20.75), (G8, True)),
    "about z, m00 0.97": Warp(W.about_z(2.0, 1.0, az=0.97), (-0.145, 1.5, 0.25), (G8, False)),     # output planes 12, 13 share their source planes
    "z flip": Warp(np.diag([-1.0, 1.0, 1.0]), (0.25, 0.5, 0.75), (G8, False)),
    "oblique 2 deg": Warp(1.02 * W.rotation(W.OBL, 2.0), (3.5, -2.25, 0.75), (G8, False)),
    "20 deg about y": Warp(W.rotation(W.Y_AX, 20.0), (0.5, 0.25, 0.75), (GLOBAL, False)),
    "shear": Warp(np.array([[0.5, 0.1, 0.0], [0.0, 1.5, 0.2], [0.1, 0.0, 2.0]]), (2.0, -3.0, 1.0), (GLOBAL, False)),
    "8 deg about y": Warp(W.rotation(W.Y_AX, 8.0), (0.5, 0.25, 0.75), (G4, False)),
    "4x minifying rotation": Warp(4.0 * W.rotation((0.5, 1.0, 0.4), 35.0), (0.5, 0.25, 0.75), (GLOBAL, False)),
    "x row near zero": Warp(np.diag([1.0, 1.0, 0.001]), (0.25, 0.5, 2.0), (G8, True)),
    "zero y row": Warp(np.diag([1.0, 0.0, 1.0]), (0.25, -2.25, 0.75), (G8, True)),
}
OUT = W.OUT
CROP_LO, crop_shape = W.CROP_LO, W.crop_shape
SWITCHES = ({}, {"ZUNI": "0"}, {"GATHER": "global"}, {"TZ": "4"}, {"NT": "256"}, {"PITCH32": "0"})


def pull_matrix(name, in_shape, out_shape=None):
    """Centre of the output box -> centre of the input + shift, translations on a 2^-10 grid (W.pull_matrix on this table)."""
    w = WARPS[name]
    out_shape = OUT[tuple(in_shape)] if out_shape is None else out_shape
    m = np.eye(4)
    m[:3, :3] = w.A
    t = (np.asarray(in_shape, f64) - 1) / 2 + np.asarray(w.shift, f64) - w.A @ ((np.asarray(out_shape, f64) - 1) / 2)
    m[:3, 3] = np.round(t * 1024) / 1024
    return m


def degenerate_matrix(in_shape, out_shape, held):
    """Identity with a quarter-voxel shift for a volume one voxel thick; ``held``: the thin axis' row is zero, so its coordinate is
    exactly 0 everywhere (inside under SciPy's [0, n - 1] rule); otherwise it is 0.25 off and every voxel is cval."""
    m = W.degenerate_matrix(in_shape, out_shape, False)
    if held:
        m[list(in_shape).index(1), :] = 0.0
    return m


def long_matrix():
    m = np.eye(4)
    m[2, 3] = 0.37
    return m


# ----------------------------------------------------------------------------- the launch rules of csrc/spline.hip, restated
BX, XCH, BAXIS = 16, 4096, 64
GTX, GTY, G_LDS_FLOATS = 64, 8, 20480
SP_GLOBAL, SP_TILE8, SP_TILE4, SP_ZUNI, SP_X4, SP_PAD32, SP_NT512, SP_VEC = (1 << k for k in range(8))
ceil_div = W.ceil_div


def skew(i):
    return i + (i >> 4)


def x_pass_plan(X):
    clen, nchunk = min(X, XCH), ceil_div(X, XCH)
    tpr = min(256, ceil_div(clen, BX))
    cpad = ceil_div(clen, BX) * BX + 2 * RUN
    pitch = skew(cpad) + 1
    rpw = min(max(1, 256 // tpr), max(1, (160 * 1024 // 4) // pitch))
    return dict(clen=clen, nchunk=nchunk, tpr=tpr, rpw=rpw, pitch=pitch, lds=rpw * pitch * 4)


def axis_plan(n, nouter):
    """axis_kernel<64> along an axis of length n: interior and mirrored blocks per column, and the launches of the 65 535 fold."""
    if n <= 1:
        return dict(interior=0, mirrored=0, launches=0)
    nblk = ceil_div(n, BAXIS)
    inner = sum(1 for b in range(nblk) if b * BAXIS - RUN >= 0 and b * BAXIS + BAXIS + RUN <= n)
    return dict(interior=inner, mirrored=nblk - inner, launches=ceil_div(nouter, max(1, 65535 // nblk)))


def prefilter_plan(shape, dtype="f32", aligned=True):
    """prefilter_typed: the convert-only form (X == 1) or the x pass's chunking and VEC form (``aligned``: the volume's first element
    on a boundary of four samples), the blocks of both column passes and their slab launches, and the code bh_spline_path reports."""
    Z, Y, X = shape
    plan = dict(convert=X == 1, vec=False, y=axis_plan(Y, Z), z=axis_plan(Z, Y))
    if X > 1:
        plan.update(x_pass_plan(X))
        plan["vec"] = X % 4 == 0 and aligned
        plan["grid"] = ceil_div(Z * Y * plan["nchunk"], plan["rpw"])
    plan["code"] = SP_VEC if plan["vec"] else 0
    return plan


def gather_lds_floats(m, in_shape, x4, gtz, pad32):
    need = 1.0
    for a, (t, n) in enumerate(zip((gtz, GTY, GTX), in_shape)):
        e = sum(abs(m[a, j]) * (tt - 1) for j, tt in enumerate((gtz, GTY, GTX)))
        if not e < 1e6:
            return 0
        ext = int(np.floor(e + 1e-3)) + 5
        if a == 2 and x4:
            ext = (ext + 6) & ~3
        ext = min(ext, n)
        if a == 2 and pad32:
            ext = (ext + 31) & ~31
        need *= ext
    return int(need) if need <= G_LDS_FLOATS else 0


GPlan = namedtuple("GPlan", "launch gtz zuni x4 pad32 nt lds_floats code")


def gather_plan(matrix, in_shape, out_shape, dtype="f32", aligned=True, **env):
    """affine_cubic's dispatch under the BH_SPLINE_* switches given as keywords (ZUNI, GATHER, TZ, NT, PITCH32), with the code
    bh_spline_path reports (the prefilter's VEC bit by ``dtype`` and ``aligned``; the coefficients themselves are always aligned)."""
    m = np.asarray(matrix, f64)
    x4 = in_shape[2] % 4 == 0
    pad32 = not str(env.get("PITCH32", "1")).startswith("0")
    global_only = str(env.get("GATHER", "")).startswith("g")
    zuni = m[0, 1] == 0 and m[0, 2] == 0 and m[0, 0] >= 1.0 and not str(env.get("ZUNI", "1")).startswith("0")
    gtz = 4 if str(env.get("TZ", "")) == "4" else 8
    lds = 0 if global_only else gather_lds_floats(m, in_shape, x4, gtz, pad32)
    if lds == 0 and gtz == 8 and not global_only:
        gtz, lds = 4, gather_lds_floats(m, in_shape, x4, 4, pad32)
    nt = int(env["NT"]) if "NT" in env else (512 if gtz == 8 else 256)
    code = prefilter_plan(in_shape, dtype, aligned)["code"]
    if lds > 0:
        code |= (SP_TILE8 if gtz == 8 else SP_TILE4) | (SP_ZUNI if zuni else 0) | (SP_X4 if x4 else 0) | (SP_PAD32 if pad32 else 0) | \
            (SP_NT512 if nt == 512 else 0)
        return GPlan(SP_TILE8 if gtz == 8 else SP_TILE4, gtz, zuni, x4, pad32, nt, lds, code)
    return GPlan(SP_GLOBAL, gtz, zuni, x4, pad32, nt, 0, code | SP_GLOBAL)


def mirror(i, n):
    if n <= 1:
        return np.zeros_like(i)
    s2 = 2 * n - 2
    i = np.mod(i, s2)
    return np.where(i >= n, s2 - i, i)


def _boxes(m, in_shape, out_shape, crop_lo, plan):
    """The GBox of every tile: (o0 [nt, 3], org, ext, interior), integer arrays."""
    Tt = (plan.gtz, GTY, GTX)
    n_t = [ceil_div(n, t) for n, t in zip(out_shape, Tt)]
    o0 = np.stack(np.meshgrid(*[np.arange(k) * t for k, t in zip(n_t, Tt)], indexing="ij"), -1).reshape(-1, 3)
    o1 = np.minimum(o0 + np.asarray(Tt), np.asarray(out_shape)) - 1
    org, ext, interior = (np.zeros(o0.shape, i64) for _ in range(3))
    for a in range(3):
        base = m[a, 0] * (o0[:, 0] + crop_lo[0]) + m[a, 1] * (o0[:, 1] + crop_lo[1]) + m[a, 2] * (o0[:, 2] + crop_lo[2]) + m[a, 3]
        e = [m[a, j] * (o1[:, j] - o0[:, j]).astype(f64) for j in range(3)]
        lo = base + np.minimum(e[0], 0.0) + np.minimum(e[1], 0.0) + np.minimum(e[2], 0.0)
        hi = base + np.maximum(e[0], 0.0) + np.maximum(e[1], 0.0) + np.maximum(e[2], 0.0)
        slack = 1e-9 * (np.abs(lo) + np.abs(hi) + 1.0)
        lo, hi = lo - slack, hi + slack
        n = in_shape[a]
        l, h = np.maximum(np.floor(lo) - 1.0, 0.0), np.minimum(np.floor(hi) + 2.0, n - 1.0)
        og, ex = np.where(h >= l, l, 0).astype(i64), np.where(h >= l, (h - l).astype(i64) + 1, 0)
        if a == 2 and plan.x4:
            end = (og + ex + 3) & ~3
            og = np.where(ex > 0, og & ~3, og)
            ex = np.where(ex > 0, end - og, ex)
        org[:, a], ext[:, a] = og, ex
        interior[:, a] = (np.floor(lo) - 1.0 >= 0.0) & (np.floor(hi) + 2.0 <= n - 1.0)
    return o0, org, ext, interior


FORMS = ("empty", "not staged", "interior", "boundary in box", "boundary with fallback", "zuni combined", "zuni z edge", "LP == 1",
         "dy == 1")


def tile_forms(matrix, in_shape, out_shape, crop_lo, plan):
    """What gather_tile_kernel decides per tile, counted: no source voxel ("empty"), a box beyond the launch's LDS ("not staged":
    every voxel from global memory), interior tiles, boundary tiles whose voxels all find their mirrored taps in the box and boundary
    tiles with at least one voxel that falls back to global memory, and — of a ZUNI launch — tiles that combine their planes and tiles
    at a z edge (or with a plane pitch off the 16-byte grid) that take the 64-tap path; staged tiles whose flat quad list divides by
    ``LP == 1`` and by ``dy == 1``."""
    m = np.asarray(matrix, f64)[:3]
    out = dict.fromkeys(FORMS, 0)
    if plan.launch == SP_GLOBAL:
        return out
    o0, org, ext, interior = _boxes(m, in_shape, out_shape, crop_lo, plan)
    P = np.where(plan.pad32, (ext[:, 2] + 31) & ~31, ext[:, 2])
    nbox = ext[:, 0] * ext[:, 1] * P
    staged = (nbox > 0) & (nbox <= plan.lds_floats)
    inner = staged & interior.all(axis=1)
    comb = staged & ((ext[:, 1] * P) % 4 == 0) & (interior[:, 0] == 1) & (m[0, 0] >= 1.0) & plan.zuni
    # per voxel: inside, and every mirrored tap within its tile's box
    c, _ = W._coords(m, out_shape, crop_lo)
    c = [np.broadcast_to(ca, out_shape) for ca in c]
    ins = np.ones(out_shape, bool)
    for ca, n in zip(c, in_shape):
        ins &= (ca >= 0.0) & (ca <= n - 1)
    Tt = (plan.gtz, GTY, GTX)
    n_t = [ceil_div(n, t) for n, t in zip(out_shape, Tt)]
    tid = [np.arange(n) // t for n, t in zip(out_shape, Tt)]
    tile = (tid[0][:, None, None] * n_t[1] + tid[1][None, :, None]) * n_t[2] + tid[2][None, None, :]
    inbox = np.ones(out_shape, bool)
    for a in range(3):
        b = np.floor(np.where(ins, c[a], 0.0)).astype(i64) - 1
        for k in range(4):
            rel = mirror(b + k, in_shape[a]) - org[:, a][tile]
            inbox &= (rel >= 0) & (rel < ext[:, a][tile])
    need_global = np.zeros(len(o0), bool)
    np.logical_or.at(need_global, tile[ins & ~inbox], True)
    bnd = staged & ~inner
    out.update({"empty": int((nbox == 0).sum()), "not staged": int((nbox > plan.lds_floats).sum()),
                "interior": int((inner & ~comb).sum()), "boundary in box": int((bnd & ~need_global).sum()),
                "boundary with fallback": int((bnd & need_global).sum()), "zuni combined": int(comb.sum()),
                "zuni z edge": int((staged & ~comb).sum()) if plan.zuni else 0})
    if plan.x4:
        out["LP == 1"] = int((staged & (P // 4 == 1)).sum())
        out["dy == 1"] = int((staged & (ext[:, 1] == 1)).sum())
    return out


# ----------------------------------------------------------------------------- float32 restatements, with planted defects
_fma = W._fma
ZP32, GAIN32 = f32(-0.26794919243112270647), f32(6.0)
INIT_C32 = f32(1.0) / (f32(1.0) - ZP32)
INIT_A32 = -ZP32 / (f32(1.0) - ZP32)


def _half_mirror(i, n):
    s2 = 2 * n
    i = np.mod(i, s2)
    return np.where(i >= n, s2 - 1 - i, i)


def filter_axis_f32(v, axis, B, run=RUN, zero_past=False, mirror_fn=mirror, swap_init=False):
    """One pass of filter_block<B> along ``axis`` in the kernels' blocks: every block of B outputs from B + 2 run mirror-extended
    samples, the causal fma recursion from INIT_C, the anticausal one from INIT_A.  ``zero_past``: samples further than ``run`` past
    the row's end read as zeros (x_kernel pads a row that is shorter than a chunk and not a multiple of 16 so)."""
    n = v.shape[axis]
    if n <= 1:
        return v
    v = np.moveaxis(v, axis, -1)
    nblk = ceil_div(n, B)
    pos = (np.arange(nblk) * B)[:, None] + np.arange(-run, B + run)[None, :]
    s = v[..., mirror_fn(pos, n)]
    if zero_past:
        s = np.where(pos >= n + run, f32(0), s)
    L = B + 2 * run
    ic, ia = (INIT_A32, INIT_C32) if swap_init else (INIT_C32, INIT_A32)
    c = [None] * L
    c[0] = GAIN32 * s[..., 0] * ic
    for i in range(1, L):
        c[i] = _fma(ZP32, c[i - 1], GAIN32 * s[..., i])
    a = ia * c[L - 1]
    outs = [None] * B
    for i in range(L - 2, run - 1, -1):
        a = ZP32 * (a - c[i])
        if i < run + B:
            outs[i - run] = a
    r = np.stack(outs, -1).reshape(v.shape[:-1] + (nblk * B,))[..., :n]
    assert r.dtype == f32
    return np.moveaxis(r, -1, axis)


def clean_f32(vol, clean=True):
    vol = np.asarray(vol)
    return np.nan_to_num(vol, nan=0).astype(f32) if (vol.dtype.kind == "f" and clean) else vol.astype(f32)


def prefilter_f32(vol, defect=None):
    """bh_spline_prefilter in numpy float32: x in blocks of 16 (rows shorter than a chunk padded with zeros), y and z in blocks of 64.
    ``defect``: "R8" a run-in of 8; "half" half-sample mirroring; "init" INIT_C and INIT_A swapped; "nan" NaN not cleaned."""
    kw = dict(run=8 if defect == "R8" else RUN, mirror_fn=_half_mirror if defect == "half" else mirror, swap_init=defect == "init")
    v = clean_f32(vol, defect != "nan")
    with np.errstate(invalid="ignore"):
        v = filter_axis_f32(v, 2, BX, zero_past=v.shape[2] < XCH, **kw)
        v = filter_axis_f32(v, 1, BAXIS, **kw)
        return filter_axis_f32(v, 0, BAXIS, **kw)


def weights3_f32(c):
    fl = np.floor(c)
    x = (c - fl).astype(f32)
    z = f32(1.0) - x
    S = f32(1.0) / f32(6.0)
    w = [z * z * z * S, _fma(x * x * (x - f32(2.0)), f32(0.5), f32(4.0) * S), _fma(z * z * (z - f32(2.0)), f32(0.5), f32(4.0) * S),
         x * x * x * S]
    return fl.astype(i64) - 1, w


def blend_f32(tap, wx, wy, wz=None):
    """blend64 (or blend16 with wz None): ``tap(kz, ky, kx)`` float32 arrays.  The x taps 0, 2 and 1, 3 ride in two halves, folded over
    y and z with fmas; the halves add last."""
    def plane(kz):
        az = None
        for ky in range(4):
            ax = [_fma(tap(kz, ky, 2 + h), wx[2 + h], tap(kz, ky, h) * wx[h]) for h in (0, 1)]
            az = [a * wy[ky] for a in ax] if az is None else [_fma(a, wy[ky], b) for a, b in zip(ax, az)]
        return az
    if wz is None:
        az = plane(0)
        return az[0] + az[1]
    acc = None
    for kz in range(4):
        az = plane(kz)
        acc = [a * wz[kz] for a in az] if acc is None else [_fma(a, wz[kz], b) for a, b in zip(az, acc)]
    return acc[0] + acc[1]


def blend_zfirst_f32(tap, wx, wy, wz):
    """blend64_zfirst: the four z taps of every (y, x) tap by the plane combination's fma chain, then blend16."""
    def comb(ky, kx):
        return _fma(wz[3], tap(3, ky, kx), _fma(wz[2], tap(2, ky, kx), _fma(wz[1], tap(1, ky, kx), wz[0] * tap(0, ky, kx))))
    return blend_f32(lambda kz, ky, kx: comb(ky, kx), wx, wy)


def cubic_f32(vol, matrix, out_shape, crop_lo=(0, 0, 0), cval=CVAL, zuni=False, gtz=8, defect=None, coef=None):
    """The cubic warp's arithmetic in numpy float32 (a restatement to hold against the bound, not the code under test): the block
    prefilter, float64 coordinates, weights3 and the packed blend; with ``zuni`` the in-place plane combination of z-interior tiles
    and blend16.  ``defect``: those of prefilter_f32, and
        "w12"     w[1] and w[2] of the x axis exchanged in voxels below 200 counts;
        "coord32" the coordinates in float32;
        "origin"  the x taps of voxels whose first x tap is below 8 read one sample to the right (a box origin off by one);
        "zuni97"  the plane combination forced on a matrix with m00 < 1 (a plane is read after it was overwritten)."""
    m = np.asarray(matrix, f64)[:3]
    if coef is None:
        coef = prefilter_f32(vol, defect if defect in ("R8", "half", "init", "nan") else None)
    dims = coef.shape
    c, (gz, gy, gx) = W._coords(m, out_shape, crop_lo)
    if defect == "coord32":
        m32 = m.astype(f32)
        c = [(((m32[a, 0] * gz.astype(f32) + m32[a, 1] * gy.astype(f32)) + m32[a, 2] * gx.astype(f32)) + m32[a, 3]).astype(f64)
             for a in range(3)]
    c = [np.broadcast_to(ca, out_shape) for ca in c]
    inside = np.ones(tuple(out_shape), bool)
    for ca, n in zip(c, dims):
        inside &= (ca >= 0.0) & (ca <= n - 1)
    bw = [weights3_f32(np.where(inside, ca, 0.0)) for ca in c]
    idx = [[mirror(b + k, n) for k in range(4)] for (b, _), n in zip(bw, dims)]
    wz, wy, wx = (w for _, w in bw)
    if defect == "origin":
        idx[2] = [np.where(bw[2][0] < 8, np.minimum(i + 1, dims[2] - 1), i) for i in idx[2]]
    with np.errstate(invalid="ignore"):
        # a ZUNI launch blends z first everywhere: on combined planes (below), and per voxel elsewhere
        r = (blend_zfirst_f32 if zuni else blend_f32)(lambda kz, ky, kx: coef[idx[0][kz], idx[1][ky], idx[2][kx]], wx, wy, wz)
        if defect == "w12":
            r2 = blend_f32(lambda kz, ky, kx: coef[idx[0][kz], idx[1][ky], idx[2][kx]], [wx[0], wx[2], wx[1], wx[3]], wy, wz)
            r = np.where(np.abs(r) < 200, r2, r)
        if zuni or defect == "zuni97":
            assert m[0, 1] == 0 and m[0, 2] == 0
            Zo = out_shape[0]
            for oz0 in range(0, Zo, gtz):
                zs = np.arange(oz0, min(oz0 + gtz, Zo))
                c0 = m[0, 0] * (zs + crop_lo[0]).astype(f64) + m[0, 3]
                lo, hi = min(c0[0], c0[-1]), max(c0[0], c0[-1])
                slack = 1e-9 * (abs(lo) + abs(hi) + 1.0)
                if not (np.floor(lo - slack) - 1.0 >= 0.0 and np.floor(hi + slack) + 2.0 <= dims[0] - 1):
                    continue        # a z-edge tile: 64 taps per voxel
                planes = coef.copy()
                bz, wzs = weights3_f32(c0)
                for k in range(len(zs)):      # upwards, in place: plane bz takes the combination of output plane k
                    a, b, e, g = (planes[bz[k] + j] for j in range(4))
                    planes[bz[k]] = _fma(wzs[3][k], g, _fma(wzs[2][k], e, _fma(wzs[1][k], b, wzs[0][k] * a)))
                sl = slice(oz0, oz0 + len(zs))
                bzv = np.broadcast_to(bz[:, None, None], (len(zs),) + tuple(out_shape[1:]))
                r = r.copy()
                r[sl] = blend_f32(lambda kz, ky, kx: planes[bzv, idx[1][ky][sl], idx[2][kx][sl]], [w[sl] for w in wx], [w[sl] for w in wy])
    return np.where(inside, r, f32(cval)).astype(f32)


# ----------------------------------------------------------------------------- the cases
PREFILTER_SHAPES = [
    ((24, 40, 200), DTYPES), ((24, 40, 198), ("f32", "u16")), ((2, 3, 5), ("f32",)), ((5, 19, 21), ("f32", "i16")),
    ((1, 40, 200), ("f32",)), ((24, 1, 200), ("f32", "u8")), ((24, 40, 1), ("f32", "u16")), ((1, 1, 37), ("f32",)),
    ((150, 150, 8), ("f32",)), ((2, 3, 16), ("f32",)), ((2, 3, 17), ("f32",)), ((1, 5, 2048), ("f32",)), ((1, 5, 2052), ("f32",)),
    ((2, 3, 4096), ("f32",)), ((2, 3, 4097), ("f32",)), ((2, 3, 4100), ("f32", "u16")), ((70000, 2, 2), ("f32",)), ((2, 70000, 2), ("f32",)),
]


def warp_cases():
    """[(warp name, input shape, dtype)]: every warp on T200 and T198 in every type of DTYPES."""
    return [(name, shape, d) for name in WARPS for shape in (T200, T198) for d in DTYPES]


# ----------------------------------------------------------------------------- integer outputs
CAST_KINDS = ("u16", "i16", "u8")
CAST_PUSH = "similarity 2 deg 1.02"


@functools.lru_cache(maxsize=3)
def cast_volume(kind):
    """Integer inputs for the rounding rule of ``cast_like_scipy``: dim enough that the bound leaves all but a few voxels decidable
    (the bead volume / 64: background 2, beads to 940; int16: the same minus 40, both signs; uint8: counts / 8, saturating)."""
    base = np.rint(np.asarray(D.bead_volume(T200)) / 64.0)
    vol = {"u16": base.astype(np.uint16), "i16": (base - 40).astype(np.int16), "u8": np.array(D.as_dtype(D.bead_volume(T200), "u8"))}[kind]
    vol.setflags(write=False)
    return vol


def cast_push_matrix():
    """The push matrix handed to ``Transform``; the operator (and the reference) pull with its ``np.linalg.inv``."""
    return np.linalg.inv(pull_matrix(CAST_PUSH, T200, T200))


def round_half_away(V, dtype):
    info = np.iinfo(dtype)
    r = torch.where(V > 0, torch.floor(V + 0.5), torch.ceil(V - 0.5))
    return r.clamp(float(info.min), float(info.max))


def decidable(V, M, S):
    """Voxels whose float64 value lies farther from a half-integer than the bound: their rounded value is the reference's."""
    frac = (V - torch.floor(V) - 0.5).abs()
    return frac > K_CUBIC * U * M + T * S
