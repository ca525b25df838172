"""Inputs, geometries, the restated launch rules and the bound of the deskew tests (tests/test_deskew_reference.py on the CPU,
tests/test_gpu_deskew_f64.py on the GPU).

THE BOUND — derived, not measured.  Per output voxel the kernels (csrc/deskew.hip, csrc/host_deskew.hip) evaluate, in float32,

    got = div_N( fma(v1, w1, v0 * w0)_0 + fma(...)_1 + ... + fma(...)_{N-1} )

at sample positions and weights that are the float64 reference's own (oracle/reference_f64.py: deskew_f64 takes the float32
positions of ``oracle_np.deskew_coords`` and the float32 weights; integer input widens exactly).  Each averaged slice rounds
twice (the product v0 w0, then the fused multiply-add), each by at most u = 2^-24 of |v0| w0 + |v1| w1; the N - 1 additions
round a partial sum that is at most sum_k (|v0| w0 + |v1| w1) = N M; the division by N is correctly rounded (div_small).  So to
first order

    |got - V| <= (2 + (N - 1) + 1) u M = (N + 2) u M,       M = (1/N) sum_k (|v0| w0 + |v1| w1),

and the tests assert ``|got - V| <= (N + 3) u M`` at EVERY voxel — one u for the second-order terms and the float64 reference's
own rounding — and ``got == 0`` exactly wherever M == 0 (every tap outside the scanned range, or zero: a sum of exact zeros in
any precision).  M, not the volume's maximum, is the scale: a background voxel of 110 counts beside a bead of 60 000 is held to
(N + 3) x 6.6e-6 counts, where ``rel_err <= 1e-5`` let it be wrong by 0.6.

The float32 numpy oracle ``oracle_np.fast_deskew_zyx`` rounds once more per averaged slice (v0 w0, v1 w1, then their sum), which
puts its first-order worst case AT (N + 3) u M; it is held to the same bound on the CPU, and so is ``bh_host_deskew`` (the
kernels' operation order on the host's threads).  Where they were measured (tests/test_deskew_reference.py prints the figures;
DESIGN.md §3.1 keeps them),
in units of u M, worst voxel: the oracle 1.7 .. 3.1 and the host deskew 1.4 .. 3.1 at the six CPU geometries (N = 1 .. 7: 1.7 at
N = 1, 3.1 at N = 7), and both at most 3.0 at the inputs of the GPU tests (N = 1 .. 12) — the worst case of N + 2 roundings
aligning does not occur, the error grows like their random sum.

THE FILL.  With a mean fill on non-negative data without zeros: every voxel of the reference's dilated mask holds ONE value, and
that value lies within (N + 4) u relative of the reference's float64 mean — each voxel of the mean within (N + 3) u of its own
value (M == V on non-negative data), carried through a mean of non-negative terms, plus the one rounding to float32; voxels
outside the mask obey the per-voxel bound.  With a constant fill the masked voxels are the constant bit for bit.
"""

import functools

import numpy as np

from oracle import oracle_np as O

U = 2.0 ** -24
f32 = np.float32


def voxel_bound(N):
    """(N + 3) u: the factor of M the kernels' error must stay under at every voxel."""
    return (N + 3) * U


def fill_bound(N):
    """Relative distance of a float32 mean fill from the reference's float64 mean."""
    return (N + 4) * U


# ----------------------------------------------------------------------------- the check
def deskew_errors(got, V, M):
    """(max |got - V| / M in units of u over M > 0, number of voxels with M == 0 and got != 0); float64 torch tensors or arrays."""
    import torch

    got, V, M = (torch.as_tensor(t) for t in (got, V, M))
    err = (got.to(torch.float64) - V).abs_()
    pos = M > 0
    worst = float((err[pos] / M[pos]).max()) / U if bool(pos.any()) else 0.0
    return worst, int(((got != 0) & ~pos).sum())


def assert_deskew_close(got, ref, N, name, bound=None, fill=None):
    """``got`` (float32, numpy or torch, any device) against ``ref = deskew_f64(...)`` moved to the same device.
    No fill (``ref[2] is None``): the per-voxel bound everywhere and exact zeros where M == 0.  With a fill: the same outside
    the reference's mask; inside it one value — within ``fill_bound`` of the float64 mean ("mean"), or the constant bit for bit.
    Returns the worst error in units of u M (printed by the callers)."""
    import torch

    V, M, mask, fillv = ref
    g = torch.as_tensor(got).to(V.device)
    assert g.dtype == torch.float32 and tuple(g.shape) == tuple(V.shape), (name, g.dtype, tuple(g.shape), tuple(V.shape))
    bound = voxel_bound(N) if bound is None else bound
    err = (g.to(torch.float64) - V).abs_()
    bad = ~(err <= bound * M)                  # M == 0: any non-zero value is a violation; a NaN or an infinity always is
    if mask is not None:
        bad &= ~mask
    nbad = int(bad.sum())
    sel = (M > 0) if mask is None else (M > 0) & ~mask
    worst = float((err[sel] / M[sel]).max()) / U if bool(sel.any()) else 0.0
    if nbad:
        at = tuple(int(i) for i in torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {nbad} voxels outside {bound / U:.0f} u M (worst {worst:.2f} u M); first at {at}: "
                             f"got {float(g[at])!r} want {float(V[at])!r} M {float(M[at])!r}")
    if mask is not None:
        inside = g[mask]
        if inside.numel():
            v = inside[0]
            if fillv != fillv:      # nothing outside the mask: the mean of an empty selection, NaN in the reference too
                assert bool(torch.isnan(inside).all()), f"{name}: expected a NaN fill"
                return worst
            assert bool((inside == v).all()), f"{name}: the filled voxels hold more than one value"
            if fill == "mean":
                assert abs(float(v) - fillv) <= fill_bound(N) * abs(fillv), (name, float(v), fillv)
            else:
                assert fill is not None and float(v) == float(f32(fill)) == float(f32(fillv)), (name, float(v), fillv)
    return worst


# ----------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=8)
def bead_volume(shape, seed=0):
    """Camera counts as float32: a background of 110 +- 3 (Gaussian), twelve Gaussian beads (sigma 1.5 voxels) of 3 000 .. 60 000
    counts at random positions, rounded to whole counts.  No voxel is zero.  Read-only (shared between tests)."""
    rng = np.random.default_rng(1000 + seed + sum(shape))
    vol = rng.normal(110.0, 3.0, shape)
    r = np.arange(-4, 5)
    for _ in range(12):
        c = [int(rng.integers(0, n)) for n in shape]
        amp = float(rng.uniform(3000.0, 60000.0))
        idx = [np.clip(ci + r, 0, n - 1) for ci, n in zip(c, shape)]
        g = [np.exp(-0.5 * (r / 1.5) ** 2) for _ in range(3)]
        np.add.at(vol, np.ix_(*idx), amp * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :])
    vol = np.clip(np.rint(vol), 1, 65535).astype(f32)
    vol.setflags(write=False)
    return vol


def as_dtype(vol, kind):
    """The bead volume as the operator's input types: float32; uint16 (the counts); uint8 (counts / 8, saturating at 255: the
    background stays at 13 .. 15, no zeros); int16 (counts - 32768: signed, both signs present); "f32s": the int16 values as
    float32 (signed float input)."""
    if kind == "f32":
        return vol
    if kind == "u16":
        return vol.astype(np.uint16)
    if kind == "u8":
        return np.minimum(np.rint(vol / 8.0), 255).astype(np.uint8)
    if kind == "i16":
        return (vol.astype(np.int32) - 32768).astype(np.int16)
    if kind == "f32s":
        return (vol - f32(32768)).astype(f32)
    raise ValueError(kind)


def zero_block(vol):
    """A copy with a block of exact zeros inside the signal (the reference's ``data == 0`` masks them: fill path 2)."""
    Z, Y, X = vol.shape
    out = vol.copy()
    out[Z // 3: Z // 3 + max(2, Z // 6), : max(1, min(20, Y // 2)), X // 8: X // 8 + max(2, X // 4)] = 0
    return out


# ----------------------------------------------------------------------------- the launch rules of csrc/deskew.hip, restated
CANDIDATES = ((64, 4), (64, 2), (32, 4), (64, 1), (32, 1))   # (TX, J) of configurations 0 .. 4
ORDER_STD, ORDER_ROWS = (0, 1, 2, 3, 4), (1, 0, 2, 3, 4)       # no fill / mask prologue; one-pass fill
TWO_PER_CU, LDS_MAX = 80 * 1024, 160 * 1024


def geometry(shape, angle, ratio, N, keep_overhang=True):
    """deskew_geometry: (Za, Xp, px, pxct, offset, zm1), the four coordinates constants rounded to float32 once."""
    Z, Y, X = shape
    (_, _, Xp), _ = O.get_deskewed_data_shape(shape, angle, ratio, keep_overhang)
    ct = np.cos(angle * np.pi / 180.0)
    offset = ratio * ct * (Y - 1) / 2 - ratio * (Xp - 1) / 2 + (Z - 1) / 2
    return -(-Y // N), Xp, f32(ratio), f32(ratio * ct), f32(offset), f32(Z - 1)


def deskew_ix(geo, xo, zo):
    """deskew_ix in float32, operation by operation (``xo``, ``zo`` integer arrays, broadcast)."""
    _, _, px, pxct, offset, zm1 = geo
    in_z = (px * np.asarray(xo, f32) - pxct * np.asarray(zo, f32)) + offset
    g = (f32(2.0) * in_z) / zm1 - f32(1.0)
    return (((g + f32(1.0)) / f32(2.0)) * zm1).astype(f32)


def windows(shape, geo, N, XC):
    """(zlo, zcnt) of every (a, x'-chunk): the z window the kernels stage, before the clamp to ZC."""
    Za, Xp = geo[0], geo[1]
    a = np.arange(Za)[:, None]
    xo0 = np.arange(0, Xp, XC)[None, :]
    xoN = np.minimum(XC, Xp - xo0)
    zlo = np.floor(deskew_ix(geo, xo0, a * N + N - 1)).astype(np.int64)
    zhi = np.floor(deskew_ix(geo, xo0 + xoN - 1, a * N)).astype(np.int64)
    return zlo, zhi + 2 - zlo


def max_window(shape, geo, N, XC):
    return int(windows(shape, geo, N, XC)[1].max())


def cfg_lds(shape, geo, N, cfg):
    TX, J = CANDIDATES[cfg]
    return N * max_window(shape, geo, N, 64 * J) * (TX + 1) * 4


def selected_cfg(shape, angle, ratio, N, one_pass=False, keep_overhang=True):
    """launch_deskew's choice: the first configuration (in the path's order) whose tile lets two workgroups share a CU, else
    the first that fits 160 KiB, else the last.  Returns (configuration, its LDS bytes)."""
    geo = geometry(shape, angle, ratio, N, keep_overhang)
    lds = [cfg_lds(shape, geo, N, c) for c in range(5)]
    order = ORDER_ROWS if one_pass else ORDER_STD
    pick = next((c for c in order if lds[c] <= TWO_PER_CU), None)
    if pick is None:
        pick = next((c for c in order if lds[c] <= LDS_MAX), 4)
    return pick, lds[pick]


def tile_workgroups(shape, angle, ratio, N, cfg, keep_overhang=True):
    """launch_deskew_cfg's grid for configuration ``cfg``: ceil(X / TX) x ceil(Xp / (64 J)) x Za workgroups.  With the mask prologue
    each of them hands ``finalize_kernel`` (csrc/fill.hip) one block sum."""
    TX, J = CANDIDATES[cfg]
    Za, Xp = geometry(shape, angle, ratio, N, keep_overhang)[:2]
    return -(-shape[2] // TX) * -(-Xp // (64 * J)) * Za


def persistent(shape, angle, ratio, N, keep_overhang=True):
    """launch_deskew_pers for float32 input: None when the kernel declines (N > 4, X no multiple of 64, two tile buffers above
    160 KiB), else (ntiles, tiles whose window lies outside the volume, LDS bytes)."""
    Z, Y, X = shape
    if N < 1 or N > 4 or X % 64:
        return None
    geo = geometry(shape, angle, ratio, N, keep_overhang)
    zlo, zcnt = windows(shape, geo, N, 256)
    ZC = max(int(zcnt.max()), 3)
    lds = 2 * N * ZC * 65 * 4
    if lds + 256 > LDS_MAX:
        return None
    zcnt = np.minimum(zcnt, ZC)
    overhang = (zlo + zcnt <= 0) | (zlo >= Z)
    return int(zlo.size) * (X // 64), int(overhang.sum()) * (X // 64), lds


# ----------------------------------------------------------------------------- the cases
# (shape, angle, ratio, N, configuration launch_deskew selects without a fill / with the mask prologue): the smallest volumes
# that reach each configuration by the rule itself.  test_deskew_reference.py checks the column against ``selected_cfg``.
NATURAL = [
    ((100, 9, 70), 36.17, 0.371, 3, 0),
    ((100, 9, 70), 36.17, 0.371, 5, 1),    # 66 300 B of LDS: the hipFuncSetAttribute branch (> 64 KiB) taken by the rule
    ((24, 12, 40), 30.0, 0.9, 12, 2),      # generic N, register staging
    ((240, 8, 70), 36.17, 0.9, 4, 3),
    ((260, 8, 70), 36.17, 0.95, 6, 4),     # generic N; configuration 0 would need 387 KB
]
NATURAL_LDS_CFG1 = 66300

# Forced configurations (BH_DESKEW_CFG = 0 .. 4): (shape, angle, ratio).  X = 70 / 66: ragged tiles and rows not 4-aligned (the
# scalar staging path); 72: rows 4-aligned, ragged last tile (vector path on whole tiles, scalar on the last); 128: whole tiles
# (LDS-DMA on configurations 0 / 1 / 3 with float32, the vector register path on 2 / 4 and for the integer types).
FORCED_GEOMETRIES = [((48, 37, 70), 36.17, 0.371), ((31, 50, 66), 45.0, 0.9), ((48, 37, 72), 36.17, 0.371), ((31, 50, 128), 45.0, 0.9)]
# The product N x dtype x fill x geometry is 5 x 4 x 3 x 4 = 240 runs of five configurations; kept is a subset in which every
# PAIR (N, dtype), (N, fill), (N, geometry), (dtype, geometry), (fill, geometry) and (dtype, fill) occurs, except that int16 (signed
# data) runs without a mean fill: the fill rule above is stated for non-negative data.  int16 with a CONSTANT fill is run (the
# last case): the reference's mask is ``V == 0``, which signed data could meet by cancellation, and test_deskew_reference.py asserts
# that at this input it does not (V == 0 exactly where M == 0).  Built by
# ``forced_cases``: geometry g and N walk all 20 combinations; dtype and fill rotate with offsets that are coprime walks.
FORCED_N = (1, 2, 3, 4, 5)
FORCED_DTYPES = ("f32", "u16", "u8", "i16")
FORCED_FILLS = (0, "mean", 321.5)


INT16_CONSTANT = (0, 3, "i16", 321.5)


def forced_cases():
    """[(geometry index, N, dtype, fill)]: 20 (geometry, N) combinations, dtype = (g + n) mod 4, fill = (g + 2 n) mod 3 (0 for int16),
    plus the (dtype, fill) and (N, fill) pairs that walk leaves out and int16 with a constant fill."""
    cases = []
    for g in range(len(FORCED_GEOMETRIES)):
        for n, N in enumerate(FORCED_N):
            d = FORCED_DTYPES[(g + n) % 4]
            cases.append((g, N, d, 0 if d == "i16" else FORCED_FILLS[(g + 2 * n) % 3]))
    have = set(cases)
    for d in ("f32", "u16", "u8"):
        for f in FORCED_FILLS:
            if not any(c[2] == d and c[3] == f for c in have):
                cases.append((len(cases) % 4, FORCED_N[len(cases) % 5], d, f))
    for N in FORCED_N:
        for f in FORCED_FILLS:
            if not any(c[1] == N and c[3] == f for c in cases):
                cases.append((len(cases) % 4, N, "f32", f))
    cases.append(INT16_CONSTANT)
    return cases


# The persistent kernel's walk: (shape, angle, ratio, N, tiles per workgroup a 256-CU device is sure to walk).  A workgroup
# walks ceil(ntiles / CUs) consecutive tiles.  The first geometry has 2 400 tiles, 1 104 of them overhang (runs of them for
# ``advance`` and ``emit`` to cross).  The two (24, 40x, 128) geometries have 536: three consecutive tiles per workgroup on the 179
# workgroups that get any, but fewer than 3 x 256 in all, so (24, 576, 128) and (24, 575, 128) — the same geometry, 1 152 tiles —
# stand beside them for the test's ``ntiles >= 3 x multi_processor_count``.  The last two rows walk the N = 2 and N = 4 kernels (800
# tiles, 316 of them overhang, two buffers of 68 640 B; 1 200 tiles, 716 overhang, 139 360 B).
PERSISTENT = [
    ((48, 400, 128), 36.17, 0.25, 1, 2400),
    ((24, 402, 128), 36.17, 0.371, 3, 536),     # Y % N == 0
    ((24, 401, 128), 36.17, 0.371, 3, 536),     # ragged last slab: one replicated row
    ((24, 576, 128), 36.17, 0.371, 3, 1152),
    ((24, 575, 128), 36.17, 0.371, 3, 1152),    # ragged last slab
    ((16, 400, 128), 36.17, 0.25, 2, 800),      # N = 2 and N = 4: the instantiations the (N, fill mode) launch table could mis-map
    ((16, 800, 128), 36.17, 0.25, 4, 1200),
]
PERSISTENT_DECLINED = ((240, 8, 64), 36.17, 0.9, 4)      # two buffers of 242 KB
CUS = 256

# Edges: (shape, angle, ratio, N, keep_overhang, what)
EDGES = [
    ((2, 1, 1), 36.17, 0.371, 1, True, "the smallest volume"),
    ((3, 2, 5), 36.17, 0.371, 4, True, "Y < N: one slab, two replicated rows"),
    ((64, 30, 40), 30.0, 0.25, 2, False, "keep_overhang=False"),
    ((56, 39, 64), 36.17, 0.25, 2, True, "Xp = 256: one whole x' chunk, every store 16 bytes"),
    ((56, 40, 64), 36.17, 0.25, 2, True, "Xp = 257 = 1 mod 4: rows off 16-byte alignment, a second x' chunk of one voxel"),
]

# CPU geometries of the measured positions in the module docstring: N = 1, 2, 3, 4, 5, 7, keep_overhang both ways
CPU_GEOMETRIES = [
    ((20, 7, 9), 36.17, 0.371, 1, True), ((20, 7, 9), 36.17, 0.371, 2, False), ((16, 10, 8), 30.0, 0.9, 3, True),
    ((30, 9, 6), 45.0, 0.25, 4, True), ((24, 11, 7), 36.17, 0.5, 5, False), ((18, 15, 6), 20.0, 0.8, 7, True),
]


def gpu_inputs():
    """Every input the GPU tests run: (shape, angle, ratio, N, keep_overhang, dtype, fill, zero block).  The CPU tests hold the
    float32 oracle and the host deskew to the same bound at each of them."""
    out = []
    for shape, angle, ratio, N, _ in NATURAL:
        out += [(shape, angle, ratio, N, True, d, f, False) for d in ("f32", "u16") for f in (0, "mean")]
    out += [FORCED_GEOMETRIES[g] + (N, True, d, f, False) for g, N, d, f in forced_cases()]
    for shape, angle, ratio, N, _ in PERSISTENT:
        out += [(shape, angle, ratio, N, True, "f32", 0, False), (shape, angle, ratio, N, True, "f32", "mean", False),
                (shape, angle, ratio, N, True, "f32", "mean", True)]
    out += [PERSISTENT_DECLINED + (True, "f32", f, False) for f in (0, "mean")]
    for shape, angle, ratio, N, keep, _ in EDGES:
        out += [(shape, angle, ratio, N, keep, "f32", f, False) for f in ((0, "mean") if keep else (0,))]
    return out


# ----------------------------------------------------------------------------- a float32 restatement, with planted defects
def deskew_f32(raw, angle, ratio, keep_overhang, N=1, fill=0, defect=None, coords64=False):
    """The kernels' arithmetic in numpy float32: positions and weights as ``oracle_np.fast_deskew_zyx``, one product and one fused
    multiply-add per averaged slice (the fma formed in float64 — the product of two float32 is exact there — and rounded once),
    slices summed in order, one correctly rounded division, then the reference's fill.
    ``defect``: "bias" — voxels below 200 counts come out 1e-5 (relative) too large;
                "shear" — the replicated rows of the last slab (zo > Y - 1) sampled with the shear of row Y - 1, not their own;
                "mean" — the fill mean taken outside the UNDILATED zero mask.
    ``coords64``: the sample positions evaluated in float64 and rounded to float32 once (not the contract: see DESIGN.md §3.1)."""
    raw = np.asarray(raw, dtype=f32)
    Z, Y, X = raw.shape
    (_, _, Xp), _ = O.get_deskewed_data_shape(raw.shape, angle, ratio, keep_overhang)
    Za = -(-Y // N)
    out = np.empty((Za, X, Xp), f32)
    for a in range(Za):
        acc = None
        for k in range(N):
            zo = a * N + k
            plane = raw[:, Y - 1 - min(zo, Y - 1), ::-1]
            zs = min(zo, Y - 1) if defect == "shear" else zo
            if coords64:
                ct = np.cos(angle * np.pi / 180)
                offset = ratio * ct * (Y - 1) / 2 - ratio * (Xp - 1) / 2 + (Z - 1) / 2
                ix = (ratio * np.arange(Xp) - ratio * ct * zs + offset).astype(f32)
            else:
                ix = O.deskew_coords(Z, Y, Xp, angle, ratio, zs)
            fl = np.floor(ix)
            w1, w0 = (ix - fl).astype(f32), ((fl + f32(1.0)) - ix).astype(f32)
            i0 = fl.astype(np.int64)
            v0 = np.where(((i0 >= 0) & (i0 < Z))[None, :], plane[np.clip(i0, 0, Z - 1), :].T, f32(0))
            v1 = np.where(((i0 + 1 >= 0) & (i0 + 1 < Z))[None, :], plane[np.clip(i0 + 1, 0, Z - 1), :].T, f32(0))
            p = (v0 * w0[None, :]).astype(f32)
            val = (v1.astype(np.float64) * w1[None, :].astype(np.float64) + p.astype(np.float64)).astype(f32)
            acc = val if acc is None else (acc + val).astype(f32)
        out[a] = acc / f32(N) if N > 1 else acc
    if defect == "bias":
        out = np.where(np.abs(out) < 200, out * f32(1.0 + 1e-5), out).astype(f32)
    if keep_overhang and (fill == "mean" or fill != 0):
        zero = out == 0
        dil = O.dilate_zero_mask(zero, 3)
        if fill == "mean":
            valid = out[~(zero if defect == "mean" else dil)]
            fv = f32(valid.mean(dtype=np.float64)) if valid.size else f32(np.nan)
        else:
            fv = f32(fill)
        out = np.where(dil, fv, out).astype(f32)
    return out
