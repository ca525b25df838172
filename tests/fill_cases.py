"""Inputs, the checker, its bound and a numpy restatement of the overhang fill (csrc/fill.hip) for tests/test_fill_reference.py (CPU)
and tests/test_gpu_fill_f64.py (GPU).

THE CONTRACT is mostly exact.  ``reference_f64.fill_overhang_f64`` gives the mask — ``vol == 0`` dilated ``iterations`` times by the
3x3x3 cube (connectivity 26) or the cross (6) —, the float64 mean of the voxels outside it, and ``kappa``.  The mask is integer
logic: a voxel inside it holds the fill value, ONE value everywhere; a voxel outside it is the input bit for bit (compared as
int32, so a NaN's payload and the sign of a zero count).  A constant fill is ``float32(constant)`` bit for bit.  Only the mean has
a bound.

THE BOUND — derived, not measured.  The kernels form

    fill = float32( (S_all - S_shell) / (n - c) ),

S_all the sum of all n voxels and S_shell the sum of the c voxels inside the mask, both of float32 values widened exactly to
float64 and added in float64 in some order (per lane, per wavefront, per workgroup, then ``finalize_kernel``); n - c is an exact
integer.  Recursive summation of m terms in any order is off by at most (m - 1) 2^-53 of the sum of the terms' magnitudes (to first
order), so the two sums together are off by at most (n - 1) 2^-53 (sum |vol| + sum |vol[mask]|) = (n - 1) 2^-53 kappa (n - c), kappa
the magnitude the two sums carry per valid voxel.  The subtraction and the division add 2^-53 relative each — of a quantity
that is at most kappa (n - c) — and the single rounding to float32 at most half an ulp, 2^-24 relative.  Divided by n - c:

    |g - fill| <= 2^-24 |fill| + (n + 1) 2^-53 kappa  <=  2^-24 |fill| + n 2^-52 kappa,

the factor 2 in 2^-52 being the slack (second-order terms, the reference's own float64 rounding).  Every input here is chosen so
that, for the reference alone, some voxel stays outside the mask and the second term stays below the first (``assert_input_ok``,
asserted on the CPU): what the GPU run checks is then one or two float32 ulps of the mean.

Non-finite data: a NaN outside the mask makes the mean NaN in the reference and here.  A NaN or an infinity INSIDE the mask (in
the shell: dilated, not itself zero) leaves the reference's mean finite but gives NaN here, because S_all - S_shell cannot undo
it; that divergence is known and asserted as it is.

THE RESTATEMENT (``fill_restated``) follows the kernels' data layout in numpy — rows of W32 = 2 ceil(X / 64) 32-bit mask words,
x-dilation by shifts inside and between the words of a row, y and z by OR-ing rows and planes, the cross per (dz, dy) with the
remaining radius along x, and ``apply_fill_kernel``'s unit, head, group and straddle addressing — and takes planted defects, each
of which the checker must reject (tests/test_fill_reference.py).
"""

import functools

import numpy as np
import torch

import deskew_cases as D

U = 2.0 ** -24
f32 = np.float32


# ----------------------------------------------------------------------------- the bound and the check
def fill_tolerance(fill, kappa, n):
    """2^-24 |fill| + n 2^-52 kappa: how far a float32 mean fill may lie from the reference's float64 mean."""
    return U * abs(fill) + n * 2.0 ** -52 * kappa


def assert_input_ok(ref, n, name):
    """The two conditions on an input, for the reference alone: a voxel outside the mask, and the summation term of the bound
    below the float32 rounding term."""
    mask, fill, kappa = ref
    assert n - int(mask.sum()) > 0, f"{name}: nothing outside the mask"
    assert n * 2.0 ** -52 * kappa < U * abs(fill), (name, n, kappa, fill)


def with_fill(ref, fill):
    """The reference of the same input under a constant fill (``fill`` a number) or the mean ("mean")."""
    return ref if fill == "mean" else (ref[0], float(fill), ref[2])


def _t(x, device):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.array(x))      # a writable, contiguous copy
    return x.to(device).contiguous()


def assert_fill_close(got, vol, ref, fill, name):
    """``got`` (float32, numpy or torch, any device) against ``ref = fill_overhang_f64(vol, ...)``; ``fill`` is "mean" or the
    constant.  Outside the mask: ``vol`` bit for bit.  Inside: one value — the constant bit for bit, or within ``fill_tolerance`` of the
    float64 mean, or NaN everywhere when the reference's mean is NaN (nothing outside the mask, or a NaN there).
    Returns |g - fill| / (2^-24 |fill|) (0 for a constant fill or an empty mask, NaN for a NaN fill)."""
    mask, fillv, kappa = ref
    g, v = _t(got, mask.device), _t(vol, mask.device)
    assert g.dtype == torch.float32 and v.dtype == torch.float32, (name, g.dtype, v.dtype)
    assert tuple(g.shape) == tuple(mask.shape) == tuple(v.shape), (name, tuple(g.shape), tuple(mask.shape))
    gi, vi = g.view(torch.int32), v.view(torch.int32)
    bad = (gi != vi) & ~mask
    nbad = int(bad.sum())
    if nbad:
        at = tuple(int(i) for i in torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {nbad} voxels outside the mask changed; first at {at}: got {float(g[at])!r} "
                             f"(0x{int(gi[at]) & 0xffffffff:08x}) input {float(v[at])!r} (0x{int(vi[at]) & 0xffffffff:08x})")
    inside = gi[mask]
    if inside.numel() == 0:
        return 0.0
    if fill != "mean":
        want = int(np.array(fill, f32).view(np.int32))
        assert float(fillv) == float(fill), (name, fillv, fill)
        wrong = inside != want
        if bool(wrong.any()):
            at = tuple(int(i) for i in torch.nonzero(mask & (gi != want))[0])
            raise AssertionError(f"{name}: {int(wrong.sum())} masked voxels are not the constant {fill!r}; first at {at}: {float(g[at])!r}")
        return 0.0
    if fillv != fillv:
        nan = torch.isnan(g[mask])
        if not bool(nan.all()):
            at = tuple(int(i) for i in torch.nonzero(mask & ~torch.isnan(g))[0])
            raise AssertionError(f"{name}: expected a NaN fill; {int((~nan).sum())} masked voxels are not; first at {at}: {float(g[at])!r}")
        return float("nan")
    differ = inside != inside[0]
    if bool(differ.any()):
        at = tuple(int(i) for i in torch.nonzero(mask & (gi != inside[0]))[0])
        raise AssertionError(f"{name}: the masked voxels hold more than one value ({int(differ.sum())} differ from the first); "
                             f"first at {at}: {float(g[at])!r}, input {float(v[at])!r}, first masked value {float(g[mask][0])!r}")
    val = float(g[mask][0])
    err, tol = abs(val - fillv), fill_tolerance(fillv, kappa, g.numel())
    assert err <= tol, f"{name}: fill {val!r}, float64 mean {fillv!r}: off by {err / (U * abs(fillv)):.3f} x 2^-24 |fill| (kappa {kappa!r})"
    return err / (U * abs(fillv)) if fillv != 0 else 0.0


# ----------------------------------------------------------------------------- inputs
def counts(shape, seed=0):
    """A writable copy of ``deskew_cases.bead_volume``: positive camera counts, no voxel zero."""
    return np.array(D.bead_volume(tuple(shape), seed))


# Word and row edges: every X puts the row end at another place of the 32-bit mask words and of the 64-bit padding.
EDGE_X = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)
EDGE_ITERATIONS = (0, 1, 2, 3, 7)
EDGE_SIDES = ("hi", "lo", "ends")


def edge_case(X, iterations, side):
    """(5, 6, X) with single zeros, one per x site, each on another (plane, row) of first / inner / last, rotating with X and the
    iteration count so that every combination occurs.  "hi": x in {31, 63, X - 1}, the top bits of words and the row's last voxel — the
    dilation carries UP into the next word, never past the row end; "lo": x in {0, 32, 64}, carrying DOWN, never before the row start;
    "ends": (z, y, X - 1) and (z, y + 1, 0), neighbours in memory and in the mask words' padding, not in the volume.
    X <= 2 has no x extent to keep a voxel outside seven 3x3x3 dilations: those volumes are (9, 24, X)."""
    i = EDGE_X.index(X)
    Z, Y = (9, 24) if X <= 2 else (5, 6)
    vol = counts((Z, Y, X))
    zs, ys = (0, Z // 2, Z - 1), (0, Y // 2, Y - 1)
    if side == "ends":
        z, y = zs[(i + iterations) % 3], (0, Y // 2, Y - 2)[i % 3]
        vol[z, y, X - 1] = 0
        vol[z, y + 1, 0] = 0
        return vol
    xs = sorted({x for x in ((31, 63, X - 1) if side == "hi" else (0, 32, 64)) if 0 <= x < X})
    for k, x in enumerate(xs):
        vol[zs[(k + i) % 3], ys[(k + i + iterations) % 3], x] = 0
    return vol


def thirty_one_case():
    """(3, 3, 200) with one zero at x = 100: 31 dilations leave x < 69 and x > 131 valid."""
    vol = counts((3, 3, 200))
    vol[1, 1, 100] = 0
    return vol


# Chunk edges: apply_fill_kernel's unit is 2048 voxels of a row (64 mask words); a row that is no multiple of 16 bytes from the
# volume's start shifts its 16-byte groups by a0 = 1 .. 3 voxels, and the last group of a unit then straddles into the next unit's
# first word.
CHUNK_X = (2047, 2048, 2049, 2050, 2051, 4097, 6145)
CHUNK_ISO_ROWS = tuple(range(13)) + (15, 16, 17)
CHUNK_ISO_X = tuple(range(2044, 2052)) + tuple(range(4092, 4100))


def chunk_case(X):
    """(3, 7, X), one pattern per row of the 21.  Sixteen rows (0 .. 12 and 15 .. 17) hold single zeros around both chunk edges: of
    x = 2044 .. 2051 and 4092 .. 4099 every other one, the phase alternating from row to row and again every four rows, so that
    each of the four row alignments (which repeat every four rows at odd X) meets each voxel next to an edge both as a zero and as
    a neighbour of one.  Row 13: the run 2040 .. 2060.  Row 14 (the first row of the last plane): all zeros — three dilations mask rows
    0 .. 3 of every plane from it and leave rows 4 .. 6.  Rows 18 and 19: the last four and the last five voxels (the ``x + 3 < X`` tail).
    Row 20: 2 % random zeros.
    The run WITHOUT dilation is the discriminating one for single bits: every planted zero is then one voxel to fill beside one to
    leave.  With three dilations the zero row masks rows 0 .. 3 of every plane whole (full words and 16-byte stores across the chunk
    edges, the heads of misaligned rows), and the patterns merge on the rows 4 .. 6 that stay partly valid."""
    vol = counts((3, 7, X))
    rows = vol.reshape(21, X)
    for i, r in enumerate(CHUNK_ISO_ROWS):
        for x in CHUNK_ISO_X:
            if x < X and (x + i + i // 4) % 2 == 0:
                rows[r, x] = 0
    rows[13, 2040:2061] = 0
    rows[14, :] = 0
    rows[18, X - 4:] = 0
    rows[19, X - 5:] = 0
    rows[20, np.random.default_rng(X).random(X) < 0.02] = 0
    return vol


def row_alignments(shape):
    """{(row * X) % 4} over the rows: which of apply_fill_kernel's a0 = (4 - that) % 4 the volume reaches."""
    Z, Y, X = shape
    return {(r * X) % 4 for r in range(Z * Y)}


def units_per_wavefront(shape, cus):
    """apply_fill_kernel's ``per``: the grid is 8 workgroups of four wavefronts per CU, a wavefront walks
    ceil(rows * nchunk / (32 CUs)) consecutive units."""
    Z, Y, X = shape
    return -(-(Z * Y * (-(-X // 2048))) // (32 * cus))


def mask_words(shape):
    Z, Y, X = shape
    return Z * Y * 2 * (-(-X // 64))


# The walks.  NARROW: 8 256 rows of one unit each — more than the 8 192 wavefronts of a 256-CU device, so a wavefront walks two
# units and requests the second one's mask word inside the loop.  X = 71 is odd: all four alignments.  WIDE (X = 2101: two chunks,
# all four alignments, 66 mask words per row): 1 056 000 mask words against the 16 x 256 x 256 = 1 048 576 threads of
# dilate_x_kernel's grid (a thread owns ONE word there), 528 000 word pairs against the 524 288 threads of shell_kernel's grid and
# against mask0_kernel's 8 192 wavefronts, and 32 000 units, four per wavefront.  It does NOT make dilate_outer_kernel stride: a
# thread owns a PAIR of words there, on the same grid, so that loop strides only above 2 x 1 048 576 words.  ROWS does: (1040, 1024, 2)
# is 1 064 960 rows of two words — 1 064 960 pairs for the y and z passes of dilate_outer_kernel, whose second pass writes the rows
# from 1 048 576 on (the last 16 planes), and 2 129 920 words for dilate_cross_kernel (a thread owns one word), whose second pass
# writes the rows from 524 288 on; 130 units per wavefront in apply_fill_kernel.  Mask words per voxel are highest at tiny X, so
# this costs 2.1 M voxels.
WALK_NARROW = (64, 129, 71)
WALK_WIDE = (40, 400, 2101)
WALK_ROWS = (1040, 1024, 2)
CUS = 256


def dilation_threads(cus):
    """Threads of the dilation kernels' grid when it is capped: 16 workgroups of 256 per CU."""
    return 16 * cus * 256


def second_pass_row(shape, cus, words_per_thread):
    """The first row whose mask words only the SECOND pass of a dilation kernel's grid-stride loop writes (``words_per_thread``: 1 for
    dilate_x_kernel and dilate_cross_kernel, 2 for dilate_outer_kernel), or None when the loop makes one pass."""
    W32 = 2 * (-(-shape[2] // 64))
    first_word = dilation_threads(cus) * words_per_thread
    return -(-first_word // W32) if first_word < mask_words(shape) else None


def walk_narrow_case():
    """Counts with a wedge of zeros at low x that grows with z (an overhang) and 0.1 % random zeros."""
    vol = counts(WALK_NARROW)
    for z in range(WALK_NARROW[0]):
        vol[z, :, : z // 4] = 0
    vol[np.random.default_rng(7).random(vol.shape) < 1e-3] = 0
    return vol


def assert_second_pass_reached(vol, mask, cus, words_per_thread, name):
    """Zeros sit in rows whose mask words only the second pass of the dilation's grid-stride loop writes, and the reference's mask
    grows around them there: a second pass that wrote the wrong words, or none, could not give that mask."""
    row = second_pass_row(tuple(vol.shape), cus, words_per_thread)
    assert row is not None, (name, cus)
    X = vol.shape[2]
    zero = (_t(vol, mask.device) == 0).reshape(-1, X)[row:]
    grown = mask.reshape(-1, X)[row:]
    assert int(zero.sum()) > 0 and int(grown.sum()) > int(zero.sum()), (name, cus, row)


@functools.lru_cache(maxsize=1)
def _walk_rows_volume():
    vol = counts(WALK_ROWS)
    vol[np.random.default_rng(11).random(vol.shape) < 1e-3] = 0
    for z, y, x in ((0, 0, 0), (511, 1023, 1), (512, 0, 0), (700, 512, 1), (1023, 1023, 1), (1024, 0, 0), (1030, 500, 0), (1036, 1023, 1),
                    (1039, 0, 1), (1039, 1023, 0)):
        vol[z, y, x] = 0
    vol.setflags(write=False)
    return vol


def walk_rows_case():
    """(1040, 1024, 2) counts (read-only, shared) with 1e-3 random zeros and single zeros on the first and last rows of the planes either
    side of where the second passes begin (planes 512 and 1024 on 256 CUs) and of the last plane."""
    return _walk_rows_volume()


def walk_wide_case(device):
    """The wide walk's input, made on the device (33.6 M voxels): whole counts 110 +- 3, brighter blocks, a wedge of zeros at low x
    that grows with z, runs of zeros across the chunk edge at x = 2048 and 1e-4 random zeros."""
    Z, Y, X = WALK_WIDE
    gen = torch.Generator(device=device)
    gen.manual_seed(2101)
    vol = torch.round(torch.randn(WALK_WIDE, generator=gen, device=device) * 3.0 + 110.0).clamp_(1.0, 65535.0)
    vol[5:9, 100:140, 900:1300] += 30000.0
    vol[30:33, 300:310, 2040:2060] += 5000.0
    for z in range(Z):
        vol[z, :, : 3 * z] = 0
    vol[:, ::37, 2030:2070] = 0
    vol[torch.rand(WALK_WIDE, generator=gen, device=device) < 1e-4] = 0
    return vol


# Values
def value_case(what):
    """(4, 5, 40) counts with one planted zero at (1, 2, 7) and, away from its dilated ball, the value under test."""
    vol = counts((4, 5, 40))
    vol[1, 2, 7] = 0
    if what == "negative zero":
        vol[3, 4, 30] = f32(-0.0)
    elif what == "subnormals":
        vol[3, 4, 30], vol[3, 4, 20], vol[0, 0, 39] = f32(1e-45), f32(-1e-45), f32(1e-38)
    elif what == "signed":
        vol = (vol - f32(vol.mean(dtype=np.float64))).astype(f32)
        vol[1, 2, 7] = 0
        vol[3, 4, 30] = 0
    elif what == "no zeros":
        vol[1, 2, 7] = 321
    elif what == "all zeros":
        vol[:] = 0
    elif what == "nan outside":
        vol[3, 4, 30] = f32(np.nan)
    elif what == "nan in the shell":
        vol[1, 2, 8] = f32(np.nan)
    elif what == "inf in the shell":
        vol[1, 3, 6] = f32(np.inf)
    elif what != "plain":
        raise ValueError(what)
    return vol


VALUE_CASES = ("plain", "negative zero", "subnormals", "signed", "no zeros", "all zeros", "nan outside", "nan in the shell",
               "inf in the shell")
NONFINITE_SHELL = ("nan in the shell", "inf in the shell")


def small_cases():
    """Every input of the GPU tests but the two large walks (WALK_WIDE, WALK_ROWS) and the deskews: (name, volume builder, iterations, connectivity, fills).
    The CPU tests assert the input conditions and hold the restatement to the checker at each; the GPU tests run the same list."""
    out = []
    for X in EDGE_X:
        for it in EDGE_ITERATIONS:
            for side in EDGE_SIDES:
                for conn in (26, 6):
                    fills = ("mean", -7.25) if (it == 3 and side == "hi") else ("mean",)
                    out.append((f"edge X={X} {side} it={it} conn={conn}", functools.partial(edge_case, X, it, side), it, conn, fills))
    for conn in (26, 6):
        out.append((f"31 iterations conn={conn}", thirty_one_case, 31, conn, ("mean",)))
    for X in CHUNK_X:
        for it in (0, 3):
            out.append((f"chunk X={X} it={it} conn=26", functools.partial(chunk_case, X), it, 26, ("mean", 321.5)))
        out.append((f"chunk X={X} it=3 conn=6", functools.partial(chunk_case, X), 3, 6, ("mean",)))
    out.append(("narrow walk", walk_narrow_case, 3, 26, ("mean",)))
    return out


def checked_values(what):
    """Whether a value case obeys the input conditions (a finite non-zero mean with a voxel outside the mask)."""
    return what in ("plain", "negative zero", "subnormals", "signed")


# Through the deskew: Xp > 2048, where the FILLM = 1 deskew kernel writes 66-word mask rows and apply_fill_kernel takes a second
# chunk; Xp = 2073 .. 2076, one of each residue mod 4.  (shape, angle, ratio, N, Xp)
DESKEW_WIDE = [((8, Y, 8), 36.17, 0.371, 4, Xp) for Y, Xp in ((2541, 2073), (2542, 2074), (2543, 2075), (2544, 2076))]
# A mask-prologue deskew on the smallest tiles (configuration 4: 32 x 64) that hands finalize_kernel 4 x 7 x 400 = 11 200 block sums,
# more than 8 x 1024: each of its 1024 threads runs the eight-wide body once (8 192 sums), then the single-step loop twice, and the
# threads below 960 a third time (3 008 sums).
DESKEW_PARTIALS = ((24, 400, 128), 36.17, 0.371, 1, 4)
FIN_NT = 1024


# ----------------------------------------------------------------------------- the kernels' mask pipeline, restated
DEFECTS = ("no next word", "no head", "x carry", "y wrap", "mean undilated", "fill 2 ulp", "touch outside", "negative zero",
           "cross for 26")


def _pack(zero):
    """(Z, Y, X) bool -> (Z, Y, W32) uint32, bit x % 32 of word x // 32; the padding bits clear (mask0_kernel's ballot)."""
    Z, Y, X = zero.shape
    W32 = 2 * (-(-X // 64))
    bits = np.zeros((Z, Y, W32 * 32), np.uint8)
    bits[:, :, :X] = zero
    return np.packbits(bits, axis=2, bitorder="little").view("<u4").astype(np.uint32)


def _unpack(words, X):
    return np.unpackbits(words.astype("<u4").view(np.uint8), axis=2, bitorder="little")[:, :, :X].astype(bool)


def _dilate_x(words, r, carry=False):
    """dilate_x_kernel: per word o = w | (w << s) | (l >> (32 - s)) | (w >> s) | (h << (32 - s)), s = 1 .. r, l and h the neighbours
    inside the row (0 beyond it).  ``carry``: l and h the neighbours in MEMORY — the planted defect."""
    shape = words.shape
    w = words.reshape(-1, shape[2]) if not carry else words.reshape(1, -1)
    l, h = np.zeros_like(w), np.zeros_like(w)
    l[:, 1:], h[:, :-1] = w[:, :-1], w[:, 1:]
    o = w.copy()
    for s in range(1, r + 1):
        o |= (w << np.uint32(s)) | (l >> np.uint32(32 - s)) | (w >> np.uint32(s)) | (h << np.uint32(32 - s))
    return o.reshape(shape)


def _dilate_outer(words, axis, r, wrap=False):
    """dilate_outer_kernel along y (axis 1) or z (axis 0): OR of the rows / planes within r, stopped at the ends of the axis.
    ``wrap`` (axis 1): stopped only at the ends of the volume — the last rows of a plane reach the first of the next: a defect."""
    if wrap:
        Z, Y, W = words.shape
        return _dilate_outer(words.reshape(1, Z * Y, W), 1, r).reshape(Z, Y, W)
    o = words.copy()
    n = words.shape[axis]
    for d in range(1, min(r, n - 1) + 1):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[axis], b[axis] = slice(d, None), slice(None, n - d)
        o[tuple(a)] |= words[tuple(b)]
        o[tuple(b)] |= words[tuple(a)]
    return o


def _dilate_cross(words, r):
    """dilate_cross_kernel: per (dz, dy) with |dz| + |dy| <= r the row (z + dz, y + dy) dilated along x by the remaining radius."""
    Z, Y, W = words.shape
    byx = [_dilate_x(words, rx) for rx in range(r + 1)]
    o = np.zeros_like(words)
    for dz in range(-r, r + 1):
        for dy in range(-(r - abs(dz)), r - abs(dz) + 1):
            src = byx[r - abs(dz) - abs(dy)]
            z0, z1, y0, y1 = max(0, -dz), min(Z, Z - dz), max(0, -dy), min(Y, Y - dy)
            if z0 < z1 and y0 < y1:
                o[z0:z1, y0:y1] |= src[z0 + dz:z1 + dz, y0 + dy:y1 + dy]
    return o


def _apply(out, md, fill, defect):
    """apply_fill_kernel: per unit (row, chunk of 2048 voxels) the 64 mask words ``cur`` and the next chunk's first word ``curn``;
    the row's unaligned head (chunk 0, lanes below a0); eight steps of 64 lanes, lane l of step s owning the four voxels from
    xr = a0 + 256 s + 4 l, their bits fetched from word xr >> 5 and, where the group straddles it (sh > 28), the next one — which for the
    last group of a chunk is ``curn``."""
    Z, Y, X = out.shape
    W32 = md.shape[2]
    rows, words = out.reshape(Z * Y, X), md.reshape(Z * Y, W32)
    nchunk = -(-X // 2048)
    lane = np.arange(64)
    for u in range(Z * Y * nchunk):
        row, c = divmod(u, nchunk)
        cur = np.zeros(64, np.uint32)
        k = min(64, W32 - c * 64)
        cur[:k] = words[row, c * 64:c * 64 + k]
        curn = words[row, c * 64 + 64] if c * 64 + 64 < W32 else np.uint32(0)
        if defect == "no next word":
            curn = np.uint32(0)
        if not cur.any() and curn == 0:
            continue
        a0 = (4 - ((row * X) & 3)) & 3
        if c == 0 and defect != "no head":
            for ln in range(min(a0, X)):
                if (cur[0] >> np.uint32(ln)) & 1:
                    rows[row, ln] = fill
        xr = a0 + 256 * np.arange(8)[:, None] + 4 * lane[None, :]
        idx, sh = xr >> 5, (xr & 31).astype(np.uint32)
        bits = np.where(idx < 64, cur[idx & 63], curn) >> sh
        if a0 != 0:
            hi = np.where(idx + 1 < 64, cur[(idx + 1) & 63], curn)
            bits = np.where(sh > 28, bits | (hi << ((np.uint32(32) - sh) & np.uint32(31))), bits)
        bits &= np.uint32(15)
        x = c * 2048 + xr
        for e in range(4):
            sel = (((bits >> np.uint32(e)) & 1) == 1) & (x + e < X)
            rows[row, (x + e)[sel]] = fill


def fill_restated(vol, fill_value=None, iterations=3, connectivity=26, defect=None):
    """The mask pipeline of csrc/fill.hip in numpy, on its own data layout; float32 in, float32 out.  ``defect``, one of ``DEFECTS``:
      "no next word"   the last group of a chunk does not read the next chunk's first word (voxels 2048 .. 2050 of misaligned rows unfilled);
      "no head"        the unaligned head of a row skipped;
      "x carry"        x-dilation carried across the row end into the neighbouring rows' words;
      "y wrap"         y-dilation not stopped at the first and last row of a plane;
      "mean undilated" the mean taken over everything outside the UNDILATED zero mask;
      "fill 2 ulp"     the fill value two float32 ulps up;
      "touch outside"  one voxel outside the mask moved by one ulp;
      "negative zero"  -0.0 not masked (the zero test on the bit pattern);
      "cross for 26"   the cross element used for connectivity 26."""
    assert defect is None or defect in DEFECTS, defect
    vol = np.ascontiguousarray(vol, dtype=f32)
    Z, Y, X = vol.shape
    zero = (vol.view(np.int32) == 0) if defect == "negative zero" else (vol == 0)
    m0 = _pack(zero)
    r = int(iterations)
    if r == 0:
        md = m0
    elif connectivity == 6 or defect == "cross for 26":
        md = _dilate_cross(m0, r)
    else:
        md = _dilate_outer(_dilate_outer(_dilate_x(m0, r, carry=defect == "x carry"), 1, r, wrap=defect == "y wrap"), 0, r)
    dil = _unpack(md, X)
    if fill_value is None:
        inmask = zero if defect == "mean undilated" else dil
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            s_all = vol.sum(dtype=np.float64)
            s_shell = vol[inmask & ~zero].sum(dtype=np.float64)
            fill = f32((s_all - s_shell) / np.float64(vol.size - int(inmask.sum())))
    else:
        fill = f32(fill_value)
    if defect == "fill 2 ulp":
        fill = np.nextafter(np.nextafter(fill, f32(np.inf)), f32(np.inf))
    out = vol.copy()
    _apply(out, md, fill, defect)
    if defect == "touch outside":
        at = np.argwhere(~dil)[-1]
        out[tuple(at)] = np.nextafter(out[tuple(at)], f32(np.inf))
    return out
