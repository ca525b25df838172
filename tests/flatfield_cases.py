"""Inputs of the flat-field and binning wrap tests (tests/test_flatfield_reference.py on the CPU, tests/test_gpu_flatfield.py on
the GPU): the launch rules of csrc/flatfield.hip and csrc/binning.hip restated (``thresholds``), the probe / skip state machine
of ``median_hist_kernel`` (``hist_schedule``) and one tile's histogram selection (``hist_select``) in numpy, and seeded builders
of every case.  Nothing here imports GPU code.

``median_hist_kernel`` runs persistent workgroups: ``grid = min(tiles, 2 CUs)``, tile t goes to workgroup t % grid, and ``streak``
/ ``skip`` travel from one tile of a workgroup to its next.  The scripted cases give every workgroup the same sequence of wide
and narrow tiles (``SCRIPT``), sized from the compute-unit count they are built for, so that all 14 states of the machine are
visited: probed x {wide, narrow} x streak 0..3 and skipped x {wide, narrow} x streak 1..3.

Bounds.  Every median is held to ``np.median`` by equality.  The apply pass is held bit for bit to its two-operation expression
evaluated in numpy from the device's own pattern and mean.  The mean is held to ``math.fsum`` within ``sum_depth`` roundings.
End to end against ``oracle_np.flat_field_zyx``: integers keep the 2e-7 of max of the existing tests (``E2E_INT_TOL``); float32
gets ``REF_MEAN_F32_ERR + 2^-23`` of max (``E2E_F32_TOL``): the reference's own float32 pairwise mean against math.fsum,
measured on the CPU by tests/test_flatfield_reference.py at the very pattern of the test (2.7e-8 of the mean; stated here rounded up), plus
one float32 rounding of the mean and one of the result on either side.
"""

import functools
import math
from collections import namedtuple

import numpy as np

CUS = 256                      # compute units the fixed wrap shapes are sized for
FH_COLS = 128                  # pixels of one tile of median_hist_kernel
LDS_BUDGET = 144 * 1024        # of the CU's 160 KiB: the staging of median_z_kernel
SUM_GRID, BIN_GRID_PER_CU, NT_FLAT = 1024, 16, 256

E2E_INT_TOL = 2e-7
REF_MEAN_F32_ERR = 3e-8        # np.mean of the float32 (520, 521) pattern against math.fsum, of the mean: 2.7e-8 on the CPU
E2E_F32_TOL = REF_MEAN_F32_ERR + 2.0 ** -23


def _frozen(a):
    a.setflags(write=False)
    return a


# =============================================================================================== launch rules
def staging_cols(Z, keysize):
    """Columns of one tile of ``median_z_kernel`` (run_median): 64 halved while Z x cols keys exceed the budget, down to 4;
    None when four columns do not fit (the launch is refused)."""
    cols = 64
    while cols > 4 and Z * cols * keysize > LDS_BUDGET:
        cols >>= 1
    return cols if Z * cols * keysize <= LDS_BUDGET else None


def bitsearch_launch(cus, Z, keysize):
    """(cols, per_cu, grid cap) of the bit-search kernel: NT = 1024 threads for 32-bit keys, 512 for 16-bit ones."""
    nt = 1024 if keysize == 4 else 512
    cols = staging_cols(Z, keysize)
    lds = ((Z * cols * keysize + 15) & ~15) + 2 * nt * 4
    per_cu = max(1, min(8, 163840 // (lds + 256)))
    return cols, per_cu, cus * per_cu


def thresholds(cus):
    """Work above which a workgroup of each kernel takes a second trip through its loop: tiles of the histogram median
    (2 cus workgroups), tiles of the bit search (cus x per_cu, a function of Z and the key size), pixels of the pattern sum
    (1024 workgroups x 256), outputs of a binning channel (16 cus workgroups x 256)."""
    return {"hist_tiles": 2 * cus,
            "bitsearch_tiles": lambda Z, keysize: bitsearch_launch(cus, Z, keysize)[2],
            "sum_pixels": SUM_GRID * NT_FLAT,
            "bin_outputs": BIN_GRID_PER_CU * cus * NT_FLAT}


def sum_depth(pixels):
    """Roundings between the pattern and the mean that ``bh_flat_field`` reports, worst thread: the serial terms of a thread
    of ff_sum_partial_kernel (ceil(pixels / (grid x 256)), grid = min(ceil(pixels / 256), 1024)), the 8 levels of its LDS
    tree, the serial terms of a thread of ff_sum_final_kernel over the partials (ceil(grid / 256)), its 8 levels, the
    multiplication by 1 / pixels and the rounding of that reciprocal; then the two roundings of the reference it is held to
    (math.fsum rounds once, the division once) and one for the second-order terms (d^2 2^-106 < 2^-53)."""
    grid = min(-(-pixels // NT_FLAT), SUM_GRID)
    return -(-pixels // (grid * NT_FLAT)) + 8 + -(-grid // NT_FLAT) + 8 + 2 + 2 + 1


# =============================================================================================== keys
def to_keys(a):
    """The order-preserving keys of FfKey<T> for uint8 / uint16 / int16, as uint32."""
    a = np.asarray(a)
    if a.dtype == np.int16:
        return (a.view(np.uint16) ^ np.uint16(0x8000)).astype(np.uint32)
    assert a.dtype in (np.uint8, np.uint16), a.dtype
    return a.astype(np.uint32)


def from_keys(k, dtype):
    """FfKey<T>::from: the value of a key as float64."""
    k = np.asarray(k, dtype=np.uint32)
    if np.dtype(dtype) == np.int16:
        return (k.astype(np.uint16) ^ np.uint16(0x8000)).view(np.int16).astype(np.float64)
    return k.astype(np.float64)


def tile_keys(vol):
    """The keys a workgroup of median_hist_kernel loads, tile by tile: (Z, tiles, 128) with the kernel's clamped columns
    (lane l loads ca = min(x0 + 2 l, X - 2 for even X else X - 1) and cb = min(ca + 1, X - 1)); tile = y tiles_x + x0 / 128."""
    Z, Y, X = vol.shape
    tiles_x = -(-X // FH_COLS)
    x0 = np.arange(tiles_x)[:, None] * FH_COLS
    ca = np.minimum(x0 + 2 * np.arange(64)[None, :], X - 2 if X % 2 == 0 else X - 1)
    cb = np.minimum(ca + 1, X - 1)
    cols = np.stack([ca, cb], axis=-1).reshape(tiles_x, FH_COLS)
    return to_keys(vol)[:, :, cols].reshape(Z, Y * tiles_x, FH_COLS)


def tiles_wide(keys):
    """Per tile: does some pixel's key range over z reach 256 (the probe then finds a shift and the tile refines)."""
    return ((keys.max(axis=0) - keys.min(axis=0)) >= 256).any(axis=-1)


# =============================================================================================== the state machine
STATES = ([("probed", w, s) for w in ("wide", "narrow") for s in range(4)]
          + [("skipped", w, s) for w in ("wide", "narrow") for s in (1, 2, 3)])


def hist_schedule(wide, grid, reset_streak=True):
    """The probe / skip machine of median_hist_kernel for ``wide`` (bool per tile) on ``grid`` workgroups: (probed, streak the
    tile arrives with), one entry per tile.  A probed wide tile raises the streak (to 3 at most) and sets skip = 2^streak - 1;
    a probed narrow tile resets the streak (and so skip); a skipped tile lowers skip and leaves the streak.  ``reset_streak =
    False`` plants the fault of a narrow probe that keeps the streak."""
    wide = np.asarray(wide, dtype=bool)
    n = wide.size
    grid = min(grid, n)
    probed, arrive = np.zeros(n, bool), np.zeros(n, np.int64)
    streak, skip = np.zeros(grid, np.int64), np.zeros(grid, np.int64)
    for first in range(0, n, grid):
        m = min(grid, n - first)
        t = slice(first, first + m)
        p = skip[:m] == 0
        probed[t], arrive[t] = p, streak[:m]
        skip[:m] = np.where(p, skip[:m], skip[:m] - 1)
        up = np.where(wide[t], np.minimum(streak[:m] + 1, 3), 0 if reset_streak else streak[:m])
        streak[:m] = np.where(p, up, streak[:m])
        skip[:m] = np.where(p, (1 << streak[:m]) - 1, skip[:m])
    return probed, arrive


def state_counts(wide, probed, arrive):
    """Tiles per state of ``STATES``."""
    return {(pk, wk, s): int(((probed == (pk == "probed")) & (wide == (wk == "wide")) & (arrive == s)).sum())
            for pk, wk, s in STATES}


# =============================================================================================== one tile's selection
NO_SHIFT, SHIFT_ONE_BIN, SHIFT_STRADDLE = 0, 1, 2
BRANCHES = ("no shift", "shift, one bin", "shift, two bins")
Selected = namedtuple("Selected", "v1 v2 branch refine hist minlo base shift")


def _histogram(idx, rows):
    """Counts per (row, bin) of ``idx`` (samples x rows, bin or -1 for a sample that is not counted)."""
    flat = (np.arange(rows)[None, :] * 256 + idx)[idx >= 0]
    return np.bincount(flat, minlength=rows * 256).reshape(rows, 256)


def _first_above(cum, rank):
    """Per row the first bin whose running count exceeds ``rank``; 0 when none does (the kernel's initial value)."""
    hit = cum > rank[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), 0)


def hist_select(keys_tile, probed, bits=16, carry=None, keep_hist=False, keep_minlo=False, keep_split=False):
    """One tile's selection in median_hist_kernel, restated: ``keys_tile`` is (Z, 128) — or (Z, tiles, 128) with ``probed`` one
    flag per tile, the tiles being independent.  Per pixel the base and shift (the smallest key and the fewest low bits to
    drop so that the range fits 256 bins when probed; (0, 8) when not; (0, 0) for 8-bit keys), the histogram of (key - base)
    >> shift and the bins b1, b2 of the ranks k = (Z - 1) // 2 and k2 = Z // 2 with r1 = k minus the count below b1; when some
    pixel of the tile has a shift, the histogram of the dropped low bits of the samples in b1 (ranks r1 and r1 + 1 -> lo1, lo2)
    and ``minlo``, the smallest low part in b2 where that is another bin.  v1 = base + (b1 << s) + lo1; v2 = base + (b1 << s) +
    lo2 when b2 == b1, else base + (b2 << s) + minlo.  Returns the keys v1, v2, the branch per pixel (``BRANCHES``), the tile's
    ``refine`` flag and what the workgroup leaves behind (hist, minlo, base, shift).

    ``carry`` is the ``Selected`` of the same workgroup's previous tile, used only by the planted faults: ``keep_hist`` — hist
    is not zeroed at the top of the tile (what the previous tile left is counted again); ``keep_minlo`` — minlo is not reset;
    ``keep_split`` — a tile that is not probed keeps the previous tile's base and shift instead of (0, 8) (bins outside 0..255
    are not counted)."""
    keys = np.asarray(keys_tile, dtype=np.uint32)
    single = keys.ndim == 2
    if single:
        keys = keys[:, None, :]
    Z, T, _ = keys.shape
    probed = np.broadcast_to(np.asarray(probed, dtype=bool), (T,)) & (bits > 8)
    k = np.full(T * FH_COLS, (Z - 1) >> 1)
    k2 = np.full(T * FH_COLS, Z >> 1)
    mn, mx = keys.min(axis=0), keys.max(axis=0)
    bit_length = np.frexp(((mx - mn) | 1).astype(np.float64))[1]
    s_probe = np.maximum(0, bit_length - 8).astype(np.uint32)                       # 24 - clz(range | 1)
    base = np.where(probed[:, None], mn, np.uint32(0))
    shift = np.where(probed[:, None], s_probe, np.uint32(8 if bits > 8 else 0))
    if keep_split and carry is not None:
        base = np.where(probed[:, None], base, carry.base)
        shift = np.where(probed[:, None], shift, carry.shift)
    refine = (shift != 0).any(axis=1)
    d = keys - base[None]                                   # uint32: wraps like the kernel's unsigned difference
    b = (d >> shift[None]).astype(np.int64).reshape(Z, -1)
    hist = _histogram(np.where(b < 256, b, -1), T * FH_COLS)
    if keep_hist and carry is not None:
        hist = hist + carry.hist.reshape(-1, 256)
    cum = np.cumsum(hist, axis=1)
    b1, b2 = _first_above(cum, k), _first_above(cum, k2)
    below = np.where(b1 > 0, np.take_along_axis(cum, np.maximum(b1 - 1, 0)[:, None], axis=1)[:, 0], 0)
    r1 = np.where((cum > k[:, None]).any(axis=1), k - below, 0)
    low = (d & ((np.uint32(1) << shift[None]) - np.uint32(1))).astype(np.int64).reshape(Z, -1)
    in1, in2 = b == b1[None], (b == b2[None]) & (b != b1[None])
    hist2 = _histogram(np.where(in1, low, -1), T * FH_COLS)
    cum2 = np.cumsum(hist2, axis=1)
    tile_refine = np.repeat(refine, FH_COLS)
    lo1 = np.where(tile_refine, _first_above(cum2, r1), 0)
    lo2 = np.where(tile_refine, _first_above(cum2, r1 + 1), 0)
    start = carry.minlo.reshape(-1) if keep_minlo and carry is not None else np.full(T * FH_COLS, 0xFFFFFFFF, np.int64)
    minlo = np.where(tile_refine, np.minimum(start, np.where(in2, low, 0xFFFFFFFF).min(axis=0)), start)
    s = shift.reshape(-1).astype(np.int64)
    bs = base.reshape(-1).astype(np.int64)
    v1 = bs + (b1 << s) + lo1
    v2 = np.where(b2 == b1, bs + (b1 << s) + lo2, bs + (b2 << s) + np.where(tile_refine, minlo, 0))
    branch = np.where(s == 0, NO_SHIFT, np.where(b2 == b1, SHIFT_ONE_BIN, SHIFT_STRADDLE))
    left = np.where(tile_refine[:, None], hist2, hist).reshape(T, FH_COLS, 256)
    u32 = lambda a: (a & 0xFFFFFFFF).astype(np.uint32).reshape(T, FH_COLS)   # noqa: E731
    out = Selected(u32(v1), u32(v2), branch.reshape(T, FH_COLS), refine, left, minlo.reshape(T, FH_COLS), base, shift)
    return Selected(*(f[0] for f in out)) if single else out


HistRun = namedtuple("HistRun", "median wide probed arrive branch refine")


def hist_median(vol, grid, fault=None):
    """``median_hist_kernel`` over a (Z, Y, X) volume of uint8 / uint16 / int16 on ``grid`` persistent workgroups: the schedule
    (``hist_schedule``) and every tile's selection (``hist_select``), visit by visit.  Returns the (Y, X) float64 pattern and,
    per tile, wide / probed / streak on arrival / refine, and the branch per tile pixel.  ``fault``: "hist", "minlo" or "split"
    (``hist_select``'s keep_*), "streak" (``hist_schedule``'s reset_streak = False)."""
    Z, Y, X = vol.shape
    bits = 8 if vol.dtype == np.uint8 else 16
    keys = tile_keys(vol)
    T = keys.shape[1]
    wide = tiles_wide(keys) if bits > 8 else np.zeros(T, bool)
    probed, arrive = hist_schedule(wide, grid, reset_streak=fault != "streak")
    if bits == 8:
        probed = np.zeros(T, bool)                                  # 8-bit keys never probe; skip stays 0
    v1, v2 = np.zeros((T, FH_COLS), np.uint32), np.zeros((T, FH_COLS), np.uint32)
    branch, refine = np.zeros((T, FH_COLS), np.int8), np.zeros(T, bool)
    carries = fault in ("hist", "minlo", "split")
    step = min(grid, T) if carries else 64                          # tiles are independent unless a fault carries state over
    carry = None
    for first in range(0, T, step):
        t = slice(first, min(first + step, T))
        if carry is not None:                                       # a last, partial visit: the first workgroups only
            carry = Selected(*(f[:t.stop - t.start] for f in carry))
        sel = hist_select(keys[:, t], probed[t], bits, carry, keep_hist=fault == "hist", keep_minlo=fault == "minlo",
                          keep_split=fault == "split")
        v1[t], v2[t], branch[t], refine[t] = sel.v1, sel.v2, sel.branch, sel.refine
        carry = sel if carries else None
    med = from_keys(v1, vol.dtype) if Z & 1 else (from_keys(v1, vol.dtype) + from_keys(v2, vol.dtype)) * 0.5
    tiles_x = -(-X // FH_COLS)
    med = med.reshape(Y, tiles_x * FH_COLS)[:, :X]
    return HistRun(med, wide, probed, arrive, branch, refine)


# =============================================================================================== the scripted wrap cases
SCRIPT = "WNNNWWWNWWNWNWNWWWNWNWNWWWWNWNWNNNN"     # one workgroup's visits: wide or narrow
SCRIPT_DTYPES = (np.uint16, np.int16)
SCRIPT_Z = (10, 9)
ROW_Z = 9
LIBRARY = 48                                       # distinct tiles of either kind


def _range_for_shift(rng, s, n):
    """``n`` key ranges that need ``s`` dropped bits: [2^(7+s), 2^(8+s) - 1], both ends among them."""
    lo, hi = 1 << (7 + s), (1 << (8 + s)) - 1
    r = rng.integers(lo, hi + 1, n)
    r[::3], r[1::3] = lo, hi
    return r


@functools.lru_cache(maxsize=None)
def _tile_library(Z, seed=20261019):
    """(narrow, wide): two (Z, LIBRARY, 128) sets of tiles in key space.

    Narrow tiles: per pixel 0 to 5 levels of noise over an offset that differs from pixel to pixel (anywhere in the key
    space: a skipped narrow tile sits far from base 0); every eighth pixel sits 3 below a multiple of 256, so that under the
    fixed split its samples fall in two bins, and pixel 5 spans exactly 255 levels (the widest range without a shift).  A third
    of the tiles lie across key 0x8000 (int16: the sign change), two at the ends of the key space.
    Wide tiles, by ``j % 6``: 0 — one wide pixel (shift 1) at pixel 0, lane 0's first, the rest narrow; 1 — one (shift 3) at
    pixel 127, lane 63's second; 2 — one (shift 8) anywhere; 3 — every pixel clustered but for one far sample (shifts 1, 3, 8
    mixed: both ranks share a bin); 4 — every pixel bimodal, half the samples at either end of the range (even Z: the ranks
    straddle two bins); 5 — per pixel narrow, clustered, bimodal or three tied levels.  The z order is shuffled per pixel."""
    rng = np.random.default_rng(seed + Z)
    L, C = LIBRARY, FH_COLS

    def narrow():
        off = rng.integers(300, 65000, (L, C))
        off[:, ::8] = (off[:, ::8] // 256) * 256 - 3
        off[::3] = 0x8000 - 3 + rng.integers(0, 4, (L // 3 + (L % 3 > 0), C))
        off[1], off[2] = 0, 65535 - 5
        v = off[None] + rng.integers(0, 6, (Z, L, C))
        v[:, :, 5] = off[None, :, 5] // 2 + np.where(np.arange(Z)[:, None] % 2 == 0, 0, 255)
        return v

    def spread(kind, r):
        """Samples of pixels with range ``r`` (L, C): kind 1 clustered, 2 bimodal, 3 three tied levels; min and max present."""
        off = (rng.random((L, C)) * (65535 - r)).astype(np.int64)
        noise = rng.integers(0, 4, (Z, L, C))
        z = np.arange(Z)[:, None, None]
        clustered = np.where(z == Z - 1, r[None], np.where(z == 0, 0, noise))
        bimodal = np.where(z == 0, 0, np.where(z == Z - 1, r[None], np.where(z < (Z + 1) // 2, noise, r[None] - noise)))
        tied = np.where(z == 0, 0, np.where(z == Z - 1, r[None], (rng.integers(0, 3, (Z, L, C)) * r[None]) // 2))
        v = off[None] + np.where(kind[None] == 1, clustered, np.where(kind[None] == 2, bimodal, tied))
        return rng.permuted(v, axis=0)

    shifts = np.array([1, 3, 8])[rng.integers(0, 3, (L, C))]
    r = np.zeros((L, C), np.int64)
    for s in (1, 3, 8):
        r[shifts == s] = _range_for_shift(rng, s, int((shifts == s).sum()))
    variant = np.arange(L) % 6
    kind = np.zeros((L, C), np.int64)                       # 0: the narrow pixel
    one = np.zeros(L, np.int64)
    one[variant == 1] = C - 1
    one[variant == 2] = rng.integers(1, C - 1, int((variant == 2).sum()))
    lone = variant <= 2
    kind[lone, one[lone]] = 1 + np.arange(int(lone.sum())) % 3
    for v, s in ((0, 1), (1, 3), (2, 8)):
        rows = np.nonzero(variant == v)[0]
        r[rows, one[rows]] = _range_for_shift(rng, s, rows.size)
    kind[variant == 3] = 1
    kind[variant == 4] = 2
    kind[variant == 5] = rng.integers(0, 4, (int((variant == 5).sum()), C))
    kind[variant == 5, 0] = 3                               # never an all-narrow "wide" tile
    nar = narrow()
    wide = np.where(kind[None] == 0, narrow(), spread(kind, r))
    assert 0 <= nar.min() and nar.max() <= 65535 and 0 <= wide.min() and wide.max() <= 65535
    return _frozen(nar.astype(np.uint16)), _frozen(wide.astype(np.uint16))


def _from_key_space(keys, dtype):
    return keys if np.dtype(dtype) == np.uint16 else (keys ^ np.uint16(0x8000)).view(np.int16)


def script_tiles(cus):
    return len(SCRIPT) * 2 * cus


def script_wide(cus):
    """Tile t is wide iff SCRIPT[t // grid] == 'W', grid = 2 cus: every workgroup sees the script."""
    return np.repeat(np.array([c == "W" for c in SCRIPT]), 2 * cus)


@functools.lru_cache(maxsize=4)
def scripted_volume(dtype, Z, cus, row=False):
    """The scripted wrap volume for a card of ``cus`` compute units: len(SCRIPT) x 2 cus tiles, (Z, tiles / 8, 1024) — eight
    tiles per row — or, with ``row``, the (Z, 1, 128 tiles) layout that _median_tiled makes of any axis but 0, where a
    workgroup's consecutive tiles are neighbours along one row.  Tile t takes entry (t + 5 (t // grid)) % LIBRARY of the wide
    or the narrow library, so a workgroup meets a different tile on every visit."""
    nar, wide = _tile_library(Z)
    T, grid = script_tiles(cus), 2 * cus
    t = np.arange(T)
    j = (t + 5 * (t // grid)) % LIBRARY
    tiles = np.where(script_wide(cus)[None, :, None], wide[:, j], nar[:, j])
    vol = _from_key_space(tiles, dtype).reshape((Z, 1, T * FH_COLS) if row else (Z, T // 8, 8 * FH_COLS))
    return _frozen(np.ascontiguousarray(vol))


# =============================================================================================== edges of the hist kernel
HIST_EDGES = ["Z 65535", "X 2", "X 3", "uint8 Z 300", "X 130 odd Z", "X 129 even Z"]


@functools.lru_cache(maxsize=None)
def hist_edge(name):
    rng = np.random.default_rng(77)
    if name == "Z 65535":
        # pixel 0 constant: its 16-bit half of a hist word reaches 65535 and must not carry into pixel 1's half, which varies;
        # pixel 2: 32768 samples of one value and 32767 of another (the median is the majority's); pixel 3: the reverse
        v = rng.integers(900, 1100, (65535, 1, 6)).astype(np.uint16)
        v[:, 0, 0] = 1234
        v[:, 0, 2] = np.where(np.arange(65535) % 2 == 0, 700, 40000)
        v[:, 0, 3] = np.where(np.arange(65535) % 2 == 0, 40000, 700)
        return _frozen(v)
    if name in ("X 2", "X 3"):
        v = rng.integers(0, 5000, (40, 5, int(name[2:]))).astype(np.int16) - np.int16(2500)
        return _frozen(v)
    if name == "uint8 Z 300":
        return _frozen(rng.integers(0, 256, (300, 3, 200)).astype(np.uint8))
    if name == "X 130 odd Z":
        return _frozen(rng.integers(0, 65536, (37, 4, 130)).astype(np.uint16))
    if name == "X 129 even Z":
        return _frozen(rng.integers(0, 3000, (36, 4, 129)).astype(np.uint16))
    raise KeyError(name)


HIST_REFUSED = (65536, 1, 6)                       # Z past the 16-bit counters: falls to the bit search, which cannot stage it


# =============================================================================================== the bit search
BITSEARCH_DTYPES = (np.float32, np.uint16)
BITSEARCH_WRAP = [(9, 40, 64 * 52 + 5), (10, 40, 64 * 52 + 5)]     # 53 x 40 = 2120 tiles on 8 x 256 workgroups
BITSEARCH_HALVING_Z = {4: (576, 577, 1152, 1153, 2304, 2305, 4608, 4609, 9216),
                       2: (1152, 1153, 2304, 2305, 4608, 4609, 9216, 9217, 18432)}
BITSEARCH_REFUSED_Z = {4: 9217, 2: 18433}
BITSEARCH_X = 70                                   # 64 columns: a ragged second tile; 4 columns: 18 tiles
BITSEARCH_SMALL = [(1, 1, 1), (2, 1, 1), (1, 3, 70), (2, 3, 70), (7, 1, 1), (12, 5, 1), (11, 1, 200)]


@functools.lru_cache(maxsize=None)
def bitsearch_volume(dtype, shape):
    """Seeded data for the bit search: float32 of either sign on a grid of 1/4 (ties; the middle pair often equal), uint16 in
    steps of 16."""
    rng = np.random.default_rng(sum(shape) + np.dtype(dtype).itemsize)
    if np.dtype(dtype) == np.float32:
        v = np.rint(rng.normal(0.0, 40.0, shape) * 4) / 4
        v[rng.random(shape) < 0.05] *= 1e30
        return _frozen(v.astype(np.float32))
    return _frozen((rng.integers(1, 4096, shape) // 16 * 16 + 1).astype(dtype))


@functools.lru_cache(maxsize=None)
def nonfinite_cases():
    """(name, (Z, 1, X) float32 volume): +-inf among and as the middle elements, the middle pair (-inf, +inf) whose mean is NaN
    in numpy and in the kernel alike, and columns holding one NaN of either sign bit at the first, a middle and the last z,
    beside columns holding none."""
    inf, out = np.float32(np.inf), []
    pos_nan = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
    neg_nan = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    cols = [[1, 2, 3, 4, 5], [-inf, 0, inf, 1, -1], [inf, inf, inf, 0, 1], [-inf, -inf, -inf, 0, 1], [inf, -inf, inf, -inf, 7]]
    out.append(("inf odd Z", np.array(cols, np.float32).T[:, None, :]))
    cols = [[1, 2, 3, 4], [-inf, -inf, inf, inf], [inf, -inf, 3, 5], [inf, inf, inf, 1], [-inf, -inf, -inf, 1], [-inf, 2, inf, inf]]
    out.append(("inf even Z", np.array(cols, np.float32).T[:, None, :]))
    rng = np.random.default_rng(5)
    for Z in (5, 6, 40):
        for nan, sign in ((pos_nan, "+"), (neg_nan, "-")):
            v = rng.normal(0.0, 100.0, (Z, 1, 70)).astype(np.float32)
            v[0, 0, 1], v[Z // 2, 0, 3], v[Z - 1, 0, 64] = nan, nan, nan       # columns 0, 2, 4.. hold none
            v[Z // 2 - 1, 0, 69] = nan
            v[1, 0, 5], v[2, 0, 5] = inf, -inf
            out.append((f"{sign}nan Z {Z}", v))
    return tuple((n, _frozen(np.ascontiguousarray(v))) for n, v in out)


# =============================================================================================== apply, mean, end to end
APPLY_DTYPES = (np.uint8, np.uint16, np.int16, np.float32)
APPLY_SHAPES = [(31, 5, 77), (32, 5, 77), (33, 5, 77), (65, 5, 77), (3, 520, 521)]   # the last: 270 920 pixels > 1024 x 256
SUM_WRAP_SHAPE = (3, 520, 521)


@functools.lru_cache(maxsize=None)
def apply_volume(dtype, shape, zeros=True):
    """Seeded counts around a per-pixel pattern (int16: a third of the pixels negative).  With ``zeros``, pixel (0, 0) is zero
    throughout (0 / 0: nan), pixel (0, 1) has median 0 under nonzero samples (inf) and, for signed types, pixel (0, 2) has
    median 0 under negative ones (-inf)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(sum(shape) + 3 * dt.itemsize + (dt.kind == "i"))
    Z, Y, X = shape
    top = 200 if dt == np.uint8 else 3000
    pat = rng.integers(top // 10, top, (Y, X))
    if dt == np.int16:
        pat[:, ::3] = -pat[:, ::3]
    v = pat[None] + rng.integers(-6, 7, shape)
    if dt == np.float32:
        v = v + rng.random(shape)                              # full float32 mantissas: the pattern sum rounds
        v[:, :, 1::5] = -v[:, :, 1::5]
    if zeros:
        few = max(1, (Z - 1) // 2)
        v[:, 0, 0] = 0
        v[:, 0, 1] = 0
        v[:few, 0, 1] = top
        v[:, 0, 2] = 0
        v[:few, 0, 2] = -top if dt.kind in "if" else top
    return _frozen(v.astype(dt))


def apply_expression(vol, pattern, mean):
    """flat_apply_kernel in numpy from the device's own pattern (float64) and mean: integers float32(float64(v) / pat * m),
    float32 v / float32(pat) * float32(m) — two operations and no addition, so nothing can contract."""
    with np.errstate(all="ignore"):
        if vol.dtype == np.float32:
            out = vol / pattern.astype(np.float32)[None] * np.float32(mean)
        else:
            out = (vol.astype(np.float64) / pattern[None] * np.float64(mean)).astype(np.float32)
    assert out.dtype == np.float32
    return out


def same_bits(a, b):
    """float32 arrays equal bit for bit, a NaN matching any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def fsum_mean(pattern):
    """(math.fsum(pattern) / n, math.fsum(|pattern|) / n)."""
    p = np.asarray(pattern, np.float64).reshape(-1)
    return math.fsum(p.tolist()) / p.size, math.fsum(np.abs(p).tolist()) / p.size


# =============================================================================================== binning
BIN_FACTOR = (1, 2, 2)
BIN_SUM_SHAPE = (16, 600, 1200)                    # 2.88 M outputs per channel against 16 x 256 x 256 = 1 048 576
BIN_MEAN_SHAPE = (2, 8, 600, 1200)                 # 1.44 M outputs per channel


@functools.lru_cache(maxsize=None)
def binning_sum_case(swapped):
    """One uint16 channel (1, 16, 600, 1200): the smallest window sum in the last output and the largest in the first — both
    beyond the first trip of the grid-stride loop for one of them — or, ``swapped``, the other way round."""
    v = np.random.default_rng(31).integers(100, 1000, (1,) + BIN_SUM_SHAPE).astype(np.uint16)
    first, last = (slice(0, 1), slice(0, 2), slice(0, 2)), (slice(-1, None), slice(-2, None), slice(-2, None))
    lo, hi = (first, last) if swapped else (last, first)
    v[0][lo], v[0][hi] = 0, 65535
    return _frozen(v)


@functools.lru_cache(maxsize=None)
def binning_mean_case():
    """Two uint16 channels: the maximum over both, which scales every channel, sits in the last output of the second."""
    v = np.random.default_rng(32).integers(100, 1000, BIN_MEAN_SHAPE).astype(np.uint16)
    v[1, -1, -2:, -2:] = ((60001, 60002), (60003, 60005))
    return _frozen(v)


def binned_outputs(shape_zyx, factor=BIN_FACTOR):
    return int(np.prod([n // f for n, f in zip(shape_zyx, factor)]))
