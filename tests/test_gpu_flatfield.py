"""GPU: the flat-field kernels (csrc/flatfield.hip: bh_median_z, bh_flat_field) and binning (csrc/binning.hip) where their tile
and grid-stride loops wrap, and at the edges of their arguments.

``median_hist_kernel`` runs persistent workgroups that carry a probe / skip state from tile to tile; the existing tests give a
workgroup one tile, or data that never refines.  The scripted cases here (tests/flatfield_cases.py) are sized from the card's
own compute-unit count: 35 tiles per workgroup that visit all 14 states of that machine, skipped tiles narrow and wide, hist /
minlo / any_shift re-zeroed behind tiles that refined.  ``median_z_kernel`` (the bit search) gets its second trip, every
staging width and the Z on either side of each halving, X = 1, Z below the number of z groups, +-inf and NaN; the refusals are
pinned.  Every median equals ``np.median`` — no pixel excluded, no tolerance.  ``bh_flat_field`` is called through the ABI
with ``pattern`` and ``mean_out``: the pattern equals np.median, the mean is held to math.fsum within the depth of the
reduction, the output is bit-equal to the apply expression evaluated in numpy, and end to end it meets
``oracle_np.flat_field_zyx`` at the wrap shapes.  Binning equals ``oracle_np.binning_czyx`` bit for bit above the grid cap.
``-s`` shows one ``FF gpu`` line per case; DESIGN.md §3.5 keeps the table.
"""

import ctypes

import numpy as np
import pytest
import torch

import flatfield_cases as C
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

REFUSED = (ValueError, NotImplementedError)


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _dev(a, gpu):
    return torch.from_numpy(np.array(a, copy=True)).to(gpu)   # the case arrays are read-only: upload a copy


def _median_gpu(vol, gpu):
    from biahub_amd.flat_field import median_z_device

    return median_z_device(_dev(vol, gpu)).cpu().numpy()


def _np_median(vol):
    with np.errstate(all="ignore"):
        return np.median(vol, axis=0).astype(np.float64)


def _hold_median(what, got, vol, grid=None):
    """got == np.median(vol, axis=0) at every pixel, NaN matching NaN.  On failure: the first differing (y, x) and, for the
    histogram kernel (``grid`` given), the tile and the state its workgroup reached it in."""
    want = _np_median(vol)
    if np.array_equal(got, want, equal_nan=True):
        return
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    lines = [f"{what}: {len(bad)} of {want.size} pixels differ from np.median"]
    run = C.hist_median(vol, grid) if grid else None
    for y, x in bad[:6]:
        line = f"  (y {y}, x {x}): got {got[y, x]!r} want {want[y, x]!r}"
        if run is not None:
            t = y * -(-vol.shape[2] // C.FH_COLS) + x // C.FH_COLS
            line += (f"; tile {t} (visit {t // grid} of workgroup {t % grid}): {'probed' if run.probed[t] else 'skipped'}, "
                     f"{'wide' if run.wide[t] else 'narrow'}, streak {run.arrive[t]}, branch "
                     f"{C.BRANCHES[run.branch[t, x % C.FH_COLS]]}; the restatement gives {run.median[y, x]!r}")
        lines.append(line)
    pytest.fail("\n".join(lines))


# ----------------------------------------------------------------------------- the histogram kernel, scripted
def _scripted(gpu, dtype, Z, row):
    cus = _cus(gpu)
    grid = C.thresholds(cus)["hist_tiles"]
    vol = C.scripted_volume(dtype, Z, cus, row)
    tiles = vol.shape[1] * (vol.shape[2] // C.FH_COLS)
    assert tiles == len(C.SCRIPT) * grid > grid, f"{tiles} tiles do not wrap {grid} workgroups: size the case for this card"
    wide = C.tiles_wide(C.tile_keys(vol))
    assert np.array_equal(wide, C.script_wide(cus))
    states = C.state_counts(wide, *C.hist_schedule(wide, grid))
    assert len(states) == 14 and all(n >= grid for n in states.values()), states
    got = _median_gpu(vol, gpu)
    _hold_median(f"scripted {np.dtype(dtype).name} {vol.shape}", got, vol, grid)
    assert np.array_equal(_median_gpu(vol, gpu), got), "the second run differs from the first"
    print(f"FF gpu scripted {np.dtype(dtype).name} {vol.shape}: {tiles} tiles on {grid} workgroups, equal to np.median, twice")


@pytest.mark.parametrize("Z", C.SCRIPT_Z)
@pytest.mark.parametrize("dtype", C.SCRIPT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_hist_median_scripted_wrap(gpu, dtype, Z):
    """35 tiles per workgroup through all 14 states of the probe / skip machine (asserted for this card's grid), even and odd
    Z, keys across 0x8000 for int16: np.median at every pixel, and the same bits on a second run."""
    _scripted(gpu, dtype, Z, row=False)


@pytest.mark.parametrize("dtype", C.SCRIPT_DTYPES, ids=lambda d: np.dtype(d).name)
def test_hist_median_scripted_row(gpu, dtype):
    """The (Z, 1, X) layout _median_tiled makes of any axis but 0: the same script along one row."""
    _scripted(gpu, dtype, C.ROW_Z, row=True)


def test_median_tiled_other_axis_wraps(gpu):
    """_median_tiled(axis=2) of a (Y', X', Z) array is the row layout: more tiles than workgroups through the public helper."""
    from biahub_amd.flat_field import _median_tiled

    grid = C.thresholds(_cus(gpu))["hist_tiles"]
    rng = np.random.default_rng(8)
    a = rng.integers(0, 4000, (3 * grid + 1, 43, 6)).astype(np.uint16)          # 43 x (3 grid + 1) pixels: over 128 grid
    assert a.shape[0] * a.shape[1] > C.FH_COLS * grid
    assert np.array_equal(_median_tiled(a, axis=2), np.median(a, axis=2))


@pytest.mark.parametrize("name", C.HIST_EDGES)
def test_hist_median_edges(gpu, name):
    """Z = 65535 (a 16-bit half of a hist word at 65535 beside a varied neighbour; 32768 against 32767 samples), X = 2 and
    X = 3 (the paired and the unpaired loads at the clamp), uint8 at Z = 300 (never probed), ragged last tiles."""
    vol = C.hist_edge(name)
    assert vol.dtype != np.float32 and 2 <= vol.shape[2] and vol.shape[0] <= 65535      # the histogram kernel's domain
    _hold_median(name, _median_gpu(vol, gpu), vol, C.thresholds(_cus(gpu))["hist_tiles"])


def test_hist_median_refuses_z_65536(gpu):
    """Past the 16-bit counters the launch falls to the bit search, whose staging cannot hold 65536 samples per pixel."""
    with pytest.raises(REFUSED, match="does not fit"):
        _median_gpu(np.zeros(C.HIST_REFUSED, np.uint16), gpu)


# ----------------------------------------------------------------------------- the bit search
def _keysize(dtype):
    return 4 if np.dtype(dtype) == np.float32 else 2


def _force_bitsearch(monkeypatch, dtype):
    if np.dtype(dtype) != np.float32:
        monkeypatch.setenv("BH_FF_BITSEARCH", "1")


@pytest.mark.parametrize("shape", C.BITSEARCH_WRAP, ids=str)
@pytest.mark.parametrize("dtype", C.BITSEARCH_DTYPES, ids=lambda d: np.dtype(d).name)
def test_bitsearch_wrap(gpu, monkeypatch, dtype, shape):
    """More tiles than cus x per_cu workgroups, X no multiple of 64, odd and even Z: the second trip of median_z_kernel's tile
    loop, whose first barrier keeps the staged keys from the previous tile's readers.  Twice, the same bits."""
    _force_bitsearch(monkeypatch, dtype)
    cols, per_cu, cap = C.bitsearch_launch(_cus(gpu), shape[0], _keysize(dtype))
    tiles = -(-shape[2] // cols) * shape[1]
    assert tiles > cap, f"{tiles} tiles do not wrap {cap} workgroups ({per_cu} per CU): size the case for this card"
    vol = C.bitsearch_volume(dtype, shape)
    got = _median_gpu(vol, gpu)
    _hold_median(f"bit search {np.dtype(dtype).name} {shape}", got, vol)
    assert np.array_equal(_median_gpu(vol, gpu), got, equal_nan=True)
    print(f"FF gpu bit search {np.dtype(dtype).name} {shape}: {tiles} tiles on {cap} workgroups, equal to np.median, twice")


@pytest.mark.parametrize("dtype", C.BITSEARCH_DTYPES, ids=lambda d: np.dtype(d).name)
def test_bitsearch_staging_widths(gpu, monkeypatch, dtype):
    """Z on either side of every halving of the staging width (64, 32, 16, 8, 4 columns), the last Z that fits, on 70 columns
    (a ragged second tile at 64, 18 tiles at 4); one Z more is refused."""
    _force_bitsearch(monkeypatch, dtype)
    ks = _keysize(dtype)
    for Z in C.BITSEARCH_HALVING_Z[ks]:
        vol = C.bitsearch_volume(dtype, (Z, 1, C.BITSEARCH_X))
        _hold_median(f"bit search {np.dtype(dtype).name} Z {Z} ({C.staging_cols(Z, ks)} columns)", _median_gpu(vol, gpu), vol)
    with pytest.raises(REFUSED, match="does not fit"):
        _median_gpu(np.zeros((C.BITSEARCH_REFUSED_Z[ks], 1, C.BITSEARCH_X), dtype), gpu)


@pytest.mark.parametrize("dtype", C.BITSEARCH_DTYPES + (np.int16, np.uint8), ids=lambda d: np.dtype(d).name)
def test_bitsearch_small_shapes(gpu, dtype):
    """X = 1 (the bit search for integers too, without the switch), Y = 1, Z = 1 and 2 (fewer samples than z groups)."""
    for shape in C.BITSEARCH_SMALL:
        if np.dtype(dtype) in (np.int16, np.uint8) and shape[2] != 1:
            continue
        vol = C.bitsearch_volume(np.uint16 if np.dtype(dtype) != np.float32 else dtype, shape)
        if np.dtype(dtype) == np.int16:
            vol = (vol.astype(np.int32) - 2048).astype(np.int16)
        elif np.dtype(dtype) == np.uint8:
            vol = (vol // 16).astype(np.uint8)
        _hold_median(f"bit search {np.dtype(dtype).name} {shape}", _median_gpu(vol, gpu), vol)


def test_bitsearch_small_shapes_uint16_forced(gpu, monkeypatch):
    monkeypatch.setenv("BH_FF_BITSEARCH", "1")
    for shape in C.BITSEARCH_SMALL:
        vol = C.bitsearch_volume(np.uint16, shape)
        _hold_median(f"bit search uint16 {shape}", _median_gpu(vol, gpu), vol)


@pytest.mark.parametrize("name,vol", C.nonfinite_cases(), ids=[n for n, _ in C.nonfinite_cases()])
def test_float32_nonfinite(gpu, name, vol):
    """+-inf among and as the middle elements, the middle pair (-inf, +inf) -> NaN; a column holding one NaN, of either sign
    bit, first, middle or last along z, gives NaN as np.median does, and its neighbours are untouched."""
    got = _median_gpu(vol, gpu)
    _hold_median(name, got, vol)
    if "nan" in name:
        assert np.isnan(got[0, [1, 3, 64, 69]]).all() and int(np.isnan(got).sum()) == 4


def test_float32_nan_pattern_makes_the_output_nan(gpu):
    """The reference's pattern mean is NaN once one column holds a NaN, and so is its whole output."""
    from biahub_amd.flat_field import flat_field_zyx

    vol = np.array(C.apply_volume(np.float32, (5, 3, 70), zeros=False))
    vol[2, 1, 7] = np.nan
    with np.errstate(all="ignore"):
        assert np.isnan(O.flat_field_zyx(vol)).all()
    assert np.isnan(flat_field_zyx(vol)).all()


# ----------------------------------------------------------------------------- bh_flat_field through the ABI
def _flat_field_abi(vol, gpu):
    """(out float32 (Z, Y, X), pattern float64 (Y, X), mean) of bh_flat_field with ``pattern`` and ``mean_out`` given."""
    from biahub_amd import _lib
    from biahub_amd.device import _NP_TO_DT, get_context, ptr

    t = _dev(vol, gpu)
    Z, Y, X = vol.shape
    out = torch.empty((Z, Y, X), dtype=torch.float32, device=gpu)
    pattern = torch.empty((Y, X), dtype=torch.float64, device=gpu)
    mean = ctypes.c_double(-1.0)
    ctx = get_context(gpu)
    _lib.check(ctx.lib.bh_flat_field(ctx.handle, ptr(t), _NP_TO_DT[vol.dtype], Z, Y, X, ptr(out), ptr(pattern), ctypes.byref(mean)))
    return out.cpu().numpy(), pattern.cpu().numpy(), float(mean.value)


@pytest.mark.parametrize("shape", C.APPLY_SHAPES, ids=str)
@pytest.mark.parametrize("dtype", C.APPLY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_flat_field_pattern_mean_and_apply(gpu, dtype, shape):
    """Z = 31, 32, 33, 65 (the 32-plane chunks of the apply grid) on a plane that is no multiple of 256, and 270 920 pixels
    (the pattern sum's 1024 workgroups take a second term); medians of 0 under zero and nonzero samples, negative medians.
    1. the pattern equals np.median;
    2. |mean - fsum(pattern) / n| <= d 2^-53 fsum(|pattern|) / n, d = ``sum_depth`` (derived from the launch shape, not
       measured) — on the volume without zero medians, whose pattern is finite;
    3. out is bit-equal to the apply expression in numpy from the device's own pattern and mean, nan and inf included."""
    for zeros in (True, False):
        vol = C.apply_volume(dtype, shape, zeros=zeros)
        out, pattern, mean = _flat_field_abi(vol, gpu)
        _hold_median(f"pattern {np.dtype(dtype).name} {shape}", pattern, vol)
        if np.isfinite(pattern).all() and pattern.any():
            exact, exact_abs = C.fsum_mean(pattern)
            d = C.sum_depth(pattern.size)
            err = abs(mean - exact) / (2.0 ** -53 * exact_abs)
            print(f"FF gpu mean {np.dtype(dtype).name} {shape} zeros {zeros}: {mean!r} against fsum {exact!r}: {err:.2f} of 2^-53 mean |pattern|, bound {d}")
            assert err <= d, (mean, exact, d)
        want = C.apply_expression(vol, pattern, mean)
        if not C.same_bits(out, want):
            bad = np.argwhere(~((out == want) | (np.isnan(out) & np.isnan(want))))
            pytest.fail(f"apply {np.dtype(dtype).name} {shape} zeros {zeros}: {len(bad)} voxels differ from the expression, first "
                        + "; ".join(f"{tuple(b)}: {out[tuple(b)]!r} want {want[tuple(b)]!r} (v {vol[tuple(b)]!r} pattern "
                                    f"{pattern[b[1], b[2]]!r})" for b in bad[:4]) + f"; mean {mean!r}")
        if zeros:
            assert np.isnan(out[:, 0, 0]).all() and np.isposinf(out[0, 0, 1]) and np.isnan(out[-1, 0, 1])
        if shape == C.SUM_WRAP_SHAPE:                                   # the wrap case: a second run gives the same bits
            again = _flat_field_abi(vol, gpu)
            assert C.same_bits(again[0], out) and np.array_equal(again[1], pattern, equal_nan=True) and again[2] == mean


@pytest.mark.parametrize("dtype", C.APPLY_DTYPES, ids=lambda d: np.dtype(d).name)
def test_flat_field_end_to_end_at_the_wrap_shape(gpu, dtype):
    """(3, 520, 521) wraps the median's tile loop (2 600 tiles of 128 or 4 680 of 64), and the pattern sum: against
    oracle_np.flat_field_zyx, 2e-7 of max for integers, REF_MEAN_F32_ERR + 2^-23 of max for float32."""
    from biahub_amd.flat_field import flat_field_zyx

    cus = _cus(gpu)
    Z, Y, X = C.SUM_WRAP_SHAPE
    t = C.thresholds(cus)
    assert Y * X > t["sum_pixels"], "the plane does not wrap the pattern sum"
    tiles, cap = ((-(-X // 64) * Y, t["bitsearch_tiles"](Z, 4)) if np.dtype(dtype) == np.float32 else (-(-X // 128) * Y, t["hist_tiles"]))
    assert tiles > cap, f"{tiles} tiles do not wrap {cap} workgroups: size the case for this card"
    vol = C.apply_volume(dtype, C.SUM_WRAP_SHAPE, zeros=False)
    want = O.flat_field_zyx(vol).astype(np.float32)
    got = flat_field_zyx(np.array(vol))
    err = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
    tol = C.E2E_F32_TOL if np.dtype(dtype) == np.float32 else C.E2E_INT_TOL
    print(f"FF gpu end to end {np.dtype(dtype).name} {C.SUM_WRAP_SHAPE}: {err:.2e} of max, bound {tol:.2e}")
    assert got.dtype == np.float32 and err <= tol, (err, tol)


# ----------------------------------------------------------------------------- binning
@pytest.mark.parametrize("swapped", [False, True], ids=["min last, max first", "min first, max last"])
def test_binning_sum_above_the_grid_cap(gpu, swapped):
    """2.88 M outputs on 16 CUs workgroups of 256: the extremes that set the stretch sit in the first and the last output."""
    from biahub_amd.process_data import binning_czyx

    cap = C.thresholds(_cus(gpu))["bin_outputs"]
    assert C.binned_outputs(C.BIN_SUM_SHAPE) > cap, f"{C.binned_outputs(C.BIN_SUM_SHAPE)} outputs do not wrap {cap}: size the case for this card"
    v = C.binning_sum_case(swapped)
    got = binning_czyx(np.array(v), list(C.BIN_FACTOR), "sum")
    want = O.binning_czyx(v, C.BIN_FACTOR, "sum")
    assert got.dtype == want.dtype == np.uint16 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    lo, hi = (0, -1) if swapped else (-1, 0)
    assert got.reshape(-1)[lo] == 0 and got.reshape(-1)[hi] == 65535
    assert np.array_equal(binning_czyx(np.array(v), list(C.BIN_FACTOR), "sum"), got)   # and the same bits again


def test_binning_mean_two_channels_above_the_grid_cap(gpu):
    """The maximum over both channels, which scales each, sits in the last output of the second."""
    from biahub_amd.process_data import binning_czyx

    cap = C.thresholds(_cus(gpu))["bin_outputs"]
    assert C.binned_outputs(C.BIN_MEAN_SHAPE[1:]) > cap, "the channel does not wrap the binning grid: size the case for this card"
    v = C.binning_mean_case()
    got = binning_czyx(np.array(v), list(C.BIN_FACTOR), "mean")
    want = O.binning_czyx(v, C.BIN_FACTOR, "mean")
    assert got.dtype == want.dtype == np.uint16 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert got[1].reshape(-1)[-1] == 65535 and int((got == 65535).sum()) == 1
    assert np.array_equal(binning_czyx(np.array(v), list(C.BIN_FACTOR), "mean"), got)
