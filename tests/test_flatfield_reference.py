"""CPU: the numpy restatement of ``median_hist_kernel`` (tests/flatfield_cases.py: ``hist_schedule`` + ``hist_select``) against
``np.median`` on every case of tests/test_gpu_flatfield.py, and the preconditions that case list states: the scripted wrap
cases reach all 14 states of the probe / skip machine and every refinement branch, three planted faults are caught (or, for
the one that only costs time, shown to change the schedule alone), the wrap shapes exceed the launch caps at 256 compute
units, and the float32 reference's own mean is measured against ``math.fsum``.  ``-s`` shows the figures (lines starting
``FF``).

The scripted volumes are built here for a card of ``REF_CUS`` compute units (the same builder and tile library as on the GPU,
1 120 tiles instead of 17 920), the schedule alone for 64, 256 and 304.
"""

import numpy as np
import pytest

import flatfield_cases as C
from oracle import oracle_np as O

REF_CUS = 16
SCRIPTED = [(dt, Z, False) for dt in C.SCRIPT_DTYPES for Z in C.SCRIPT_Z] + [(dt, C.ROW_Z, True) for dt in C.SCRIPT_DTYPES]


def _median(vol):
    return np.median(vol, axis=0).astype(np.float64)


def _branch_counts(run):
    """{(probed?, branch): pixels} over the tiles of a run."""
    return {(p, b): int((run.branch[run.probed == p] == b).sum()) for p in (True, False) for b in range(3)}


# ----------------------------------------------------------------------------- the launch rules
def test_thresholds_at_256_compute_units():
    t = C.thresholds(C.CUS)
    assert t["hist_tiles"] == 512 and t["sum_pixels"] == 262144 and t["bin_outputs"] == 1048576
    # float32 at Z = 9: 64 columns, 2304 + 8192 bytes of LDS, eight workgroups per CU; 16-bit keys alike
    assert C.bitsearch_launch(C.CUS, 9, 4) == (64, 8, 2048) and C.bitsearch_launch(C.CUS, 10, 2) == (64, 8, 2048)
    assert C.bitsearch_launch(C.CUS, 9216, 4) == (4, 1, 256) and C.bitsearch_launch(C.CUS, 576, 4)[:2] == (64, 1)
    for shape in C.BITSEARCH_WRAP:
        for keysize in (4, 2):
            cols = C.staging_cols(shape[0], keysize)
            assert cols == 64 and shape[2] % 64 != 0
            assert -(-shape[2] // cols) * shape[1] > t["bitsearch_tiles"](shape[0], keysize)
    assert {s[0] % 2 for s in C.BITSEARCH_WRAP} == {0, 1}
    for keysize, zs in C.BITSEARCH_HALVING_Z.items():
        # either side of every halving, every width run, the last Z that fits and the first that does not
        assert [C.staging_cols(z, keysize) for z in zs] == [64, 32, 32, 16, 16, 8, 8, 4, 4]
        assert C.staging_cols(C.BITSEARCH_REFUSED_Z[keysize], keysize) is None and C.BITSEARCH_REFUSED_Z[keysize] == zs[-1] + 1
    assert -(-C.BITSEARCH_X // 64) == 2 and C.BITSEARCH_X % 64 == 6 and -(-C.BITSEARCH_X // 4) == 18
    assert C.staging_cols(C.HIST_REFUSED[0], 2) is None
    assert np.prod(C.SUM_WRAP_SHAPE[1:]) > t["sum_pixels"] and C.SUM_WRAP_SHAPE in C.APPLY_SHAPES
    assert -(-C.SUM_WRAP_SHAPE[2] // 128) * C.SUM_WRAP_SHAPE[1] > t["hist_tiles"]
    assert -(-C.SUM_WRAP_SHAPE[2] // 64) * C.SUM_WRAP_SHAPE[1] > t["bitsearch_tiles"](3, 4)
    assert sorted({s[0] for s in C.APPLY_SHAPES}) == [3, 31, 32, 33, 65] and all(s[1] * s[2] % 256 for s in C.APPLY_SHAPES)
    assert C.binned_outputs(C.BIN_SUM_SHAPE) == 2880000 > t["bin_outputs"]
    assert C.binned_outputs(C.BIN_MEAN_SHAPE[1:]) == 1440000 > t["bin_outputs"]
    assert C.script_tiles(C.CUS) == 17920 > t["hist_tiles"] and C.script_tiles(C.CUS) * 128 * 10 * 2 < 50e6
    # the mean of 270 920 pixels: 2 serial terms, 8 levels, 4 partials per thread, 8 levels, the product, its reciprocal;
    # three for the reference and the second order
    assert C.sum_depth(270920) == 2 + 8 + 4 + 8 + 2 + 3 and C.sum_depth(385) == 1 + 8 + 1 + 8 + 2 + 3


# ----------------------------------------------------------------------------- the state machine
@pytest.mark.parametrize("cus", [REF_CUS, 64, 256, 304])
def test_script_reaches_all_14_states(cus):
    """Every workgroup sees ``SCRIPT``; each of the 14 states is visited, grid times each visit of the script that has it."""
    wide = C.script_wide(cus)
    assert wide.size == C.script_tiles(cus) == len(C.SCRIPT) * 2 * cus
    probed, arrive = C.hist_schedule(wide, 2 * cus)
    counts = C.state_counts(wide, probed, arrive)
    print(f"FF schedule at {cus} CUs: " + ", ".join(f"{p[0]}{w[0]}{s}:{n // (2 * cus)}" for (p, w, s), n in counts.items()))
    assert len(counts) == 14 and all(n > 0 and n % (2 * cus) == 0 for n in counts.values()), counts
    assert sum(counts.values()) == wide.size
    per_visit = {k: n // (2 * cus) for k, n in counts.items()}
    assert per_visit == {("probed", "wide", 0): 3, ("probed", "wide", 1): 2, ("probed", "wide", 2): 1, ("probed", "wide", 3): 1,
                         ("probed", "narrow", 0): 2, ("probed", "narrow", 1): 1, ("probed", "narrow", 2): 1,
                         ("probed", "narrow", 3): 1, ("skipped", "wide", 1): 1, ("skipped", "wide", 2): 4,
                         ("skipped", "wide", 3): 7, ("skipped", "narrow", 1): 2, ("skipped", "narrow", 2): 2,
                         ("skipped", "narrow", 3): 7}, per_visit   # 35 visits: 13 probed, 22 skipped


def test_schedule_by_hand():
    """One workgroup, written out: W probes and is wide (streak 1, skip 1); the next tile is skipped; a narrow probe resets."""
    wide = np.array([c == "W" for c in "WNWWNNNNWN"])
    probed, arrive = C.hist_schedule(wide, 1)
    # W probe, wide: streak 1, skip 1 | N skipped | W probe, wide: streak 2, skip 3 | W, N, N skipped | N probe, narrow: streak 0
    # | N probe | W probe, wide: streak 1, skip 1 | N skipped
    assert probed.tolist() == [True, False, True, False, False, False, True, True, True, False]
    assert arrive.tolist() == [0, 1, 1, 2, 2, 2, 2, 0, 0, 1]
    two_p, two_a = C.hist_schedule(np.repeat(wide, 2), 2)          # two workgroups, each its own copy
    assert two_p.tolist() == np.repeat(probed, 2).tolist() and two_a.tolist() == np.repeat(arrive, 2).tolist()


# ----------------------------------------------------------------------------- the restatement against np.median
@pytest.mark.parametrize("dtype,Z,row", SCRIPTED, ids=[f"{np.dtype(d).name}-Z{z}{'-row' if r else ''}" for d, z, r in SCRIPTED])
def test_scripted_case_restated_equals_np_median(dtype, Z, row):
    """``hist_schedule`` + ``hist_select`` over the scripted volume give np.median at every pixel; the tiles are wide where the
    script says; all 14 states; on probed tiles all three branches, on skipped tiles the two with a shift (a tile of 16-bit
    keys that is not probed has shift 8 at every pixel: "no shift" on a tile that is not probed is the 8-bit input's,
    test_hist_edges_restated_equal_np_median) — the straddling branch needs an even Z."""
    vol = C.scripted_volume(dtype, Z, REF_CUS, row)
    T = C.script_tiles(REF_CUS)
    assert vol.shape == ((Z, 1, 128 * T) if row else (Z, T // 8, 1024)) and vol.dtype == dtype
    run = C.hist_median(vol, 2 * REF_CUS)
    assert np.array_equal(run.wide, C.script_wide(REF_CUS))
    assert np.array_equal(run.refine, run.wide | ~run.probed)
    want = _median(vol)
    assert np.array_equal(run.median, want), np.argwhere(run.median != want)[:5]
    states = C.state_counts(run.wide, run.probed, run.arrive)
    assert all(n > 0 for n in states.values()), states
    br = _branch_counts(run)
    print(f"FF scripted {np.dtype(dtype).name} Z {Z}{' row' if row else ''}: pixels per branch, probed "
          f"{[br[True, b] for b in range(3)]} skipped {[br[False, b] for b in range(3)]}")
    assert br[True, C.NO_SHIFT] > 0 and br[True, C.SHIFT_ONE_BIN] > 0 and br[False, C.SHIFT_ONE_BIN] > 0
    assert br[False, C.NO_SHIFT] == 0
    if Z % 2 == 0:
        assert br[True, C.SHIFT_STRADDLE] > 0 and br[False, C.SHIFT_STRADDLE] > 0
    keys = C.tile_keys(vol)
    if np.dtype(dtype) == np.int16:
        assert (keys.min(axis=0) < 0x8000).any() and ((keys.min(axis=0) < 0x8000) & (keys.max(axis=0) >= 0x8000)).any()
    shifts = {int(s) for s in np.maximum(0, np.frexp(((keys.max(axis=0) - keys.min(axis=0)) | 1).astype(float))[1] - 8).ravel()}
    assert {0, 1, 3, 8} <= shifts
    wide_tiles = keys[:, run.wide]
    lone = ((wide_tiles.max(axis=0) - wide_tiles.min(axis=0)) >= 256)
    assert (lone[lone.sum(axis=1) == 1][:, 0]).any() and (lone[lone.sum(axis=1) == 1][:, 127]).any()   # lane 0's first, lane 63's second


@pytest.mark.parametrize("name", C.HIST_EDGES)
def test_hist_edges_restated_equal_np_median(name):
    vol = C.hist_edge(name)
    run = C.hist_median(vol, 2 * C.CUS)
    assert np.array_equal(run.median, _median(vol)), name
    if name == "uint8 Z 300":
        assert not run.probed.any() and not run.refine.any() and (run.branch == C.NO_SHIFT).all()
    if name == "Z 65535":
        assert (vol[:, 0, 0] == vol[0, 0, 0]).all() and np.unique(vol[:, 0, 1]).size > 100
        assert int((vol[:, 0, 2] == 700).sum()) == 32768 and int((vol[:, 0, 3] == 700).sum()) == 32767
        assert run.median[0, 2] == 700.0 and run.median[0, 3] == 40000.0


def test_one_tile_by_hand():
    """A single (Z, 128) tile through ``hist_select``: the three branches on chosen pixels, probed and not."""
    keys = np.full((4, 128), 1000, np.uint32)
    keys[:, 1] = (10, 300, 310, 5000)          # range 4990: shift 5; ranks 1, 2 -> 300, 310 share bin (290 >> 5) = 9
    keys[:, 2] = (10, 20, 4000, 5000)          # ranks straddle bins
    keys[:, 3] = (7, 7, 9, 9)                  # no shift
    sel = C.hist_select(keys, True)
    assert sel.refine and sel.branch[[0, 1, 2, 3]].tolist() == [C.NO_SHIFT, C.SHIFT_ONE_BIN, C.SHIFT_STRADDLE, C.NO_SHIFT]
    assert (sel.v1[[0, 1, 2, 3]].tolist(), sel.v2[[0, 1, 2, 3]].tolist()) == ([1000, 300, 20, 7], [1000, 310, 4000, 9])
    assert sel.base[1] == 10 and sel.shift[1] == 5 and sel.shift[3] == 0
    fixed = C.hist_select(keys, False)         # base 0, shift 8: 300 and 310 share bin 1; 7 and 9 share bin 0
    assert fixed.refine and (fixed.shift == 8).all() and (fixed.base == 0).all()
    assert fixed.branch[[0, 1, 2, 3]].tolist() == [C.SHIFT_ONE_BIN, C.SHIFT_ONE_BIN, C.SHIFT_STRADDLE, C.SHIFT_ONE_BIN]
    assert np.array_equal(fixed.v1, sel.v1) and np.array_equal(fixed.v2, sel.v2)
    eight = C.hist_select(np.minimum(keys, 255), True, bits=8)
    assert not eight.refine and (eight.branch == C.NO_SHIFT).all()


# ----------------------------------------------------------------------------- planted faults
@pytest.mark.parametrize("fault", ["hist", "minlo", "split"])
def test_planted_value_faults_change_a_scripted_case(fault):
    """hist not zeroed at the top of a workgroup's next tile; minlo not reset; a skipped tile keeping the previous tile's base
    and shift instead of (0, 8): each makes the scripted uint16 case at Z = 10 differ from np.median."""
    vol = C.scripted_volume(np.uint16, 10, REF_CUS)
    want = _median(vol)
    got = C.hist_median(vol, 2 * REF_CUS, fault=fault).median
    changed = int((got != want).sum())
    print(f"FF planted '{fault}': {changed} of {want.size} pixels differ from np.median")
    assert changed > 0
    one_visit = vol[:, : 2 * REF_CUS // 8]      # no more tiles than workgroups: the faults need a second tile to show
    assert np.array_equal(C.hist_median(one_visit, 2 * REF_CUS, fault=fault).median, _median(one_visit))


def test_planted_streak_fault_changes_the_schedule_only():
    """A narrow probe that keeps the streak is a performance fault, not a correctness one: the schedule differs (more tiles
    take the fixed split, the states probed-narrow with a streak multiply), the values do not."""
    vol = C.scripted_volume(np.uint16, 10, REF_CUS)
    good, bad = C.hist_median(vol, 2 * REF_CUS), C.hist_median(vol, 2 * REF_CUS, fault="streak")
    moved = int((good.probed != bad.probed).sum())
    print(f"FF planted 'streak': {moved} of {good.probed.size} tiles change between probed and skipped; values equal")
    assert moved > 0 and int(bad.probed.sum()) < int(good.probed.sum())
    assert np.array_equal(bad.median, good.median)


# ----------------------------------------------------------------------------- the other inputs
def test_nonfinite_cases_are_what_they_say():
    with np.errstate(all="ignore"):
        cases = dict(C.nonfinite_cases())
        odd, even = np.median(cases["inf odd Z"], axis=0)[0], np.median(cases["inf even Z"], axis=0)[0]
        assert odd.tolist()[:4] == [3.0, 0.0, np.inf, -np.inf] and odd[4] == 7.0
        assert even[0] == 2.5 and np.isnan(even[1]) and even[2] == 4.0 and even[3] == np.inf and even[4] == -np.inf and even[5] == np.inf
        for name, v in cases.items():
            if "nan" in name:
                med = np.median(v, axis=0)[0]
                holds = np.isnan(v).any(axis=0)[0]
                assert np.array_equal(np.isnan(med), holds) and sorted(np.nonzero(holds)[0].tolist()) == [1, 3, 64, 69]
                assert (np.signbit(v[np.isnan(v)]) == (name[0] == "-")).all()
    assert np.isnan(np.median(np.array([[1, 2], [np.nan, 3], [5, 4]], np.float32), axis=0)).tolist() == [True, False]


def test_apply_volumes_hold_zero_medians():
    for dt in C.APPLY_DTYPES:
        for shape in C.APPLY_SHAPES:
            v = C.apply_volume(dt, shape)
            med = np.median(v, axis=0)
            assert med[0, 0] == 0 and not v[:, 0, 0].any() and med[0, 1] == 0 and v[:, 0, 1].any() and med[0, 2] == 0
            out = C.apply_expression(v, med.astype(np.float64), 1.0)
            assert np.isnan(out[:, 0, 0]).all() and np.isposinf(out[0, 0, 1]) and np.isnan(out[-1, 0, 1])
            if np.dtype(dt).kind in "if":
                assert np.isneginf(out[0, 0, 2]) and (med < 0).any()
            clean = np.median(C.apply_volume(dt, shape, zeros=False), axis=0)
            assert (clean != 0).all()


def test_reference_float32_mean_against_fsum():
    """The reference expression takes ``pattern.mean()`` of a float32 pattern: numpy's pairwise float32 sum.  Its error against
    math.fsum at the pattern of the end-to-end test is the reference's share of that test's float32 bound."""
    vol = C.apply_volume(np.float32, C.SUM_WRAP_SHAPE, zeros=False)
    pattern = np.median(vol, axis=0)
    assert pattern.dtype == np.float32
    exact, exact_abs = C.fsum_mean(pattern)
    err = abs(float(pattern.mean()) - exact) / abs(exact)
    print(f"FF reference float32 mean of {pattern.shape}: {float(pattern.mean())!r} against fsum {exact!r}: {err:.2e} of the mean")
    assert err <= C.REF_MEAN_F32_ERR
    assert C.E2E_F32_TOL == C.REF_MEAN_F32_ERR + 2.0 ** -23
    want = O.flat_field_zyx(vol)
    assert want.dtype == np.float32 and np.isfinite(want).all()


def test_binning_cases_put_their_extremes_where_the_loop_wraps():
    for swapped in (False, True):
        v = C.binning_sum_case(swapped)
        s = v[0].astype(np.float32).reshape(16, 1, 300, 2, 600, 2).sum(axis=(1, 3, 5)).reshape(-1)
        lo, hi = (0, -1) if swapped else (-1, 0)
        assert s[lo] == 0 == s.min() and s[hi] == 4 * 65535 == s.max() and (s == s.min()).sum() == 1 == (s == s.max()).sum()
    m = C.binning_mean_case()
    means = m.astype(np.float32).reshape(2, 8, 1, 300, 2, 600, 2).mean(axis=(2, 4, 6))
    assert means.max() == means[1].reshape(-1)[-1] and (means == means.max()).sum() == 1
