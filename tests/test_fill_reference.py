"""CPU: the float64 reference of the overhang fill (oracle/reference_f64.py: dilate_mask_cross, fill_overhang_f64), the checker
the GPU kernels are held to in tests/test_gpu_fill_f64.py (tests/fill_cases.py derives its bound), and the claims about the inputs.

The reference is held to a brute-force ball, to the golden volumes of the legacy fill and to the numpy oracles; every input of
the GPU tests is shown to keep a voxel outside the mask and to keep the summation term of the bound below one float32 rounding
of the mean; a numpy restatement of the kernels' mask words and of ``apply_fill_kernel``'s addressing satisfies the checker at
every such input, and with each of nine planted defects it does not.  Every case prints one ``F64 fill ...`` line (``-s``).
"""

import numpy as np
import pytest
import torch

import deskew_cases as D
import fill_cases as F
from conftest import GOLDEN
from oracle import oracle_np as O
from oracle import reference_f64 as R

SMALL = F.small_cases()


def _ref(vol, it, conn):
    return R.fill_overhang_f64(vol, None, it, conn)


def _rejected(got, vol, ref, fill, name):
    try:
        F.assert_fill_close(got, vol, ref, fill, name)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------- the reference is the definition
@pytest.mark.parametrize("shape", [(5, 6, 7), (1, 9, 4), (4, 1, 1), (3, 8, 40)])
def test_reference_masks_are_the_balls(shape):
    """``dilate_mask`` is the Chebyshev ball and ``dilate_mask_cross`` the L1 ball of radius ``iterations`` about the set voxels,
    cut at the array's faces: against the distances, one voxel at a time."""
    rng = np.random.default_rng(sum(shape))
    seed = rng.random(shape) < 0.03
    seed[tuple(n - 1 for n in shape)] = True
    zz, yy, xx = np.nonzero(seed)
    g = np.indices(shape)
    d = [np.abs(g[a][..., None] - c[None, None, None, :]) for a, c in enumerate((zz, yy, xx))]
    cheb, l1 = np.maximum(np.maximum(d[0], d[1]), d[2]).min(axis=3), (d[0] + d[1] + d[2]).min(axis=3)
    for it in (0, 1, 2, 3, 5):
        assert np.array_equal(R.dilate_mask(torch.from_numpy(seed), it).numpy(), cheb <= it), it
        assert np.array_equal(R.dilate_mask_cross(torch.from_numpy(seed), it).numpy(), l1 <= it), it


def test_cross_reference_reproduces_the_legacy_golden_volumes():
    """The voxels the reference project's ``_fill_overhang_with_mean`` changed in its five volumes are ``dilate_mask_cross``'s mask."""
    z = np.load(GOLDEN / "legacy_fill.npz")
    for j in range(5):
        vol, it, want = z[f"in{j}"], int(z[f"it{j}"]), z[f"out{j}"]
        mask, fill, kappa = R.fill_overhang_f64(vol, None, it, 6)
        assert np.array_equal(mask.numpy(), want != vol), j
        F.assert_input_ok((mask, fill, kappa), vol.size, f"golden {j}")
        assert abs(float(want[mask.numpy()][0]) - fill) <= 2e-6 * abs(fill), j     # the reference's own float32 mean


def test_reference_fill_is_the_oracles():
    """Connectivity 26: ``oracle_np.dilate_zero_mask``'s mask, and ``oracle_np.fill_overhang``'s value to float32 rounding; a constant
    comes back as given; all zeros give NaN and an infinite kappa."""
    for vol, it in ((F.chunk_case(2049), 3), (F.edge_case(65, 2, "hi"), 2), (F.walk_narrow_case(), 3), (F.value_case("signed"), 1)):
        mask, fill, kappa = R.fill_overhang_f64(vol, None, it, 26)
        assert isinstance(fill, float) and mask.dtype == torch.bool
        assert np.array_equal(mask.numpy(), O.dilate_zero_mask(vol == 0, it))
        want = O.fill_overhang(vol, None, it)
        assert abs(float(want[mask.numpy()][0]) - fill) <= F.U * abs(fill)
        valid = vol[~mask.numpy()].astype(np.float64)
        assert kappa == pytest.approx((np.abs(vol.astype(np.float64)).sum() + np.abs(vol[mask.numpy()].astype(np.float64)).sum()) / valid.size, rel=1e-14)
        assert R.fill_overhang_f64(vol, -7.25, it, 26)[1] == -7.25
    mask, fill, kappa = R.fill_overhang_f64(np.zeros((2, 3, 4), np.float32))
    assert bool(mask.all()) and fill != fill and kappa == float("inf")
    with pytest.raises(ValueError):
        R.fill_overhang_f64(np.zeros((2, 3, 4), np.float32), connectivity=18)


# ----------------------------------------------------------------------------- the inputs reach what they claim
def test_inputs_reach_their_code():
    """Alignments, chunk counts, units per wavefront, mask words and partial counts of the inputs, at the 256 CUs the sizes were
    chosen for (the GPU tests assert the same with the device's own count)."""
    for X in F.CHUNK_X:
        shape = (3, 7, X)
        if X % 2:
            assert F.row_alignments(shape) == {0, 1, 2, 3}, X
        assert -(-X // 2048) == (1 if X <= 2048 else 2 if X <= 4096 else 3 if X <= 6144 else 4), X
    assert F.row_alignments(F.WALK_NARROW) == {0, 1, 2, 3} and F.row_alignments(F.WALK_WIDE) == {0, 1, 2, 3}
    assert F.WALK_NARROW[2] <= 2048 and F.units_per_wavefront(F.WALK_NARROW, F.CUS) == 2
    assert F.WALK_WIDE[2] > 2048 and F.units_per_wavefront(F.WALK_WIDE, F.CUS) == 4
    assert F.mask_words(F.WALK_WIDE) > F.dilation_threads(F.CUS)            # dilate_x_kernel's grid-stride loop (a thread owns a word)
    assert F.second_pass_row(F.WALK_WIDE, F.CUS, 1) is not None and F.second_pass_row(F.WALK_WIDE, F.CUS, 2) is None   # not dilate_outer's
    assert F.mask_words(F.WALK_WIDE) // 2 > 8 * F.CUS * 256                 # shell_kernel's (a thread owns a pair of words)
    assert F.mask_words(F.WALK_WIDE) // 2 > 8 * F.CUS * 4                   # mask0_kernel's (a wavefront owns a pair)
    assert F.mask_words(F.WALK_ROWS) // 2 > F.dilation_threads(F.CUS)       # dilate_outer_kernel's, y and z (a thread owns a pair)
    assert F.mask_words(F.WALK_ROWS) > F.dilation_threads(F.CUS)            # dilate_cross_kernel's and dilate_x_kernel's
    assert F.second_pass_row(F.WALK_ROWS, F.CUS, 2) == 1024 * 1024 and F.second_pass_row(F.WALK_ROWS, F.CUS, 1) == 512 * 1024
    assert F.units_per_wavefront(F.WALK_ROWS, F.CUS) == 130
    for shape, angle, ratio, N, Xp in F.DESKEW_WIDE:
        assert O.get_deskewed_data_shape(shape, angle, ratio, True)[0][2] == Xp
    assert {c[4] % 4 for c in F.DESKEW_WIDE} == {0, 1, 2, 3} and all(c[4] > 2048 for c in F.DESKEW_WIDE)
    shape, angle, ratio, N, cfg = F.DESKEW_PARTIALS
    assert D.tile_workgroups(shape, angle, ratio, N, cfg) == 4 * 7 * 400 >= 8 * F.FIN_NT + 1
    assert D.cfg_lds(shape, D.geometry(shape, angle, ratio, N), N, cfg) <= D.LDS_MAX


@pytest.mark.parametrize("conn,words_per_thread", [(26, 2), (6, 1)])
def test_rows_walk_obeys_the_conditions_and_reaches_the_second_pass(conn, words_per_thread):
    """(1040, 1024, 2): the input conditions for the reference alone, and zeros with a grown mask in the rows that only the second pass
    of dilate_outer_kernel (connectivity 26) and of dilate_cross_kernel (6) writes at 256 CUs.  Over a million rows: the restatement,
    a Python loop per row, is not run here."""
    vol = F.walk_rows_case()
    ref = _ref(vol, 3, conn)
    F.assert_input_ok(ref, vol.size, "rows walk")
    F.assert_second_pass_reached(vol, ref[0], F.CUS, words_per_thread, "rows walk")


@pytest.mark.parametrize("name,build,it,conn,fills", SMALL, ids=[c[0] for c in SMALL])
def test_inputs_obey_the_conditions_and_the_restatement_the_checker(name, build, it, conn, fills):
    """Per input of the GPU tests: a voxel stays outside the mask and n 2^-52 kappa < 2^-24 |fill| for the reference alone; the numpy
    restatement of the kernels' words and addressing then satisfies the checker, with every fill the GPU tests run."""
    vol = build()
    assert bool((vol == 0).any()) and bool((vol[vol != 0] > 0).all()), name
    ref = _ref(vol, it, conn)
    F.assert_input_ok(ref, vol.size, name)
    for fill in fills:
        got = F.fill_restated(vol, None if fill == "mean" else fill, it, conn)
        worst = F.assert_fill_close(got, vol, F.with_fill(ref, fill), fill, name)
        print(f"F64 fill restated {name} fill {fill}: {worst:.3f} x 2^-24 |fill|")


@pytest.mark.parametrize("what", F.VALUE_CASES)
def test_value_inputs_and_the_restatement(what):
    """-0.0 is masked, subnormals are not, signed data stays inside the kappa condition; without zeros nothing changes; all zeros
    and a NaN outside the mask give NaN; a NaN or an infinity in the shell gives NaN where the reference's mean is finite."""
    vol = F.value_case(what)
    ref = _ref(vol, 3, 26)
    mask = ref[0].numpy()
    if F.checked_values(what):
        F.assert_input_ok(ref, vol.size, what)
    if what == "negative zero":
        assert mask[3, 4, 30] and np.signbit(vol[3, 4, 30])
    if what == "subnormals":
        assert not mask[3, 4, 30] and not mask[3, 4, 20] and not mask[0, 0, 39] and int(mask.sum()) == int(_ref(F.value_case("plain"), 3, 26)[0].sum())
    if what == "signed":
        assert bool((vol < 0).any()) and bool((vol > 0).any())
    if what == "no zeros":
        assert not mask.any()
    if what in ("all zeros", "nan outside"):
        assert ref[1] != ref[1]
    if what in F.NONFINITE_SHELL:
        assert np.isfinite(ref[1]) and int((~np.isfinite(vol) & mask).sum()) == 1
        ref = (ref[0], float("nan"), ref[2])       # the known divergence: S_all - S_shell cannot undo it
    got = F.fill_restated(vol, None, 3, 26)
    F.assert_fill_close(got, vol, ref, "mean", what)
    F.assert_fill_close(F.fill_restated(vol, -7.25, 3, 26), vol, F.with_fill(ref, -7.25), -7.25, what)
    if what == "no zeros":
        assert np.array_equal(got.view(np.int32), vol.view(np.int32))


# ----------------------------------------------------------------------------- the numpy oracles under the checker
def test_numpy_oracles_under_the_checker():
    """``oracle_np.fill_overhang`` (float64 mean) against the reference through the checker, mean and constant.
    ``oracle_np.fill_overhang_with_mean`` (SciPy's dilation) takes its mean as the reference project does, ``data[~dilated].mean()`` in
    FLOAT32 — bit for bit the golden volumes' — so the checker's premise (float64 sums) does not hold for it: measured, in units of
    2^-24 |fill|, 1.16 at the (4, 5, 40) input with a negative zero, 10.2 at the signed one (its sum cancels), 0.11 .. 0.40 at the others.  Its mask, its untouched voxels and its single value are held by the
    checker exactly (as a constant fill of its own value); its value is held to numpy's pairwise float32 summation: blocks of 128
    terms on eight accumulators (at most 16 + 3 additions deep), a tree of ceil(log2(m / 128)) levels above them, one division —
    (20 + ceil(log2(m / 128))) 2^-24 of the mean magnitude of the m valid voxels."""
    for vol, it in ((F.chunk_case(2051), 3), (F.chunk_case(4097), 0), (F.edge_case(64, 3, "hi"), 3), (F.edge_case(33, 7, "ends"), 7),
                    (F.walk_narrow_case(), 3), (F.value_case("negative zero"), 3), (F.value_case("signed"), 2)):
        ref = _ref(vol, it, 26)
        worst = F.assert_fill_close(O.fill_overhang(vol, None, it), vol, ref, "mean", "fill_overhang")
        print(f"F64 fill oracle_np.fill_overhang {vol.shape} it {it}: {worst:.3f} x 2^-24 |fill|")
        F.assert_fill_close(O.fill_overhang(vol, 321.5, it), vol, F.with_fill(ref, 321.5), 321.5, "fill_overhang constant")
        if it > 0:
            mask, fill, kappa = _ref(vol, it, 6)
            got = O.fill_overhang_with_mean(vol, it)
            val = float(got[mask.numpy()][0])
            F.assert_fill_close(got, vol, (mask, val, kappa), val, "fill_overhang_with_mean")
            valid = np.abs(vol[~mask.numpy()].astype(np.float64))
            depth = 20 + max(0, int(np.ceil(np.log2(valid.size / 128))))
            print(f"F64 fill oracle_np.fill_overhang_with_mean {vol.shape} it {it}: {abs(val - fill) / (F.U * abs(fill)):.3f} x 2^-24 |fill| "
                  f"(float32 pairwise bound {depth * valid.mean() / abs(fill):.1f})")
            assert abs(val - fill) <= depth * F.U * valid.mean()


# ----------------------------------------------------------------------------- the checks bite
def _bites(defect, vol, it, conn=26, fill="mean"):
    ref = _ref(vol, it, conn)
    good = F.fill_restated(vol, None if fill == "mean" else fill, it, conn)
    F.assert_fill_close(good, vol, F.with_fill(ref, fill), fill, defect)
    bad = F.fill_restated(vol, None if fill == "mean" else fill, it, conn, defect=defect)
    return _rejected(bad, vol, F.with_fill(ref, fill), fill, defect)


@pytest.mark.parametrize("X", [x for x in F.CHUNK_X if x % 2 and x > 2048])
@pytest.mark.parametrize("it", [0, 3])
def test_defect_last_group_without_the_next_word(X, it):
    """Voxels 2048 .. 2048 + a0 - 1 of a misaligned row belong to the LAST group of the first chunk, whose bits lie in the next
    chunk's first word: left unfilled, the checker sees more than one value inside the mask.  With a mean and a constant fill."""
    assert _bites("no next word", F.chunk_case(X), it) and _bites("no next word", F.chunk_case(X), it, fill=321.5)


@pytest.mark.parametrize("X", [x for x in F.CHUNK_X if x % 2])
def test_defect_head_skipped(X):
    """Rows 1 .. 3 (all masked after three dilations of the zero row) start 1 .. 3 voxels before a 16-byte boundary."""
    assert _bites("no head", F.chunk_case(X), 3) and _bites("no head", F.chunk_case(X), 3, fill=321.5)


@pytest.mark.parametrize("X,it", [(64, 1), (64, 3), (64, 7), (128, 1), (128, 2)])
def test_defect_x_dilation_across_the_row_end(X, it):
    """A zero at x = X - 1 with X a multiple of 64 (no padding bits in between): carried into the next row's words, the dilation
    reaches that row's voxels 0 .. r - 1."""
    vol = F.edge_case(X, it, "hi")
    z, y, x = np.argwhere(vol == 0)[-1]
    assert x == X - 1 and (z, y) != (vol.shape[0] - 1, vol.shape[1] - 1)
    assert _bites("x carry", vol, it)


def test_defect_y_dilation_across_the_plane_end():
    """Every edge input with one or two dilations and a zero on the last row of a plane that has a successor, or on the first row of
    one that has a predecessor."""
    n = 0
    for X in F.EDGE_X:
        for it in (1, 2):
            for side in ("hi", "lo"):
                vol = F.edge_case(X, it, side)
                Z, Y, _ = vol.shape
                if any((y == Y - 1 and z < Z - 1) or (y == 0 and z > 0) for z, y, x in np.argwhere(vol == 0)):
                    assert _bites("y wrap", vol, it), (X, it, side)
                    n += 1
    assert n >= 20


VALUE_DEFECT_CASES = [c for c in SMALL if (c[0].startswith("edge") and " hi " in c[0] and c[2] in (1, 3) and c[3] == 26)
                      or (c[0].startswith("chunk") and c[2] == 3)]


@pytest.mark.parametrize("name,build,it,conn,fills", VALUE_DEFECT_CASES, ids=[c[0] for c in VALUE_DEFECT_CASES])
def test_defects_of_the_value(name, build, it, conn, fills):
    """The mean over the undilated mask, a fill two float32 ulps off, one untouched voxel moved by one ulp."""
    vol = build()
    for defect in ("mean undilated", "fill 2 ulp", "touch outside"):
        assert _bites(defect, vol, it, conn), (name, defect)
    assert _bites("touch outside", vol, it, conn, fill=321.5), name


def test_defect_negative_zero_not_masked():
    assert _bites("negative zero", F.value_case("negative zero"), 3) and _bites("negative zero", F.value_case("negative zero"), 0, fill=5.0)


@pytest.mark.parametrize("X", F.EDGE_X)
def test_defect_cross_for_connectivity_26(X):
    for it in (1, 2, 3, 7):
        for side in F.EDGE_SIDES:
            assert _bites("cross for 26", F.edge_case(X, it, side), it), (X, it, side)


def test_checker_rejects_plain_mistakes():
    """A second value inside the mask, a finite fill where NaN is due, a NaN where a value is due, the sign of a zero outside."""
    vol = F.value_case("plain")
    ref = _ref(vol, 3, 26)
    good = F.fill_restated(vol)
    mask = ref[0].numpy()
    at = tuple(np.argwhere(mask)[3])
    bad = good.copy()
    bad[at] = np.nextafter(bad[at], np.float32(0))
    assert _rejected(bad, vol, ref, "mean", "two values")
    assert _rejected(good, vol, (ref[0], float("nan"), ref[2]), "mean", "finite for NaN")
    assert _rejected(np.where(mask, np.float32(np.nan), vol), vol, ref, "mean", "NaN for finite")
    vz = F.value_case("subnormals")
    rz = _ref(vz, 0, 26)
    flushed = F.fill_restated(vz, None, 0)
    flushed[3, 4, 20] = 0.0
    assert _rejected(flushed, vz, rz, "mean", "a flushed subnormal")
