"""GPU: the bit-mask overhang fill (csrc/fill.hip: mask0_kernel, dilate_x_kernel, dilate_outer_kernel, dilate_cross_kernel,
shell_kernel, finalize_kernel, apply_fill_kernel) against the float64 reference (oracle/reference_f64.py: fill_overhang_f64).

The mask must be the reference's bit for bit, a voxel outside it the input bit for bit, a constant fill the constant bit for bit,
and a mean fill within ``2^-24 |fill| + n 2^-52 kappa`` of the float64 mean: the bound is derived at the head of tests/fill_cases.py,
which also holds the inputs; tests/test_fill_reference.py shows on the CPU that every input keeps the bound at one or two float32
ulps, that a numpy restatement of the kernels' addressing passes, and that nine planted defects do not.

What runs here and nowhere else under a comparison: the second and later 2048-voxel chunks of a row with all four row
alignments and the group that straddles into the next chunk's first word; two, four and 130 units per wavefront (the in-loop
prefetch); the grid-stride loops of mask0, dilate_x and the shell sum (the wide walk) and of dilate_outer and dilate_cross, where the
loop's second pass begins at other word counts (the rows walk); finalize_kernel's eight-wide loop; 2, 7 and 31
dilations; the cross element at word, row and plane edges; -0.0, subnormals, signed and non-finite data.  The properties that
make an input reach its code are asserted with the device's own CU count.  Every case prints one ``F64 fill ...`` line (``-s``).
"""

import functools

import numpy as np
import pytest
import torch

import deskew_cases as D
import fill_cases as F
from oracle import reference_f64 as R

pytestmark = pytest.mark.gpu

SMALL = F.small_cases()
SWITCHES = ("BH_DESKEW_CFG", "BH_DESKEW_PERS", "BH_DESKEW_ONEPASS", "BH_DESKEW_ROWS_KERNEL")


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _run(gpu, vol, fill, it, conn):
    from biahub_amd.deskew import fill_overhang

    t = vol if isinstance(vol, torch.Tensor) else torch.from_numpy(vol).to(gpu)
    return fill_overhang(t, None if fill == "mean" else fill, it, conn)


def _check_small(gpu, cases):
    """Each case's volume once, its reference once (on the CPU: the volumes are small), every fill of the case on the GPU."""
    worst_of_all = 0.0
    for name, build, it, conn, fills in cases:
        vol = build()
        ref = R.fill_overhang_f64(vol, None, it, conn)
        F.assert_input_ok(ref, vol.size, name)
        for fill in fills:
            worst = F.assert_fill_close(_run(gpu, vol, fill, it, conn), vol, F.with_fill(ref, fill), fill, name)
            print(f"F64 fill {name} {vol.shape} fill {fill}: {worst:.3f} x 2^-24 |fill| "
                  f"(bound {F.fill_tolerance(ref[1], ref[2], vol.size) / (F.U * abs(ref[1])):.3f})")
            worst_of_all = max(worst_of_all, worst)
    return worst_of_all


# ----------------------------------------------------------------------------- word and row edges
@pytest.mark.parametrize("X", F.EDGE_X)
def test_fill_word_and_row_edges_vs_float64(gpu, X):
    """Rows that end at, one before and one after a 32-bit mask word and the 64-bit row padding, single zeros at the first and last
    bit of words, on first, inner and last rows and planes, and at the row end beside the next row's start: 0, 1, 2, 3 and 7 dilations
    with the cube and the cross, a mean fill and a negative constant."""
    cases = [c for c in SMALL if c[0].startswith(f"edge X={X} ")]
    assert len(cases) == len(F.EDGE_ITERATIONS) * len(F.EDGE_SIDES) * 2
    _check_small(gpu, cases)


def test_fill_31_dilations_and_32_refused(gpu):
    """The largest radius the host accepts — the shifts by 32 - s reach 1 — with both elements; 32 is refused on the host with its
    message, nothing runs, and the context is as good as before."""
    cases = [c for c in SMALL if c[0].startswith("31 iterations")]
    assert len(cases) == 2
    _check_small(gpu, cases)
    vol = F.thirty_one_case()
    with pytest.raises(ValueError, match=r"dilation_iterations must be in \[0,31\], got 32"):
        _run(gpu, vol, "mean", 32, 26)
    _check_small(gpu, cases[:1])


def test_legacy_entry_on_an_edge_volume(gpu):
    """``_fill_overhang_with_mean`` (numpy in, numpy out, the cross) at a volume whose rows end one voxel after a mask word."""
    from biahub_amd.deskew import _fill_overhang_with_mean

    vol = F.edge_case(65, 2, "hi")
    ref = R.fill_overhang_f64(vol, None, 2, 6)
    F.assert_input_ok(ref, vol.size, "legacy")
    worst = F.assert_fill_close(_fill_overhang_with_mean(vol, dilation_iterations=2), vol, ref, "mean", "legacy entry")
    print(f"F64 fill legacy entry {vol.shape}: {worst:.3f} x 2^-24 |fill|")


# ----------------------------------------------------------------------------- chunk edges
@pytest.mark.parametrize("X", F.CHUNK_X)
def test_fill_chunk_edges_vs_float64(gpu, X):
    """Rows of 2047 .. 6145 voxels: one to four 2048-voxel units per row, at odd X with all four row alignments; zeros on both sides
    of x = 2048 and 4096, a run across the first, a whole row, the last four and five voxels, random zeros.  0 and 3 dilations of
    the cube with a mean and a constant fill, 3 of the cross."""
    shape = (3, 7, X)
    if X % 2:
        assert F.row_alignments(shape) == {0, 1, 2, 3}
    if X > 2048:
        assert -(-X // 2048) >= 2
    cases = [c for c in SMALL if c[0].startswith(f"chunk X={X} ")]
    assert len(cases) == 3
    _check_small(gpu, cases)


# ----------------------------------------------------------------------------- the walks
def test_fill_walk_two_units_per_wavefront(gpu):
    """More one-unit rows than the device has wavefronts in apply_fill_kernel's grid: each wavefront walks two consecutive units
    and requests the second one's mask word before it stores the first."""
    cus = _cus(gpu)
    assert F.WALK_NARROW[2] <= 2048 and F.units_per_wavefront(F.WALK_NARROW, cus) >= 2, cus
    assert F.row_alignments(F.WALK_NARROW) == {0, 1, 2, 3}
    _check_small(gpu, [c for c in SMALL if c[0] == "narrow walk"])


def test_fill_walk_grid_stride_loops(gpu):
    """33.6 M voxels, once: more mask words than dilate_x_kernel's grid has threads, more word pairs than shell_kernel's and
    mask0_kernel's grids cover, two chunks per row and about four units per wavefront across them, all four alignments.  Input and
    reference are made on the device.  (dilate_outer_kernel, where a thread owns a pair of words, makes one pass here: the rows walk
    below is its input.)"""
    cus = _cus(gpu)
    shape = F.WALK_WIDE
    words = F.mask_words(shape)
    assert words > F.dilation_threads(cus), (words, cus)   # dilate_x_kernel: a thread owns one word
    assert words // 2 > 8 * cus * 256, (words, cus)        # shell_kernel: a thread owns a pair of words
    assert words // 2 > 8 * cus * 4, (words, cus)          # mask0_kernel: a wavefront owns a pair
    assert shape[2] > 2048 and F.units_per_wavefront(shape, cus) >= 2, cus
    assert F.row_alignments(shape) == {0, 1, 2, 3}
    vol = F.walk_wide_case(gpu)
    ref = R.fill_overhang_f64(vol, None, 3, 26)
    F.assert_input_ok(ref, vol.numel(), "wide walk")
    worst = F.assert_fill_close(_run(gpu, vol, "mean", 3, 26), vol, ref, "mean", "wide walk")
    print(f"F64 fill wide walk {shape} fill mean: {worst:.3f} x 2^-24 |fill| "
          f"(bound {F.fill_tolerance(ref[1], ref[2], vol.numel()) / (F.U * abs(ref[1])):.3f}; {int(ref[0].sum())} voxels masked)")


@pytest.mark.parametrize("conn,words_per_thread", [(26, 2), (6, 1)], ids=["cube: dilate_outer", "cross: dilate_cross"])
def test_fill_walk_dilation_second_pass(gpu, conn, words_per_thread):
    """1 064 960 rows of two mask words (2.1 M voxels): more word PAIRS than the dilation grid has threads, so the y and z passes of
    dilate_outer_kernel make a second pass (connectivity 26), and more words, so dilate_cross_kernel does (6); zeros sit, and the
    mask grows, in the rows that only the second pass writes.  130 units per wavefront in apply_fill_kernel."""
    cus = _cus(gpu)
    shape = F.WALK_ROWS
    assert F.mask_words(shape) // words_per_thread > F.dilation_threads(cus), (F.mask_words(shape), cus)
    vol = torch.from_numpy(np.array(F.walk_rows_case())).to(gpu)
    ref = R.fill_overhang_f64(vol, None, 3, conn)
    F.assert_input_ok(ref, vol.numel(), "rows walk")
    F.assert_second_pass_reached(vol, ref[0], cus, words_per_thread, "rows walk")
    worst = F.assert_fill_close(_run(gpu, vol, "mean", 3, conn), vol, ref, "mean", f"rows walk conn={conn}")
    print(f"F64 fill rows walk conn={conn} {shape} fill mean: {worst:.3f} x 2^-24 |fill| "
          f"(bound {F.fill_tolerance(ref[1], ref[2], vol.numel()) / (F.U * abs(ref[1])):.3f}; {int(ref[0].sum())} voxels masked)")


# ----------------------------------------------------------------------------- values
@pytest.mark.parametrize("what", F.VALUE_CASES)
def test_fill_values_vs_float64(gpu, what):
    """-0.0 is masked and comes back as the fill; 1e-45, -1e-45 and 1e-38 are not and come back unchanged; signed data; no zeros: the
    input bit for bit; all zeros and a NaN outside the mask: NaN, as the reference; a NaN or an infinity in the shell: NaN where
    the reference's mean is finite (the known divergence: sum(all) - sum(shell) cannot undo it); a negative constant throughout."""
    vol = F.value_case(what)
    ref = R.fill_overhang_f64(vol, None, 3, 26)
    if F.checked_values(what):
        F.assert_input_ok(ref, vol.size, what)
    if what in F.NONFINITE_SHELL:
        assert np.isfinite(ref[1])
        ref = (ref[0], float("nan"), ref[2])
    got = _run(gpu, vol, "mean", 3, 26)
    worst = F.assert_fill_close(got, vol, ref, "mean", what)
    print(f"F64 fill values [{what}] fill mean: {worst:.3f} x 2^-24 |fill|")
    F.assert_fill_close(_run(gpu, vol, -7.25, 3, 26), vol, F.with_fill(ref, -7.25), -7.25, what + ", constant")
    g = got.cpu().numpy()
    if what == "negative zero":
        assert g[3, 4, 30] == g[1, 2, 7] and g[3, 4, 30] != 0
    if what == "subnormals":
        assert [g[3, 4, 30], g[3, 4, 20], g[0, 0, 39]] == [np.float32(1e-45), np.float32(-1e-45), np.float32(1e-38)]
    if what == "no zeros":
        assert np.array_equal(g.view(np.int32), vol.view(np.int32))
    if what == "all zeros":
        assert np.isnan(g).all()


# ----------------------------------------------------------------------------- through the deskew
@functools.lru_cache(maxsize=2)
def _deskew_input(gpu, shape, zb):
    vol = D.bead_volume(shape)
    return torch.from_numpy(np.array(D.zero_block(vol) if zb else vol)).to(gpu)


@functools.lru_cache(maxsize=2)
def _deskew_reference(gpu, shape, angle, ratio, N, zb):
    """deskew_f64 on the GPU with the mean fill, once per input, left unchanged."""
    return R.deskew_f64(_deskew_input(gpu, shape, zb), angle, ratio, True, N, "mean")


def _deskew(gpu, monkeypatch, case, fill, zb=False, **switches):
    from biahub_amd.deskew import deskew_fill_path, fast_deskew_zyx

    shape, angle, ratio, N = case
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv("BH_DESKEW_" + name, str(value))
    out = fast_deskew_zyx(_deskew_input(gpu, shape, zb), angle, ratio, True, N, fill)
    path = deskew_fill_path(gpu)
    for name in switches:
        monkeypatch.delenv("BH_DESKEW_" + name)
    return out, path


def _check_deskew(gpu, name, got, case, fill, zb=False):
    shape, angle, ratio, N = case
    V, M, mask, mean = _deskew_reference(gpu, shape, angle, ratio, N, zb)
    worst = D.assert_deskew_close(got, (V, M, mask, mean if fill == "mean" else float(fill)), N, name, fill=fill)
    off = abs(float(got[mask][0]) - mean) / (F.U * abs(mean)) if fill == "mean" else 0.0
    print(f"F64 fill deskew {name} {shape} N{N} -> {tuple(V.shape)} fill {fill}: {off:.3f} x 2^-24 |fill| (bound {N + 4}), "
          f"voxels {worst:.2f} u M (bound {N + 3})")


@pytest.mark.parametrize("shape,angle,ratio,N,Xp", F.DESKEW_WIDE, ids=[f"Xp={c[4]}" for c in F.DESKEW_WIDE])
def test_fill_behind_the_deskew_second_chunk_vs_float64(gpu, monkeypatch, shape, angle, ratio, N, Xp):
    """Deskewed rows of 2073 .. 2076 voxels, one of each residue mod 4: the mask prologue's deskew kernel writes 66-word mask rows and
    apply_fill_kernel takes a second chunk behind it (path 0).  At Xp = 2073 also the one-pass fill (path 1), a constant fill, and
    an input with a block of exact zeros, which sends the one-pass fill through the conditional mask pipeline (path 2)."""
    from biahub_amd.deskew import get_deskewed_data_shape

    case = (shape, angle, ratio, N)
    out_shape = get_deskewed_data_shape(shape, angle, ratio, True, N)[0]
    assert out_shape[2] == Xp > 2048 and 2 * (-(-Xp // 64)) == 66
    if Xp % 2:
        assert F.row_alignments(tuple(out_shape)) == {0, 1, 2, 3}
    got, path = _deskew(gpu, monkeypatch, case, "mean", ONEPASS=0)
    assert path == 0
    _check_deskew(gpu, "mask prologue", got, case, "mean")
    if Xp == F.DESKEW_WIDE[0][4]:
        got, path = _deskew(gpu, monkeypatch, case, "mean")
        assert path == 1
        _check_deskew(gpu, "one pass", got, case, "mean")
        got, path = _deskew(gpu, monkeypatch, case, 321.5, ONEPASS=0)
        assert path == 0
        _check_deskew(gpu, "mask prologue", got, case, 321.5)
        got, path = _deskew(gpu, monkeypatch, case, "mean", zb=True)
        assert path == 2
        _check_deskew(gpu, "data zeros, conditional pipeline", got, case, "mean", zb=True)


def test_fill_finalize_eight_wide_partials_vs_float64(gpu, monkeypatch):
    """A mask-prologue deskew on the 32 x 64 tiles of configuration 4 hands finalize_kernel one block sum per workgroup — 11 200, more
    than 8 x 1024: each of its 1024 threads runs the eight-wide body once, then the single-step loop twice, the threads below 960 a third
    time."""
    shape, angle, ratio, N, cfg = F.DESKEW_PARTIALS
    assert D.tile_workgroups(shape, angle, ratio, N, cfg) >= 8 * F.FIN_NT + 1
    assert D.cfg_lds(shape, D.geometry(shape, angle, ratio, N), N, cfg) <= D.LDS_MAX
    case = (shape, angle, ratio, N)
    got, path = _deskew(gpu, monkeypatch, case, "mean", CFG=cfg, PERS=0, ONEPASS=0)
    assert path == 0
    _check_deskew(gpu, f"cfg {cfg} forced, {D.tile_workgroups(shape, angle, ratio, N, cfg)} partials", got, case, "mean")
