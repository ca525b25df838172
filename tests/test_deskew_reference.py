"""CPU: the float64 reference of the deskew (oracle/reference_f64.py: deskew_f64), the bound the GPU kernels are held to in
tests/test_gpu_deskew_f64.py (tests/deskew_cases.py derives it), and the claims of the cases table.

The reference is held to a brute-force triple loop; the float32 numpy oracle and libbhcore's host deskew (``bh_host_deskew``,
which needs no GPU and restates the kernels' operation order) are held to the bound at every input of the GPU tests; the
restated launch rules are shown to select the configuration each case names; and planted defects show that the bound bites where
``rel_err <= 1e-5`` does not.

Volumes with more than 12 input columns are cut to their first 12 here (the x axis of the input is the y' axis of the output and
independent in the transform: the geometry, the positions and the fill's pattern along a and x' are those of the whole volume),
so the numpy oracle stays quick.  Every case prints one ``F64 deskew ...`` line (``-s`` shows them; DESIGN.md §3.1 keeps the range).
"""

import numpy as np
import pytest
import torch

import deskew_cases as D
from conftest import rel_err
from oracle import oracle_np as O
from oracle import reference_f64 as R

SLAB = 12
INPUTS = D.gpu_inputs()


def _id(c):
    shape, angle, ratio, N, keep, dtype, fill, zb = c
    return f"{shape} {angle} {ratio} N{N} {dtype} fill {fill}{'' if keep else ' no overhang'}{' zero block' if zb else ''}"


def _volume(shape, dtype, zb):
    vol = D.bead_volume(shape)[:, :, :SLAB]
    vol = D.as_dtype(D.zero_block(vol) if zb else vol, dtype)
    return np.array(vol)   # contiguous, writable


# ----------------------------------------------------------------------------- the reference is the definition
def brute_force(raw, angle, ratio, keep, N):
    """out[a, y', x'] = (1/N) sum_k lerp(in[:, Y - 1 - min(aN + k, Y - 1), X - 1 - y'], ix(x', aN + k)), one voxel at a time."""
    raw = np.asarray(raw, np.float64)
    Z, Y, X = raw.shape
    (_, _, Xp), _ = O.get_deskewed_data_shape(raw.shape, angle, ratio, keep)
    Za = -(-Y // N)
    V, M = np.zeros((Za, X, Xp)), np.zeros((Za, X, Xp))
    for a in range(Za):
        for k in range(N):
            ix = O.deskew_coords(Z, Y, Xp, angle, ratio, a * N + k)
            yin = Y - 1 - min(a * N + k, Y - 1)
            for xo in range(Xp):
                fl = np.floor(ix[xo])
                w1, w0 = float(np.float32(ix[xo] - fl)), float(np.float32((fl + np.float32(1.0)) - ix[xo]))
                z0 = int(fl)
                for yo in range(X):
                    v0 = raw[z0, yin, X - 1 - yo] if 0 <= z0 < Z else 0.0
                    v1 = raw[z0 + 1, yin, X - 1 - yo] if 0 <= z0 + 1 < Z else 0.0
                    V[a, yo, xo] += v0 * w0 + v1 * w1
                    M[a, yo, xo] += abs(v0) * w0 + abs(v1) * w1
    return V / N, M / N


@pytest.mark.parametrize("shape,angle,ratio,N,keep", [((6, 5, 3), 36.17, 0.371, 1, True), ((7, 5, 2), 30.0, 0.9, 2, True),
                                                      ((9, 4, 3), 45.0, 0.5, 3, False), ((5, 2, 2), 36.17, 0.371, 4, True)])
def test_reference_equals_the_triple_loop(shape, angle, ratio, N, keep):
    rng = np.random.default_rng(sum(shape))
    for raw in (rng.integers(1, 60000, shape).astype(np.float32), (rng.random(shape) * 200 - 100).astype(np.float32)):
        V, M, mask, fill = R.deskew_f64(raw, angle, ratio, keep, N)
        wantV, wantM = brute_force(raw, angle, ratio, keep, N)
        assert mask is None and fill is None and V.dtype == torch.float64 and tuple(V.shape) == wantV.shape
        assert np.abs(V.numpy() - wantV).max() <= 1e-13 * np.abs(wantV).max()
        assert np.abs(M.numpy() - wantM).max() <= 1e-13 * np.abs(wantM).max()
        assert np.array_equal(M.numpy() == 0, wantM == 0)


def test_reference_fill_is_the_oracles_fill():
    """The mask is ``V == 0`` dilated as ``oracle_np.dilate_zero_mask`` does; the fill the float64 mean of the rest or the constant;
    ``keep_overhang=False`` and a fill of 0 never fill; the filled volume is the float32 oracle's to float32 rounding."""
    raw = D.zero_block(D.bead_volume((20, 9, 8)))   # a writable copy
    V, M, mask, fill = R.deskew_f64(raw, 36.17, 0.371, True, 2, "mean")
    want_mask = O.dilate_zero_mask(V.numpy() == 0, 3)
    assert np.array_equal(mask.numpy(), want_mask) and 0 < want_mask.sum() < want_mask.size
    assert fill == pytest.approx(V.numpy()[~want_mask].mean(), rel=1e-14)
    filled = torch.where(mask, fill, V).numpy()
    assert rel_err(filled, O.fast_deskew_zyx(raw, 36.17, 0.371, True, 2, "mean")) <= 1e-6
    assert R.deskew_f64(raw, 36.17, 0.371, True, 2, 7.5)[3] == 7.5
    assert R.deskew_f64(raw, 36.17, 0.371, True, 2, 0)[2] is None
    assert R.deskew_f64(raw, 36.17, 0.371, False, 2, "mean")[2] is None
    m = np.random.default_rng(1).random((5, 6, 7)) < 0.05
    assert np.array_equal(R.dilate_mask(torch.from_numpy(m), 3).numpy(), O.dilate_zero_mask(m, 3))
    assert np.array_equal(R.dilate_mask(torch.from_numpy(m), 1).numpy(), O.dilate_zero_mask(m, 1))


# ----------------------------------------------------------------------------- float32 implementations under the bound
@pytest.mark.parametrize("case", INPUTS, ids=_id)
def test_oracle_and_host_deskew_within_the_bound(case, lib_built):
    """``oracle_np.fast_deskew_zyx`` and ``bh_host_deskew`` against ``deskew_f64`` at an input of the GPU tests: the per-voxel bound,
    exact zeros where M == 0 (and, without data zeros, nowhere else), the fill rule."""
    from biahub_amd.deskew import _fast_deskew_czyx

    shape, angle, ratio, N, keep, dtype, fill, zb = case
    vol = _volume(shape, dtype, zb)
    ref = R.deskew_f64(vol, angle, ratio, keep, N, fill)
    oracle = O.fast_deskew_zyx(vol, angle, ratio, keep, N, fill)
    host = _fast_deskew_czyx(vol[None], device="cpu", ls_angle_deg=angle, px_to_scan_ratio=ratio, keep_overhang=keep,
                             average_n_slices=N, overhang_fill=fill)[0]
    wo = D.assert_deskew_close(oracle, ref, N, "oracle " + _id(case), fill=fill)
    wh = D.assert_deskew_close(host, ref, N, "host " + _id(case), fill=fill)
    print(f"F64 deskew {_id(case)}: oracle {wo:.2f} host {wh:.2f} u M (bound {N + 3})")
    if fill == 0 and not zb:
        assert np.array_equal(oracle == 0, ref[1].numpy() == 0) and np.array_equal(host == 0, ref[1].numpy() == 0)


@pytest.mark.parametrize("shape,angle,ratio,N,keep", D.CPU_GEOMETRIES)
def test_oracle_position_under_the_bound(shape, angle, ratio, N, keep, lib_built):
    """Six small geometries, N = 1, 2, 3, 4, 5, 7, bead volumes and their signed variants, uncut: where the float32 oracle, the
    host deskew and the float32 restatement of tests/deskew_cases.py sit in units of u M.  Exact zeros agree in every case."""
    from biahub_amd.deskew import _host_deskew_zyx

    for dtype in ("f32", "f32s", "i16"):
        vol = np.array(D.as_dtype(D.bead_volume(shape), dtype))
        ref = R.deskew_f64(vol, angle, ratio, keep, N)
        got = {"oracle": O.fast_deskew_zyx(vol, angle, ratio, keep, N), "host": _host_deskew_zyx(vol, angle, ratio, keep, N),
               "restated": D.deskew_f32(vol, angle, ratio, keep, N)}
        worst = {k: D.assert_deskew_close(v, ref, N, f"{k} {shape} {dtype}") for k, v in got.items()}
        for v in got.values():
            assert np.array_equal(v == 0, ref[1].numpy() == 0)
        print(f"F64 deskew {shape} N{N} {dtype}: " + " ".join(f"{k} {w:.2f}" for k, w in worst.items()) + f" u M (bound {N + 3})")


def test_host_deskew_refuses_an_unknown_dtype_code(lib_built):
    """A dtype code that is none of the four: ``bh_host_deskew`` returns BH_ERR_INVALID with the message naming the code, at
    the smallest volume."""
    import ctypes as C

    from biahub_amd import _lib
    from biahub_amd.deskew import get_deskewed_data_shape

    shape, angle, ratio = (2, 1, 1), 36.17, 0.371
    vol = np.ones(shape, np.float32)
    out = np.zeros(get_deskewed_data_shape(shape, angle, ratio, True)[0], np.float32)
    for code in (4, -1, 99):
        assert code not in (_lib.DT_F32, _lib.DT_U16, _lib.DT_U8, _lib.DT_I16)
        status = _lib.load().bh_host_deskew(vol.ctypes.data_as(C.c_void_p), code, *shape, angle, ratio, 1, 1, _lib.FILL_NONE, 0.0,
                                            out.ctypes.data_as(C.c_void_p), None, 1)
        assert status == _lib.BH_ERR_INVALID and _lib.last_error() == f"unsupported input dtype code {code}"
        with pytest.raises(ValueError, match=f"unsupported input dtype code {code}"):
            _lib.check(status)


# ----------------------------------------------------------------------------- the cases table
def test_cases_select_the_configuration_they_name():
    """``launch_deskew``'s rule, restated, over the natural-selection geometries: the named configuration without a fill and with
    the mask prologue; the one-pass fill (whose order starts at configuration 1) takes 1 where the table says 0 and the same
    elsewhere.  The forced geometries fit 160 KiB in every configuration; the refusal case does not in configuration 0."""
    for shape, angle, ratio, N, cfg in D.NATURAL:
        assert D.selected_cfg(shape, angle, ratio, N)[0] == cfg, (shape, N)
        assert D.selected_cfg(shape, angle, ratio, N, one_pass=True)[0] == max(cfg, 1), (shape, N)
        assert D.persistent(shape, angle, ratio, N) is None          # X is no multiple of 64: the tile kernel, always
    assert {c[4] for c in D.NATURAL} == {0, 1, 2, 3, 4}
    assert D.selected_cfg(*D.NATURAL[1][:4]) == (1, D.NATURAL_LDS_CFG1) and 64 * 1024 < D.NATURAL_LDS_CFG1 <= D.TWO_PER_CU
    assert D.NATURAL[2][3] > 4 and D.NATURAL[4][3] > 4                # the generic-N kernels
    shape, angle, ratio, N, _ = D.NATURAL[4]
    assert D.cfg_lds(shape, D.geometry(shape, angle, ratio, N), N, 0) > D.LDS_MAX
    for shape, angle, ratio in D.FORCED_GEOMETRIES:
        for N in D.FORCED_N:
            geo = D.geometry(shape, angle, ratio, N)
            assert all(D.cfg_lds(shape, geo, N, c) <= D.LDS_MAX for c in range(5))
    assert sorted(g[0][2] % 64 == 0 for g in D.FORCED_GEOMETRIES) == [False, False, False, True]
    assert [g[0][2] % 4 == 0 for g in D.FORCED_GEOMETRIES] == [False, False, True, True]


def test_forced_cases_cover_every_pair():
    cases = D.forced_cases()
    assert len(cases) <= 30
    for N in D.FORCED_N:
        assert {c[2] for c in cases if c[1] == N} == set(D.FORCED_DTYPES)
        assert {c[3] for c in cases if c[1] == N} == set(D.FORCED_FILLS)
        assert {c[0] for c in cases if c[1] == N} == set(range(len(D.FORCED_GEOMETRIES)))
    for g in range(len(D.FORCED_GEOMETRIES)):
        assert {c[2] for c in cases if c[0] == g} == set(D.FORCED_DTYPES)
        assert {c[3] for c in cases if c[0] == g} == set(D.FORCED_FILLS)
    for d in D.FORCED_DTYPES:
        assert {c[3] for c in cases if c[2] == d} == ({0, 321.5} if d == "i16" else set(D.FORCED_FILLS))
    # int16 with a constant fill: no cancellation at that input, so the reference's mask V == 0 is the geometric one (M == 0)
    g, N, dtype, fill = D.INT16_CONSTANT
    shape, angle, ratio = D.FORCED_GEOMETRIES[g]
    V, M, mask, _ = R.deskew_f64(np.array(D.as_dtype(D.bead_volume(shape), dtype)), angle, ratio, True, N, fill)
    assert dtype == "i16" and bool(((V == 0) == (M == 0)).all()) and bool((V < 0).any()) and bool((V > 0).any())
    assert 0 < int(mask.sum()) < mask.numel()


def test_persistent_cases_walk_many_tiles():
    """ntiles as the table claims; every workgroup of a 256-CU device that gets tiles gets at least three consecutive ones, and
    the geometries named for it have 3 x 256 tiles or more; overhang tiles in runs; the declined geometry is declined for its LDS
    alone; the Xp edges are what they say."""
    for shape, angle, ratio, N, ntiles in D.PERSISTENT:
        got = D.persistent(shape, angle, ratio, N)
        assert got is not None and got[0] == ntiles and got[2] + 256 <= D.LDS_MAX
        assert -(-ntiles // D.CUS) >= 3
        assert got[1] >= ntiles // 4                                  # a good part of the walk is overhang tiles
    assert sum(c[4] >= 3 * D.CUS for c in D.PERSISTENT) >= 3
    assert any(c[0][1] % c[3] == 0 for c in D.PERSISTENT) and any(c[0][1] % c[3] for c in D.PERSISTENT)
    shape, angle, ratio, N = D.PERSISTENT_DECLINED
    assert shape[2] % 64 == 0 and N <= 4 and D.persistent(shape, angle, ratio, N) is None
    assert D.cfg_lds(shape, D.geometry(shape, angle, ratio, N), N, 0) == 242320    # per buffer; two are needed
    xp = {what: D.geometry(shape, angle, ratio, N, keep)[1] for shape, angle, ratio, N, keep, what in D.EDGES}
    assert [v for k, v in xp.items() if k.startswith("Xp")] == [256, 257]
    for shape, angle, ratio, N, keep, what in D.EDGES:
        if what.startswith("Xp"):
            assert D.persistent(shape, angle, ratio, N, keep) is not None


# ----------------------------------------------------------------------------- the bound bites
MUTANT_INPUTS = [((48, 37, 70), 36.17, 0.371, 2), ((24, 401, 128), 36.17, 0.371, 3), ((31, 50, 66), 45.0, 0.9, 4)]


@pytest.mark.parametrize("shape,angle,ratio,N", MUTANT_INPUTS)
def test_planted_defects_fail_the_bound(shape, angle, ratio, N):
    """The float32 restatement passes; each planted defect fails.  The bias also passes ``rel_err <= 1e-5`` against the float32
    oracle, the assertion of tests/test_gpu_parity.py (asserted here); the wrong mean stands at 8e-4 .. 4e-3 of the volume's
    maximum (printed), which that assertion catches too.  A NaN or an infinity in a few voxels fails as well, with and without
    a fill."""
    vol = _volume(shape, "f32", False)
    ref = R.deskew_f64(vol, angle, ratio, True, N, "mean")
    plain = (ref[0], ref[1], None, None)
    oracle = O.fast_deskew_zyx(vol, angle, ratio, True, N, "mean")
    good = D.deskew_f32(vol, angle, ratio, True, N)
    good_filled = D.deskew_f32(vol, angle, ratio, True, N, "mean")
    D.assert_deskew_close(good, plain, N, "restated")
    D.assert_deskew_close(good_filled, ref, N, "restated, mean fill", fill="mean")

    biased = D.deskew_f32(vol, angle, ratio, True, N, 0, defect="bias")
    assert rel_err(biased, O.fast_deskew_zyx(vol, angle, ratio, True, N)) <= 1e-5
    with pytest.raises(AssertionError, match="outside"):
        D.assert_deskew_close(biased, plain, N, "bias")

    assert shape[1] % N      # a ragged last slab
    with pytest.raises(AssertionError, match="outside"):
        D.assert_deskew_close(D.deskew_f32(vol, angle, ratio, True, N, 0, defect="shear"), plain, N, "shear")

    assert bool((~ref[2]).any())
    wrong_mean = D.deskew_f32(vol, angle, ratio, True, N, "mean", defect="mean")
    with pytest.raises(AssertionError):
        D.assert_deskew_close(wrong_mean, ref, N, "mean over the undilated mask", fill="mean")
    print(f"F64 deskew mutant mean {shape}: rel_err against the oracle {rel_err(wrong_mean, oracle):.2e}")

    outside = np.flatnonzero(~ref[2].numpy().ravel())
    for bad_value in (np.nan, np.inf):
        for out, r, fill in ((good, plain, 0), (good_filled, ref, "mean")):
            broken = out.copy()
            broken.ravel()[outside[:: max(1, outside.size // 10)]] = bad_value
            with pytest.raises(AssertionError, match="outside"):
                D.assert_deskew_close(broken, r, N, f"{bad_value} in ten voxels", fill=fill)
    with pytest.raises(AssertionError):     # and inside the fill
        D.assert_deskew_close(np.where(ref[2].numpy(), np.float32(np.nan), good_filled), ref, N, "NaN fill", fill="mean")


def test_positions_in_float64_rounded_once_are_another_operator():
    """Not the contract: sample positions evaluated in float64 and rounded once differ from the reference's
    float32 operation order by an ulp of the position, which moves the weights by ~1e-6 — far outside the bound."""
    for shape, angle, ratio, N in MUTANT_INPUTS[:2]:
        vol = _volume(shape, "f32", False)
        V, M, _, _ = R.deskew_f64(vol, angle, ratio, True, N)
        worst, _ = D.deskew_errors(torch.from_numpy(D.deskew_f32(vol, angle, ratio, True, N, coords64=True)), V, M)
        print(f"F64 deskew positions in float64 {shape} N{N}: {worst:.1f} u M (bound {N + 3})")
        assert worst > N + 3
