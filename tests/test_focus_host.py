"""CPU: the host side of focus finding — bh_focus_band_table against the float64 restatement's mask
(tests/focus_ref.py), argument validation of both entry points without a GPU, and the reference's z chain
(estimate_stabilization.py:900-1220) on hand-computed values."""

import ctypes as C
import json
import warnings

import numpy as np
import pytest
from click.testing import CliRunner

import focus_ref as R
from conftest import GOLDEN

META = json.loads((GOLDEN / "focus_cases.json").read_text())
CASES = META["cases"]


def _full_mask(Y, X, lo, hi):
    """The table's half-spectrum intervals expanded to the full plane: bin (ky, kx) and its mirror (-ky, -kx)."""
    m = np.zeros((Y, X), dtype=bool)
    for ky in range(Y):
        for kx in range(lo[ky], hi[ky]):
            m[ky, kx] = True
            m[(Y - ky) % Y, (X - kx) % X] = True
    return m


PLANES = sorted({(c["shape"][1], c["shape"][2], c["pixel_size"]) for c in CASES}) + [(800, 800, 0.1494)]


@pytest.mark.parametrize("Y,X,pixel", PLANES, ids=[f"{y}x{x}_p{p}" for y, x, p in PLANES])
def test_band_table_equals_the_restatement_mask(lib_built, Y, X, pixel):
    from biahub_amd.focus import band_table

    lo, hi, n = band_table(Y, X, pixel, R.NA_DET, R.LAMBDA_ILL)
    ref = R.band_mask(Y, X, pixel)
    assert lo.shape == hi.shape == (Y,) and (lo <= hi).all() and hi.max() <= X // 2 + 1
    assert np.array_equal(_full_mask(Y, X, lo, hi), ref)
    assert n == int(ref.sum()) and n > 0


def test_golden_records_the_band_sizes(lib_built):
    from biahub_amd.focus import band_table

    assert {c["name"] for c in CASES} >= {"min16_f32", "u16_z2"} and len({c["pixel_size"] for c in CASES}) >= 2
    for c in CASES:
        assert band_table(c["shape"][1], c["shape"][2], c["pixel_size"], META["NA_det"], META["lambda_ill"], META["midband_fractions"])[2] == c["n_bins"]


def test_band_without_bins(lib_built):
    from biahub_amd.focus import band_table

    # 16 x 16 at 0.1494 um: the first non-zero radius is 1 / (16 * 0.1494) = 0.418 cycles/um; the band (0.054, 0.0594) holds no bin
    lo, hi, n = band_table(16, 16, 0.1494, R.NA_DET, R.LAMBDA_ILL, (0.01, 0.011))
    assert n == 0 and np.array_equal(lo, hi)
    assert not R.band_mask(16, 16, 0.1494, fractions=(0.01, 0.011)).any()


def test_invalid_arguments_are_refused_without_a_device(lib_built):
    from biahub_amd import _lib

    lib = _lib.load()
    Y = X = 16
    lo, hi, n = (C.c_int32 * 64)(), (C.c_int32 * 64)(), C.c_int64()
    good_t = dict(Y=Y, X=X, pixel=0.1494, na=1.35, lam=0.5, flo=0.125, fhi=0.25, lo=lo, hi=hi, n=C.byref(n))

    def table(**kw):
        a = dict(good_t, **kw)
        return lib.bh_focus_band_table(a["Y"], a["X"], a["pixel"], a["na"], a["lam"], a["flo"], a["fhi"], a["lo"], a["hi"], a["n"])

    assert table() == _lib.BH_OK
    bad_optics = [dict(pixel=0.0), dict(pixel=-1.0), dict(pixel=float("nan")), dict(pixel=float("inf")), dict(na=0.0), dict(na=float("nan")),
                  dict(lam=0.0), dict(lam=float("inf")), dict(flo=0.25, fhi=0.25), dict(flo=0.3, fhi=0.25), dict(flo=float("nan"))]
    bad_extents = [dict(Y=15), dict(X=17), dict(Y=14), dict(X=8), dict(Y=0), dict(Y=2 ** 20, X=2 ** 20)]
    for kw in bad_optics + bad_extents + [dict(lo=None), dict(hi=None), dict(n=None)]:
        assert table(**kw) == _lib.BH_ERR_INVALID, kw
        assert _lib.last_error()

    # the device entry validates before its first device call: a block of host memory stands in for the context and the window
    fake_ctx, fake_win = C.create_string_buffer(4096), C.create_string_buffer(4096)
    power, total = (C.c_double * 4)(), C.c_double()
    good_p = dict(ctx=C.cast(fake_ctx, C.c_void_p), win=C.cast(fake_win, C.c_void_p), dt=_lib.DT_U16, Z=4, Y=Y, X=X, ps=Y * X, rs=X, pixel=0.1494,
                  na=1.35, lam=0.5, flo=0.125, fhi=0.25, mb=0, power=power, total=C.byref(total))

    def band_power(**kw):
        a = dict(good_p, **kw)
        return lib.bh_focus_band_power(a["ctx"], a["win"], a["dt"], a["Z"], a["Y"], a["X"], a["ps"], a["rs"], a["pixel"], a["na"], a["lam"],
                                       a["flo"], a["fhi"], a["mb"], a["power"], a["total"])

    bad = [dict(ctx=None), dict(win=None), dict(power=None), dict(dt=_lib.DT_F16), dict(dt=17), dict(dt=-1), dict(Z=0), dict(Z=-3),
           dict(rs=X - 1), dict(ps=Y * X - 1), dict(ps=0), dict(rs=0)] + bad_optics + bad_extents
    for kw in bad:
        assert band_power(**kw) == _lib.BH_ERR_INVALID, kw
        assert _lib.last_error()


def test_z_transforms_from_focus_indices():
    from biahub_amd.estimate_stabilization import z_transforms_from_focus

    t = z_transforms_from_focus([5, 7, 4, 0])
    assert t.shape == (4, 4, 4) and np.array_equal(t[0], np.eye(4))
    assert [m[0, 3] for m in t] == [0.0, 2.0, -1.0, -5.0]  # an empty timepoint (0) lands at 0 - 5, as in the reference
    for m in t:
        m = m.copy()
        m[0, 3] = 0
        assert np.array_equal(m, np.eye(4))
    # a leading 0: the reference is the first non-zero index, the first matrix is the identity all the same
    t = z_transforms_from_focus([0, 6, 8])
    assert [m[0, 3] for m in t] == [0.0, 0.0, 2.0]
    with pytest.raises(ValueError, match="only zeros"):
        z_transforms_from_focus([0, 0, 0])


def _write_csv(path, rows):
    path.write_text("position,time_idx,channel,focus_idx\n" + "".join(",".join(str(v) for v in r) + "\n" for r in rows))


def test_get_mean_z_positions(tmp_path):
    from biahub_amd.estimate_stabilization import get_mean_z_positions

    f = tmp_path / "positions_focus.csv"
    _write_csv(f, [("A/1/0", 1, "c", 4), ("A/1/0", 0, "c", 3), ("B/1/0", 0, "c", 6), ("B/1/0", 1, "c", 0), ("C/1/0", 0, "c", 12),
                   ("C/1/0", 1, "c", 5), ("A/1/0", 2, "c", 0), ("B/1/0", 2, "c", 0), ("C/1/0", 2, "c", 0)])
    mean = get_mean_z_positions(f, method="mean")
    median = get_mean_z_positions(f, method="median")
    assert mean[:2].tolist() == [7.0, 4.5] and np.isnan(mean[2]) and mean.shape == (3,)   # (3 + 6 + 12) / 3, (4 + 5) / 2: zeros skipped
    assert median[:2].tolist() == [6.0, 4.5] and np.isnan(median[2])
    with pytest.raises(ValueError):
        get_mean_z_positions(f, method="mode")


def test_focus_csv_merge_rule():
    from biahub_amd.estimate_stabilization import merge_focus_rows

    new = [("B/1/0", 1, "c", 9), ("B/1/0", 0, "c", 8), ("A/1/0", 0, "c", 3)]
    old = [("A/1/0", 0, "c", 30), ("A/1/0", 1, "c", 31), ("C/1/0", 0, "c", 32), ("B/1/0", 1, "c", 33)]
    # new rows win on (position, time_idx); the rest of the old file stays; sorted by position, then time
    assert merge_focus_rows(new, old) == [("A/1/0", 0, "c", 3), ("A/1/0", 1, "c", 31), ("B/1/0", 0, "c", 8), ("B/1/0", 1, "c", 9),
                                          ("C/1/0", 0, "c", 32)]
    assert merge_focus_rows(new) == [("A/1/0", 0, "c", 3), ("B/1/0", 0, "c", 8), ("B/1/0", 1, "c", 9)]


def test_focus_finding_settings_defaults():
    from biahub_amd.settings import EstimateStabilizationSettings, FocusFindingSettings

    s = FocusFindingSettings()
    assert (s.average_across_wells, s.average_across_wells_method, s.skip_beads_fov, s.center_crop_xy) == (False, "mean", "0", [800, 800])
    with pytest.raises(ValueError):
        FocusFindingSettings(average_across_wells_method="mode")
    with pytest.raises(ValueError):
        FocusFindingSettings(crop=[1, 2])
    e = EstimateStabilizationSettings(stabilization_estimation_channel="c", stabilization_channels=["c"], stabilization_type="z",
                                      focus_finding_settings={"center_crop_xy": [48, 40]})
    assert e.stabilization_method == "focus-finding" and isinstance(e.focus_finding_settings, dict)
    assert FocusFindingSettings(**e.focus_finding_settings).center_crop_xy == [48, 40]


def test_centre_window():
    from biahub_amd.estimate_stabilization import centre_window

    assert centre_window(64, 64, [48, 40]) == (slice(12, 52), slice(8, 56))  # center_crop_xy is (x, y)
    assert centre_window(2048, 2048, [800, 800]) == (slice(624, 1424), slice(624, 1424))
    assert centre_window(65, 31, [31, 33]) == (slice(16, 48), slice(0, 30))   # odd crops lose a pixel, as the reference's do
    for crop in ([800, 800], [64, 66], [66, 64], [0, 8]):
        with pytest.raises(ValueError, match="not available|does not fit"):
            centre_window(64, 64, crop)


def test_focus_from_power_and_threshold():
    from biahub_amd.focus import focus_from_power

    # a triangle: half maximum (relative to the peak's base) is crossed 1.5 samples either side of the peak -> FWHM 3
    p = np.array([0.0, 1.0, 2.0, 3.0, 2.0, 1.0, 0.0])
    assert focus_from_power(p) == 3 and focus_from_power(p, threshold_FWHM=3.0) == 3
    assert focus_from_power(p, threshold_FWHM=3.01) is None
    assert focus_from_power([1.0, 5.0, 5.0, 2.0]) == 1           # first occurrence
    assert focus_from_power([4.0, 1.0, 1.0, 2.0], mode="min") == 1
    assert focus_from_power([9.0, 1.0, 2.0]) == 0 and focus_from_power([1.0, 2.0, 9.0]) == 2  # peaks at the stack's ends
    with pytest.raises(ValueError):
        focus_from_power(p, mode="median")


def test_focus_from_transverse_band_host_paths():
    """What runs without a device: Z == 1, the refused options, and odd extents (the float64 host restatement, with a warning)."""
    from biahub_amd.focus import compute_midband_power, focus_from_transverse_band

    kw = dict(NA_det=R.NA_DET, lambda_ill=R.LAMBDA_ILL, pixel_size=0.1494)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert focus_from_transverse_band(np.ones((1, 32, 32), np.uint16), **kw) == 0
    for opt in (dict(polynomial_fit_order=4), dict(plot_path="x.pdf"), dict(enable_subpixel_precision=True)):
        with pytest.raises(NotImplementedError):
            focus_from_transverse_band(np.ones((3, 32, 32), np.uint16), **kw, **opt)
    with pytest.raises(ValueError):
        focus_from_transverse_band(np.ones((3, 32, 32), np.uint16), **kw, mode="mid")
    v = R.make_window((5, 33, 31), "uint16", 3, seed=3)
    ref = R.midband_power(v, 0.1494)
    with pytest.warns(UserWarning, match="odd extent"):
        got = compute_midband_power(v, **kw)
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    with pytest.warns(UserWarning, match="odd extent"):
        assert focus_from_transverse_band(v, **kw) == 3
    with pytest.warns(UserWarning, match="odd extent"):
        assert focus_from_transverse_band(v, **kw, threshold_FWHM=100) is None


def test_cli_refusals(tmp_path):
    from biahub_amd import io
    from biahub_amd.cli import cli

    io.create_empty_plate(tmp_path / "in.zarr", [("A", "1", "0")], ["ch0"], (2, 1, 4, 32, 40), scale=(1, 1, 0.2, 0.1, 0.1))
    cfg = tmp_path / "est.yml"
    base = "stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\n"

    def run(text):
        cfg.write_text(base + text)
        return CliRunner().invoke(cli, ["estimate-stabilization", "-i", str(tmp_path / "in.zarr/A/1/0"), "-o", str(tmp_path / "out"), "-c", str(cfg)])

    for kind in ("xy", "xyz"):  # the default method is focus-finding
        res = run(f"stabilization_type: {kind}\n")
        assert res.exit_code != 0 and "StackReg" in res.output and "'z'" in res.output, res.output
    res = run("stabilization_type: z\nstabilization_method: beads\n")
    assert res.exit_code != 0 and "not available" in res.output
    res = run("stabilization_type: z\neval_transform_settings:\n  validation_window_size: 3\n")
    assert res.exit_code != 0 and "eval_transform_settings" in res.output
    res = run("stabilization_type: z\n")  # the default centre crop of 800 x 800 does not fit a 32 x 40 FOV
    assert res.exit_code != 0 and "center_crop_xy" in res.output
    res = run("stabilization_type: z\nfocus_finding_settings:\n  crop: 3\n")
    assert res.exit_code != 0
