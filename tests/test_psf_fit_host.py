"""CPU: the float64 restatement of the bead fits (tests/psf_fit_ref.py) against what the reference recorded
(tests/golden/psf_fit_cases.json, written by tests/golden/make_psf_fit_golden.py), and the host-side pieces of
``characterize-psf``: the 1-D peak widths, ``CharacterizeSettings``, the tables' columns, the report files, the dtype check.
"""

import numpy as np
import pandas as pd
import pytest
import yaml
from click.testing import CliRunner

import psf_fit_ref as R
from biahub_amd import characterize_psf as cp
from biahub_amd import io
from biahub_amd.cli import cli
from biahub_amd.settings import CharacterizeSettings
from biahub_amd.utils.config import yaml_to_model

META = R.load_golden()
CASES = {c["name"]: c for c in META["cases"]}
# the restatement runs the code that wrote the fixture: it must land on the recorded truth far inside what the GPU is held to
RECOMPUTE = 1e-8


def _check_bead(sample, spacing, fits):
    for kind in R.KINDS:
        rec = fits[kind]
        p0 = R.initial_guess(sample, spacing, kind)
        np.testing.assert_allclose(p0, rec["guess"], rtol=1e-12, atol=0)
        t = R.fit(kind, sample, spacing, p0)
        assert t["ok"]
        p = t["p"].copy()
        if kind == "z":
            p[3] = abs(p[3])
        sde = np.array(rec["truth_sde"])
        assert np.max(np.abs(p - rec["truth_p"]) / sde) <= RECOMPUTE
        assert np.max(np.abs(t["sde"] - sde) / sde) <= RECOMPUTE
        assert np.max(np.abs(p - rec["ref_p"]) / sde) <= rec["ref_dev"] + RECOMPUTE
        n = len(rec["ref_sde"])
        assert np.max(np.abs(t["sde"][:n] - rec["ref_sde"]) / sde[:n]) <= rec["ref_sde_dev"] + RECOMPUTE
        assert rec["ref_dev"] <= META["bounds"][kind]["ref_dev"] <= 1e-2


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_the_recorded_reference(name):
    c = CASES[name]
    vol, starts, shapes = R.make_case_volume(c)
    assert vol.dtype == np.dtype(c["dtype"]) and list(shapes[0]) == c["crop"]
    sample = R.to_sample(R.crop(vol, starts[0], shapes[0]), c["offset"], c["gain"])
    assert sample.dtype == np.int32 and int(sample.sum(dtype=np.int64)) == c["sample_sum"]  # the generator's voxels have not moved
    _check_bead(sample, c["spacing"], c["fits"])


def test_restatement_reproduces_the_recorded_reference_on_the_batch():
    b = META["batch"]
    vol, starts, shapes = R.make_batch_volume(b)
    assert int(vol.astype(np.int64).sum()) == b["volume_sum"] and len(starts) == b["count"] == len(b["beads"])
    for st, sh, bead in zip(starts, shapes, b["beads"]):
        _check_bead(R.to_sample(R.crop(vol, st, sh), 0.0, 1.0), b["spacing"], bead["fits"])


def test_truncation_not_rounding_and_float32_arithmetic():
    """offset -100, gain 0.5 on odd counts ends in .5, which astype(int32) cuts; a float32 patch stays float32 in NumPy."""
    assert R.to_sample(np.array([[[301, 303, 50]]], dtype=np.uint16), -100.0, 0.5).tolist() == [[[100, 101, 0]]]
    x = np.array([[[1000.3, 16777.217]]], dtype=np.float32)
    f32 = ((x + np.float32(-100.25)) * np.float32(0.37)).astype(np.int32)
    assert np.array_equal(R.to_sample(x, -100.25, 0.37), f32)


def test_columns_are_the_references():
    assert list(cp.FIT_COLUMNS) == META["columns"] == R.COLUMNS
    assert [cp.FIT_COLUMNS[i] for i in cp._NON_NEGATIVE] == R.NON_NEGATIVE


# ------------------------------------------------------------------------------------------------------------ peak widths
def _separable(pz, py, px):
    return (pz[:, None, None] * py[None, :, None] * px[None, None, :]).astype(np.float64)


def test_peak_widths_of_a_triangle():
    """0 1 2 3 4 3 2 1 0: prominence 4, half height 2, crossed at 2 and 6 -> 4 samples wide on every axis."""
    tri = np.array([0, 1, 2, 3, 4, 3, 2, 1, 0.0])
    got = cp.calculate_peak_widths(_separable(tri, tri, tri), (0.25, 0.15, 0.2))
    np.testing.assert_allclose(got, (4 * 0.25, 4 * 0.15, 4 * 0.2), rtol=1e-12)


def test_peak_widths_off_centre_and_failure():
    """The centre index is taken as the peak whether it is one or not; a failure on any axis zeroes all three."""
    tri = np.array([0, 1, 2, 3, 4, 3, 2, 1, 0.0])
    shifted = np.array([0, 0, 1, 2, 3, 4, 3, 2, 1.0])  # maximum at 5, centre index 4 is on the slope: width 0 (with a warning)
    with pytest.warns(Warning):
        got = cp.calculate_peak_widths(_separable(shifted, tri, tri), (1.0, 1.0, 1.0))
    assert got[0] == 0.0 and got[1] == got[2] == 4.0
    assert cp.calculate_peak_widths(np.zeros((3, 3, 3)), (1.0, 1.0, 1.0)) == (0.0, 0.0, 0.0)  # flat: prominence 0, width 0
    assert cp.calculate_peak_widths(np.zeros((3, 3, 3), dtype=object), (1.0, 1.0, 1.0)) == (0.0, 0.0, 0.0)  # scipy raises: the except


def test_robust_peak_widths_of_a_parabola():
    """y = 100 - 4 (i - 5)^2: the four samples around the top fit it exactly (vertex 5, peak 100); samples >= 25 are kept,
    and 50 is crossed between 36 and 64 on each side: at 1.5 and 8.5 -> 7 samples wide."""
    par = 100.0 - 4.0 * (np.arange(11) - 5.0) ** 2
    flat = np.ones(11)
    patch = par[:, None, None] * flat[None, :, None] * flat[None, None, :]
    got = cp.calculate_robust_peak_widths(patch, (0.25, 0.15, 0.15))
    assert got[0] == pytest.approx(7 * 0.25, rel=1e-12)
    assert got[1] == 0.0 and got[2] == 0.0  # flat profiles: no parabola, no crossings -> the reference's except
    cube = _separable(par, par, par) / 1e4
    np.testing.assert_allclose(cp.calculate_robust_peak_widths(cube, (0.25, 0.15, 0.2)), (7 * 0.25, 7 * 0.15, 7 * 0.2), rtol=1e-12)


# --------------------------------------------------------------------------------------------------------------- settings
def test_characterize_settings_defaults_and_yaml_round_trip(tmp_path):
    s = CharacterizeSettings()
    assert (list(s.block_size), s.blur_kernel_size, s.nms_distance, s.min_distance, s.threshold_abs, s.max_num_peaks,
            list(s.exclude_border), s.patch_size, s.axis_labels, s.offset, s.gain, s.use_robust_1d_fwhm, s.fwhm_plot_type) == (
        [64, 64, 32], 3, 32, 50, 200.0, 2000, [5, 10, 5], None, ["AXIS0", "AXIS1", "AXIS2"], 0.0, 1.0, False, "3D")
    s = CharacterizeSettings(block_size=[8, 8, 8], patch_size=(3.75, 2.7, 2.7), axis_labels=["Z", "Y", "X"], offset=-100.0, gain=0.5,
                             use_robust_1d_fwhm=True, fwhm_plot_type="1D", exclude_border=[1, 2, 3])
    (tmp_path / "c.yml").write_text(yaml.safe_dump(s.model_dump(mode="json")))  # a tuple field: JSON mode writes it as a list
    loaded = yaml_to_model(tmp_path / "c.yml", CharacterizeSettings)
    assert loaded == s and loaded.patch_size == (3.75, 2.7, 2.7)
    (tmp_path / "d.yml").write_text("patch_size: [3.75, 2.7, 2.7]\naxis_labels: [Z, Y, X]\noffset: -100\ngain: 0.5\n")
    d = yaml_to_model(tmp_path / "d.yml", CharacterizeSettings)
    assert (d.patch_size, d.offset, d.gain, d.max_num_peaks) == ((3.75, 2.7, 2.7), -100.0, 0.5, 2000)
    with pytest.raises(ValueError):
        CharacterizeSettings(fwhm_plot_type="2D")
    with pytest.raises(ValueError):
        CharacterizeSettings(no_such_field=1)


# ----------------------------------------------------------------------------------------------------------------- report
def test_report_files_and_csv_columns(tmp_path):
    rng = np.random.default_rng(5)
    n = 3  # fewer than the 5 beads the reference's plots insist on
    fit = pd.DataFrame(rng.uniform(0.5, 2.0, (n, len(cp.FIT_COLUMNS))), columns=list(cp.FIT_COLUMNS))
    fit["zyx_snr"] = fit["zyx_amp"] / 2.0
    widths = pd.DataFrame(rng.uniform(0.5, 2.0, (n, 6)), columns=["z_mu", "y_mu", "x_mu", *cp.PEAK_WIDTH_COLUMNS])
    beads = [rng.poisson(100, (7, 9, 9)).astype(np.uint16) for _ in range(n)]
    out = tmp_path / "report"
    cp.generate_report(out, "in.zarr/A/1/0", "in.zarr", beads, np.arange(9).reshape(3, 3), fit, widths, (0.25, 0.15, 0.15),
                       ("Z", "Y", "X"), "3D")
    assert (out / "psf_gaussian_fit.csv").read_text().splitlines()[0].split(",") == META["columns"] + ["zyx_snr"]
    assert (out / "psf_1d_peak_width.csv").read_text().splitlines()[0].split(",") == ["z_mu", "y_mu", "x_mu", "1d_z_fwhm", "1d_y_fwhm",
                                                                                      "1d_x_fwhm"]
    assert len(pd.read_csv(out / "psf_gaussian_fit.csv")) == n
    for f in ("peaks.pkl", "psf_analysis_report.md", "plots/beads_psf_slices.png", "plots/fwhm_vs_Z.png", "plots/fwhm_vs_Y.png",
              "plots/fwhm_vs_X.png", "plots/psf_amp_xy.png", "plots/psf_amp_z.png"):
        assert (out / f).stat().st_size > 0, f
    report = (out / "psf_analysis_report.md").read_text()
    assert "* Detected: 3" in report and "* Skipped: 0" in report and "plots/fwhm_vs_Z.png" in report
    try:
        import markdown  # noqa: F401
    except ImportError:
        assert not (out / "psf_analysis_report.html").exists()
    else:
        assert (out / "psf_analysis_report.html").exists()
    with pytest.raises(ValueError):
        cp._make_plots(out, beads, fit, widths, (0.25, 0.15, 0.15), ("Z", "Y", "X"), "2D")


def test_bead_boxes_follow_numpy_slicing():
    margins = np.array([15.0, 18.0, 18.0])
    starts, shapes, offsets = cp.bead_boxes((20, 40, 40), [[10, 20, 20], [16, 35, 20], [3, 20, 20]], margins)
    # inside; cut short at the far border of z and y; start -4 along z counts from the far end: [16, 11) is empty -> dropped
    assert starts.tolist() == [[3, 11, 11], [9, 26, 11]] and shapes.tolist() == [[15, 18, 18], [11, 14, 18]]
    assert offsets == [(3, 11, 11), (11, 28, 11)]
    vol = np.arange(20 * 40 * 40).reshape(20, 40, 40)
    assert vol[9:24, 26:44, 11:29].shape == (11, 14, 18) and vol[-4:11, 11:29, 11:29].size == 0


def test_cli_refuses_a_dtype_float32_cannot_hold(tmp_path):
    store = tmp_path / "beads.zarr"
    io.create_empty_plate(store, [("A", "1", "0")], ["beads"], (1, 1, 8, 16, 16), chunks=(1, 1, 8, 16, 16), scale=(1, 1, 0.25, 0.15, 0.15),
                          dtype=np.float64)
    cfg = tmp_path / "c.yml"
    cfg.write_text("axis_labels: [Z, Y, X]\n")
    res = CliRunner().invoke(cli, ["characterize-psf", "-i", str(store / "A/1/0"), "-c", str(cfg), "-o", str(tmp_path / "out")])
    assert res.exit_code != 0 and "float64" in res.output and not (tmp_path / "out").exists()
    with pytest.raises(ValueError, match="int32"):
        cp.characterize_psf(np.zeros((8, 16, 16), dtype=np.int32), (0.25, 0.15, 0.15), CharacterizeSettings(), tmp_path / "out", "x", "x")
