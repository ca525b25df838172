"""StackReg translation, host side: the float64 restatement (tests/stackreg_ref.py) against scipy and against
the known shifts of its scenes, the constants against the header, the focus-index filling against the reference's pandas
expression, the settings and the matrix layouts.  None of this needs a GPU."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import stackreg_ref as R

ROOT = Path(__file__).resolve().parent.parent
KINDS = [(noise, dt) for noise in (False, True) for dt in ("float32", "uint16")]


def test_constants_mirror_the_header():
    text = (ROOT / "include" / "bhcore.h").read_text()
    header = {m.group(1): float(m.group(2)) for m in re.finditer(r"#define BH_STACKREG_(\w+) ([-+0-9.eE]+)\s", text)}
    mine = {"MIN_SIDE_FOR_NEXT": R.MIN_SIDE_FOR_NEXT, "EPS": R.EPS, "MAX_ITER": R.MAX_ITER, "LAMBDA0": R.LAMBDA0,
            "LAMBDA_FACTOR": R.LAMBDA_FACTOR, "FLAT_REL": R.FLAT_REL, "COND_REL": R.COND_REL, "CONVERGED": R.CONVERGED,
            "ITERCAP": R.ITERCAP, "DEGENERATE": R.DEGENERATE}
    assert header == {k: float(v) for k, v in mine.items()}


def test_pyramid_shapes():
    levels = lambda H, W: [v.shape for v in R.pyramid(np.ones((H, W)))]  # noqa: E731
    assert levels(20, 23) == [(20, 23)]
    assert levels(24, 47) == [(24, 47), (12, 24)]
    assert levels(49, 63) == [(49, 63), (25, 32), (13, 16)]
    assert levels(96, 128) == [(96, 128), (48, 64), (24, 32), (12, 16)]
    ramp = np.add.outer(np.arange(49.0), 2.0 * np.arange(63.0))  # a linear ramp survives the filter away from the borders
    assert np.allclose(R.reduce_level(ramp)[1:-1, 1:-1], ramp[::2, ::2][1:-1, 1:-1], rtol=0, atol=1e-12)


def _independent_sums(v_mov, v_ref, d):
    """The seven sums from scipy's prefilter and sampler and a padded central difference."""
    from scipy import ndimage

    H, W = v_ref.shape
    cm = ndimage.spline_filter(v_mov, order=3, mode="mirror")
    cr = ndimage.spline_filter(v_ref, order=3, mode="mirror")
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    M = ndimage.map_coordinates(cm, [yy + d[0], xx + d[1]], order=3, mode="mirror", prefilter=False)
    pad = np.pad(cr, 1, mode="reflect")
    gy, gx = 0.5 * (pad[2:, 1:-1] - pad[:-2, 1:-1]), 0.5 * (pad[1:-1, 2:] - pad[1:-1, :-2])
    m = (yy + d[0] >= 0) & (yy + d[0] <= H - 1) & (xx + d[1] >= 0) & (xx + d[1] <= W - 1)
    r = (M - v_ref)[m]
    gy, gx = gy[m], gx[m]
    return np.array([m.sum(), r @ r, r @ gy, r @ gx, gy @ gy, gy @ gx, gx @ gx])


@pytest.mark.parametrize("d", [(0.0, 0.0), (0.37, -1.62), (-2.5, 3.25), (5.0, -3.0), (-0.001, 0.999), (11.75, -17.1)])
def test_cost_against_scipy(d):
    H, W = 37, 52
    scene = R.blobs(H, W, seed=5)
    v_ref = R.clip_to_f64(R.render(H, W, scene, (0.0, 0.0), dtype=np.float64))
    v_mov = R.clip_to_f64(R.render(H, W, scene, (1.7, -2.3), dtype=np.float64))
    mine = R.evaluate(v_mov, R.spline_coefficients(v_mov), v_ref, R.spline_coefficients(v_ref), d)
    theirs = _independent_sums(v_mov, v_ref, d)
    assert mine[0] == theirs[0] > 0
    np.testing.assert_allclose(mine, theirs, rtol=1e-10, atol=0)


def test_cost_empty_domain():
    v = R.clip_to_f64(R.render(20, 23, R.blobs(20, 23, seed=3)))
    c = R.spline_coefficients(v)
    assert R.evaluate(v, c, v, c, (20.0, 0.0))[0] == 0
    assert R.evaluate(v, c, v, c, (19.0, -22.0))[0] == 1


@pytest.mark.parametrize("noise,dtype_name", KINDS)
@pytest.mark.parametrize("index", range(len(R.CASES)), ids=[c[0] for c in R.CASES])
def test_recovery_of_known_shifts(index, noise, dtype_name):
    _, shift, _, status, iterations = R.reference_result(index, noise, dtype_name)
    err = float(np.abs(shift - np.array(R.CASES[index][3])).max())
    print(f"{R.CASES[index][0]} noise={noise} {dtype_name}: error {err:.4f} px, {iterations} iterations")
    assert status == R.CONVERGED  # the fixture condition: every case converges
    if not noise:
        assert err < 0.1  # the fixture condition
    assert err <= (R.RECOVERY_BOUND_NOISY if noise else R.RECOVERY_BOUND_NOISELESS)
    if R.CASES[index][3] == (0.0, 0.0) and not noise:
        assert shift[0] == 0.0 and shift[1] == 0.0


def test_degenerate_frames():
    H, W = 32, 40
    frame = R.render(H, W, R.blobs(H, W, seed=9), dtype=np.uint16)
    flat = np.full((H, W), 100, dtype=np.uint16)
    stripes = np.tile((100 + 50 * np.sin(np.arange(W) / 3.0)).astype(np.float32), (H, 1))
    for other in (flat, np.zeros((H, W), dtype=np.uint16), stripes):
        for pair in ((1, 0), (0, 1)):
            shift, mse, status, _ = R.register_pairs(np.stack([frame.astype(np.float32), other.astype(np.float32)]), [pair])
            assert status[0] == R.DEGENERATE and (shift == 0).all() and np.isfinite(mse).all()


def test_focus_index_filling_against_pandas():
    pd = pytest.importorskip("pandas")
    from biahub_amd.estimate_stabilization import fill_focus_indices

    nan = float("nan")
    columns = [[3, 4, 0, 5], [0, 0, 7, 0, 9], [0, 3, 3], [5], [nan, 4, 0, 6], [2.0, nan, 0, 8], [0, 0, 4, 5, 0, 0], [7, 0, 0, 0, 1]]
    for col in columns:
        focus_idx = pd.Series(col)
        expected = focus_idx.replace(0, np.nan).ffill().fillna(focus_idx.mean()).astype(int).to_list()
        assert fill_focus_indices(col) == expected, col
    assert fill_focus_indices([0, 0, 7, 0, 9]) == [3, 3, 7, 7, 9]  # the mean counts the zeros: 16 / 5
    with pytest.raises(ValueError):
        fill_focus_indices([nan, nan])


def test_stack_reg_settings():
    from pydantic import ValidationError

    from biahub_amd.settings import EstimateStabilizationSettings, FocusFindingSettings, StackRegSettings

    s = StackRegSettings()
    assert s.center_crop_xy == [800, 800] and s.skip_beads_fov == "0" and s.t_reference == "first"
    assert s.focus_finding_settings == FocusFindingSettings()
    assert StackRegSettings(focus_finding_settings=None).focus_finding_settings is None
    assert StackRegSettings(focus_finding_settings={"center_crop_xy": [64, 32]}).focus_finding_settings.center_crop_xy == [64, 32]
    with pytest.raises(ValidationError):
        StackRegSettings(crop=3)
    with pytest.raises(ValidationError):
        StackRegSettings(t_reference="mean")
    with pytest.raises(ValidationError):
        StackRegSettings(focus_finding_settings={"crop": 3})
    e = EstimateStabilizationSettings(stabilization_estimation_channel="a", stabilization_channels=["a"], stabilization_type="xy")
    assert e.stack_reg_settings is None and e.stabilization_method == "focus-finding"


def test_matrices():
    from biahub_amd.estimate_stabilization import xy_transforms_from_stackreg
    from biahub_amd.stackreg import matrices_from_shifts

    shifts = np.array([[1.5, -2.0], [0.25, 4.0], [-3.0, 0.5]])  # (y, x)
    first = matrices_from_shifts(shifts, "first")
    prev = matrices_from_shifts(shifts, "previous")
    assert first.shape == prev.shape == (4, 3, 3) and first.dtype == np.float64
    assert np.array_equal(first[0], np.eye(3)) and np.array_equal(prev[0], np.eye(3))
    run = np.zeros(2)
    for t in range(1, 4):
        run = run + shifts[t - 1]
        for m, s in ((first[t], shifts[t - 1]), (prev[t], run)):
            assert m[0, 2] == s[1] and m[1, 2] == s[0]  # pystackreg: [0, 2] is x, [1, 2] is y
            m = m.copy()
            m[0, 2] = m[1, 2] = 0
            assert np.array_equal(m, np.eye(3))
    zyx = xy_transforms_from_stackreg(prev)
    assert zyx.shape == (4, 4, 4)
    for t in range(4):
        expected = np.eye(4)
        expected[1, 3], expected[2, 3] = prev[t][1, 2], prev[t][0, 2]  # [1, 3] is y, [2, 3] is x
        assert np.array_equal(zyx[t], expected)


def test_cli_refuses_xyz_with_average_across_wells(tmp_path):
    from click.testing import CliRunner

    from biahub_amd import io
    from biahub_amd.cli import cli

    io.create_empty_plate(tmp_path / "in.zarr", [("A", "1", "0")], ["ch0"], (2, 1, 4, 32, 40), scale=(1, 1, 0.2, 0.1, 0.1))
    cfg = tmp_path / "est.yml"
    cfg.write_text("stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\nstabilization_type: xyz\n"
                   "focus_finding_settings:\n  average_across_wells: true\n  center_crop_xy: [32, 32]\n"
                   "stack_reg_settings:\n  center_crop_xy: [32, 32]\n  focus_finding_settings:\n    center_crop_xy: [32, 32]\n")
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", str(tmp_path / "in.zarr/A/1/0"), "-o", str(tmp_path / "out"), "-c", str(cfg)])
    assert res.exit_code != 0 and "average_across_wells" in res.output, res.output
    cfg.write_text("stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\nstabilization_type: xy\n"
                   "stack_reg_settings:\n  center_crop_xy: [32, 32]\n")  # the nested focus window of 800 x 800 does not fit
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", str(tmp_path / "in.zarr/A/1/0"), "-o", str(tmp_path / "out"), "-c", str(cfg)])
    assert res.exit_code != 0 and "StackReg" in res.output and "center_crop_xy" in res.output, res.output
