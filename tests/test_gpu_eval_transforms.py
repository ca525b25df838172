"""GPU: ``eval_transform_settings`` end to end.  The real estimators (phase cross-correlation, focus finding by mid-band power)
are driven into producing one outlier; ``estimate-stabilization`` runs once without the block (the raw list) and once with it,
and the second file must be ``evaluate_transforms`` of the first (biahub_amd/registration/utils.py, held to the reference's
recorded results by tests/test_eval_transforms_host.py).

Tolerance.  The raw lists are integer shifts; the filled entries come out of float64 ``interp1d`` (error of order 1e-14) and
through a YAML round trip that keeps every bit: 1e-9 absolute, as for the host tests.

Focus finding: the estimator reproduces the planted planes 1 + [0, 0, 1, 1, 1, 9, 2, 2, 2, 3] of the (12, 64, 64) stacks exactly
on an MI355X, so the raw z translations are those offsets, t = 5 alone is flagged and gets 1.5.
"""

from pathlib import Path

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

import focus_ref as R
from biahub_amd import io
from biahub_amd.cli import cli
from biahub_amd.registration.utils import evaluate_transforms, validate_transforms

pytestmark = pytest.mark.gpu

ATOL = 1e-9
PNG = b"\x89PNG\r\n\x1a\n"
EVAL = ("eval_transform_settings:\n  validation_window_size: 3\n  validation_tolerance: {}\n  interpolation_window_size: 3\n"
        "  interpolation_type: linear\nverbose: true\n")


def _estimate(root, pos, out, text):
    cfg = root / f"{out}.yml"
    cfg.write_text(text)
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", str(pos), "-o", str(root / out), "-c", str(cfg), "--local"])
    assert res.exit_code == 0, res.output
    return root / out


def _list(path):
    return np.array(yaml.safe_load(Path(path).read_text())["affine_transform_zyx_list"])


def test_phase_cross_corr_outlier_is_interpolated_then_stabilized(gpu, tmp_path):
    y_rolls = (0, 1, 2, 3, 4, -9, 6, 7)  # the y values of the fixture case "outlier_after_bootstrap"
    shape = (16, 32, 40)
    base = (np.random.default_rng(11).random(shape) * 1000 + 100).astype(np.float32)
    store = tmp_path / "in.zarr"
    io.create_empty_plate(store, [("A", "1", "0")], ["ch0"], (len(y_rolls), 1) + shape, scale=(1, 1, 0.2, 0.1, 0.1))
    pos = io.open_ome_zarr(store / "A/1/0")
    for t, r in enumerate(y_rolls):
        pos.data[t, 0] = np.roll(base, r, axis=1)
    head = "stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\nstabilization_type: xyz\nstabilization_method: phase-cross-corr\n"
    raw = _list(_estimate(tmp_path, store / "A/1/0", "raw", head) / "xyz_stabilization_settings" / "A_1_0.yml")
    assert not (tmp_path / "raw" / "translation_plots").exists()
    assert raw.shape == (8, 4, 4)
    jump = raw[5][:3, 3] - raw[4][:3, 3]
    print("raw translations:", raw[:, :3, 3].tolist())
    assert sorted(np.abs(jump).tolist()) == [0.0, 0.0, 13.0]  # the outlier is real
    out = _estimate(tmp_path, store / "A/1/0", "ev", head + EVAL.format(3.5))
    got = _list(out / "xyz_stabilization_settings" / "A_1_0.yml")
    want = np.asarray(evaluate_transforms(raw.tolist(), shape, validation_window_size=3, validation_tolerance=3.5,
                                          interpolation_window_size=3, interpolation_type="linear"))
    assert got.shape == raw.shape and np.abs(got - want).max() <= ATOL
    assert np.abs(got[5] - (raw[4] + raw[6]) / 2).max() <= ATOL
    for t in (0, 1, 2, 3, 4, 6, 7):
        assert np.array_equal(got[t], raw[t]), t
    assert (out / "translation_plots" / "A_1_0.png").read_bytes()[:8] == PNG
    res = CliRunner().invoke(cli, ["stabilize", "-i", str(store / "A/1/0"), "-c", str(out / "xyz_stabilization_settings" / "A_1_0.yml"),
                                   "-o", str(tmp_path / "stab.zarr"), "--local"])
    assert res.exit_code == 0, res.output


def test_focus_finding_z_outlier_is_interpolated(gpu, tmp_path):
    offsets = [0, 0, 1, 1, 1, 9, 2, 2, 2, 3]
    p0, shape = 1, (12, 64, 64)
    store = tmp_path / "in.zarr"
    io.create_empty_plate(store, [("A", "1", "0")], ["ch0"], (len(offsets), 1) + shape, chunks=(1, 1) + shape,
                          scale=(1, 1, 0.5, 0.1494, 0.1494), dtype=np.uint16)
    pos = io.open_ome_zarr(store / "A/1/0")
    for t, d in enumerate(offsets):
        pos.data[t, 0] = R.make_window(shape, "uint16", p0 + d, seed=300 + t)
    head = ("stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\nstabilization_type: z\n"
            "focus_finding_settings:\n  center_crop_xy: [48, 40]\n")
    raw = _list(_estimate(tmp_path, store / "A/1/0", "raw", head) / "z_stabilization_settings" / "A_1_0.yml")
    print("raw z translations:", raw[:, 0, 3].tolist())
    assert raw.shape == (10, 4, 4) and raw[:, 0, 3].tolist() == [float(d) for d in offsets]  # the jump at t = 5
    validated = validate_transforms(raw.tolist(), shape, window_size=3, tolerance=2.5)
    flagged = [t for t, m in enumerate(validated) if m is None]
    assert flagged == [5]  # at least one: the comparison below cannot pass empty
    out = _estimate(tmp_path, store / "A/1/0", "ev", head + EVAL.format(2.5))
    got = _list(out / "z_stabilization_settings" / "A_1_0.yml")
    want = np.asarray(evaluate_transforms(raw.tolist(), shape, validation_window_size=3, validation_tolerance=2.5,
                                          interpolation_window_size=3, interpolation_type="linear"))
    assert got.shape == raw.shape and np.abs(got - want).max() <= ATOL
    assert abs(got[5, 0, 3] - 1.5) <= ATOL and not np.array_equal(got, raw)
    assert (out / "translation_plots" / "A_1_0.png").read_bytes()[:8] == PNG
