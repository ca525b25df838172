"""Host: transform validation and interpolation over time (biahub_amd/registration/utils.py: evaluate_transforms and its parts)
against results recorded from the reference (tests/golden/eval_transforms.json, written by make_eval_transforms_golden.py), and
the wiring of ``eval_transform_settings`` into ``estimate-stabilization`` and ``estimate-registration`` with planted estimates.

Tolerance.  The values are shifts of order 1 - 100 out of float64 ``interp1d``, whose error is of order 1e-14; outputs are held
to 1e-9 absolute, which only allows for another scipy build.  Which timepoints are flagged must agree exactly.
"""

import copy
import json
from pathlib import Path

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

META = json.loads((Path(__file__).resolve().parent / "golden" / "eval_transforms.json").read_text())
CASES = {c["name"]: c for c in META["cases"]}
ATOL = 1e-9
PNG = b"\x89PNG\r\n\x1a\n"


def _kwargs(case):
    kw = copy.deepcopy(case["kwargs"])
    if isinstance(kw["transforms"], dict):
        kw["transforms"] = np.asarray(kw["transforms"]["ndarray"])
    if "shape_zyx" in kw:
        kw["shape_zyx"] = tuple(kw["shape_zyx"])
    return kw


def _call(case, kw):
    from biahub_amd.registration import utils as U

    return {"evaluate": U.evaluate_transforms, "interpolate": U.interpolate_transforms}[case["function"]](**kw)


def _translation(z=0.0, y=0.0, x=0.0):
    m = np.eye(4)
    m[:3, 3] = (z, y, x)
    return m.tolist()


def _y(mats):
    return [m[1][3] for m in mats]


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if "output" in c])
def test_outputs_equal_the_reference(name):
    from biahub_amd.registration.utils import validate_transforms

    case = CASES[name]
    kw = _kwargs(case)
    given = copy.deepcopy(kw["transforms"])
    got = _call(case, kw)
    assert isinstance(got, list) and all(isinstance(m, list) for m in got) and len(got) == len(case["output"])
    worst = max(float(np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64)).max()) for g, w in zip(got, case["output"]))
    print(f"{name}: max |got - reference| = {worst:.3g}")
    assert worst <= ATOL
    # the argument is left as it was given
    if isinstance(given, np.ndarray):
        assert np.array_equal(kw["transforms"], given)
    else:
        assert kw["transforms"] == given
    if case["function"] == "evaluate":
        t = given.tolist() if isinstance(given, np.ndarray) else copy.deepcopy(given)
        before = copy.deepcopy(t)
        validated = validate_transforms(t, kw["shape_zyx"], window_size=kw["validation_window_size"], tolerance=kw["validation_tolerance"])
        assert t == before
        assert [m is None for m in validated] == [m is None for m in case["validated"]]
        assert [i for i, (a, b) in enumerate(zip(before, validated)) if a is not None and b is None] == case["flagged"]
        assert all(a == b for a, b in zip(validated, case["validated"]) if b is not None)  # the kept ones untouched


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if "raises" in c])
def test_failures_equal_the_reference(name):
    case = CASES[name]
    kw = _kwargs(case)
    given = copy.deepcopy(kw["transforms"])
    kind = {"ValueError": ValueError, "Warning": Warning}[case["raises"]["type"]]
    with pytest.raises(kind) as e:
        _call(case, kw)
    assert type(e.value) is kind
    if name != "cubic_three_points":  # that text is scipy's own
        assert str(e.value) == case["raises"]["message"]
    assert kw["transforms"] == given


def test_what_the_cases_are_about():
    """The recorded results show what each case was made for, so that a regenerated fixture cannot drift into saying nothing."""
    c = CASES
    assert c["clean_drift"]["flagged"] == [] and c["clean_drift"]["output"] == c["clean_drift"]["kwargs"]["transforms"]
    assert c["outlier_after_bootstrap"]["flagged"] == [5] and _y(c["outlier_after_bootstrap"]["output"]) == [0, 1, 2, 3, 4, 5, 6, 7]
    o = c["outlier_and_none"]
    assert o["flagged"] == [5, 7] and o["kwargs"]["transforms"][6] is None and o["output"][7] == o["kwargs"]["transforms"][4]
    assert c["outlier_in_bootstrap"]["validated"][1] is not None and c["outlier_in_bootstrap"]["flagged"]  # accepted, then pulls the mean
    gap = c["long_gap_window_1"]
    assert [i for i, m in enumerate(gap["kwargs"]["transforms"]) if m is not None] == [0, 1, 7, 8, 9]
    assert gap["output"][4] == gap["kwargs"]["transforms"][1]  # equidistant from 1 and 7: the earlier one
    assert abs(c["cubic_local"]["output"][6][0][3] - 0.36) < 1e-12 and abs(c["cubic_global_is_linear"]["output"][6][0][3] - 0.37) < 1e-12
    assert c["cubic_three_points"]["raises"]["type"] == "ValueError"
    assert c["ndarray_input"]["output"] == c["outlier_after_bootstrap"]["output"]
    one, small = c["similarity_one_plane"], c["similarity_one_plane_small"]
    assert one["kwargs"]["transforms"] == small["kwargs"]["transforms"] and one["flagged"] == [6] and small["flagged"] == []
    assert "Required: 3, Provided: 2" in c["short_for_validation"]["raises"]["message"]
    assert c["short_for_interpolation"]["raises"]["message"] == "Not enough transforms for interpolation. Required: 5, Provided: 3"


def test_check_transforms_difference_and_echo(capsys):
    from biahub_amd.registration.utils import check_transforms_difference, evaluate_transforms

    a, b = _translation(), _translation(0.0, 3.0, 4.0)
    assert check_transforms_difference(a, b, (16, 32, 40), threshold=5.001)  # every grid point moves by (3, 4): a distance of 5
    assert not check_transforms_difference(a, b, (16, 32, 40), threshold=4.999)
    assert check_transforms_difference(a, a, (16, 32, 40), threshold=0.0)  # accepted on <=
    assert check_transforms_difference(a, b, (16, 32, 40), 5.0, verbose=True)
    assert capsys.readouterr().out == "MSE of transformed points: 5.00; threshold: 5.00\n"
    kw = _kwargs(CASES["outlier_and_none"])
    evaluate_transforms(verbose=True, **kw)
    out = capsys.readouterr().out
    for line in ("[Bootstrap] Accepting transform at timepoint 2 (no validation)", "Transform at timepoint 4 is valid",
                 "Transform at timepoint 5 is invalid and will be interpolated", "Transform at timepoint 6 is None and will be interpolated",
                 "Interpolating missing transforms at timepoints: [5, 6, 7]", "Interpolated timepoint 5 using neighbors: [2, 3, 4]",
                 "Not enough interpolation neighbors were found for timepoint 7 using closest valid transform at timepoint 4"):
        assert line in out, line


def test_settings_model():
    from biahub_amd.settings import EstimateRegistrationSettings, EstimateStabilizationSettings, EvalTransformSettings

    ev = EvalTransformSettings()
    assert (ev.validation_window_size, ev.validation_tolerance, ev.interpolation_window_size, ev.interpolation_type) == (10, 1000.0, 3, "linear")
    assert EvalTransformSettings(interpolation_type="cubic").interpolation_type == "cubic"
    for bad in (dict(interpolation_type="quadratic"), dict(window=3)):
        with pytest.raises(ValueError):
            EvalTransformSettings(**bad)
    s = EstimateStabilizationSettings(stabilization_estimation_channel="c", stabilization_channels=["c"], stabilization_type="z",
                                      eval_transform_settings={})
    assert s.eval_transform_settings == {} and s.eval_transform_settings is not None  # an empty block is the defaults, not absence
    r = EstimateRegistrationSettings(target_channel_name="a", source_channel_name="b", eval_transform_settings={"validation_window_size": 4})
    assert EvalTransformSettings(**r.eval_transform_settings).validation_window_size == 4


def test_plot_translations(tmp_path):
    from biahub_amd.registration.utils import plot_translations

    path = tmp_path / "sub" / "plot.png"
    plot_translations(np.asarray(CASES["clean_drift"]["output"]), path)
    assert path.read_bytes()[:8] == PNG


# ------------------------------------------------------------------------------------------------------------------- the CLI
STAB = "stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\n"
EVAL = "eval_transform_settings:\n  validation_window_size: {}\n  validation_tolerance: {}\n  interpolation_window_size: {}\n"


def _store(tmp_path, T, name="in.zarr"):
    from biahub_amd import io

    io.create_empty_plate(tmp_path / name, [("A", "1", "0")], ["ch0"], (T, 1, 4, 32, 40), scale=(1, 1, 0.2, 0.1, 0.1))
    return str(tmp_path / name / "A/1/0")


def _stabilization(tmp_path, pos, out, text):
    from biahub_amd.cli import cli

    cfg = tmp_path / f"{out}.yml"
    cfg.write_text(STAB + text)
    return CliRunner().invoke(cli, ["estimate-stabilization", "-i", pos, "-o", str(tmp_path / out), "-c", str(cfg), "--local"])


def _written(path):
    return yaml.safe_load(Path(path).read_text())["affine_transform_zyx_list"]


def test_cli_refuses_a_short_store_before_any_work(tmp_path, monkeypatch):
    import biahub_amd.estimate_stabilization as E

    def never(*a, **k):
        raise AssertionError("an estimator ran")

    for name in ("estimate_z_stabilization", "estimate_xy_stabilization", "estimate_xyz_stabilization_pcc"):
        monkeypatch.setattr(E, name, never)
    res = _stabilization(tmp_path, _store(tmp_path, 2, "t2.zarr"), "out2", "stabilization_type: z\n" + EVAL.format(3, 100.0, 3))
    assert res.exit_code != 0 and not (tmp_path / "out2").exists(), res.output
    for word in ("eval_transform_settings", "validation_window_size", "3", "2 timepoint", "reference raises"):
        assert word in res.output, (word, res.output)
    pos4 = _store(tmp_path, 4, "t4.zarr")
    res = _stabilization(tmp_path, pos4, "out4", "stabilization_type: xyz\nstabilization_method: phase-cross-corr\n" + EVAL.format(3, 100.0, 5))
    assert res.exit_code != 0 and not (tmp_path / "out4").exists(), res.output
    for word in ("eval_transform_settings", "interpolation_window_size", "5", "4 timepoint"):
        assert word in res.output, (word, res.output)
    assert "validation_window_size" not in res.output[res.output.index("Error:"):]  # ahead of it the settings are echoed
    # an empty block is the defaults: a validation window of 10 on 4 timepoints
    res = _stabilization(tmp_path, pos4, "out4", "stabilization_type: xy\neval_transform_settings: {}\n")
    assert res.exit_code != 0 and "validation_window_size is 10" in res.output and not (tmp_path / "out4").exists(), res.output
    from biahub_amd.cli import cli

    cfg = tmp_path / "reg.yml"
    cfg.write_text("target_channel_name: ch0\nsource_channel_name: ch0\nestimation_method: ants\n" + EVAL.format(3, 100.0, 5))
    res = CliRunner().invoke(cli, ["estimate-registration", "-s", pos4, "-t", pos4, "-o", str(tmp_path / "reg" / "out.yml"), "-c", str(cfg)])
    assert res.exit_code != 0 and "eval_transform_settings.interpolation_window_size is 5" in res.output, res.output
    assert not (tmp_path / "reg" / "out.yml").exists() and not (tmp_path / "reg" / "xyz_transforms").exists()


# z and xy estimates whose product is an outlier at other timepoints than either part: z jumps at t = 5, xy at t = 7
Z_PLANT = [_translation(z=v) for v in (0, 0, 1, 1, 1, 9, 2, 2, 2, 3)]
XY_PLANT = [_translation(y=v, x=-v) for v in (0, 1, 1, 2, 2, 3, 3, -20, 4, 4)]
SHAPE = (4, 32, 40)
EV = dict(validation_window_size=3, validation_tolerance=2.5, interpolation_window_size=3, interpolation_type="linear")


def _plant_focus(monkeypatch):
    import biahub_amd.estimate_stabilization as E

    monkeypatch.setattr(E, "estimate_z_stabilization", lambda *a, **k: {"A_1_0": np.asarray(Z_PLANT)})
    monkeypatch.setattr(E, "estimate_xy_stabilization", lambda *a, **k: {"A_1_0": copy.deepcopy(XY_PLANT)})


def test_cli_xyz_focus_finding_evaluates_three_lists_on_their_own(tmp_path, monkeypatch):
    from biahub_amd.registration.utils import evaluate_transforms

    _plant_focus(monkeypatch)
    pos = _store(tmp_path, 10)
    crops = "focus_finding_settings:\n  center_crop_xy: [16, 16]\nstack_reg_settings:\n  center_crop_xy: [16, 16]\n  focus_finding_settings:\n    center_crop_xy: [16, 16]\n"
    res = _stabilization(tmp_path, pos, "raw", "stabilization_type: xyz\n" + crops)
    assert res.exit_code == 0, res.output
    xyz_raw = [(np.asarray(a) @ np.asarray(b)).tolist() for a, b in zip(XY_PLANT, Z_PLANT)]
    assert _written(tmp_path / "raw/xyz_stabilization_settings/A_1_0.yml") == xyz_raw
    assert _written(tmp_path / "raw/z_stabilization_settings/A_1_0.yml") == Z_PLANT
    assert _written(tmp_path / "raw/xy_stabilization_settings/A_1_0.yml") == XY_PLANT
    assert not (tmp_path / "raw/translation_plots").exists()
    res = _stabilization(tmp_path, pos, "ev", "stabilization_type: xyz\nverbose: true\n" + crops + EVAL.format(3, 2.5, 3))
    assert res.exit_code == 0, res.output
    want = {kind: evaluate_transforms(t, SHAPE, **EV) for kind, t in (("xyz", xyz_raw), ("z", Z_PLANT), ("xy", XY_PLANT))}
    got = {kind: _written(tmp_path / f"ev/{kind}_stabilization_settings/A_1_0.yml") for kind in want}
    for kind in want:
        assert np.abs(np.asarray(got[kind]) - np.asarray(want[kind])).max() <= ATOL, kind
    assert want["z"] != Z_PLANT and want["xy"] != XY_PLANT and abs(want["z"][5][0][3] - 1.5) < 1e-12
    recomposed = np.asarray([np.asarray(a) @ np.asarray(b) for a, b in zip(want["xy"], want["z"])])
    # the plant tells the two apart: in the product t = 5 is flagged for its z and gets y = 2.5 from t = 4 and 6, in xy alone it stays 3
    assert np.abs(recomposed - np.asarray(want["xyz"])).max() > 0.25
    assert np.abs(recomposed - np.asarray(got["xyz"])).max() > 0.25
    # one plot, for the xyz file
    assert sorted(p.name for p in (tmp_path / "ev/translation_plots").iterdir()) == ["A_1_0.png"]
    assert (tmp_path / "ev/translation_plots/A_1_0.png").read_bytes()[:8] == PNG


@pytest.mark.parametrize("kind", ["z", "xy"])
def test_cli_z_and_xy_focus_finding(tmp_path, monkeypatch, kind):
    from biahub_amd.registration.utils import evaluate_transforms

    _plant_focus(monkeypatch)
    pos = _store(tmp_path, 10)
    crops = ("focus_finding_settings:\n  center_crop_xy: [16, 16]\n" if kind == "z" else
             "stack_reg_settings:\n  center_crop_xy: [16, 16]\n  focus_finding_settings:\n    center_crop_xy: [16, 16]\n")
    res = _stabilization(tmp_path, pos, "ev", f"stabilization_type: {kind}\n" + crops + EVAL.format(3, 2.5, 3))
    assert res.exit_code == 0, res.output
    plant = Z_PLANT if kind == "z" else XY_PLANT
    want = evaluate_transforms(plant, SHAPE, **EV)
    assert want != plant
    assert np.abs(np.asarray(_written(tmp_path / f"ev/{kind}_stabilization_settings/A_1_0.yml")) - np.asarray(want)).max() <= ATOL
    assert not (tmp_path / "ev/translation_plots").exists()  # not verbose


def test_cli_pcc_interpolation_failure_names_the_fov(tmp_path, monkeypatch):
    import biahub_amd.estimate_stabilization as E

    t8 = [_translation(z=0.01 * t * t) for t in range(12)]
    t8[5] = t8[6] = None
    monkeypatch.setattr(E, "estimate_xyz_stabilization_pcc", lambda *a, **k: {"A_1_0": copy.deepcopy(t8)})
    res = _stabilization(tmp_path, _store(tmp_path, 12), "ev", "stabilization_type: xyz\nstabilization_method: phase-cross-corr\n"
                         "eval_transform_settings:\n  validation_window_size: 3\n  interpolation_window_size: 2\n  interpolation_type: cubic\n")
    assert res.exit_code != 0 and "A_1_0" in res.output and "eval_transform_settings" in res.output, res.output
    assert "Usage:" in res.output and not (tmp_path / "ev/xyz_stabilization_settings").exists()


def test_cli_beads_stabilization_fills_the_missing(tmp_path, monkeypatch):
    import biahub_amd.registration.beads as B
    from biahub_amd.registration.utils import evaluate_transforms

    plant = [None, _translation(0.0, 1.0, -1.0), None, _translation(0.2, 3.0, -2.0), _translation(0.2, 4.0, -2.5), _translation(0.3, 5.0, -3.0)]
    monkeypatch.setattr(B, "estimate_tczyx", lambda **k: copy.deepcopy(plant))
    pos = _store(tmp_path, 6)
    text = "stabilization_type: xyz\nstabilization_method: beads\n"
    res = _stabilization(tmp_path, pos, "raw", text)
    assert res.exit_code != 0 and "no transform could be estimated for timepoint(s) [2] (empty data); interpolating over them " \
        "(eval_transform_settings) is not available in biahub_amd" in res.output.replace("\n", " ").replace("  ", " "), res.output
    assert not (tmp_path / "raw/xyz_stabilization_settings.yml").exists()
    res = _stabilization(tmp_path, pos, "ev", text + "verbose: true\n" + EVAL.format(3, 100.0, 3))
    assert res.exit_code == 0, res.output
    got = _written(tmp_path / "ev/xyz_stabilization_settings.yml")
    with_identity = [np.eye(4).tolist()] + plant[1:]
    want = evaluate_transforms(with_identity, SHAPE, validation_window_size=3, validation_tolerance=100.0, interpolation_window_size=3)
    assert got[0] == np.eye(4).tolist() and [got[t] for t in (1, 3, 4, 5)] == [plant[t] for t in (1, 3, 4, 5)]
    assert np.abs(np.asarray(got) - np.asarray(want)).max() <= ATOL
    # t = 2: linear through the originally valid 0, 1, 3, 4, 5 of its window, which between 1 and 3 is their mean
    assert np.abs(np.asarray(got[2]) - (np.asarray(plant[1]) + np.asarray(plant[3])) / 2).max() <= ATOL
    assert (tmp_path / "ev/translation_plots/beads.png").read_bytes()[:8] == PNG
    # a list that cannot be interpolated: the refusal names the FOV
    monkeypatch.setattr(B, "estimate_tczyx", lambda **k: [None] * 6)
    res = _stabilization(tmp_path, pos, "none", text + EVAL.format(3, 100.0, 3))
    assert res.exit_code != 0 and "A/1/0" in res.output and "At least two valid transforms" in res.output, res.output


@pytest.mark.parametrize("method", ["beads", "ants"])
def test_cli_estimate_registration(tmp_path, monkeypatch, method):
    import biahub_amd.registration.ants as A
    import biahub_amd.registration.beads as B
    from biahub_amd.cli import cli
    from biahub_amd.registration.utils import evaluate_transforms

    plant = [_translation(y=v) for v in (0, 1, 2, 3, 4, -9, 6, 7)]
    if method == "beads":
        plant[6] = None
    state = {"plant": plant}
    monkeypatch.setattr(B if method == "beads" else A, "estimate_tczyx", lambda **k: copy.deepcopy(state["plant"]))
    pos = _store(tmp_path, 8)
    cfg = tmp_path / "reg.yml"
    head = f"target_channel_name: ch0\nsource_channel_name: ch0\nestimation_method: {method}\n"

    def run(text, out, position=pos):
        cfg.write_text(head + text)
        return CliRunner().invoke(cli, ["estimate-registration", "-s", position, "-t", position, "-o", str(tmp_path / out / "out.yml"), "-c", str(cfg)])

    res = run("", "raw")
    if method == "beads":  # without the block a missing timepoint stays refused, in today's words
        assert res.exit_code != 0 and "timepoint(s) [6]" in res.output and "is not available in biahub_amd" in res.output
    else:
        assert res.exit_code == 0 and _written(tmp_path / "raw/out.yml") == plant, res.output
    res = run(EVAL.format(3, 3.5, 3), "ev")
    assert res.exit_code == 0, res.output
    model = yaml.safe_load((tmp_path / "ev/out.yml").read_text())
    want = evaluate_transforms(plant, SHAPE, validation_window_size=3, validation_tolerance=3.5, interpolation_window_size=3)
    assert model["stabilization_type"] == "affine" and model["stabilization_method"] == method
    assert np.abs(np.asarray(model["affine_transform_zyx_list"]) - np.asarray(want)).max() <= ATOL
    assert _y(want)[5] != -9 and want != plant
    assert not (tmp_path / "ev/translation_plots").exists()
    res = run("verbose: true\n" + EVAL.format(3, 3.5, 3), "verbose")
    assert res.exit_code == 0, res.output
    assert (tmp_path / f"verbose/translation_plots/{method}_registration.png").read_bytes()[:8] == PNG
    # one transform: nothing to evaluate, whatever the windows are
    state["plant"] = [_translation(y=2.0)]
    res = run(EVAL.format(3, 3.5, 3), "one", _store(tmp_path, 1, "one.zarr"))
    assert res.exit_code == 0 and "One transform was estimated, no need to evaluate" in res.output, res.output
    model = yaml.safe_load((tmp_path / "one/out.yml").read_text())
    assert model["affine_transform_zyx"] == _translation(y=2.0) and "affine_transform_zyx_list" not in model
    res = run("", "one_plain", str(tmp_path / "one.zarr" / "A/1/0"))
    assert res.exit_code == 0 and "no need to evaluate" not in res.output
    assert yaml.safe_load((tmp_path / "one_plain/out.yml").read_text()) == model


# ------------------------------------------------------------------------------------- the reference's example configs, as shipped
CONFIGS = Path(__file__).resolve().parent / "golden" / "reference_estimate_configs"  # copies of the reference's settings/*.yml


@pytest.mark.parametrize("name", sorted(p.name for p in CONFIGS.glob("*.yml")))
def test_cli_reference_example_configs_run_as_shipped(tmp_path, monkeypatch, name):
    """Each of the six parses, gets past the settings checks on a store with enough timepoints (their windows are 10 and 3, their
    centre crops 800 x 800) and writes the evaluated plant; the estimators are planted, so no device is needed."""
    import biahub_amd.estimate_stabilization as E
    import biahub_amd.registration.beads as B
    from biahub_amd import io
    from biahub_amd.cli import cli
    from biahub_amd.registration.utils import evaluate_transforms

    T, zyx = 14, (2, 808, 808)
    # an outlier beyond the tolerance of 100, after the bootstrap window of 10 (of 10 estimated ones for beads, which miss two)
    values = (0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 300, 7)
    plant = [_translation(0.0, v, -v) for v in values]
    beads = [None] + plant[1:4] + [None] + plant[5:]
    per_fov = lambda *a, **k: {"A_1_1": copy.deepcopy(plant)}  # noqa: E731
    for est in ("estimate_z_stabilization", "estimate_xy_stabilization", "estimate_xyz_stabilization_pcc"):
        monkeypatch.setattr(E, est, per_fov)
    monkeypatch.setattr(B, "estimate_tczyx", lambda **k: copy.deepcopy(beads))
    io.create_empty_plate(tmp_path / "in.zarr", [("A", "1", "1")], ["Phase3D", "GFP EX488 EM525-45"], (T, 2) + zyx, chunks=(1, 1, 1) + zyx[1:],
                          scale=(1, 1, 0.2, 0.1, 0.1))
    pos, out = str(tmp_path / "in.zarr/A/1/1"), tmp_path / "out"
    kw = dict(validation_window_size=10, validation_tolerance=100.0, interpolation_window_size=3, interpolation_type="linear")
    assert yaml.safe_load((CONFIGS / name).read_text())["eval_transform_settings"] == kw
    if "registration" in name:
        res = CliRunner().invoke(cli, ["estimate-registration", "-s", pos, "-t", pos, "-o", str(out / "reg.yml"), "-c", str(CONFIGS / name)])
        assert res.exit_code == 0, res.output
        files, want = [out / "reg.yml"], evaluate_transforms(beads, zyx, **kw)
        plot = out / "translation_plots" / "beads_registration.png"
    else:
        res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", pos, "-o", str(out), "-c", str(CONFIGS / name), "--local"])
        assert res.exit_code == 0, res.output
        if "beads" in name:
            files, want = [out / "xyz_stabilization_settings.yml"], evaluate_transforms([np.eye(4).tolist()] + beads[1:], zyx, **kw)
            plot = out / "translation_plots" / "beads.png"
        else:
            kind = name.split("_")[4]
            files = [out / f"{kind}_stabilization_settings" / "A_1_1.yml"]
            product = [(np.asarray(m) @ np.asarray(m)).tolist() for m in plant]  # xyz = xy @ z, and both parts are the plant
            want = evaluate_transforms(product if name.endswith("xyz_focus-finding.yml") else plant, zyx, **kw)
            plot = out / "translation_plots" / "A_1_1.png"
    # the outlier went, the missing ones are filled
    assert np.abs(np.asarray(want[12]) - (np.asarray(want[11]) + np.asarray(want[13])) / 2).max() < 1e-12 and all(m is not None for m in want)
    for f in files:
        assert np.abs(np.asarray(_written(f)) - np.asarray(want)).max() <= ATOL, f
    assert plot.read_bytes()[:8] == PNG  # every one of them sets verbose
