"""Host side of the estimate-stitch refinement: the float64 restatement (tests/stitch_pcc_ref.py) and the
product's graph and solver code against fixtures recorded from the reference (tests/golden/make_stitch_pcc_golden.py), and the
command line's refusals.  Nothing here needs a GPU."""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import pytest
import scipy
import yaml
from click.testing import CliRunner

import stitch_pcc_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden"
META = json.loads((GOLDEN / "stitch_pcc.json").read_text())
EDGE_CASES = META["edge_cases"]
# the restatement is float64 numpy / scipy: across builds of their libraries it moves by rounding noise (~1e-15 relative) only
F64_NOISE = 1e-12


def _run(*args):
    from biahub_amd.cli import cli, expand_eat_all

    return CliRunner().invoke(cli, expand_eat_all([str(a) for a in args]))


@pytest.fixture(scope="module")
def restated():
    out = {}
    for c in EDGE_CASES:
        a, b = R.cut_pair(c["seed"], tuple(c["tile"]), c["relation"], c["overlap"], tuple(c["disp"]), c["dtype"], c["flipud"], c["fliplr"])
        out[c["name"]] = R.register_edge(a, b, c["relation"], c["overlap"], c["flipud"], c["fliplr"])
    return out


def test_golden_covers_the_cases():
    assert len(EDGE_CASES) == 30 and sum(c["zero_confidence"] for c in EDGE_CASES) == 6
    assert {c["relation"] for c in EDGE_CASES} == {R.BELOW, R.RIGHT} and {c["dtype"] for c in EDGE_CASES} == {"uint16", "float32"}
    assert {(c["flipud"], c["fliplr"]) for c in EDGE_CASES} == {(False, False), (True, False), (False, True), (True, True)}
    assert {(tuple(c["tile"]), c["overlap"]) for c in EDGE_CASES} == {((64, 64), 48), ((96, 96), 32), ((75, 64), 48), ((64, 75), 48),
                                                                       ((96, 96), 33), ((320, 320), 300)}
    assert all(c["margin"] >= META["min_margin"] == 0.6 for c in EDGE_CASES)
    assert all(c["confidence"] >= 0.6 for c in EDGE_CASES if not c["zero_confidence"])


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c["name"] for c in EDGE_CASES])
def test_restatement_matches_the_reference_edges(case, restated):
    got = restated[case["name"]]
    nominal = (case["tile"][0] - case["overlap"], 0) if case["relation"] == R.BELOW else (0, case["tile"][1] - case["overlap"])
    assert list(got["shift"]) == case["shift"] == [nominal[0] + case["disp"][0], nominal[1] + case["disp"][1]]
    if case["zero_confidence"]:
        assert got["confidence"] == 0.0 and case["confidence"] == 0.0
    else:
        assert abs(got["confidence"] - case["confidence"]) <= case["deviation"]["confidence"] + F64_NOISE
    assert R.peak_margin(got["corr"]) >= 0.6


def test_restatement_matches_the_stored_reference_arrays(restated):
    stored = [c for c in EDGE_CASES if c["stored"]]
    assert len(stored) == 2 and {c["relation"] for c in stored} == {R.BELOW, R.RIGHT}
    with np.load(GOLDEN / "stitch_pcc.npz") as z:
        for c in stored:
            got = restated[c["name"]]
            for key, ref in (("prepared_a", got["prepared"][0]), ("prepared_b", got["prepared"][1]), ("corr", got["corr"])):
                arr = z[f"{c['name']}/{key}"]
                assert arr.shape == ref.shape == ((48, 64) if c["relation"] == R.BELOW else (64, 48))
                dev = np.abs(arr - ref).max() / np.abs(ref).max()
                assert dev <= c["deviation"]["corr" if key == "corr" else "prepared"] + F64_NOISE, (c["name"], key, dev)


@pytest.mark.parametrize("name", list(META["graphs"]))
def test_curve_order_and_edges(name):
    from biahub_amd.estimate_stitch import hilbert_edges, parse_grid_names

    g = META["graphs"][name]
    cells = parse_grid_names([f"A/1/{x:03d}{y:03d}" for x, y in g["cells"]])
    assert cells == [tuple(c) for c in g["cells"]]
    want_order = [tuple(p) for p in g["order"]]
    want_edges = [(tuple(a), tuple(b)) for a, b in g["edges"]]
    for order, edges in (hilbert_edges(cells), R.edge_list(cells)):
        assert order == want_order
        assert [(a, b) for a, b, _ in edges] == want_edges
        assert all(rel == (R.BELOW if b == (a[0], a[1] + 1) else R.RIGHT) for a, b, rel in edges)


def test_parse_grid_names_refuses_other_names():
    from biahub_amd.estimate_stitch import hilbert_edges, parse_grid_names

    for bad in ("0", "A/1/12345", "0010020", "00a002", "A/1/"):
        with pytest.raises(ValueError, match="XXXYYY"):
            parse_grid_names([bad])
    assert hilbert_edges([(3, 4)]) == ([(3, 4)], []) and hilbert_edges([]) == ([], [])


@pytest.mark.parametrize("k", range(len(META["solves"])), ids=[f"{s['graph']}{'_outlier' if s['outlier'] else ''}" for s in META["solves"]])
def test_optimal_positions_equal_the_reference(k):
    """The reference's solver is approximate (L-BFGS-B on an L1 objective with finite-difference gradients): a consistent graph
    can come back a pixel from the truth, so the reference's own answer is pinned, under the scipy that recorded it."""
    from biahub_amd.estimate_stitch import optimal_positions

    s = META["solves"][k]
    edges = [(ia, ib, tuple(sh)) for ia, ib, sh in s["edges"]]
    n = len(s["guess_i"])
    got = optimal_positions(edges, n, s["guess_i"], s["guess_j"])
    assert got.shape == (n, 2) and got.dtype == np.int64 and (got.min(axis=0) == 0).all()
    if scipy.__version__ != META["scipy_version"]:
        pytest.skip(f"positions were recorded with scipy {META['scipy_version']}; this is {scipy.__version__}: L-BFGS-B's iterates, "
                    "and with them the truncated positions, are pinned for that version only")
    assert got.tolist() == s["positions"]
    assert R.solve_positions(edges, n, s["guess_i"], s["guess_j"]).tolist() == s["positions"]


def test_solves_include_an_outlier():
    assert any(s["outlier"] for s in META["solves"]) and any(not s["outlier"] for s in META["solves"])


# ---- command line -------------------------------------------------------------------------------------------------------
def _grid_plate(tmp_path, names=("000000", "000001", "001000", "001001"), tile=(24, 40), z_slices=2):
    rng = np.random.default_rng(5)
    wells = {"A/1": {n: rng.integers(0, 1000, tile).astype(np.uint16) for n in names}}
    stage = {f"A/1/{n}": (7.0 * k, 11.0 * (k % 2)) for k, n in enumerate(names)}
    positions = R.write_plate(tmp_path / "in.zarr", wells, stage, z_slices=z_slices)
    return positions, wells, stage


def test_help_lists_the_new_options():
    res = _run("estimate-stitch", "--help")
    assert res.exit_code == 0
    for opt in ("--pcc-channel-name", "--pcc-z-index", "--pcc-overlap", "--add_offset"):
        assert opt in res.output
    assert "no effect" in res.output


@pytest.mark.parametrize("args, words", [
    (("--pcc-channel-name", "DAPI"), "DAPI"),
    (("--pcc-channel-name", "Phase", "--pcc-z-index", "2"), "--pcc-z-index"),
    (("--pcc-channel-name", "Phase", "--pcc-z-index", "-1"), "--pcc-z-index"),
    (("--pcc-channel-name", "Phase", "--pcc-overlap", "15"), "--pcc-overlap"),
    (("--pcc-channel-name", "Phase", "--pcc-overlap", "25"), "--pcc-overlap"),  # beyond Y = 24: the well has a neighbour below
    (("--pcc-channel-name", "Phase", "--pcc-overlap", "41"), "--pcc-overlap"),
])
def test_refusals_come_before_any_work(tmp_path, args, words):
    positions, _, _ = _grid_plate(tmp_path)
    out = tmp_path / "s.yml"
    res = _run("estimate-stitch", "-i", *positions, "-o", out, *args)
    assert res.exit_code == 2 and words in res.output and not out.exists(), res.output


def test_bad_fov_names_are_refused(tmp_path):
    positions, _, _ = _grid_plate(tmp_path, names=("000000", "000001", "1", "001001"))
    out = tmp_path / "s.yml"
    res = _run("estimate-stitch", "-i", *positions, "-o", out, "--pcc-channel-name", "Phase")
    assert res.exit_code == 2 and "reference biahub package" in res.output and "'1'" in res.output and not out.exists()


@pytest.mark.parametrize("flags", [(), ("--fliplr",), ("--flipud", "--flipxy"), ("--add_offset",)])
def test_without_the_flag_the_yaml_is_the_metadata_path(tmp_path, flags):
    from biahub_amd.stitch import estimate_stitch_translations

    positions, _, stage = _grid_plate(tmp_path)
    out = tmp_path / "s.yml"
    res = _run("estimate-stitch", "-i", *positions, "-o", out, *flags, "--pcc-z-index", "1", "--pcc-overlap", "16")
    assert res.exit_code == 0, res.output
    got = yaml.safe_load(out.read_text())["total_translation"]
    a = np.array([[0.0, *stage[n]] for n in stage])
    a -= a.min(axis=0)
    if "--fliplr" in flags:
        a[:, 2] *= -1
    if "--flipud" in flags:
        a[:, 1] *= -1
    if "--flipxy" in flags:
        a[:, [1, 2]] = a[:, [2, 1]]
    a -= np.minimum(a.min(axis=0), 0)
    want = {n: [float(v) for v in np.round(a[k], 2)] for k, n in enumerate(stage)}
    assert got == want
    stage_um = {n: (10.0, -300.0 + y * 0.5, 1000.0 + x * 0.25) for n, (y, x) in stage.items()}
    assert got == estimate_stitch_translations(stage_um, (2.0, 0.5, 0.25), fliplr="--fliplr" in flags, flipud="--flipud" in flags,
                                               flipxy="--flipxy" in flags)


def test_read_plane_reads_the_plane(tmp_path):
    from biahub_amd import io

    positions, wells, _ = _grid_plate(tmp_path, tile=(24, 40))
    arr = io.open_ome_zarr(positions[2]).data
    assert np.array_equal(arr.read_plane(0, 1, 1), wells["A/1"]["001000"])
    assert not arr.read_plane(0, 1, 0).any() and not arr.read_plane(0, 0, 1).any()
    assert np.array_equal(arr.read_plane(0, 1, 1), arr.read_volume(0, 1)[1])
    with pytest.raises(IndexError):
        arr.read_plane(0, 1, 2)
