"""GPU: bh_stitch_edge_shifts (csrc/stitch_pcc.hip) against the float64 restatement (tests/stitch_pcc_ref.py), and
``estimate-stitch --pcc-channel-name`` end to end.

Margins.  The kernels are a float32 evaluation of the restatement's formula, as the reference's pipeline is.  The fixtures
record, per case, how far the reference's float32 pipeline is from the restatement (tests/golden/make_stitch_pcc_golden.py):
prepared strips and shifted correlation as max |ref - restatement| / max |restatement|, confidence as an absolute difference.
The GPU is held to 4 x that figure, per case: the factor covers another FFT factorisation and another summation order.  Shifts
are integers and must be equal; a confidence that is exactly 0 in the restatement (the peak's window read as an empty numpy
slice) must be exactly 0.

Measured on an MI355X, worst over the 30 cases of got / allowed: prepared strips 0.020, correlation 0.018 (the float32 rounding
of the two test outputs; the call works in float64), confidence 4.2e-7; every shift equal.
"""

import json
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from click.testing import CliRunner

import stitch_pcc_ref as R
from biahub_amd.cli import cli, expand_eat_all
from biahub_amd.estimate_stitch import edge_shifts, optimal_positions

pytestmark = pytest.mark.gpu

META = json.loads((Path(__file__).resolve().parent / "golden" / "stitch_pcc.json").read_text())
EDGE_CASES = META["edge_cases"]
FACTOR = 4.0


def _key(c):
    return (tuple(c["tile"]), c["overlap"], c["dtype"], c["flipud"], c["fliplr"])


GROUPS: dict = {}
for _c in EDGE_CASES:
    GROUPS.setdefault(_key(_c), []).append(_c)


@pytest.fixture(scope="module")
def cases():
    """name -> (tile a, tile b, restatement), computed once and only read."""
    out = {}
    for c in EDGE_CASES:
        a, b = R.cut_pair(c["seed"], tuple(c["tile"]), c["relation"], c["overlap"], tuple(c["disp"]), c["dtype"], c["flipud"], c["fliplr"])
        out[c["name"]] = (a, b, R.register_edge(a, b, c["relation"], c["overlap"], c["flipud"], c["fliplr"]))
    return out


def _call(gpu, group, cases, **kw):
    c0 = group[0]
    ta = [torch.from_numpy(cases[c["name"]][0]).to(gpu) for c in group]
    tb = [torch.from_numpy(cases[c["name"]][1]).to(gpu) for c in group]
    res = edge_shifts(ta, tb, [c["relation"] for c in group], overlap=c0["overlap"], flipud=c0["flipud"], fliplr=c0["fliplr"], **kw)
    return ta, tb, res


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _rel(got, ref):
    return float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("key", list(GROUPS), ids=[f"{k[0][0]}x{k[0][1]}_o{k[1]}_{k[2]}_ud{int(k[3])}_lr{int(k[4])}" for k in GROUPS])
def test_batch_matches_the_restatement(gpu, cases, key):
    group = GROUPS[key]
    assert {c["relation"] for c in group} == {R.BELOW, R.RIGHT}  # one call, mixed relations
    ta, tb, (shifts, conf, prepared, corr) = _call(gpu, group, cases, return_intermediates=True)
    keep = [t.clone() for t in ta + tb]
    torch.cuda.synchronize()
    failures = []
    for k, c in enumerate(group):
        ref = cases[c["name"]][2]
        dev = c["deviation"]
        r_prep = max(_rel(prepared[k][i], ref["prepared"][i]) for i in (0, 1))
        r_corr = _rel(corr[k], ref["corr"])
        d_conf = abs(conf[k] - ref["confidence"])
        print(f"{c['name']}: shift {shifts[k].tolist()} (ref {list(ref['shift'])}) confidence {conf[k]:.9f} (ref {ref['confidence']:.9f}) "
              f"prepared {r_prep:.3e} / {FACTOR * dev['prepared']:.3e} corr {r_corr:.3e} / {FACTOR * dev['corr']:.3e} "
              f"|d confidence| {d_conf:.3e} / {FACTOR * dev['confidence']:.3e}")
        if shifts[k].tolist() != [float(v) for v in ref["shift"]] or shifts[k].tolist() != [float(v) for v in c["shift"]]:
            failures.append((c["name"], "shift", shifts[k].tolist(), ref["shift"]))
        if c["zero_confidence"]:
            if ref["confidence"] != 0.0 or conf[k] != 0.0:
                failures.append((c["name"], "confidence must be exactly 0", conf[k]))
        elif not d_conf <= FACTOR * dev["confidence"]:
            failures.append((c["name"], "confidence", d_conf, FACTOR * dev["confidence"]))
        if not r_prep <= FACTOR * dev["prepared"]:
            failures.append((c["name"], "prepared", r_prep, FACTOR * dev["prepared"]))
        if not r_corr <= FACTOR * dev["corr"]:
            failures.append((c["name"], "corr", r_corr, FACTOR * dev["corr"]))
    assert all(torch.equal(_bits(t), _bits(k_)) for t, k_ in zip(ta + tb, keep))  # inputs are untouched
    assert not failures, failures


def test_inputs_are_untouched_and_production_call_agrees(gpu, cases):
    group = GROUPS[((64, 64), 48, "float32", False, False)]
    ta = [torch.from_numpy(cases[c["name"]][0]).to(gpu) for c in group]
    tb = [torch.from_numpy(cases[c["name"]][1]).to(gpu) for c in group]
    before = [t.clone() for t in ta + tb]
    shifts, conf = edge_shifts(ta, tb, [c["relation"] for c in group], overlap=48)
    s2, c2, _, _ = edge_shifts(ta, tb, [c["relation"] for c in group], overlap=48, return_intermediates=True)
    torch.cuda.synchronize()
    assert all(torch.equal(t, b) for t, b in zip(ta + tb, before))
    assert np.array_equal(shifts, s2) and np.array_equal(conf, c2)  # the optional outputs change nothing
    assert shifts.tolist() == [[float(v) for v in c["shift"]] for c in group]


@pytest.mark.parametrize("key", [((64, 64), 48, "uint16", True, False), ((320, 320), 300, "float32", True, False)],
                         ids=["64x64_o48", "320x320_o300"])
def test_batch_equals_single_calls_bit_for_bit(gpu, cases, key):
    group = GROUPS[key]
    _, _, (shifts, conf, prepared, corr) = _call(gpu, group, cases, return_intermediates=True)
    for k, c in enumerate(group):
        _, _, (s1, c1, p1, r1) = _call(gpu, [c], cases, return_intermediates=True)
        assert np.array_equal(s1[0], shifts[k]) and c1[0] == conf[k], c["name"]
        assert torch.equal(p1[0][0], prepared[k][0]) and torch.equal(p1[0][1], prepared[k][1]) and torch.equal(r1[0], corr[k]), c["name"]


def test_bad_arguments_are_value_errors(gpu):
    t = torch.zeros((32, 40), dtype=torch.uint16, device=gpu)
    for kw, rel in ((dict(overlap=15), [R.BELOW]), (dict(overlap=33), [R.BELOW]), (dict(overlap=41), [R.RIGHT]), (dict(overlap=16), [2])):
        with pytest.raises(ValueError):
            edge_shifts([t], [t], rel, **kw)
    with pytest.raises(ValueError):
        edge_shifts([t], [t.to(torch.float32)], [R.BELOW], overlap=16)
    with pytest.raises(ValueError):
        edge_shifts([t.to(torch.float64)], [t.to(torch.float64)], [R.BELOW], overlap=16)
    shifts, conf = edge_shifts([t], [t], [R.RIGHT], overlap=33)  # within X = 40: the strip axis of RIGHT is X
    assert shifts.shape == (1, 2) and conf.shape == (1,)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def _run(*args):
    return CliRunner().invoke(cli, expand_eat_all([str(a) for a in args]))


def _well(seed, grid_xy, tile, overlap, errors, dtype, flipud=False, fliplr=False):
    tiles = R.well_tiles(seed, grid_xy, tile, overlap, errors, dtype, flipud, fliplr)
    names = {c: f"{c[0]:03d}{c[1]:03d}" for c in tiles}
    fovs = {names[c]: tiles[c] for c in sorted(tiles)}
    stage = {names[c]: (float(c[1] * (tile[0] - overlap)), float(c[0] * (tile[1] - overlap))) for c in tiles}
    return fovs, stage


def test_estimate_stitch_refines_a_2x2_well_and_stitch_consumes_it(gpu, tmp_path):
    errors = {(1, 0): (3, -4), (0, 1): (-2, 5), (1, 1): (4, 2)}
    fovs, stage = _well(31, (2, 2), (320, 320), 300, errors, "uint16")
    wells = {"A/1": fovs}
    stage_px = {f"A/1/{n}": v for n, v in stage.items()}
    positions = R.write_plate(tmp_path / "in.zarr", wells, stage_px, chunks_yx=(160, 320))
    cfg = tmp_path / "s.yml"
    res = _run("estimate-stitch", "-i", *positions, "-o", cfg, "--pcc-channel-name", "Phase", "--pcc-z-index", 1)
    assert res.exit_code == 0, res.output
    assert "Confidence scores:" in res.output and res.output.count("]: 0.") + res.output.count("]: 1.") == 4
    got = yaml.safe_load(cfg.read_text())["total_translation"]
    want = R.expected_translations(wells, stage_px, 300, solver=optimal_positions)
    print(got, want)
    assert got == want
    assert any(got[n][1:] != [float(v) for v in stage_px[n]] for n in got)  # the refinement moved something
    out = tmp_path / "out.zarr"
    res = _run("stitch", "-i", *positions, "-c", cfg, "-o", out)
    assert res.exit_code == 0, res.output
    assert (out / "A" / "1" / "0").is_dir()


def test_estimate_stitch_refines_a_3x2_well_with_fliplr(gpu, tmp_path):
    errors = {(1, 0): (2, 3), (2, 0): (-1, -3), (0, 1): (3, 1), (1, 1): (-2, -2), (2, 1): (1, 4)}
    fovs, stage = _well(48, (3, 2), (96, 96), 32, errors, "float32", fliplr=True)
    single = {"000000": fovs["000000"]}
    wells = {"A/1": fovs, "B/2": single}
    stage_px = {**{f"A/1/{n}": v for n, v in stage.items()}, "B/2/000000": (5.0, 9.0)}
    positions = R.write_plate(tmp_path / "in.zarr", wells, stage_px)
    cfg = tmp_path / "s.yml"
    res = _run("estimate-stitch", "-i", *positions, "-o", cfg, "--pcc-channel-name", "Phase", "--pcc-z-index", 1, "--pcc-overlap", 32,
               "--fliplr", "--add_offset")
    assert res.exit_code == 0, res.output
    got = yaml.safe_load(cfg.read_text())["total_translation"]
    want = R.expected_translations(wells, stage_px, 32, fliplr=True, solver=optimal_positions)
    print(got, want)
    assert got == want and got["B/2/000000"] == [0.0, 0.0, 0.0]  # a single-FOV well keeps its metadata shifts
