"""GPU: bh_focus_band_power (csrc/focus.hip) and biahub_amd/focus.py against the float64 restatement (tests/focus_ref.py), and
``estimate-stabilization`` with ``stabilization_type: z`` / ``focus-finding`` end to end into ``stabilize``.

Margins.  The device transforms in float32, as the reference's complex64 pipeline does, and sums |F| in float64.  The fixture
records, per case, how far the float32 evaluation of the restatement (scipy.fft, complex64) is from the float64 one, as
max |P32 - P64| / max P64 (tests/golden/make_focus_golden.py).  The GPU is held to 4 x that figure, per case and per slice: the
factor covers another FFT factorisation and another summation order.  The focus index must be equal; the fixture's generator
asserts that the float64 powers of every case decide it by a margin of at least 1e-3.

Measured on an MI355X, got / allowed per case: 0.278 for the (5, 16, 16) window (28 bins, recorded deviation 1.7e-7), 0.006 to
0.040 for the six others; every focus index equal.
"""

import csv
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from click.testing import CliRunner

import focus_ref as R
from biahub_amd import io
from biahub_amd.cli import cli, expand_eat_all
from biahub_amd.focus import _device_window, compute_midband_power, focus_from_transverse_band, midband_power_and_sum

pytestmark = pytest.mark.gpu

META = json.loads((Path(__file__).resolve().parent / "golden" / "focus_cases.json").read_text())
CASES = {c["name"]: c for c in META["cases"]}
FACTOR = 4.0
OPTICS = dict(NA_det=META["NA_det"], lambda_ill=META["lambda_ill"])


@pytest.fixture(scope="module")
def windows():
    """name -> (window, float64 powers of the restatement), computed once and only read."""
    out = {}
    for name, c in CASES.items():
        v = R.case_window(c)
        v.setflags(write=False)
        out[name] = (v, R.midband_power(v, c["pixel_size"]))
    return out


def _ratio(got, ref, case):
    """worst slice: |got - ref| / max ref, over the allowed FACTOR x the case's recorded float32 deviation"""
    return float(np.abs(got - ref).max() / ref.max() / (FACTOR * case["f32_dev"]))


@pytest.mark.parametrize("name", list(CASES))
def test_power_and_index_against_the_restatement(gpu, windows, name):
    c = CASES[name]
    v, ref = windows[name]
    got, total = midband_power_and_sum(v, pixel_size=c["pixel_size"], device=gpu, **OPTICS)
    assert got.dtype == np.float64 and got.shape == (c["shape"][0],)
    ratio = _ratio(got, ref, c)
    print(f"{name}: got / allowed = {ratio:.4f}")
    assert ratio <= 1.0
    assert focus_from_transverse_band(v, pixel_size=c["pixel_size"], device=gpu, **OPTICS) == R.focus_index(ref) == c["focus"]
    if v.dtype != np.float32:
        assert total == float(v.astype(np.int64).sum())  # exact
    else:
        assert abs(total - v.astype(np.float64).sum()) <= 1e-12 * v.astype(np.float64).sum()
    again, total2 = midband_power_and_sum(v, pixel_size=c["pixel_size"], device=gpu, **OPTICS)
    assert np.array_equal(got, again) and total2 == total  # the same bits


@pytest.mark.parametrize("name", ["f32_50x36", "u16_200x200"])
def test_chunked_call(gpu, windows, name):
    """Z = 7 and Z = 11 in chunks of 3 slices: a chunk edge and a shorter last chunk."""
    c = CASES[name]
    v, ref = windows[name]
    assert c["shape"][0] in (7, 11)
    got, total = midband_power_and_sum(v, pixel_size=c["pixel_size"], device=gpu, max_batch=3, **OPTICS)
    assert _ratio(got, ref, c) <= 1.0 and int(np.argmax(got)) == c["focus"]
    assert abs(total - v.astype(np.float64).sum()) <= 1e-12 * v.astype(np.float64).sum()
    one, _ = midband_power_and_sum(v, pixel_size=c["pixel_size"], device=gpu, max_batch=1, **OPTICS)
    assert _ratio(one, ref, c) <= 1.0


@pytest.mark.parametrize("name", ["u8_96x64_last", "u16_64x96"])
def test_window_read_in_place(gpu, windows, name):
    """The window inside a larger volume, at odd y0 and x0 and with a row stride that is no multiple of 4, is read through its
    strides and gives the bits of its contiguous copy."""
    c = CASES[name]
    v, ref = windows[name]
    Z, Y, X = v.shape
    y0, x0 = 3, 5
    rng = np.random.default_rng(1)
    vol = rng.integers(0, 200, (Z, Y + 7, X + 9)).astype(v.dtype)
    assert vol.shape[2] % 4 != 0
    vol[:, y0:y0 + Y, x0:x0 + X] = v
    vol_t = torch.from_numpy(vol).to(gpu)
    view = vol_t[:, y0:y0 + Y, x0:x0 + X]
    assert not view.is_contiguous() and _device_window(view, gpu)[0].data_ptr() == view.data_ptr()  # no copy is made
    in_place, s1 = midband_power_and_sum(view, pixel_size=c["pixel_size"], **OPTICS)
    copied, s2 = midband_power_and_sum(view.contiguous(), pixel_size=c["pixel_size"], **OPTICS)
    from_host, s3 = midband_power_and_sum(v, pixel_size=c["pixel_size"], device=gpu, **OPTICS)
    assert np.array_equal(in_place, copied) and np.array_equal(in_place, from_host)
    assert s1 == s2 == s3 == float(v.astype(np.int64).sum())
    assert _ratio(in_place, ref, c) <= 1.0
    assert focus_from_transverse_band(view, pixel_size=c["pixel_size"], **OPTICS) == c["focus"]
    # every alignment of the first element, with the window's last rows ending at the volume's end
    for dx in range(4):
        sub = vol_t[:, 7:, dx:dx + 32]
        got = compute_midband_power(sub, pixel_size=c["pixel_size"], **OPTICS)
        assert np.array_equal(got, compute_midband_power(sub.contiguous(), pixel_size=c["pixel_size"], **OPTICS))


def test_empty_volume_and_band_without_bins(gpu, windows):
    zeros = np.zeros((4, 32, 32), np.uint16)
    power, total = midband_power_and_sum(zeros, pixel_size=0.1494, device=gpu, **OPTICS)
    assert np.array_equal(power, np.zeros(4)) and total == 0.0
    assert focus_from_transverse_band(zeros, pixel_size=0.1494, device=gpu, **OPTICS) == 0
    v, _ = windows["min16_f32"]
    power, total = midband_power_and_sum(v, pixel_size=0.1494, midband_fractions=(0.01, 0.011), device=gpu, **OPTICS)
    assert np.array_equal(power, np.zeros(v.shape[0])) and total > 0  # as in the reference: an empty mask sums to 0


# ---------------------------------------------------------------------------------------------------------------- end to end
FOCUS = {("A", "1", "0"): [3, 4, 2, 5], ("B", "2", "0"): [2, 2, 3, 1]}


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    root = tmp_path_factory.mktemp("focus_plate")
    store = root / "in.zarr"
    io.create_empty_plate(store, list(FOCUS), ["ch0", "ch1"], (4, 2, 7, 64, 64), chunks=(1, 1, 7, 64, 64), scale=(1, 1, 0.5, 0.1494, 0.1494),
                          dtype=np.uint16)
    data = {}
    for k, (key, focus) in enumerate(FOCUS.items()):
        pos = io.open_ome_zarr(store / "/".join(key))
        for t, f in enumerate(focus):
            data[key, t] = R.make_window((7, 64, 64), "uint16", f, seed=100 + 10 * k + t)
            pos.data[t, 1] = data[key, t]
    return root, store, data


def _estimate(root, store, out, extra=""):
    cfg = root / f"{out}.yml"
    cfg.write_text("stabilization_estimation_channel: ch1\nstabilization_channels: [ch0, ch1]\nstabilization_type: z\n"
                   "focus_finding_settings:\n  center_crop_xy: [48, 40]\n" + extra)
    res = CliRunner().invoke(cli, expand_eat_all(["estimate-stabilization", "-i", *[str(store / "/".join(k)) for k in FOCUS], "-o", str(root / out),
                                                  "-c", str(cfg), "--local"]))
    assert res.exit_code == 0, res.output
    assert "Estimating z stabilization parameters with focus finding" in res.output
    return root / out


def test_cli_estimate_z_then_stabilize(gpu, plate):
    root, store, data = plate
    out = _estimate(root, store, "est")
    for key, focus in FOCUS.items():
        est = yaml.safe_load((out / "z_stabilization_settings" / ("_".join(key) + ".yml")).read_text())
        mats = np.array(est["affine_transform_zyx_list"])
        assert mats.shape == (4, 4, 4)
        for t, m in enumerate(mats):
            want = np.eye(4)
            want[0, 3] = 0 if t == 0 else focus[t] - focus[0]
            assert np.array_equal(m, want), (key, t, m)
        assert est["stabilization_type"] == "z" and est["stabilization_method"] == "focus-finding" and est["time_indices"] == "all"
        assert est["stabilization_estimation_channel"] == "ch1" and est["stabilization_channels"] == ["ch0", "ch1"]
        assert est["output_voxel_size"] == [1, 1, 0.5, 0.1494, 0.1494]
    with open(out / "positions_focus.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["position", "time_idx", "channel", "focus_idx"]
    assert rows[1:] == [["/".join(key), str(t), "ch1", str(f)] for key in sorted(FOCUS) for t, f in enumerate(FOCUS[key])]
    assert not (out / "z_focus_positions").exists() and not (out / "z_transforms").exists()
    # a second run on one position merges into the existing table: same rows
    cfg = root / "est.yml"
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", str(store / "B/2/0"), "-o", str(out), "-c", str(cfg), "--local"])
    assert res.exit_code == 0 and "Using existing focus CSV file." in res.output, res.output
    with open(out / "positions_focus.csv", newline="") as f:
        assert list(csv.reader(f)) == rows
    # stabilize consumes the file: plane z of the output is plane z + (f_t - f_0) of the input, the in-focus plane lands at f_0
    key, focus = ("A", "1", "0"), FOCUS[("A", "1", "0")]
    stab = root / "stab.zarr"
    res = CliRunner().invoke(cli, ["stabilize", "-i", str(store / "A/1/0"), "-c", str(out / "z_stabilization_settings" / "A_1_0.yml"), "-o", str(stab),
                                   "--local"])
    assert res.exit_code == 0, res.output
    sp = io.open_ome_zarr(stab / "A/1/0")
    for t in range(4):
        d = focus[t] - focus[0]
        vol, got = data[key, t].astype(np.float32), np.asarray(sp.data[t, 1])
        for z in range(7):
            want = vol[z + d] if 0 <= z + d < 7 else np.zeros_like(vol[0])
            assert np.abs(got[z] - want).max() <= 1e-5 * vol.max(), (t, z)


def test_cli_average_across_wells(gpu, plate):
    root, store, _ = plate
    out = _estimate(root, store, "avg", "  average_across_wells: true\n")
    assert sorted(p.name for p in (out / "z_stabilization_settings").iterdir()) == ["average.yml"]
    mats = np.array(yaml.safe_load((out / "z_stabilization_settings" / "average.yml").read_text())["affine_transform_zyx_list"])
    mean = [(a + b) / 2 for a, b in zip(*FOCUS.values())]  # 2.5, 3, 2.5, 3
    assert [m[0, 3] for m in mats] == [0.0] + [v - mean[0] for v in mean[1:]]
    out = _estimate(root, store, "med", "  average_across_wells: true\n  average_across_wells_method: median\n")
    mats2 = np.array(yaml.safe_load((out / "z_stabilization_settings" / "average.yml").read_text())["affine_transform_zyx_list"])
    assert np.array_equal(mats2, mats)  # the median of two values is their mean
