"""GPU: bh_stackreg_translation (csrc/stackreg.hip) and biahub_amd/stackreg.py against the float64 restatement
(tests/stackreg_ref.py), and ``estimate-stabilization`` with ``stabilization_type: xy`` / ``xyz`` and ``focus-finding`` end to end
into ``stabilize`` and back.

Margins.  Device and restatement run the same float64 algorithm and differ in summation order only, so both stop inside the
same basin: their shifts agree within EPS, the algorithm's own stop constant (without an accept/reject tie, far below it; the
worst difference is printed and recorded in §3.13).  Against the true shift of the synthetic scenes the device is held to the
restatement's own worst error on these fixtures (stackreg_ref.RECOVERY_BOUND_*) plus EPS.  With ``t_reference: previous`` the
matrix of timepoint t is the sum of t pairwise shifts, each within the bound: it is held to t times the bound.

Measured on an MI355X: worst |device - restatement| over the 28 cases 8.9e-16 px, every status and iteration count equal; the
closed loop leaves 0.0005 px.
"""

import warnings

import numpy as np
import pytest
import torch
import yaml
from click.testing import CliRunner

import stackreg_ref as R
from biahub_amd import io
from biahub_amd.cli import cli, expand_eat_all
from biahub_amd.stackreg import _frames_on_device, register_stack, register_translation_pairs

pytestmark = pytest.mark.gpu

KINDS = [(noise, dt) for noise in (False, True) for dt in ("float32", "uint16")]


@pytest.mark.parametrize("noise,dtype_name", KINDS)
@pytest.mark.parametrize("index", range(len(R.CASES)), ids=[c[0] for c in R.CASES])
def test_shift_against_the_restatement_and_the_truth(gpu, index, noise, dtype_name):
    tyx, ref_shift, ref_mse, ref_status, ref_iters = R.reference_result(index, noise, dtype_name)
    shift, mse, status, iters = register_translation_pairs(tyx, [(1, 0)], device=gpu)
    assert shift.shape == (1, 2) and shift.dtype == np.float64 and status.dtype == np.int32
    diff = float(np.abs(shift[0] - ref_shift).max())
    err = float(np.abs(shift[0] - np.array(R.CASES[index][3])).max())
    print(f"{R.CASES[index][0]} noise={noise} {dtype_name}: |gpu - restatement| = {diff:.3e} px, |gpu - truth| = {err:.4f} px, "
          f"iterations {int(iters[0])} / {ref_iters}")
    assert status[0] == ref_status == R.CONVERGED
    assert diff <= R.EPS
    assert err <= (R.RECOVERY_BOUND_NOISY if noise else R.RECOVERY_BOUND_NOISELESS) + R.EPS
    assert abs(mse[0] - ref_mse) <= 1e-3 * ref_mse + 1e-12
    if R.CASES[index][3] == (0.0, 0.0) and not noise:
        assert shift[0, 0] == 0.0 and shift[0, 1] == 0.0 and mse[0] == 0.0  # identical frames: exactly zero


@pytest.fixture(scope="module")
def stack5():
    """Five frames of 49 x 63 with a cumulative drift, uint16, Poisson noise; only read."""
    H, W = 49, 63
    scene = R.blobs(H, W, seed=77)
    drift = np.array([(0.0, 0.0), (1.2, -0.8), (2.1, -2.0), (1.5, -3.3), (3.4, -4.1)])
    tyx = np.stack([R.render(H, W, scene, tuple(s), noise_seed=200 + t, dtype=np.uint16) for t, s in enumerate(drift)])
    tyx.setflags(write=False)
    return tyx, drift


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_read_in_place(gpu, stack5):
    """A window of a larger resident array, at odd offsets and with a row stride that is no multiple of 4, is read through its
    strides and gives the bits of its contiguous copy and of the uploaded host array."""
    tyx, _ = stack5
    T, H, W = tyx.shape
    big = np.random.default_rng(3).integers(0, 500, (T, H + 7, W + 10)).astype(np.uint16)
    big[:, 3:3 + H, 5:5 + W] = tyx
    big_t = torch.from_numpy(big).to(gpu)
    view = big_t[:, 3:3 + H, 5:5 + W]
    pairs = [(1, 0), (2, 1), (4, 0)]
    assert not view.is_contiguous() and _frames_on_device(view, [0, 1, 2, 3, 4], gpu)[0].data_ptr() == view.data_ptr()  # no copy
    in_place = register_translation_pairs(view, pairs)
    assert _same(in_place, register_translation_pairs(view.contiguous(), pairs))
    assert _same(in_place, register_translation_pairs(tyx, pairs, device=gpu))
    # the pairs' frames as a run inside the stack: the view starts at frame 2
    assert _same(register_translation_pairs(view, [(3, 2), (4, 3)]), register_translation_pairs(tyx[2:], [(1, 0), (2, 1)], device=gpu))


def test_int16_negatives_read_as_zero(gpu, stack5):
    tyx, _ = stack5
    signed = tyx.astype(np.int16) - 300  # the background of 100 and the blobs' skirts go negative
    assert (signed < 0).mean() > 0.2
    pairs = [(1, 0), (2, 0)]
    assert _same(register_translation_pairs(signed, pairs, device=gpu),
                 register_translation_pairs(np.clip(signed, 0, None), pairs, device=gpu))
    u8 = (tyx // 8).astype(np.uint8)
    assert _same(register_translation_pairs(u8, pairs, device=gpu), register_translation_pairs(u8.astype(np.float32), pairs, device=gpu))


def test_batch_independence(gpu, stack5):
    tyx, _ = stack5
    pairs = [(1, 0), (2, 1), (3, 2), (4, 3), (4, 0)]
    batch = register_translation_pairs(tyx, pairs, device=gpu)
    assert _same(batch, register_translation_pairs(tyx, pairs, device=gpu))  # two runs: the same bits
    for k in (0, 2, 4):
        alone = register_translation_pairs(tyx, [pairs[k]], device=gpu)
        assert all(np.array_equal(a[0], b[k]) for a, b in zip(alone, batch)), k
    for max_frames in (2, 3):  # chunked over T: runs of pairs that name at most 2 or 3 frames
        assert _same(batch, register_translation_pairs(tyx, pairs, device=gpu, max_frames=max_frames))
    ref = R.register_pairs(tyx, pairs)
    assert np.abs(batch[0] - ref[0]).max() <= R.EPS and np.array_equal(batch[2], ref[2])


def test_register_stack(gpu, stack5):
    tyx, drift = stack5
    tol = R.RECOVERY_BOUND_NOISY + R.EPS
    first = register_stack(tyx, reference="first", device=gpu)
    prev = register_stack(tyx, reference="previous", device=gpu)
    assert first.shape == prev.shape == (5, 3, 3) and first.dtype == np.float64
    assert np.array_equal(first[0], np.eye(3)) and np.array_equal(prev[0], np.eye(3))
    for t in range(1, 5):
        assert abs(first[t, 1, 2] - drift[t, 0]) <= tol and abs(first[t, 0, 2] - drift[t, 1]) <= tol
        assert abs(prev[t, 1, 2] - drift[t, 0]) <= t * tol and abs(prev[t, 0, 2] - drift[t, 1]) <= t * tol  # t pairwise errors add up
    pairwise, _, _, _ = register_translation_pairs(tyx, [(t, t - 1) for t in range(1, 5)], device=gpu)
    run = np.zeros(2)
    for t in range(1, 5):
        run = run + pairwise[t - 1]
        assert prev[t, 1, 2] == run[0] and prev[t, 0, 2] == run[1]
    two = register_stack(tyx[:2], reference="previous", device=gpu)  # T = 2
    assert np.array_equal(two, first[:2])
    assert np.array_equal(register_stack(tyx[:1], device=gpu), np.eye(3)[None])  # T = 1: nothing to register
    with pytest.raises(ValueError):
        register_stack(tyx, reference="mean", device=gpu)


def test_degenerate_inputs(gpu, stack5):
    tyx, _ = stack5
    same = np.stack([tyx[1], tyx[1], tyx[1]])
    shift, mse, status, _ = register_translation_pairs(same, [(1, 0), (2, 1)], device=gpu)
    assert (shift == 0.0).all() and (status == 0).all() and (mse == 0.0).all()
    for blank in (np.full_like(tyx[0], 100), np.zeros_like(tyx[0])):
        stack = np.stack([tyx[0], blank, tyx[2]])
        shift, mse, status, _ = register_translation_pairs(stack, [(1, 0), (0, 1), (2, 0)], device=gpu)
        assert status.tolist() == [2, 2, 0] and (shift[:2] == 0.0).all() and np.isfinite(shift).all() and np.isfinite(mse).all()
        with pytest.warns(UserWarning, match="frames 1"):
            mats = register_stack(stack, reference="first", device=gpu)
        assert np.array_equal(mats[1], np.eye(3)) and np.isfinite(mats).all()
        with pytest.warns(UserWarning, match="frames 1.*2"):  # frame 1 as moving, then as reference
            register_stack(stack, reference="previous", device=gpu)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        register_stack(tyx[:3], device=gpu)
    nonfinite = tyx[:2].astype(np.float32)
    nonfinite[1, 5, 5] = np.inf
    shift, mse, status, _ = register_translation_pairs(nonfinite, [(1, 0)], device=gpu)
    assert status[0] == 2 and (shift == 0.0).all()
    with pytest.raises(ValueError):
        register_translation_pairs(tyx, [(5, 0)], device=gpu)


# ---------------------------------------------------------------------------------------------------------------- end to end
FOCUS = {("A", "1", "0"): [2, 3, 1, 2], ("B", "2", "0"): [1, 1, 2, 3]}
DRIFT = {("A", "1", "0"): [(0, 0), (1, -2), (3, 1), (-2, 2)], ("B", "2", "0"): [(0, 0), (-1, 0), (0, 3), (2, -3)]}  # (y, x)
WINDOWS = ("focus_finding_settings:\n  center_crop_xy: [48, 40]\n"
           "stack_reg_settings:\n  center_crop_xy: [64, 48]\n  focus_finding_settings:\n    center_crop_xy: [48, 40]\n")
BOUND = R.RECOVERY_BOUND_NOISELESS + R.EPS


@pytest.fixture(scope="module")
def plate(tmp_path_factory):
    """2 positions x 4 timepoints, C = 2, Z = 5, 64 x 80: the scene at its focus slice, displaced by an integer drift."""
    root = tmp_path_factory.mktemp("stackreg_plate")
    store = root / "in.zarr"
    io.create_empty_plate(store, list(FOCUS), ["ch0", "ch1"], (4, 2, 5, 64, 80), chunks=(1, 1, 5, 64, 80), scale=(1, 1, 0.5, 0.1494, 0.1494),
                          dtype=np.uint16)
    for k, key in enumerate(FOCUS):
        pos = io.open_ome_zarr(store / "/".join(key))
        scene = R.blobs(64, 80, seed=40 + k)
        for t, (f, s) in enumerate(zip(FOCUS[key], DRIFT[key])):
            pos.data[t, 1] = R.focus_volume(5, 64, 80, scene, f, s)
    return root, store


def _estimate(root, inputs, out, kind, extra=""):
    cfg = root / f"{out}.yml"
    cfg.write_text(f"stabilization_estimation_channel: ch1\nstabilization_channels: [ch0, ch1]\nstabilization_type: {kind}\n" + WINDOWS + extra)
    res = CliRunner().invoke(cli, expand_eat_all(["estimate-stabilization", "-i", *[str(p) for p in inputs], "-o", str(root / out), "-c", str(cfg),
                                                  "--local"]))
    assert res.exit_code == 0, res.output
    return root / out


def _matrices(path):
    est = yaml.safe_load(path.read_text())
    return np.array(est["affine_transform_zyx_list"]), est


@pytest.mark.parametrize("t_reference", ["first", "previous"])
def test_cli_xy(gpu, plate, t_reference):
    root, store = plate
    out = _estimate(root, [store / "/".join(k) for k in FOCUS], f"xy_{t_reference}", "xy", f"  t_reference: {t_reference}\n")
    assert sorted(p.name for p in (out / "xy_stabilization_settings").iterdir()) == ["A_1_0.yml", "B_2_0.yml"]
    assert not (out / "xy_transforms").exists() and (out / "positions_focus.csv").exists()
    for key in FOCUS:
        mats, est = _matrices(out / "xy_stabilization_settings" / ("_".join(key) + ".yml"))
        assert mats.shape == (4, 4, 4) and est["stabilization_type"] == "xy" and est["stabilization_method"] == "focus-finding"
        assert np.array_equal(mats[0], np.eye(4))
        for t in range(4):
            tol = BOUND * (t if t_reference == "previous" and t > 0 else 1)
            assert abs(mats[t][1, 3] - DRIFT[key][t][0]) <= tol and abs(mats[t][2, 3] - DRIFT[key][t][1]) <= tol, (key, t, mats[t])
            rest = mats[t].copy()
            rest[1, 3] = rest[2, 3] = 0
            assert np.array_equal(rest, np.eye(4))


def test_cli_xyz_then_stabilize_and_back(gpu, plate):
    root, store = plate
    out = _estimate(root, [store / "/".join(k) for k in FOCUS], "xyz", "xyz")
    for kind in ("xyz", "z", "xy"):
        assert sorted(p.name for p in (out / f"{kind}_stabilization_settings").iterdir()) == ["A_1_0.yml", "B_2_0.yml"]
    for key, focus in FOCUS.items():
        name = "_".join(key) + ".yml"
        xyz, est = _matrices(out / "xyz_stabilization_settings" / name)
        z, _ = _matrices(out / "z_stabilization_settings" / name)
        xy, _ = _matrices(out / "xy_stabilization_settings" / name)
        assert est["stabilization_type"] == "xyz" and est["output_voxel_size"] == [1, 1, 0.5, 0.1494, 0.1494]
        for t in range(4):
            want = np.eye(4)
            want[0, 3] = 0 if t == 0 else focus[t] - focus[0]
            assert np.array_equal(z[t], want)
            assert np.array_equal(xyz[t], xy[t] @ z[t])
            assert abs(xyz[t][1, 3] - DRIFT[key][t][0]) <= BOUND and abs(xyz[t][2, 3] - DRIFT[key][t][1]) <= BOUND
    # stabilize consumes the xyz file; on the stabilised store the estimate finds nothing left to correct
    stab = root / "stab.zarr"
    res = CliRunner().invoke(cli, ["stabilize", "-i", str(store / "A/1/0"), "-c", str(out / "xyz_stabilization_settings" / "A_1_0.yml"), "-o", str(stab),
                                   "--local"])
    assert res.exit_code == 0, res.output
    back = _estimate(root, [stab / "A/1/0"], "back", "xy")
    mats, _ = _matrices(back / "xy_stabilization_settings" / "A_1_0.yml")
    worst = float(np.abs(mats[:, 1:3, 3]).max())
    print(f"closed loop: worst residual xy shift {worst:.4f} px")
    assert worst <= 2 * BOUND
