"""GPU: the life cycle of the cached hipFFT plan sets through their one owner (csrc/context.hip: build_plans, destroy_plans,
stream_plans, cached_plans).  What the three families compute is held by their own tests (test_gpu_focus.py,
test_gpu_stitch_pcc.py, test_gpu_pcc_f64.py, test_gpu_parity.py); here the sets are released and rebuilt, moved to another
stream and back, and built side by side from integers that coincide.

Slices (float32 R2C, csrc/focus.hip) and strips (float64 D2Z / Z2D, csrc/stitch_pcc.hip) promise repeatable bits, so their results
are compared bit for bit.  Volumes (csrc/deconv.hip: bh_phase_cross_corr on the library route) are held as
test_pcc_library_route_vs_float64 holds them: the shift equal to the float64 reference's, the correlation volume inside
``pcc_bounds`` of it; the shifts of two runs are equal.  No tolerance of its own.
"""

import json
from pathlib import Path

import numpy as np
import pytest
import torch

import focus_ref
import pcc_cases as P
import stitch_pcc_ref as S
from biahub_amd.device import get_context
from biahub_amd.estimate_stabilization import phase_cross_corr_device
from biahub_amd.estimate_stitch import edge_shifts
from biahub_amd.focus import midband_power_and_sum
from fft_metrics import assert_fft_close, pcc_bounds
from oracle import reference_f64

pytestmark = pytest.mark.gpu

FOCUS_META = json.loads((Path(__file__).resolve().parent / "golden" / "focus_cases.json").read_text())
FOCUS_CASE = next(c for c in FOCUS_META["cases"] if c["name"] == "f32_50x36")
OPTICS = dict(NA_det=FOCUS_META["NA_det"], lambda_ill=FOCUS_META["lambda_ill"])
# (shape, environment): a 3-D plan pair; the same shape decomposed on request; a power-of-two shape, decomposed by rule
VOLUMES = [((10, 20, 50), {}), ((10, 20, 50), {"BH_FFT_SEPARABLE": "1"}), ((8, 32, 64), {"BH_FFT_BACKEND": "hipfft"})]
# the cache is keyed by the shape alone, so the two kinds of plan of (10, 20, 50) never share a workspace
GROUPS = (VOLUMES[:1], VOLUMES[1:])
NORM, REMOVED, SHIFT = None, True, 2  # the mean-removed pair of the mixed-sign shift, no normalisation


@pytest.fixture(scope="module")
def inputs(gpu):
    """The window, the tiles, the volume pairs and their float64 references: built once and only read."""
    window = focus_ref.case_window(FOCUS_CASE)
    assert window.shape[0] % 3 != 0  # max_batch = 3: full batches and a shorter last one
    tiles = [S.cut_pair(11 + rel, (64, 64), rel, 48, (1, -2), "uint16") for rel in (S.BELOW, S.RIGHT)]
    ta = [torch.from_numpy(a).to(gpu) for a, _ in tiles]
    tb = [torch.from_numpy(b).to(gpu) for _, b in tiles]
    pairs = {}
    for shape in {s for s, _ in VOLUMES}:
        a, b = (torch.from_numpy(x).to(gpu) for x in P.class_inputs(*P.pair(shape, SHIFT), REMOVED))
        pairs[shape] = (a, b) + tuple(reference_f64.phase_cross_corr_f64(a, b, NORM))
    return window, ta, tb, pairs


def run_cached(gpu, inputs, monkeypatch, volumes):
    """Slices, strips and the volume settings ``volumes`` on whatever the cache holds, nothing released in between:
    (power, sum, strip shifts, confidences, [volume shift per setting]).  Each correlation volume is checked against its float64
    reference on the way, on the stream that computed it."""
    window, ta, tb, pairs = inputs
    power, total = midband_power_and_sum(window, pixel_size=FOCUS_CASE["pixel_size"], device=gpu, max_batch=3, **OPTICS)
    shifts, conf = edge_shifts(ta, tb, [S.BELOW, S.RIGHT], overlap=48)
    volume_shifts = []
    for shape, env in volumes:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        a, b, want_shift, want_corr = pairs[shape]
        shift, corr = phase_cross_corr_device(a, b, NORM, want_corr=True)
        for k in env:
            monkeypatch.delenv(k)
        assert np.array_equal(shift, want_shift), (shape, env, shift, want_shift)
        assert_fft_close(corr, want_corr, *pcc_bounds(NORM, REMOVED), f"{shape} {env}")
        volume_shifts.append(shift)
    return power, total, shifts, conf, volume_shifts


def run_all(gpu, inputs, monkeypatch):
    """Every input, each group of settings on a fresh workspace."""
    out = []
    for volumes in GROUPS:
        get_context(gpu).release_workspace()
        out.append(run_cached(gpu, inputs, monkeypatch, volumes))
    return out


def assert_same(got, want):
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]                    # slices: the same bits
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])      # strips: the same bits
    assert len(got[4]) == len(want[4]) and all(np.array_equal(a, b) for a, b in zip(got[4], want[4]))


def test_release_and_rebuild(gpu, inputs, monkeypatch):
    ctx = get_context(gpu)
    first = run_all(gpu, inputs, monkeypatch)
    assert all(int(np.argmax(r[0])) == FOCUS_CASE["focus"] for r in first)
    assert ctx.workspace_bytes() > 0
    ctx.release_workspace()
    assert ctx.workspace_bytes() == 0
    for got, want in zip(run_all(gpu, inputs, monkeypatch), first):
        assert_same(got, want)


def test_restream(gpu, inputs, monkeypatch):
    """Every set is cached on the default stream, then used on another stream (get_context rebinds the context, which re-streams
    every set it holds), then on the default stream again."""
    side = torch.cuda.Stream(gpu)
    for volumes in GROUPS:
        get_context(gpu).release_workspace()
        first = run_cached(gpu, inputs, monkeypatch, volumes)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert_same(run_cached(gpu, inputs, monkeypatch, volumes), first)
            side.synchronize()
        assert_same(run_cached(gpu, inputs, monkeypatch, volumes), first)
        torch.cuda.synchronize()


def test_families_do_not_meet(gpu, inputs):
    """Two slices of (48, 64) and two strips of (48, 64): the same integers, a float32 R2C plan and a float64 D2Z / Z2D pair.
    Whichever is built first, each call returns the bits it returns on a workspace of its own."""
    ctx = get_context(gpu)
    window = focus_ref.make_window((2, 48, 64), "float32", 1, seed=5)
    pairs = [S.cut_pair(21 + k, (64, 64), S.BELOW, 48, (k, 1), "uint16") for k in range(2)]
    ta = [torch.from_numpy(a).to(gpu) for a, _ in pairs]
    tb = [torch.from_numpy(b).to(gpu) for _, b in pairs]

    def slices():
        return midband_power_and_sum(window, pixel_size=0.25, device=gpu, **OPTICS)

    def strips():
        return edge_shifts(ta, tb, [S.BELOW, S.BELOW], overlap=48)

    ctx.release_workspace()
    power, total = slices()
    assert power.min() > 0
    ctx.release_workspace()
    shifts, conf = strips()
    for calls in ((slices, strips), (strips, slices)):
        ctx.release_workspace()
        got = {f: f() for f in calls}
        assert np.array_equal(got[slices][0], power) and got[slices][1] == total
        assert np.array_equal(got[strips][0], shifts) and np.array_equal(got[strips][1], conf)
