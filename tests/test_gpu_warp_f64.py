"""GPU: the linear and nearest affine warps (bh_affine: csrc/affine.hip, affine_zwalk.inc, affine_zoblique.inc) on every launch
against the float64 reference (oracle/reference_f64.py: warp_f64), per voxel.

``|got - V| <= K 2^-24 M`` at every voxel — K = 16 for lerp8 (linear with an edge clamp), 28 for the generic path (linear with the
ZEROS boundary), 0 for nearest —, exact zeros where M == 0, ``cval`` bit for bit outside, never a NaN or an infinity: the bounds
are derived at the head of tests/warp_cases.py, which also holds the inputs (beads of 3 000 .. 60 000 counts on a background of
110), the matrices and the restated launch rules; tests/test_warp_reference.py shows on the CPU that every warp reaches the launch
it names and every form the kernels choose per tile and per wave, that float32 restatements sit under the bounds, and that the
bounds bite.

Every run asserts the launch ``bh_affine_path`` reports against the restated rule, and every case also runs with
BH_AFFINE_NOZWALK=1: the staged-tile kernel, the anchor of the bit-identity tests in test_gpu_parity.py, held to float64 itself.
What runs here and nowhere else under a comparison: the ZEROS boundary, block geometries 1 and 2 and blocks whose box is not
staged, uint8 / int16 on the tile and block kernels, a float32 volume whose first element is off the 16-byte grid, volumes one
voxel thick, tiles without a source voxel, a z flip, and a +inf beside a -inf.  Every case prints ``F64 warp ...`` lines (``-s``).
"""

import functools

import numpy as np
import pytest
import torch

import warp_cases as W
from oracle import reference_f64 as R

pytestmark = pytest.mark.gpu

SWITCHES = ("BH_AFFINE_NOZWALK", "BH_AFFINE_NOOBLIQUE", "BH_AFFINE_GATHER", "BH_AFFINE_GBLOCK", "BH_AFFINE_GATHER_ZX", "BH_ZW_NOLDS",
            "BH_ZW_WAVES", "BH_ZO_WAVES")
INTERPS = ("linear", "nearestneighbor")


@functools.lru_cache(maxsize=6)
def _input(shape, dtype, nonfinite=False, off_grid=False):
    """(the operator's input on the GPU, the same values as float32 for the reference: every input type widens exactly).
    ``off_grid``: a contiguous float32 view whose first element sits 4 bytes past a 16-byte boundary."""
    vol = np.array(W.volume(shape, dtype, nonfinite))
    ref = torch.from_numpy(vol.astype(np.float32)).cuda()
    if not off_grid:
        return torch.from_numpy(vol).cuda(), ref
    assert vol.dtype == np.float32
    buf = torch.empty(vol.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1: 1 + vol.size].view(vol.shape)
    view.copy_(ref)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view, ref


def run(gpu, monkeypatch, vol, m, out, lo, interp, boundary, **switches):
    """One bh_affine under the given BH_AFFINE_* switches (all others unset); returns (result, the launch it reports)."""
    from biahub_amd.register import affine_device, affine_path

    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv("BH_AFFINE_" + name, str(value))
    full = tuple(a + n for a, n in zip(lo, out))
    got = affine_device(vol, m, full, interp, boundary, W.CVAL, lo, out)
    path = affine_path(gpu)
    for name in switches:
        monkeypatch.delenv("BH_AFFINE_" + name)
    return got, path


def check(what, got, ref, interp, boundary):
    K = W.bound(interp, boundary)
    worst = W.assert_warp_close(got, ref, K, what, cval=None if boundary == W.ZEROS else W.CVAL)
    print(f"F64 warp {what}: {worst:.2f} u M (bound {K})")


def launches(gpu, monkeypatch, label, inp, m, shape, out, lo, dtype, interp, boundary, aligned=True, blocks=False):
    """The launch the rule selects (its code asserted) and the staged-tile kernel (BH_AFFINE_NOZWALK=1), each against float64 and
    bit-identical to each other; with ``blocks`` also block geometries 1 and 2 and BH_AFFINE_GATHER=0.  Returns the default result."""
    vol, vol32 = inp
    ref = R.warp_f64(vol32, m, out, lo, interp, boundary, W.CVAL)
    want = W.host_plan(m, shape, out, dtype, interp, boundary, aligned).path
    got, path = run(gpu, monkeypatch, vol, m, out, lo, interp, boundary)
    assert path == want, (label, path, want)
    tag = f"{dtype} {interp} boundary {boundary} [{label} {shape}{'' if lo == (0, 0, 0) else ' crop'}]"
    check(f"{W.PATH_NAMES[path]} | {tag}", got, ref, interp, boundary)
    tile, path = run(gpu, monkeypatch, vol, m, out, lo, interp, boundary, NOZWALK=1)
    assert path == W.TILE, label
    check(f"staged tiles, forced | {tag}", tile, ref, interp, boundary)
    assert torch.equal(got, tile), (label, interp, boundary)
    if blocks:
        assert want == W.BLOCKS, label
        for env in (dict(GBLOCK=1), dict(GBLOCK=2), dict(GATHER=0)):
            other, path = run(gpu, monkeypatch, vol, m, out, lo, interp, boundary, **env)
            assert path == (W.TILE if "GATHER" in env else W.BLOCKS), (label, env)
            check(f"{W.PATH_NAMES[path]} {env} | {tag}", other, ref, interp, boundary)
            assert torch.equal(got, other), (label, env)
    return got


# ----------------------------------------------------------------------------- every warp on the launch it is meant for
@pytest.mark.parametrize("name,shape,dtype,aligned", W.linear_cases(), ids=lambda v: str(v))
def test_warp_edge_clamp_vs_float64(gpu, monkeypatch, name, shape, dtype, aligned):
    """ITK and SCIPY_CONSTANT, linear and nearest: the whole output box (ragged in every axis, tiles wholly outside the source and
    tiles across every face) and a crop that starts mid-tile, which must equal that part of the whole."""
    m, out = W.pull_matrix(name, shape), W.OUT[shape]
    inp = _input(shape, dtype)
    for boundary in (W.ITK, W.SCIPY):
        for interp in INTERPS:
            whole = launches(gpu, monkeypatch, name, inp, m, shape, out, (0, 0, 0), dtype, interp, boundary, aligned)
            cs, lo = W.crop_shape(out), W.CROP_LO
            part = launches(gpu, monkeypatch, name, inp, m, shape, cs, lo, dtype, interp, boundary, aligned)
            assert torch.equal(part, whole[lo[0]: lo[0] + cs[0], lo[1]: lo[1] + cs[1], lo[2]: lo[2] + cs[2]]), (name, interp, boundary)


# ----------------------------------------------------------------------------- the ZEROS boundary
@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("name", W.ZEROS_WARPS)
def test_warp_zeros_boundary_vs_float64(gpu, monkeypatch, name, dtype):
    """Out-of-range neighbours count as cval (-3.5): the ``cover`` term, the ``> -2`` guard and the zeroed weights of axis_plan, on the
    tile kernel and on the compact blocks (no walk takes this boundary), linear and nearest, rows aligned and not."""
    for k, shape in enumerate(W.WARPS[name].shapes):
        m, out = W.pull_matrix(name, shape), W.OUT[shape]
        for interp in INTERPS:
            plan = W.host_plan(m, shape, out, dtype, interp, W.ZEROS, k == 0)
            assert plan.path in (W.TILE, W.BLOCKS)
            whole = launches(gpu, monkeypatch, name, _input(shape, dtype), m, shape, out, (0, 0, 0), dtype, interp, W.ZEROS, k == 0,
                             blocks=plan.path == W.BLOCKS)
            cs, lo = W.crop_shape(out), W.CROP_LO
            part = launches(gpu, monkeypatch, name, _input(shape, dtype), m, shape, cs, lo, dtype, interp, W.ZEROS, k == 0)
            assert torch.equal(part, whole[lo[0]: lo[0] + cs[0], lo[1]: lo[1] + cs[1], lo[2]: lo[2] + cs[2]]), (name, interp)


# ----------------------------------------------------------------------------- compact blocks, every geometry
@pytest.mark.parametrize("dtype", ["f32", "u16", "i16", "u8"])
@pytest.mark.parametrize("name", W.BLOCK_WARPS)
def test_warp_compact_blocks_vs_float64(gpu, monkeypatch, name, dtype):
    """BH_AFFINE_GBLOCK = 0 / 1 / 2 and the tile kernel's own gather (BH_AFFINE_GATHER=0): each against float64, all bit-identical.
    The 4x minifying rotation has blocks whose box exceeds the 12 288 and 16 384 floats a block may stage (taps from global memory)
    beside blocks that stage theirs."""
    shape = W.WARPS[name].shapes[0]
    m, out = W.pull_matrix(name, shape), W.OUT[shape]
    if name == "4x minifying rotation":
        assert all(W.block_forms(m, shape, out, (0, 0, 0), G)["not staged"] > 0 for G in W.GEO)
    for interp, boundary in (("linear", W.ITK), ("linear", W.SCIPY), ("nearestneighbor", W.ITK)):
        launches(gpu, monkeypatch, name, _input(shape, dtype), m, shape, out, (0, 0, 0), dtype, interp, boundary, blocks=True)
    launches(gpu, monkeypatch, name, _input(shape, dtype), m, shape, W.crop_shape(out), W.CROP_LO, dtype, "linear", W.ITK, blocks=True)


# ----------------------------------------------------------------------------- NaN, +inf, -inf, and a +inf beside a -inf
@pytest.mark.parametrize("name", W.NONFINITE_WARPS)
def test_warp_nonfinite_taps_vs_float64(gpu, monkeypatch, name):
    """``np.nan_to_num`` per tap: an isolated NaN, +inf and -inf and a +inf next to a -inf (along y inside a tile, along z on a tile
    seam), on every launch.  The reference blends the cleaned taps (+-FLT_MAX) into a finite value; a kernel that forms
    FLT_MAX - (-FLT_MAX) on the way returns an infinity or a NaN, which no bound admits."""
    for k, shape in enumerate(W.WARPS[name].shapes):
        m, out = W.pull_matrix(name, shape), W.OUT[shape]
        inp = _input(shape, "f32", True)
        for interp, boundary in (("linear", W.ITK), ("linear", W.SCIPY), ("linear", W.ZEROS), ("nearestneighbor", W.ITK)):
            want = W.host_plan(m, shape, out, "f32", interp, boundary, k == 0).path
            got = launches(gpu, monkeypatch, name + ", non-finite", inp, m, shape, out, (0, 0, 0), "f32", interp, boundary, k == 0,
                           blocks=want == W.BLOCKS)
            assert bool(torch.isfinite(got).all())
        cs, lo = W.crop_shape(out), W.CROP_LO
        part = launches(gpu, monkeypatch, name + ", non-finite", inp, m, shape, cs, lo, "f32", "linear", W.ITK, k == 0)
        whole, _ = run(gpu, monkeypatch, inp[0], m, out, (0, 0, 0), "linear", W.ITK)
        assert torch.equal(part, whole[lo[0]: lo[0] + cs[0], lo[1]: lo[1] + cs[1], lo[2]: lo[2] + cs[2]]), name


# ----------------------------------------------------------------------------- a volume off the 16-byte grid
@pytest.mark.parametrize("name", ["identity", "similarity 2 deg 1.02", "oblique 2 deg", "20 deg about y", "shear"])
def test_warp_float32_volume_off_the_16_byte_grid(gpu, monkeypatch, name):
    """``Xi % 4 == 0`` but the first element 4 bytes past a 16-byte boundary: no 16-byte staging, no LDS ring, no oblique walk — by
    the pointer test alone.  Against float64, and bit-identical to the same volume on the grid."""
    from biahub_amd.device import as_device_volume

    shape = W.WARPS[name].shapes[0]
    m, out = W.pull_matrix(name, shape), W.OUT[shape]
    for nonfinite in (False, True):
        view, ref32 = _input(shape, "f32", nonfinite, True)
        assert as_device_volume(view)[0].data_ptr() == view.data_ptr()      # handed to bh_affine as it is, not copied
        for interp, boundary in (("linear", W.ITK), ("linear", W.ZEROS), ("nearestneighbor", W.SCIPY)):
            plan = W.host_plan(m, shape, out, "f32", interp, boundary, aligned=False)
            assert not plan.x4 and plan.zslot == 0 and plan.path != W.OBLIQUE
            got = launches(gpu, monkeypatch, name + ", off the grid", (view, ref32), m, shape, out, (0, 0, 0), "f32", interp, boundary,
                           aligned=False, blocks=plan.path == W.BLOCKS)
            on_grid, _ = run(gpu, monkeypatch, _input(shape, "f32", nonfinite)[0], m, out, (0, 0, 0), interp, boundary)
            assert torch.equal(got, on_grid), (name, interp, boundary)


# ----------------------------------------------------------------------------- volumes one voxel thick
@pytest.mark.parametrize("dtype", ["f32", "u16", "u8"])
@pytest.mark.parametrize("shape", W.DEGENERATE, ids=str)
def test_warp_degenerate_volumes_vs_float64(gpu, monkeypatch, shape, dtype):
    """Zi == 1, Yi == 1, Xi == 1: both taps of that axis are the one sample there is.  The z walk takes the first two (Xi >= 2),
    the tile kernel the third; every boundary, linear and nearest."""
    out = W.DEGENERATE_OUT[shape]
    for similar in (False, True):
        m = W.degenerate_matrix(shape, out, similar)
        for boundary in (W.ITK, W.SCIPY, W.ZEROS):
            for interp in INTERPS:
                launches(gpu, monkeypatch, "similarity" if similar else "quarter-voxel shift", _input(shape, dtype), m, shape, out,
                         (0, 0, 0), dtype, interp, boundary)


def test_path_report_forgets_the_launch_after_a_refused_call(gpu, monkeypatch):
    from biahub_amd.register import affine_device, affine_path

    shape = W.T200
    got, path = run(gpu, monkeypatch, _input(shape, "f32")[0], W.pull_matrix("identity", shape), W.OUT[shape], (0, 0, 0), "linear", W.ITK)
    assert path == W.ZWALK
    bad = np.eye(4)
    bad[1, 2] = np.nan
    with pytest.raises((ValueError, RuntimeError), match="NaN"):
        affine_device(_input(shape, "f32")[0], bad, W.OUT[shape], "linear", W.ITK)
    assert affine_path(gpu) == -1


@pytest.mark.parametrize("shape", [W.T200, W.T198], ids=str)
def test_warp_overflow_rescue_at_its_clamp(gpu, monkeypatch, shape):
    """A shift whose y fraction is 0xffffff80 / 2^32 — it widens to 1.0f — on the volume that holds a +inf above a neighbour of
    -1.25 x 2^105: the plain blend overflows and the rescue's quarter-scale blend rounds to 2^126, above FLT_MAX / 4, so the result
    is finite only if the rescue clamps before it scales back (tests/test_warp_reference.py walks through the arithmetic).  On the
    z walk by the rule and on the staged tiles; every voxel under the bound, which admits no infinity."""
    out = W.OUT[shape]
    m = np.eye(4)
    m[:3, 3] = (-6.0, -10.0 + (1.0 - 2.0 ** -25), -64.0)
    assert int(R.llround_q32(m[:3])[1, 3]) & 0xFFFFFFFF == 0xFFFFFF80
    inp = _input(shape, "f32", True)
    for boundary in (W.ITK, W.SCIPY):
        got = launches(gpu, monkeypatch, "shift to the clamp, non-finite", inp, m, shape, out, (0, 0, 0), "f32", "linear", boundary,
                       shape == W.T200)
        z, y, x = W.NONFINITE_BIG[1]
        assert float(got[z + 6, y + 10, x + 64]) == W.FLT_MAX      # the blend at fraction 1.0f of the partner and FLT_MAX
