"""GPU: the cubic B-spline warp (csrc/spline.hip: the three prefilter passes, the LDS-tiled and the global 64-tap gather, the in-place
plane combination) on every launch against the float64 reference (oracle/reference_f64.py: spline_coef_f64, cubic_warp_f64), per voxel.

``|coef - C| <= 32 u A + T S`` for the prefilter alone and ``|got - V| <= 48 u M + T S`` for the warp, u = 2^-24, A and M the local scales
the reference returns, S the volume's largest |sample| and T = 270 x 0.268^20: exact zeros where the scale is zero, ``cval`` bit for bit
outside, never a NaN or an infinity.  tests/cubic_cases.py derives the bounds and holds the inputs (beads of 3 000 .. 60 000 counts on
a background of 110), the matrices and the restated launch rules; tests/test_cubic_reference.py shows on the CPU that the reference is
SciPy's, that every case reaches the forms it names, that float32 restatements sit under the bounds and that the bounds bite.

Every run asserts the launches ``bh_spline_path`` reports against the restated rule.  Every case prints ``F64 cubic ...`` lines (``-s``).
"""

import functools

import numpy as np
import pytest
import torch

import cubic_cases as C
import warp_cases as W
from oracle import reference_f64 as R

pytestmark = pytest.mark.gpu

ENV = ("GATHER", "ZUNI", "TZ", "NT", "PITCH32")
_NP_CODE = {"float32": "DT_F32", "uint16": "DT_U16", "int16": "DT_I16", "uint8": "DT_U8"}


def _offset_view(vol, elements):
    """A contiguous device view of ``vol`` whose first element sits ``elements`` samples past a 256-byte boundary."""
    buf = np.zeros(vol.size + 16, vol.dtype)
    buf[elements: elements + vol.size] = vol.ravel()
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 256 == 0
    view = t[elements: elements + vol.size].view(vol.shape)
    assert view.is_contiguous() and view.data_ptr() == t.data_ptr() + elements * vol.dtype.itemsize
    return view


def prefilter(gpu, t):
    """bh_spline_prefilter on a device tensor; returns (coefficients, the code bh_spline_path reports)."""
    from biahub_amd import _lib
    from biahub_amd.device import get_context, ptr
    from biahub_amd.register import spline_path

    coef = torch.empty(tuple(t.shape), dtype=torch.float32, device=t.device)
    assert coef.data_ptr() % 16 == 0
    ctx = get_context(gpu)
    code = getattr(_lib, _NP_CODE[str(t.dtype).replace("torch.", "")])
    _lib.check(ctx.lib.bh_spline_prefilter(ctx.handle, ptr(t), code, *(int(n) for n in t.shape), ptr(coef)))
    return coef, spline_path(gpu)


def check_prefilter(what, coef, vol):
    Cf, A = R.spline_coef_f64(vol), R.spline_scale_f64(vol)
    worst = C.assert_close(coef.cpu(), Cf, A, C.sample_max(vol), C.K_PRE, what)
    print(f"F64 cubic prefilter {what}: {worst:.2f} u A (bound {C.K_PRE})")


@pytest.mark.parametrize("shape,dtypes", C.PREFILTER_SHAPES, ids=str)
def test_prefilter_vs_float64(gpu, shape, dtypes):
    """Every input type, the scalar staging form, axes shorter than the run-in and of length 1 (the convert kernel), interior blocks
    of both column passes, tpr 1 -> 2, rpw 2 -> 1 and a ragged last workgroup, one full chunk and a last chunk of 1 and of 4, and the
    65 535 fold of each column pass."""
    for dtype in dtypes:
        vol = C.volume(shape, dtype)
        plan = C.prefilter_plan(shape, dtype)
        coef, code = prefilter(gpu, torch.from_numpy(np.array(vol)).cuda())
        assert code == plan["code"], (shape, dtype, code, plan)
        check_prefilter(f"{dtype} {shape} {'VEC' if plan['vec'] else 'scalar' if not plan['convert'] else 'convert'}", coef, vol)


@pytest.mark.parametrize("dtype,elements", [("f32", 1), ("u16", 1), ("f32", 3), ("u8", 2)])
def test_prefilter_volume_off_the_grid(gpu, dtype, elements):
    """X % 4 == 0 but the first sample off the boundary of four samples (float32: 4 bytes past 16; uint16: 2 bytes past 8): the scalar
    staging form by the pointer test alone, bit-identical to the volume on the grid."""
    vol = np.array(C.volume(C.T200, dtype))
    on, code_on = prefilter(gpu, torch.from_numpy(vol).cuda())
    view = _offset_view(vol, elements)
    assert view.data_ptr() % (4 * vol.dtype.itemsize) == elements * vol.dtype.itemsize
    off, code_off = prefilter(gpu, view)
    assert code_on == C.SP_VEC and code_off == 0 == C.prefilter_plan(C.T200, dtype, aligned=False)["code"]
    check_prefilter(f"{dtype} {C.T200} {elements} samples off the grid", off, vol)
    assert torch.equal(on, off)


# ----------------------------------------------------------------------------- the warp
@functools.lru_cache(maxsize=4)
def _input(shape, dtype, nan=False):
    vol = np.array(C.nan_volume(shape) if nan else C.volume(shape, dtype))
    return torch.from_numpy(vol).cuda(), torch.from_numpy(vol.astype(np.float32)).cuda(), C.sample_max(vol)


def run(gpu, monkeypatch, vol, m, out, lo, **switches):
    """One cubic bh_affine under the given BH_SPLINE_* switches (all others unset); returns (result, bh_spline_path's code)."""
    from biahub_amd.register import affine_device, affine_path, spline_path

    for name in ENV:
        monkeypatch.delenv("BH_SPLINE_" + name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv("BH_SPLINE_" + name, str(value))
    full = tuple(a + n for a, n in zip(lo, out))
    got = affine_device(vol, m, full, "cubic", W.SCIPY, C.CVAL, lo, out)
    assert affine_path(gpu) == W.CUBIC
    code = spline_path(gpu)
    for name in switches:
        monkeypatch.delenv("BH_SPLINE_" + name)
    return got, code


def launches(gpu, monkeypatch, label, inp, m, shape, out, lo, dtype, switches=C.SWITCHES):
    """The launch the rule selects and every forced form, each against float64 with its code asserted; the runs that blend 64 taps
    per voxel (every launch that does not combine planes, the global one among them) bit-identical, and so the launches that combine
    planes among themselves.  Returns the rule's result."""
    vol, vol32, S = inp
    V, M, inside = R.cubic_warp_f64(vol32, m, out, lo, C.CVAL)
    first, anchor, zanchor = None, None, None
    for env in switches:
        plan = C.gather_plan(m, shape, out, dtype, True, **env)
        got, code = run(gpu, monkeypatch, vol, m, out, lo, **env)
        assert code == plan.code, (label, env, code, plan)
        worst = C.assert_close(got, V, M, S, C.K_CUBIC, f"{label} {env}", inside, C.CVAL)
        form = "global" if plan.launch == C.SP_GLOBAL else f"tiles of {plan.gtz}{' zuni' if plan.zuni else ''} nt {plan.nt} pad32 {int(plan.pad32)}"
        print(f"F64 cubic warp {form} | {dtype} [{label} {shape}{'' if tuple(lo) == (0, 0, 0) else ' crop'}] {env}: {worst:.2f} u M "
              f"(bound {C.K_CUBIC})")
        first = got if first is None else first
        if plan.launch == C.SP_GLOBAL or not plan.zuni:
            anchor = got if anchor is None else anchor
            assert torch.equal(got, anchor), (label, env)
        else:      # every voxel of a plane-combining launch blends z first, whatever the tiles, threads and pitch
            zanchor = got if zanchor is None else zanchor
            assert torch.equal(got, zanchor), (label, env)
    return first


@pytest.mark.parametrize("name,shape,dtype", C.warp_cases(), ids=str)
def test_cubic_warp_vs_float64(gpu, monkeypatch, name, shape, dtype):
    """The whole ragged output box (tiles wholly outside the source and tiles across every face) by the rule and under each of
    BH_SPLINE_ZUNI=0, _GATHER=global, _TZ=4, _NT=256 and _PITCH32=0, and a crop that starts mid-tile, which must equal that part of the
    whole bit for bit."""
    m, out = C.pull_matrix(name, shape), C.OUT[shape]
    inp = _input(shape, dtype)
    whole = launches(gpu, monkeypatch, name, inp, m, shape, out, (0, 0, 0), dtype)
    cs, lo = C.crop_shape(out), C.CROP_LO
    part, code = run(gpu, monkeypatch, inp[0], m, cs, lo)
    assert code == C.gather_plan(m, shape, cs, dtype).code
    assert torch.equal(part, whole[lo[0]: lo[0] + cs[0], lo[1]: lo[1] + cs[1], lo[2]: lo[2] + cs[2]]), name


@pytest.mark.parametrize("name", list(C.WARPS))
def test_cubic_warp_nan_taps_vs_float64(gpu, monkeypatch, name):
    """A NaN inside a tile and one on a tile seam read as 0 (``clean`` in the x pass): finite everywhere and under the bound."""
    for shape in (C.T200, C.T198):
        m, out = C.pull_matrix(name, shape), C.OUT[shape]
        got = launches(gpu, monkeypatch, name + ", NaN", _input(shape, "f32", True), m, shape, out, (0, 0, 0), "f32")
        assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("held", [True, False], ids=["held at 0", "a quarter off"])
@pytest.mark.parametrize("shape", W.DEGENERATE, ids=str)
def test_cubic_warp_degenerate_volumes_vs_float64(gpu, monkeypatch, shape, held):
    """Zi == 1, Yi == 1, Xi == 1 under SciPy's [0, n - 1] rule: a matrix row of zeros holds the thin axis at exactly 0 (all four taps
    of that axis are the one sample; Yi == 1 makes every box one row high: ``dy == 1``), any other leaves it and everything is cval."""
    out = W.DEGENERATE_OUT[shape]
    m = C.degenerate_matrix(shape, out, held)
    for dtype in ("f32", "u16"):
        got = launches(gpu, monkeypatch, f"degenerate, {'held' if held else 'off'}", _input(shape, dtype), m, shape, out, (0, 0, 0), dtype)
        inside = R.cubic_geometry_f64(shape, m, out, None, "cpu")[0]
        assert bool(inside.any()) == held
        if not held:
            assert bool((got == float(np.float32(C.CVAL))).all())


@pytest.mark.parametrize("shape", [C.LONG, C.LONG2], ids=str)
def test_cubic_warp_coordinates_near_2048_and_beyond(gpu, monkeypatch, shape):
    """Rows of 2200 and of 9000 shifted by 0.37 voxels in x: a float32 coordinate carries the fraction to 1.2e-4 at x = 2048 and to
    5e-4 beyond 4096.  On the row of 9000 that defect, planted in the restatement, costs 200 u M (tests/test_cubic_reference.py); on
    the row of 2200 it stays inside the bound."""
    m = C.long_matrix()
    launches(gpu, monkeypatch, "0.37 voxel x shift", _input(shape, "f32"), m, shape, shape, (0, 0, 0), "f32")


@pytest.mark.parametrize("kind", C.CAST_KINDS)
def test_transform_apply_order_3_integer_outputs(gpu, monkeypatch, kind):
    """``Transform.apply(order=3)`` on integer volumes: ``got == round_half_away(V)``, saturated, at every voxel whose V lies farther
    from a half-integer than the bound; at most 1 % of the voxels may be left out."""
    from biahub_amd.core.transform import Transform

    for name in ENV:
        monkeypatch.delenv("BH_SPLINE_" + name, raising=False)
    vol = np.array(C.cast_volume(kind))
    push = C.cast_push_matrix()
    got = Transform(push).apply(vol, order=3)
    assert got.dtype == vol.dtype and got.shape == vol.shape
    V, M, inside = R.cubic_warp_f64(torch.from_numpy(vol.astype(np.float32)).cuda(), np.linalg.inv(push), vol.shape, None, 0.0)
    ok = C.decidable(V, M, C.sample_max(vol))
    left_out = 1.0 - float(ok.double().mean())
    want = C.round_half_away(V, vol.dtype)
    g = torch.from_numpy(got.astype(np.int64)).cuda().double()
    wrong = int(((g != want) & ok).sum())
    print(f"F64 cubic cast {kind}: {left_out:.4%} of the voxels within the bound of a half-integer, {wrong} wrong among the others, "
          f"{int((g != want).sum())} in all")
    assert left_out <= 0.01 and wrong == 0


def test_spline_path_forgets_the_launch_after_a_refused_call_and_a_linear_warp(gpu, monkeypatch):
    from biahub_amd.register import affine_device, spline_path

    shape = C.T200
    vol = _input(shape, "f32")[0]
    m = C.pull_matrix("identity", shape)
    _, code = run(gpu, monkeypatch, vol, m, C.OUT[shape], (0, 0, 0))
    assert code == C.gather_plan(m, shape, C.OUT[shape]).code and code > 0
    bad = np.eye(4)
    bad[1, 2] = np.nan
    with pytest.raises((ValueError, RuntimeError), match="NaN"):
        affine_device(vol, bad, C.OUT[shape], "cubic", W.SCIPY)
    assert spline_path(gpu) == -1
    run(gpu, monkeypatch, vol, m, C.OUT[shape], (0, 0, 0))
    affine_device(vol, m, C.OUT[shape], "linear", W.ITK)
    assert spline_path(gpu) == -1
