"""CPU: the float64 reference of the cubic B-spline warp (oracle/reference_f64.py: spline_coef_f64, cubic_warp_f64), the bounds the GPU
kernels are held to in tests/test_gpu_cubic_f64.py (tests/cubic_cases.py derives them) and the claims of the case tables.

The reference is pinned to SciPy itself and to ``oracle_np``; the first-order error fields the constants K_PRE and K_CUBIC rest on are
evaluated on every GPU input; float32 restatements of filter_block, weights3, blend64 and blend16 are held to the bounds on the same
inputs; the restated launch rules are shown to reach every form the kernels choose per launch and per tile; and planted defects show
where the bound bites and ``rel_err <= 1e-5`` does not.

The warp restatements run on slabs of output rows (low face, middle, high face: a slab has every x and z of the box), so the numpy
code stays quick.  Every case prints ``F64 cubic ...`` lines (``-s`` shows them; DESIGN.md §3.3 keeps the figures).
"""

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import cubic_cases as C
import warp_cases as W
from oracle import oracle_np as O
from oracle import reference_f64 as R

EPS = 2.0 ** -53


# ----------------------------------------------------------------------------- the reference is SciPy's
PIN_SHAPES = [(5, 6, 7), (1, 4, 9), (2, 3, 5), (3, 1, 2), (5, 5, 1), (6, 7), (1, 37), (2, 12), (3, 3)]


@pytest.mark.parametrize("shape", PIN_SHAPES, ids=str)
def test_reference_is_scipy_to_float64_rounding(shape):
    """3-D volumes and 2-D images, axes of length 1, 2, 3 and 5, a crop: the coefficients against ``scipy.ndimage.spline_filter`` and
    ``oracle_np.spline_prefilter``, the warp against ``affine_transform(order=3, mode="constant", output=float64)`` and
    ``oracle_np.spline_affine_pull``, each within 256 x 2^-53 of the local scale; ``inside`` is SciPy's own decision."""
    rng = np.random.default_rng(sum(shape))
    nd = len(shape)
    v = rng.normal(100.0, 30.0, shape)
    v[tuple(0 for _ in shape)] = np.nan
    clean = np.nan_to_num(v, nan=0)
    coef, A = R.spline_coef_f64(v).numpy(), R.spline_scale_f64(v).numpy()
    assert (np.abs(coef) <= A * (1 + 1e-12)).all()
    for want in (ndi.spline_filter(clean, 3, output=np.float64, mode="mirror"), O.spline_prefilter(clean)):
        assert (np.abs(coef - want) <= 256 * EPS * A).all(), shape
    m = np.eye(nd + 1)
    m[:nd, :nd] += rng.normal(0, 0.1, (nd, nd))
    m[:nd, nd] = rng.normal(0, 0.5, nd)
    for a, n in enumerate(shape):
        if n == 1:
            m[a, :] = 0.0      # the only coordinate inside [0, 0]
    out = tuple(n + 3 for n in shape)
    V, M, inside = (t.numpy() for t in R.cubic_warp_f64(v, m, out, None, C.CVAL))
    cv = float(np.float32(C.CVAL))
    assert inside.any() and (~inside).any()
    for want in (ndi.affine_transform(clean, m, output_shape=out, order=3, mode="constant", cval=cv, output=np.float64),
                 O.spline_affine_pull(clean, m, out, cv, np.float64)):
        assert (np.abs(V - want) <= 256 * EPS * M).all(), shape
        assert np.array_equal(want == cv, ~inside | (V == cv))
    assert (np.abs(V[inside]) <= M[inside] * (1 + 1e-12)).all() and (M[~inside] == abs(cv)).all()
    lo = tuple(1 for _ in shape)
    sub = tuple(n - 2 for n in out)
    part = R.cubic_warp_f64(v, m, sub, lo, C.CVAL)
    sl = tuple(slice(1, 1 + n) for n in sub)
    assert all(np.array_equal(p.numpy(), w[sl]) for p, w in zip(part, (V, M, inside)))


def test_scale_is_the_absolute_impulse_response():
    """A's kernel: sqrt(3) |z|^|k| is the absolute value of the prefilter's impulse response, its row sum is 3 per axis, and an axis of
    length 1 is left alone."""
    imp = np.zeros(41)
    imp[20] = 1.0
    h = R.spline_coef_f64(imp).numpy()
    A = R.spline_scale_f64(imp).numpy()
    assert np.abs(np.abs(h) - A).max() <= 1e-12 and abs(A.sum() - 3.0) <= 1e-9
    assert abs(float(R.spline_scale_f64(np.ones((1, 7, 9))).max()) - 9.0) <= 1e-9


# ----------------------------------------------------------------------------- the cases of the GPU tests
def _slabs(out, lo, rows=2):
    Yo = out[1]
    return [((lo[0], lo[1] + y0, lo[2]), (out[0], min(rows, Yo - y0), out[2])) for y0 in sorted({0, max(0, Yo // 2 - 1), max(0, Yo - rows)})]


def _warp_inputs():
    """(label, volume, matrix, in shape, out shape, dtype) of every warp the GPU tests run (the crops compute part of the same grid)."""
    for name, shape, dtype in C.warp_cases():
        yield name, C.volume(shape, dtype), C.pull_matrix(name, shape), shape, C.OUT[shape], dtype
    for name in C.WARPS:
        for shape in (C.T200, C.T198):
            yield name + ", NaN", C.nan_volume(shape), C.pull_matrix(name, shape), shape, C.OUT[shape], "f32"
    for shape in W.DEGENERATE:
        for held in (True, False):
            for dtype in ("f32", "u16"):
                out = W.DEGENERATE_OUT[shape]
                yield f"degenerate {held}", C.volume(shape, dtype), C.degenerate_matrix(shape, out, held), shape, out, dtype
    for shape in (C.LONG, C.LONG2):
        yield "0.37 voxel x shift", C.volume(shape, "f32"), C.long_matrix(), shape, shape, "f32"


def test_error_fields_and_restatements_at_every_prefilter_input():
    """On every volume the GPU test hands to bh_spline_prefilter: the first-order rounding field E stays under K_PRE u A (what K_PRE
    rests on), and the float32 restatement of the three passes, in the kernels' blocks, stays under the bound with room to spare."""
    field, restated = {}, {}
    for shape, dtypes in C.PREFILTER_SHAPES:
        for dtype in dtypes:
            vol = C.volume(shape, dtype)
            A, Cf = R.spline_scale_f64(vol), R.spline_coef_f64(vol)
            ratio = float((C.rounding_field(vol) / A.clamp_min(1e-300)).max())
            assert ratio <= C.K_PRE, (shape, dtype, ratio)
            u = C.assert_close(C.prefilter_f32(vol), Cf, A, C.sample_max(vol), C.K_PRE, f"restated prefilter {shape} {dtype}")
            field[dtype], restated[dtype] = max(field.get(dtype, 0.0), ratio), max(restated.get(dtype, 0.0), u)
    print("F64 cubic prefilter, first-order field E / (u A) by input type:", {k: round(v, 2) for k, v in field.items()}, "K_PRE", C.K_PRE)
    print("F64 cubic prefilter restated, worst u A by input type:", {k: round(v, 2) for k, v in restated.items()}, "bound", C.K_PRE)
    assert max(restated.values()) <= C.K_PRE / 8


def test_error_fields_and_restatements_at_every_warp_input():
    """On slabs of every warp of the GPU tests: the first-order field (coefficients' error, weights' error, twelve roundings of the
    blend) stays under K_CUBIC u M, and the restated weights3 / blend64 / blend64_zfirst / blend16-on-combined-planes under the bound."""
    field, restated, shared = {}, {}, {}
    cv = float(np.float32(C.CVAL))
    for label, vol, m, shape, out, dtype in _warp_inputs():
        plan = C.gather_plan(m, shape, out, dtype)
        S = C.sample_max(vol)
        if id(vol) not in shared:      # the volumes are cached, read-only arrays: one set of fields and coefficients each
            shared[id(vol)] = (vol, C.error_fields(vol), C.prefilter_f32(vol))
        _, fields, coef32 = shared[id(vol)]
        for lo, sub in _slabs(out, (0, 0, 0)):
            F, M, V = C.cubic_error_field(vol, m, sub, lo, fields=fields)
            inside = R.cubic_geometry_f64(shape, m, sub, lo)[0]
            V, M = torch.where(inside, V, torch.tensor(cv, dtype=torch.float64)), torch.where(inside, M, torch.tensor(abs(cv), dtype=torch.float64))
            pos = inside & (M > 0)
            ratio = float((F[pos] / M[pos]).max()) if bool(pos.any()) else 0.0
            assert ratio <= C.K_CUBIC, (label, shape, dtype, ratio)
            key = "NaN" if "NaN" in label else dtype
            field[key] = max(field.get(key, 0.0), ratio)
            for zuni in {False, bool(plan.zuni)}:
                got = C.cubic_f32(vol, m, sub, lo, zuni=zuni, gtz=plan.gtz, coef=coef32)
                u = C.assert_close(got, V, M, S, C.K_CUBIC, f"restated {label} {shape} {dtype} zuni {zuni}", inside, C.CVAL)
                k2 = (key, "z first" if zuni else "64 taps")
                restated[k2] = max(restated.get(k2, 0.0), u)
    print("F64 cubic warp, first-order field F / (u M) by input:", {k: round(v, 2) for k, v in field.items()}, "K_CUBIC", C.K_CUBIC)
    print("F64 cubic warp restated, worst u M:", {f"{a} {b}": round(v, 2) for (a, b), v in restated.items()}, "bound", C.K_CUBIC)
    assert max(restated.values()) <= C.K_CUBIC / 8


# ----------------------------------------------------------------------------- the case tables keep their promises
def test_prefilter_plans_reach_every_form():
    """No row length needs more than 64 KiB of LDS (so the branch that raises the limit cannot be taken), and the shapes of the GPU
    test reach what they name."""
    for X in list(range(2, 4200)) + [2 ** 20 + 3, 2 ** 30 - 1]:
        p = C.x_pass_plan(X)
        assert p["lds"] <= 64 * 1024 and (p["rpw"] - 1) * p["tpr"] < 256 and p["tpr"] * C.BX >= p["clen"], X
    P = C.prefilter_plan
    assert P((24, 40, 200))["vec"] and not P((24, 40, 198))["vec"] and not P((24, 40, 200), aligned=False)["vec"]
    assert P((24, 40, 1))["convert"] and not P((1, 1, 37))["convert"]
    assert P((1, 40, 200))["z"]["launches"] == 0 and P((24, 1, 200))["y"]["launches"] == 0
    assert P((150, 150, 8))["y"]["interior"] == 1 == P((150, 150, 8))["z"]["interior"] and P((24, 40, 200))["y"]["interior"] == 0
    assert (P((2, 3, 16))["tpr"], P((2, 3, 17))["tpr"]) == (1, 2)
    assert (P((1, 5, 2048))["rpw"], P((1, 5, 2052))["rpw"]) == (2, 1) and 5 % P((1, 5, 2048))["rpw"] == 1      # a ragged last workgroup
    assert [P((2, 3, X))["nchunk"] for X in (4096, 4097, 4100)] == [1, 2, 2] and P((2, 3, 4100))["vec"] and not P((2, 3, 4097))["vec"]
    assert (P((70000, 2, 2))["y"]["launches"], P((70000, 2, 2))["z"]["launches"]) == (2, 1)
    assert (P((2, 70000, 2))["y"]["launches"], P((2, 70000, 2))["z"]["launches"]) == (1, 2)
    assert P((70000, 2, 2))["z"]["interior"] > 0 and P((2, 70000, 2))["y"]["interior"] > 0


def test_every_warp_reaches_the_launch_it_names_and_every_tile_form_is_reached():
    """The restated dispatch sends every warp to the launch its table entry names, the table holds an 8-plane, a 4-plane and a global
    launch, and over the runs of the GPU test (switches included) every per-tile form is reached in both staging forms."""
    seen = {}
    launches = set()
    for name, w in C.WARPS.items():
        m = C.pull_matrix(name, C.T200)
        plan = C.gather_plan(m, C.T200, C.OUT[C.T200])
        assert (plan.launch, bool(plan.zuni)) == w.launch, (name, plan)
        launches.add(plan.launch)
    assert launches == {C.SP_GLOBAL, C.SP_TILE8, C.SP_TILE4}
    runs = [(name, C.pull_matrix(name, shape), shape, C.OUT[shape], lo, sub) for name in C.WARPS for shape in (C.T200, C.T198)
            for lo, sub in (((0, 0, 0), C.OUT[shape]), (C.CROP_LO, C.crop_shape(C.OUT[shape])))]
    runs += [(f"degenerate {held}", C.degenerate_matrix(s, W.DEGENERATE_OUT[s], held), s, W.DEGENERATE_OUT[s], (0, 0, 0), W.DEGENERATE_OUT[s])
             for s in W.DEGENERATE for held in (True, False)]
    for name, m, shape, out, lo, sub in runs:
        for env in C.SWITCHES if lo == (0, 0, 0) else ({},):
            plan = C.gather_plan(m, shape, sub, **env)
            staging = "global" if plan.launch == C.SP_GLOBAL else ("quads" if plan.x4 else "dwords")
            for k, n in C.tile_forms(m, shape, sub, lo, plan).items():
                seen[(staging, k)] = seen.get((staging, k), 0) + n
            seen[(staging, "launches")] = seen.get((staging, "launches"), 0) + 1
            seen[("gtz", plan.gtz if plan.launch != C.SP_GLOBAL else 0)] = 1
    print("F64 cubic forms:", seen)
    for staging in ("quads", "dwords"):
        for k in ("empty", "interior", "boundary in box", "zuni combined", "zuni z edge"):
            assert seen[(staging, k)] > 0, (staging, k)
        # By the box arithmetic no case can reach these: the launch asks for the LDS of the largest box its matrix can need, so every
        # tile with a source voxel is staged; and a box clipped to the volume holds the mirror image of every tap that left it (the
        # image of tap -1 is 1 <= floor(hi) + 2, that of tap n is n - 2 >= floor(lo) - 1).  The per-voxel fallback to global memory is
        # a guard; the global launch runs the same function on every voxel.
        assert seen[(staging, "not staged")] == 0 and seen[(staging, "boundary with fallback")] == 0
    assert seen[("quads", "LP == 1")] > 0 and seen[("quads", "dy == 1")] > 0 and seen[("global", "launches")] > 0
    assert seen[("gtz", 8)] and seen[("gtz", 4)]
    # the named special cases: dx <= 4 under the natural pitch, dy == 1 on the volume one row high
    m = C.pull_matrix("x row near zero", C.T200)
    assert C.tile_forms(m, C.T200, C.OUT[C.T200], (0, 0, 0), C.gather_plan(m, C.T200, C.OUT[C.T200], PITCH32="0"))["LP == 1"] > 0
    s = (24, 1, 200)
    m = C.degenerate_matrix(s, W.DEGENERATE_OUT[s], True)
    assert C.tile_forms(m, s, W.DEGENERATE_OUT[s], (0, 0, 0), C.gather_plan(m, s, W.DEGENERATE_OUT[s]))["dy == 1"] > 0


# ----------------------------------------------------------------------------- the bound bites where rel_err does not
# defect: (warp, volume, passes ``rel_err <= 1e-5``, passes the per-voxel bound) as observed
DEFECTS = {
    "R8": ("similarity 2 deg 1.02", "bead", True, False), "half": ("similarity 2 deg 1.02", "bead", False, False),
    "init": ("similarity 2 deg 1.02", "bead", True, True), "w12": ("similarity 2 deg 1.02", "bead", False, False),
    "coord32": (None, "long", False, False), "origin": ("similarity 2 deg 1.02", "bead", False, False),
    "nan": ("similarity 2 deg 1.02", "nan", False, False), "zuni97": ("about z, m00 0.97", "bead", False, False),
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects(defect):
    """Each defect planted in the restatement (cubic_cases.cubic_f32 names them), against the per-voxel bound and against the old
    assertion, ``rel_err <= 1e-5`` of the volume's maximum.  Observed: a run-in of 8 passes the old assertion (5.7e-7) and fails the
    bound (192 u M at a background voxel beside a bead); half-sample mirroring (2.5e-3), w[1] and w[2] exchanged below 200 counts
    (4.7e-3: camera noise between neighbours moves a background voxel by counts, as with the linear warp's wrong y tap), a box origin
    off by one (1.7e-4), an uncleaned NaN and the plane combination on m00 = 0.97 (3.6e-2: output planes 12 and 13 share their source
    planes and the second reads the first's result) fail both.
    Float32 coordinates fail both on the row of 9000 (8.8e-5; 200 u M at x = 3221, the flank of a bead; the clean restatement stays at
    0.36 there); on (9, 9, 2200) they cost 14.7 u M at x = 2169 — inside K_CUBIC = 48, three quarters of which is the prefilter's
    worst-case share — which is why the GPU test runs both rows.  One defect does NOT fail the bound and cannot: INIT_C and INIT_A
    exchanged change a result by |z|^20 = 3.6e-12 of a sample — the run-in exists so that the start value does not matter, it is
    below float32 resolution by construction, and T accounts for exactly that."""
    name, which, _, _ = DEFECTS[defect]
    if which.startswith("long"):
        out = C.LONG if which == "long2200" else C.LONG2
        vol, m = C.volume(out, "f32"), C.long_matrix()
        slabs = [((0, 0, 0), out)]
    else:
        vol = C.nan_volume(C.T200) if which == "nan" else C.volume(C.T200, "f32")
        m, out = C.pull_matrix(name, C.T200), C.OUT[C.T200]
        slabs = [((0, 10, 0), (36, 3, 330)), ((0, 28, 0), (36, 3, 330)), ((0, 44, 0), (36, 3, 330))]      # the NaNs map to y = 29 and 25
    S = C.sample_max(vol)
    old, passes_new, what = 0.0, True, ""
    for lo, sub in slabs:
        V, M, inside = R.cubic_warp_f64(vol, m, sub, lo, C.CVAL)
        C.assert_close(C.cubic_f32(vol, m, sub, lo), V, M, S, C.K_CUBIC, "no defect", inside, C.CVAL)
        got = C.cubic_f32(vol, m, sub, lo, defect=defect.split()[0])
        with np.errstate(invalid="ignore"):
            e = np.abs(got.astype(np.float64) - V.numpy()).max() / S
        old = max(old, e) if e == e else float("inf")
        try:
            C.assert_close(got, V, M, S, C.K_CUBIC, defect, inside, C.CVAL)
        except AssertionError as err:
            passes_new, what = False, str(err)[:160]
    passes_old = bool(old <= 1e-5)
    print(f"F64 cubic defect {defect}: rel_err {old:.3g} ({'passes' if passes_old else 'fails'} the old assertion), bound "
          f"{'passes' if passes_new else 'fails'} {what}")
    assert (passes_old, passes_new) == DEFECTS[defect][2:], (defect, old, what)


# ----------------------------------------------------------------------------- integer outputs
@pytest.mark.parametrize("kind", C.CAST_KINDS)
def test_integer_cast_inputs_leave_the_rounding_decidable(kind):
    """The reference alone: on the inputs of the GPU's integer test at most 1 % of the voxels lie within the bound of a half-integer,
    the restatement rounds to the reference's integer at every other voxel, and both signs / the saturation are present."""
    vol = np.array(C.cast_volume(kind))
    pull = np.linalg.inv(C.cast_push_matrix())
    left, total, neg, sat = 0, 0, False, False
    info = np.iinfo(vol.dtype)
    for lo, sub in _slabs(vol.shape, (0, 0, 0), rows=3) + [((0, 20, 0), (24, 6, 200))]:
        V, M, inside = R.cubic_warp_f64(vol, pull, sub, lo, 0.0)
        ok = C.decidable(V, M, C.sample_max(vol))
        left, total = left + int((~ok).sum()), total + ok.numel()
        got = torch.from_numpy(C.cubic_f32(vol, pull, sub, lo, cval=0.0, zuni=True)).double()
        r = torch.where(got > 0, torch.floor(got + 0.5), torch.ceil(got - 0.5)).clamp(float(info.min), float(info.max))
        assert bool((r == C.round_half_away(V, vol.dtype))[ok].all()), kind
        neg, sat = neg or bool((V < 0).any()), sat or bool((V > info.max).any())
    print(f"F64 cubic cast {kind}: {left / total:.4%} of the reference's voxels within the bound of a half-integer")
    assert left / total <= 0.01
    if kind == "i16":
        assert neg
    if kind == "u8":
        assert sat
