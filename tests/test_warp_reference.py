"""CPU: the float64 reference of the affine warp (oracle/reference_f64.py: warp_f64), the bounds the GPU kernels are held to in
tests/test_gpu_warp_f64.py (tests/warp_cases.py derives them), and the claims of the case tables.

The reference is held to a triple loop and, through the distance of its Q32.32 position grid from the float64 coordinate, to
``oracle_np.affine_pull`` evaluated in float64; float32 restatements of lerp8 and of the generic accumulation are held to the bounds
at every input of the GPU tests; the restated launch rules are shown to send every warp to the kernel its name promises and to reach
every per-wave and per-tile form the kernels decide for themselves; and planted defects show where the bound bites and
``rel_err <= 1e-5`` does not.

The restatements run on three slabs of three output rows of each output box (low face, middle, high face: positions are per voxel, a
slab has every x and z of the box), so the numpy code stays quick.  Every case prints one ``F64 warp ...`` line (``-s`` shows them;
DESIGN.md §3.3 keeps the range).
"""

from fractions import Fraction

import numpy as np
import pytest
import torch

import warp_cases as W
from conftest import rel_err
from oracle import oracle_np as O
from oracle import reference_f64 as R

ALL_MATRICES = [(name, shape) for name, w in W.WARPS.items() for shape in w.shapes]


# ----------------------------------------------------------------------------- the reference is the definition
def test_llround_rounds_half_away_from_zero():
    h = 2.0 ** -33
    m = np.array([[h, -h, 3 * h, -3 * h], [5 * h, 2.0 ** -32, -1.25, 0.0], [1.0, 0.7, -0.7, 1e-12]])
    want = [[1, -1, 2, -2], [3, 1, -5368709120, 0], [1 << 32, round(Fraction(0.7) * 2 ** 32), -round(Fraction(0.7) * 2 ** 32), 0]]
    assert R.llround_q32(m).tolist() == want
    assert np.rint(np.array([5 * h]) * 2.0 ** 32)[0] == 2.0        # numpy's rule differs exactly there


def _corners(out_shape, lo):
    return [(lo[0] + (out_shape[0] - 1) * a, lo[1] + (out_shape[1] - 1) * b, lo[2] + (out_shape[2] - 1) * c)
            for a in (0, 1) for b in (0, 1) for c in (0, 1)]


@pytest.mark.parametrize("name,shape", ALL_MATRICES, ids=str)
def test_q32_grid_is_the_operator_to_a_third_of_a_nanovoxel(name, shape):
    """|cq / 2^32 - c| <= 2^-33 (|z| + |y| + |x| + 1) against the exact rational coordinate, at every corner of the output box and
    of its crop (the coordinate is affine: its error is extreme at corners), and the float64 coordinate lies within its rounding
    of the same value.  No entry of a case matrix sits on a half in Q32.32, where llround and rint would part."""
    m = W.pull_matrix(name, shape)
    mq = R.llround_q32(m[:3])
    assert (np.abs(m[:3] * 2.0 ** 32 - np.floor(m[:3] * 2.0 ** 32) - 0.5) > 0).all()
    out = W.OUT[shape]
    for z, y, x in _corners(out, (0, 0, 0)) + _corners(W.crop_shape(out), W.CROP_LO):
        for a in range(3):
            exact = Fraction(m[a, 0]) * z + Fraction(m[a, 1]) * y + Fraction(m[a, 2]) * x + Fraction(m[a, 3])
            cq = int(mq[a, 0]) * z + int(mq[a, 1]) * y + int(mq[a, 2]) * x + int(mq[a, 3])
            assert abs(Fraction(cq, 1 << 32) - exact) <= Fraction(abs(z) + abs(y) + abs(x) + 1, 1 << 33)
            c = ((m[a, 0] * z + m[a, 1] * y) + m[a, 2] * x) + m[a, 3]
            mag = abs(m[a, 0] * z) + abs(m[a, 1] * y) + abs(m[a, 2] * x) + abs(m[a, 3])
            assert abs(Fraction(c) - exact) <= Fraction(4 * mag) * Fraction(1, 1 << 52)


def _neighbourhood_range(vol, c):
    """max - min of the cleaned volume over the 3 x 3 x 3 neighbourhood of rint(c), clamped: it holds every tap of two evaluations
    whose positions differ by far less than a voxel, also when a floor flips at an integer coordinate."""
    from scipy.ndimage import maximum_filter, minimum_filter

    v = np.nan_to_num(np.asarray(vol, np.float32), nan=0).astype(np.float64)
    rng = maximum_filter(v, 3, mode="nearest") - minimum_filter(v, 3, mode="nearest")
    idx = [np.clip(np.rint(ca).astype(np.int64), 0, n - 1) for ca, n in zip(c, v.shape)]
    return rng[idx[0], idx[1], idx[2]]


@pytest.mark.parametrize("name,shape", [(n, w.shapes[0]) for n, w in W.WARPS.items()], ids=str)
def test_reference_against_affine_pull_in_float64(name, shape):
    """warp_f64 against ``oracle_np.affine_pull(dtype=float64)``: linear with an edge clamp within 3 delta (max - min over the
    neighbourhood), delta the distance of the Q32.32 grid from the float64 coordinate at the box's far corner — a floor that flips
    at an integer coordinate moves the value by no more —; ZEROS to float64 rounding; nearest and ``inside`` bit for bit."""
    m = W.pull_matrix(name, shape)
    out = W.OUT[shape]
    vol = W.volume(shape, "f32")
    delta = 2.0 ** -33 * (sum(out) + 1) + 2.0 ** -50 * float(np.abs(m[:3]).sum(axis=1).max() * max(out))
    c, _ = W._coords(m[:3], out, (0, 0, 0))
    c = [np.broadcast_to(ca, out) for ca in c]
    rng = _neighbourhood_range(vol, c)
    for boundary in (W.ITK, W.SCIPY, W.ZEROS):
        V, M, inside = (t.numpy() for t in R.warp_f64(vol, m, out, (0, 0, 0), "linear", boundary, W.CVAL))
        want = O.affine_pull(vol, m, out, 1, boundary, W.CVAL, dtype=np.float64)
        tol = 64 * 2.0 ** -53 * M + (0 if boundary == W.ZEROS else 3 * delta * rng)
        worst = np.abs(V - want) - tol
        assert (worst <= 0).all(), (name, boundary, np.unravel_index(worst.argmax(), out), float(worst.max()))
        assert np.array_equal(V[~inside], np.full(int((~inside).sum()), float(np.float32(W.CVAL))))
        Vn, Mn, inside_n = (t.numpy() for t in R.warp_f64(vol, m, out, (0, 0, 0), "nearestneighbor", boundary, W.CVAL))
        assert np.array_equal(Vn, O.affine_pull(vol, m, out, 0, boundary, W.CVAL).astype(np.float64))
        assert np.array_equal(inside_n, inside)


def _triple_loop(vol, m, out_shape, lo, interp, boundary, cval):
    v = np.nan_to_num(np.asarray(vol, np.float32), nan=0).astype(np.float64)
    dims = v.shape
    mq = R.llround_q32(m[:3]).tolist()
    cv = float(np.float32(cval))
    V, M = np.zeros(out_shape), np.zeros(out_shape)
    for oz in range(out_shape[0]):
        for oy in range(out_shape[1]):
            for ox in range(out_shape[2]):
                p = (oz + lo[0], oy + lo[1], ox + lo[2])
                c = [((m[a, 0] * p[0] + m[a, 1] * p[1]) + m[a, 2] * p[2]) + m[a, 3] for a in range(3)]
                if boundary == W.ITK:
                    inside = all(-0.5 <= ca < n - 0.5 for ca, n in zip(c, dims))
                elif boundary == W.SCIPY:
                    inside = all(0 <= ca <= n - 1 for ca, n in zip(c, dims))
                else:
                    inside = True
                if not inside:
                    V[oz, oy, ox], M[oz, oy, ox] = cv, abs(cv)
                    continue
                if interp != "linear":
                    i = [int(np.floor(ca + 0.5)) for ca in c]
                    ok = all(0 <= ia < n for ia, n in zip(i, dims))
                    val = v[tuple(min(max(ia, 0), n - 1) for ia, n in zip(i, dims))] if (ok or boundary == W.ITK) else cv
                    V[oz, oy, ox], M[oz, oy, ox] = val, abs(val)
                    continue
                if boundary == W.ZEROS:
                    base = [int(np.floor(ca)) for ca in c]
                    frac = [ca - b for ca, b in zip(c, base)]
                else:
                    cq = [mq[a][0] * p[0] + mq[a][1] * p[1] + mq[a][2] * p[2] + mq[a][3] for a in range(3)]
                    base = [q >> 32 for q in cq]
                    frac = [(q & 0xFFFFFFFF) / 2.0 ** 32 for q in cq]
                acc, big = 0.0, abs(cv) if boundary == W.ZEROS else 0.0
                for d in np.ndindex(2, 2, 2):
                    i = [b + k for b, k in zip(base, d)]
                    w = np.prod([f if k else 1 - f for f, k in zip(frac, d)])
                    ok = all(0 <= ia < n for ia, n in zip(i, dims))
                    t = cv if (boundary == W.ZEROS and not ok) else v[tuple(min(max(ia, 0), n - 1) for ia, n in zip(i, dims))]
                    acc += w * t
                    big = max(big, abs(t))
                V[oz, oy, ox], M[oz, oy, ox] = acc, big
    return V, M


@pytest.mark.parametrize("boundary", [W.ITK, W.SCIPY, W.ZEROS])
def test_reference_equals_the_triple_loop(boundary):
    rng = np.random.default_rng(5 + boundary)
    vol = (rng.random((5, 6, 7)) * 200 - 100).astype(np.float32)
    vol[2, 3, 3], vol[1, 1, 5], vol[3, 4, 1] = np.nan, np.inf, -np.inf
    m = np.eye(4)
    m[:3, :3] = 0.9 * W.rotation((1.0, 0.3, -0.2), 12.0)
    m[:3, 3] = (-1.5, 0.25, -0.5)
    out, lo = (6, 7, 9), (1, 0, 2)
    for interp in ("linear", "nearestneighbor"):
        V, M, inside = R.warp_f64(vol, m, out, lo, interp, boundary, W.CVAL)
        wantV, wantM = _triple_loop(vol, m, out, lo, interp, boundary, W.CVAL)
        assert V.dtype == torch.float64 and tuple(V.shape) == out
        assert np.abs(V.numpy() - wantV).max() <= 1e-13 * np.abs(wantV).max()
        assert np.array_equal(M.numpy(), wantM)


# ----------------------------------------------------------------------------- the case table keeps its promises
@pytest.mark.parametrize("name", list(W.WARPS))
def test_every_warp_reaches_the_launch_it_names(name):
    w = W.WARPS[name]
    shape = w.shapes[0]
    m = W.pull_matrix(name, shape)
    assert W.host_plan(m, shape, W.OUT[shape]).path == w.path, name
    assert W.host_plan(m, shape, W.OUT[shape], nozwalk=True).path == W.TILE


def _linear_runs():
    """(name, shape, dtype, aligned, matrix, out, crop_lo) of every default-launch linear run of the GPU tests, crops included."""
    for name, shape, dtype, aligned in W.linear_cases():
        m = W.pull_matrix(name, shape)
        yield name, shape, dtype, aligned, m, W.OUT[shape], (0, 0, 0)
        yield name, shape, dtype, aligned, m, W.crop_shape(W.OUT[shape]), W.CROP_LO


def test_every_per_tile_and_per_wave_form_is_reached():
    """What the kernels decide for themselves and cannot report, from the restated box arithmetic over the runs of the GPU tests:
    every tile form in every staging form, the flat-list divisions' special cases, both walks' forms, 1 .. 4 DMA instructions per
    plane in both LDS rings, and the compact blocks staged and not staged in each geometry."""
    tiles, walk, obl, blocks = {}, {"x edge": 0, "register ring": 0, "lds ring": {}}, {"slow waves": 0, "slow planes": 0, "ring planes": {}}, {}
    for name, shape, dtype, aligned, m, out, lo in _linear_runs():
        for boundary in (W.ITK,):
            plan = W.host_plan(m, shape, out, dtype, "linear", boundary, aligned)
            if plan.path == W.ZWALK:
                got = W.zwalk_forms(m, shape, out, lo, plan, dtype)
                for k in ("x edge", "register ring"):
                    walk[k] += got[k]
                for nq, n in got["lds ring"].items():
                    walk["lds ring"][nq] = walk["lds ring"].get(nq, 0) + n
            elif plan.path == W.OBLIQUE:
                got = W.oblique_forms(m, shape, out, lo, plan, dtype)
                for k in ("slow waves", "slow planes"):
                    obl[k] += got[k]
                for nq, n in got["ring planes"].items():
                    obl["ring planes"][nq] = obl["ring planes"].get(nq, 0) + n
            elif plan.path == W.BLOCKS:
                for G in W.GEO:
                    got = W.block_forms(m, shape, out, lo, G)
                    for k, n in got.items():
                        blocks[(G, k)] = blocks.get((G, k), 0) + n
            # the staged-tile kernel runs every case: by its own rule, or under BH_AFFINE_NOZWALK=1
            tplan = W.host_plan(m, shape, out, dtype, "linear", boundary, aligned, nozwalk=True)
            form = W.staging_form(tplan, dtype)
            for k, n in W.tile_forms(m, shape, out, lo, tplan).items():
                tiles[(form, k)] = tiles.get((form, k), 0) + n
    print("F64 warp forms: tiles", tiles, "z walk", walk, "oblique walk", obl, "blocks", blocks)
    for form in ("f32 quads", "f32 dwords", "16-bit groups of 8", "per sample"):
        for k in ("empty", "fallback", "interior", "boundary"):
            assert tiles[(form, k)] > 0, (form, k)
    for form in ("f32 quads", "16-bit groups of 8"):
        assert tiles[(form, "L == 1")] > 0 and tiles[(form, "dy == 1")] > 0, form
    assert walk["x edge"] > 0 and walk["register ring"] > 0 and sorted(walk["lds ring"]) == [1, 2, 3, 4], walk
    assert obl["slow waves"] > 0 and obl["slow planes"] > 0 and sorted(obl["ring planes"]) == [1, 2, 3, 4], obl
    for G in W.GEO:
        assert blocks[(G, "staged")] > 0 and blocks[(G, "not staged")] > 0 and blocks[(G, "empty")] > 0, (G, blocks)
    # the tile kernel by its own rule, in each staging form, and Yi == 1 (dy == 1 by the volume itself)
    own = {W.staging_form(p, d) for n, s, d, al, m, out, lo in _linear_runs()
           for p in [W.host_plan(m, s, out, d, "linear", W.ITK, al)] if p.path == W.TILE}
    assert own == {"f32 quads", "f32 dwords", "16-bit groups of 8", "per sample"}, own


# ----------------------------------------------------------------------------- the restatements sit under the bounds
def _slabs(out, lo):
    Yo = out[1]
    return [((lo[0], lo[1] + y0, lo[2]), (out[0], min(3, Yo - y0), out[2])) for y0 in sorted({0, max(0, Yo // 2 - 1), max(0, Yo - 3)})]


def _restatement_units(vol, m, out, lo, interp, boundary, name, slabs=None):
    worst = 0.0
    for slo, sshape in (_slabs(out, lo) if slabs is None else slabs):
        ref = R.warp_f64(vol, m, sshape, slo, interp, boundary, W.CVAL)
        got = W.warp_f32(vol, m, sshape, slo, interp, boundary, W.CVAL)
        worst = max(worst, W.assert_warp_close(got, ref, W.bound(interp, boundary), name, cval=None if boundary == W.ZEROS else W.CVAL))
    return worst


def _planted_slabs(m, out):
    """Boxes of 7 x 7 x 7 output voxels around every planted non-finite value (every voxel whose taps reach it, under the warps
    that run on that volume; none of them minifies by more than 3)."""
    sites = [p for w in W.NONFINITE.values() for p in (w["nan"], w["pinf"], w["ninf"]) + w["pair"]] + list(W.NONFINITE_BIG)
    boxes = []
    for p in sites:
        o = np.rint(np.linalg.solve(m, np.array(p + (1,), np.float64))[:3]).astype(int)
        lo = tuple(int(min(max(v - 3, 0), n - 1)) for v, n in zip(o, out))
        hi = tuple(int(min(max(v + 4, 1), n)) for v, n in zip(o, out))
        if all(h > a for h, a in zip(hi, lo)):
            boxes.append((lo, tuple(h - a for h, a in zip(hi, lo))))
    assert boxes
    return boxes


def test_restated_lerp8_is_under_the_bound_at_every_gpu_input():
    worst = {}
    for name, shape, dtype, aligned, m, out, lo in _linear_runs():
        if lo != (0, 0, 0):
            continue        # a cropped launch computes a sub-box of the same position grid: nothing new for the arithmetic
        for boundary in (W.ITK, W.SCIPY):
            u = _restatement_units(W.volume(shape, dtype), m, out, lo, "linear", boundary, f"{name} {shape} {dtype}")
            worst[dtype] = max(worst.get(dtype, 0.0), u)
    for name in W.NONFINITE_WARPS:
        for shape in W.WARPS[name].shapes:
            m, out = W.pull_matrix(name, shape), W.OUT[shape]
            for boundary in (W.ITK, W.SCIPY):
                u = _restatement_units(W.volume(shape, "f32", True), m, out, (0, 0, 0), "linear", boundary, f"{name} {shape} non-finite",
                                       _slabs(out, (0, 0, 0)) + _planted_slabs(m, out))
                worst["non-finite"] = max(worst.get("non-finite", 0.0), u)
    print("F64 warp restated lerp8, worst u M by input type:", {k: round(v, 2) for k, v in worst.items()}, "bound", W.K_LERP)
    assert max(worst.values()) <= W.K_LERP


def test_restated_generic_path_is_under_the_bound_at_every_gpu_input():
    worst = {}
    for name in W.ZEROS_WARPS:
        for k, shape in enumerate(W.WARPS[name].shapes):
            for dtype in W.DTYPES:
                u = _restatement_units(W.volume(shape, dtype), W.pull_matrix(name, shape), W.OUT[shape], (0, 0, 0), "linear", W.ZEROS,
                                       f"{name} {shape} {dtype} zeros")
                worst[dtype] = max(worst.get(dtype, 0.0), u)
                for boundary in (W.ITK, W.SCIPY, W.ZEROS):
                    assert _restatement_units(W.volume(shape, dtype), W.pull_matrix(name, shape), W.OUT[shape], (0, 0, 0),
                                              "nearestneighbor", boundary, name) == 0.0
    for name in W.NONFINITE_WARPS:      # the GPU test runs linear ZEROS and nearest ITK on the non-finite volume too
        for shape in W.WARPS[name].shapes:
            m, out = W.pull_matrix(name, shape), W.OUT[shape]
            slabs = _slabs(out, (0, 0, 0)) + _planted_slabs(m, out)
            vol = W.volume(shape, "f32", True)
            u = _restatement_units(vol, m, out, (0, 0, 0), "linear", W.ZEROS, f"{name} {shape} non-finite zeros", slabs)
            worst["non-finite"] = max(worst.get("non-finite", 0.0), u)
            assert _restatement_units(vol, m, out, (0, 0, 0), "nearestneighbor", W.ITK, name, slabs) == 0.0
    print("F64 warp restated generic path (ZEROS), worst u M by input type:", {k: round(v, 2) for k, v in worst.items()},
          "bound", W.K_ZEROS)
    assert max(worst.values()) <= W.K_ZEROS


def test_rescue_of_an_overflowing_blend_stays_finite_at_the_clamp():
    """A +inf (cleaned to FLT_MAX) above a y neighbour of -1.25 x 2^105, at a y fraction that widens to 1.0f: the plain blend
    overflows, and the rescue's quarter-scale blend rounds up to 2^126 — above FLT_MAX / 4 = 2^126 - 2^102, so scaling it back by 4
    without the clamp (or with a clamp at 2^126) returns the infinity the rescue exists to avoid.  The restatement, which clamps at
    FLT_MAX / 4 like ``lerp8f_clean``, and the reference stay finite, within the bound; so does the whole neighbourhood of that pair
    in the non-finite volume under the similarity warp."""
    fmax, partner = np.float32(W.FLT_MAX), np.float32(W.BIG_PARTNER)
    one = np.ones(4, np.float32)
    P = [[[partner * one, partner * one], [fmax * one, fmax * one]] for _ in (0, 1)]
    qy = np.array([0xFFFFFF80, 0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFFC0], np.int64)
    qz, qx = np.array([0, 0x80000000, 0xFFFFFFFF, 12345], np.int64), np.array([0, 0x40000000, 0xFFFFFFFF, 999], np.int64)
    assert (qy.astype(np.uint32).astype(np.float32) * np.float32(2.0 ** -32) == 1.0).all()
    with np.errstate(over="ignore", invalid="ignore"):
        plain = W.lerp8_f32(P, qz, qy, qx, rescue=False)
        quarter = W._fma(one, fmax * np.float32(0.25) - partner * np.float32(0.25), partner * np.float32(0.25))
    assert not np.isfinite(plain).any()
    assert (quarter.astype(np.float64) > W.FLT_MAX / 4).all() and float(np.float32(W.FLT_MAX / 4)) == 2.0 ** 126 - 2.0 ** 102
    got = W.lerp8_f32(P, qz, qy, qx)
    fy = (qy & 0xFFFFFFFF) / 2.0 ** 32
    want = (1 - fy) * float(partner) + fy * W.FLT_MAX
    assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - want) <= W.K_LERP * W.U * W.FLT_MAX).all()
    name, shape = "similarity 2 deg 1.02", W.T200
    m, out = W.pull_matrix(name, shape), W.OUT[shape]
    o = np.rint(np.linalg.solve(m, np.array(W.NONFINITE_BIG[0] + (1,), np.float64))[:3]).astype(int)
    lo = tuple(int(max(v - 3, 0)) for v in o)
    box = tuple(int(min(v + 4, n)) - a for v, n, a in zip(o, out, lo))
    vol = W.volume(shape, "f32", True)
    for boundary in (W.ITK, W.SCIPY):
        ref = R.warp_f64(vol, m, box, lo, "linear", boundary, W.CVAL)
        assert float(ref[1].max()) == W.FLT_MAX and bool(torch.isfinite(ref[0]).all())      # the pair is in the box
        W.assert_warp_close(W.warp_f32(vol, m, box, lo, "linear", boundary, W.CVAL), ref, W.K_LERP, "beside the big partner", cval=W.CVAL)


# ----------------------------------------------------------------------------- the bound bites where rel_err does not
# defect: (passes ``rel_err <= 1e-5``, passes the per-voxel bound) as the issue lists them
DEFECTS = {"bias": (True, False), "ytap": (True, False), "frac16": (True, False), "noclamp": (False, False), "overflow": (False, False)}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defects(defect):
    """Each defect planted in the restated lerp8, on the bead volume under the 2 deg / 1.02 similarity ("overflow": the volume with
    the non-finite values): the old assertion, ``rel_err <= 1e-5`` against the float32 oracle, and the per-voxel bound.
    Listed to pass the old and fail the new: bias, ytap, frac16; to fail both: noclamp, overflow.  Observed: as listed (bias:
    rel_err 7e-8, 169 u M; frac16: 6e-6, 264 u M; noclamp: 6e-5; overflow: infinities) except "ytap", which fails BOTH (rel_err
    9e-3) — see the comment at the assertion."""
    name, shape = "similarity 2 deg 1.02", W.T200
    vol = W.volume(shape, "f32", defect == "overflow")
    m, out = W.pull_matrix(name, shape), W.OUT[shape]
    ref = R.warp_f64(vol, m, out, (0, 0, 0), "linear", W.ITK, W.CVAL)
    oracle = O.affine_pull(vol, m, out, 1, W.ITK, W.CVAL)
    clean = W.warp_f32(vol, m, out, (0, 0, 0), "linear", W.ITK, W.CVAL)
    W.assert_warp_close(clean, ref, W.K_LERP, "no defect", cval=W.CVAL)
    got = W.warp_f32(vol, m, out, (0, 0, 0), "linear", W.ITK, W.CVAL, defect=defect)
    with np.errstate(invalid="ignore", over="ignore"):
        old = rel_err(got, oracle)
    passes_old = bool(old <= 1e-5)
    try:
        W.assert_warp_close(got, ref, W.K_LERP, defect, cval=W.CVAL)
        passes_new, what = True, ""
    except AssertionError as e:
        passes_new, what = False, str(e)
    print(f"F64 warp defect {defect}: rel_err {old:.3g} ({'passes' if passes_old else 'fails'}), bound "
          f"{'passes' if passes_new else 'fails'} {what}")
    assert not passes_new, defect
    want_old = DEFECTS[defect][0]
    if defect == "ytap":
        # A background voxel's two y taps differ by the camera noise (sigma 3 counts, up to ~15 between neighbours), so the wrong
        # row moves a voxel of 110 counts by several counts: 1e-5 of the brightest bead (0.6 counts) sees that too.  The defect
        # is kept as listed, not shrunk until the old assertion misses it.
        want_old = False
    assert passes_old == want_old, (defect, old)
