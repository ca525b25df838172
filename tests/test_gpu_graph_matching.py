"""GPU: ``bh_edge_consistency_cost`` (csrc/graphmatch.hip) against the table-and-``linear_sum_assignment`` value of
tests/graph_match_ref.py, and ``GraphMatcher.match`` on the device against the restatement's matches.

The bound.  Every element must lie within ``16 * 2^-24 * |ref|`` of the restatement, and an exact zero must be zero.  The
restatement sums at most 16 float32 entries in float32 and divides: n + 1 <= 17 roundings of relative size 2^-24 on
non-negative terms.  The kernel sums the same entries and divides in float64 and rounds once, which is within half a unit
of the exact mean, so the two differ by at most the restatement's own error; 16 units cover the up to 15 additions and the
division.  (The kernel's matching is optimal for the exact |a - b|; the float32 rounding of the entries can make the
restatement's optimum smaller by less than that again.)  The bound comes from this count, not from the kernel's output.

Figures printed on an MI355X (``-s`` shows them; worst |got - ref| / |ref| in units of 2^-24 over the non-zero elements, and the
number of exact zeros):

    tile edge (1, 1) 0.00; (1, 67) 1.32; (67, 1) 0.00; (15, 63) 1.99; (15, 64) 1.94; (15, 65) 2.81; (16, 63) 2.30; (16, 64) 2.46;
        (16, 65) 1.97; (17, 63) 2.23; (17, 64) 2.34; (17, 65) 1.99 (no zeros)
    counts all 1 (19, 69)                0.00 (one entry a pair: equal bit for bit)
    counts 0 .. 16, roots (21, 73)       2.78, 196 exact zeros
    kmax = 16 full rows (17, 65)         2.07
    unsorted signed angles (21, 70)      2.79
    rows of equal values (19, 66)        2.41, 421 exact zeros
    wrap (4117, 193), 256 compute units  1.60; 1032 tiles on a grid of 1024 workgroups; the second launch returned the same bytes
    matcher, 60 x 60 beads               53 matches without and 53 with the cross check, equal to the restatement's
"""

import numpy as np
import pytest
import torch

import graph_match_ref as R
from biahub_amd.core.graph_matching import (Graph, GraphMatcher, edge_consistency_cost_device, edge_consistency_cost_packed,
                                            edge_consistency_plan, pack_rows)

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -24
BOUND = 16 * UNIT
TN, TM = 16, 64  # the workgroup's tile of pairs (asserted against the plan below)


def _rows(rng, n, counts, kind):
    """n attribute rows (float32 values as float64 arrays): ``lengths`` uniform in [1, 60), ``angles`` signed and unsorted,
    ``roots`` square roots of small integers (many exact ties), ``equal`` one value repeated along each row."""
    out = []
    for i in range(n):
        k = int(counts[i])
        if kind == "lengths":
            r = np.sort(rng.uniform(1, 60, k))  # knn rows arrive ascending
        elif kind == "angles":
            r = rng.uniform(-np.pi, np.pi, k)
        elif kind == "roots":
            r = np.sqrt(rng.integers(1, 12, k).astype(np.float64))
        else:
            r = np.full(k, np.sqrt(float(rng.integers(1, 4))))
        out.append(r.astype(np.float32).astype(np.float64))
    return out


def _hold(name, got, want):
    assert got.shape == want.shape and got.dtype == np.float32, name
    zero = want == 0
    assert np.all(got[zero] == 0), f"{name}: an exact zero of the restatement is not zero"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = err[~zero] / np.abs(want[~zero].astype(np.float64))
    worst = float(rel.max() / UNIT) if rel.size else 0.0
    print(f"GRAPHMATCH gpu {name} {want.shape}: worst {worst:.2f} units of 2^-24, {int(zero.sum())} exact zeros")
    assert np.all(err <= BOUND * np.abs(want.astype(np.float64))), f"{name}: worst {worst:.2f} units, allowed 16"
    return worst


def _run(gpu, rows_a, rows_b, default):
    return edge_consistency_cost_device(rows_a, rows_b, default, gpu)


def test_plan_matches_the_tile_the_cases_are_sized_for(gpu):
    tn, tm, tiles, cap = edge_consistency_plan(TN + 1, TM + 1)
    assert (tn, tm, tiles) == (TN, TM, 4) and cap >= 1
    assert edge_consistency_plan(TN, TM)[2] == 1 and edge_consistency_plan(0, 5)[2] == 0


SHAPES = [(1, 1), (1, 67), (67, 1)] + [(n, m) for n in (TN - 1, TN, TN + 1) for m in (TM - 1, TM, TM + 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_edges(gpu, shape):
    """One pair, one row, one column, and one less than, equal to and one more than the tile in each direction; counts 1 .. 6, so
    both k_i < k_j and k_i > k_j occur, on sorted lengths."""
    n, m = shape
    rng = np.random.default_rng(100 * n + m)
    a = _rows(rng, n, rng.integers(1, 7, n), "lengths")
    b = _rows(rng, m, rng.integers(1, 7, m), "lengths")
    _hold("tile edge", _run(gpu, a, b, 1e6), R.edge_cost_rows(a, b, 1e6))


def test_counts_of_one(gpu):
    rng = np.random.default_rng(1)
    a, b = _rows(rng, TN + 3, np.ones(TN + 3), "lengths"), _rows(rng, TM + 5, np.ones(TM + 5), "lengths")
    got = _run(gpu, a, b, 1e6)
    _hold("counts all 1", got, R.edge_cost_rows(a, b, 1e6))
    assert np.array_equal(got, np.abs(np.array(a) - np.array(b).T).astype(np.float32))  # one entry, nothing to sum


def test_mixed_counts_zero_to_kmax(gpu):
    """Counts 0 .. 16 on both sides in one matrix: 0 gives ``default_cost`` (a whole row or column of it), every combination of
    shorter and longer rows, kmax = 16."""
    rng = np.random.default_rng(2)
    ca, cb = rng.integers(0, 17, TN + 5), rng.integers(0, 17, TM + 9)
    ca[:3], cb[:3] = (0, 16, 1), (16, 0, 1)
    a, b = _rows(rng, len(ca), ca, "roots"), _rows(rng, len(cb), cb, "roots")
    got, want = _run(gpu, a, b, 1e6), R.edge_cost_rows(a, b, 1e6)
    _hold("counts 0 .. 16, roots", got, want)
    assert np.all(got[ca == 0, :] == np.float32(1e6)) and np.all(got[:, cb == 0] == np.float32(1e6))
    assert ((ca[:, None] < cb[None, :]) & (ca[:, None] > 0)).any() and ((ca[:, None] > cb[None, :]) & (cb[None, :] > 0)).any()


def test_full_rows_of_sixteen(gpu):
    rng = np.random.default_rng(3)
    a, b = _rows(rng, TN + 1, np.full(TN + 1, 16), "lengths"), _rows(rng, TM + 1, np.full(TM + 1, 16), "lengths")
    _hold("kmax = 16 full rows", _run(gpu, a, b, 1e6), R.edge_cost_rows(a, b, 1e6))


def test_unsorted_signed_angles(gpu):
    rng = np.random.default_rng(4)
    ca, cb = rng.integers(0, 9, 21), rng.integers(0, 9, 70)
    a, b = _rows(rng, 21, ca, "angles"), _rows(rng, 70, cb, "angles")
    got = _run(gpu, a, b, np.pi)
    _hold("unsorted signed angles", got, R.edge_cost_rows(a, b, np.pi))
    assert np.all(got[ca == 0, :] == np.float32(np.pi))


def test_rows_of_equal_values_tie(gpu):
    rng = np.random.default_rng(5)
    a, b = _rows(rng, 19, rng.integers(1, 12, 19), "equal"), _rows(rng, 66, rng.integers(1, 12, 66), "equal")
    want = R.edge_cost_rows(a, b, 1e6)
    _hold("rows of equal values", _run(gpu, a, b, 1e6), want)
    assert (want == 0).sum() > 50  # equal rows against equal rows of the same value: exact zeros


def test_grid_wraps_and_repeats_bit_equal(gpu):
    """n x 193 with n from the card's compute-unit count, so that the tiles exceed the capped grid and workgroups take a second
    trip through their grid-stride loop (asserted).  The rows are drawn from 7 and 5 distinct rows (periods that share no
    factor with the tile), so the restatement is 35 assignments gathered into the matrix; two launches return the same bytes."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    cap = edge_consistency_plan(1, 1)[3] * cus
    m = 3 * TM + 1
    n = TN * (cap // 4 + 1) + 5
    tiles = edge_consistency_plan(n, m)[2]
    assert cap < tiles < 2 * cap, f"({n}, {m}): {tiles} tiles do not wrap a grid of {cap} workgroups once: size the case for this card"
    rng = np.random.default_rng(6)
    pool_a = _rows(rng, 7, [5, 3, 0, 7, 5, 1, 11], "roots")
    pool_b = _rows(rng, 5, [5, 6, 2, 0, 9], "lengths")
    table = R.edge_cost_rows(pool_a, pool_b, 1e6)
    ia, ib = np.arange(n) % 7, np.arange(m) % 5
    want = table[ia[:, None], ib[None, :]]
    attr_a, cnt_a = pack_rows([pool_a[i] for i in ia], 11)
    attr_b, cnt_b = pack_rows([pool_b[j] for j in ib], 11)
    first = edge_consistency_cost_packed(attr_a, cnt_a, attr_b, cnt_b, 1e6, gpu).cpu().numpy()
    _hold("wrap", first, want)
    again = edge_consistency_cost_packed(attr_a, cnt_a, attr_b, cnt_b, 1e6, gpu).cpu().numpy()
    assert first.tobytes() == again.tobytes()


def test_refusals(gpu):
    with pytest.raises(ValueError, match="kmax"):
        edge_consistency_cost_packed(np.zeros((2, 17), np.float32), np.zeros(2, np.int32), np.zeros((2, 17), np.float32), np.zeros(2, np.int32), 1.0, gpu)
    with pytest.raises(ValueError, match="at most 16"):
        edge_consistency_cost_device([np.zeros(17)], [np.zeros(3)], 1.0, gpu)
    # counts beyond the row are clamped, never followed past it
    attr = np.arange(6, dtype=np.float32).reshape(2, 3)
    got = edge_consistency_cost_packed(attr, np.array([99, -4], np.int32), attr, np.array([3, 3], np.int32), 7.0, gpu).cpu().numpy()
    assert got[0, 0] == 0 and got[0, 1] == 3 and np.all(got[1] == 7.0)


SEED = 11  # not tie-sensitive: with the kernel's arithmetic (float64 sum, one rounding) evaluated on the host, seeds 11, 12 and 13
# all give the restatement's matches, with and without the cross check


def _bead_sets(seed=SEED):
    """60 reference beads in a 64 x 256 x 256 box; the moving set is a rigid motion of them (2 degrees about z, a few voxels of
    shift) with 0.3-voxel jitter, 5 beads dropped and 5 spurious ones added, shuffled."""
    rng = np.random.default_rng(seed)
    ref = rng.uniform(0, 1, (60, 3)) * np.array([64.0, 256.0, 256.0])
    t = np.radians(2.0)
    rot = np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])
    centre = np.array([32.0, 128.0, 128.0])
    mov = (ref - centre) @ rot.T + centre + np.array([1.5, -4.0, 3.0]) + rng.normal(0, 0.3, ref.shape)
    mov = np.concatenate([mov[5:], rng.uniform(0, 1, (5, 3)) * np.array([64.0, 256.0, 256.0])])
    return mov[rng.permutation(len(mov))], ref


@pytest.mark.parametrize("cross_check", [False, True])
def test_matcher_on_the_device_returns_the_restatements_matches(gpu, cross_check):
    mov, ref = _bead_sets()
    kw = dict(cost_threshold=0.10, max_ratio=0.8, cross_check=cross_check)
    want = R.match(mov, ref, k=5, **kw)
    gm, gr = Graph.from_nodes(mov, mode="knn", k=5), Graph.from_nodes(ref, mode="knn", k=5)
    got = GraphMatcher(device=gpu, **kw).match(gm, gr)
    print(f"GRAPHMATCH gpu matcher cross_check={cross_check}: {len(want)} matches")
    assert len(want) >= 10 and got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(GraphMatcher(device="cpu", **kw).match(gm, gr), want)
