"""Plain numpy + scipy restatement of the Hungarian graph matching of ``biahub/core/graph_matching.py``: the yardstick of
tests/test_graph_matching_host.py (the package's host functions equal it bit for bit) and of tests/test_gpu_graph_matching.py
(the kernel lies within a derived bound of it).  Nothing here imports the package.

The pieces, in the order the reference runs them:
  knn_edges, neighbours, edge_attributes   the graph: edges in search order, the attribute dictionaries with their overwrite rule
  pair_cost, edge_cost_rows, edge_cost     per pair the float32 table |a_p - b_q|, linear_sum_assignment, the float32 mean
  cost_matrix                              the weighted sum of the terms, accumulated into float32 in the reference's order
  solve_assignment                         padded assignment, quantile and ratio tests
  filter_matches                           distance quantiles, direction, 2-D angle
  match                                    one direction, or both with the cross check
"""

import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial.distance import cdist

WEIGHTS = {"dist": 0.5, "edge_length": 1.0, "edge_angle": 1.0, "pca_dir": 0.0, "pca_aniso": 0.0, "edge_descriptor": 0.0}


def knn_edges(points, k):
    """(i, j) for every node i and each of its k + 1 nearest points j that is not i itself, in the search's order."""
    from sklearn.neighbors import NearestNeighbors

    n = len(points)
    if n <= 1:
        return []
    _, idx = NearestNeighbors(n_neighbors=min(k + 1, n)).fit(points).kneighbors(points)
    return [(i, j) for i in range(n) for j in idx[i] if i != j]


def neighbours(edges, n):
    out = [[] for _ in range(n)]
    for i, j in edges:
        out[i].append(j)
    return out


def edge_attributes(points32, edges, kind):
    """{(i, j): value}: every edge writes its value under both orientations of its key, later edges over earlier ones."""
    table = {}
    for i, j in edges:
        d = points32[j] - points32[i]
        v = float(np.linalg.norm(d)) if kind == "distance" else float(np.arctan2(d[1], d[0]))
        table[(i, j)] = v
        table[(j, i)] = v
    return table


def attribute_rows(points, edges, kind):
    """Per node the values of its edges (i, neighbour), neighbours in edge order."""
    p32 = np.asarray(points, dtype=np.float32)
    table = edge_attributes(p32, edges, kind)
    return [np.array([table[(i, j)] for j in nb], dtype=np.float64) for i, nb in enumerate(neighbours(edges, len(p32)))]


def pair_cost(a, b):
    """One element: the k_a x k_b float32 table, its optimal assignment, the float32 mean of the matched entries."""
    table = np.empty((len(a), len(b)), dtype=np.float32)
    for p in range(len(a)):
        for q in range(len(b)):
            table[p, q] = abs(float(a[p]) - float(b[q]))
    rows, cols = linear_sum_assignment(table)
    return table[rows, cols].mean()


def edge_cost_rows(rows_a, rows_b, default_cost):
    out = np.full((len(rows_a), len(rows_b)), default_cost, dtype=np.float32)
    for i, a in enumerate(rows_a):
        for j, b in enumerate(rows_b):
            if len(a) and len(b):
                out[i, j] = pair_cost(a, b)
    return out


def edge_cost(points_a, edges_a, points_b, edges_b, kind, default_cost):
    return edge_cost_rows(attribute_rows(points_a, edges_a, kind), attribute_rows(points_b, edges_b, kind), default_cost)


def cost_matrix(points_a, edges_a, points_b, edges_b, weights=None, normalize=False, metric="euclidean"):
    """dist, edge_length, edge_angle (2-D), in that order, each added as ``total += w * term`` to a float32 total (the PCA and
    descriptor terms have weight 0 by default and are not restated)."""
    w = {**WEIGHTS, **(weights or {})}
    a32, b32 = np.asarray(points_a, dtype=np.float32), np.asarray(points_b, dtype=np.float32)
    total = np.zeros((len(a32), len(b32)), dtype=np.float32)
    if w["dist"] > 0:
        term = cdist(a32, b32, metric=metric)
        if normalize and term.max() > 0:
            term = term / term.max()
        total += w["dist"] * term
    if w["edge_length"] > 0:
        term = edge_cost(points_a, edges_a, points_b, edges_b, "distance", 1e6)
        if normalize and term.max() > 0:
            term = term / term.max()
        total += w["edge_length"] * term
    if w["edge_angle"] > 0 and a32.shape[1] == 2:
        if edges_a and edges_b:
            term = edge_cost(points_a, edges_a, points_b, edges_b, "angle", np.pi)
        else:
            term = np.full(total.shape, np.pi, dtype=np.float32)
        if normalize:
            term = term / np.pi
        total += w["edge_angle"] * term
    assert w["pca_dir"] == 0 and w["pca_aniso"] == 0 and w["edge_descriptor"] == 0
    return total


def solve_assignment(C, cost_threshold=0.9, max_ratio=None):
    n_a, n_b = C.shape
    n = max(n_a, n_b)
    padded = np.full((n, n), 1e6, dtype=np.float32)
    padded[:n_a, :n_b] = C
    rows, cols = linear_sum_assignment(padded)
    threshold = np.quantile(C, cost_threshold)
    out = []
    for i, j in zip(rows, cols):
        if i >= n_a or j >= n_b:
            continue
        if C[i, j] >= threshold:
            continue
        if max_ratio is not None:
            ordered = np.sort(C[i, :])
            if len(ordered) > 1 and C[i, j] / (ordered[1] + 1e-10) > max_ratio:
                continue
        out.append((i, j))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def filter_matches(matches, points_a, points_b, angle_threshold=0, direction_threshold=0, min_distance_quantile=0.01,
                   max_distance_quantile=0.95):
    a32, b32 = np.asarray(points_a, dtype=np.float32), np.asarray(points_b, dtype=np.float32)
    if len(matches) == 0:
        return matches
    if min_distance_quantile != 0 or max_distance_quantile != 0:
        dist = np.linalg.norm(a32[matches[:, 0]] - b32[matches[:, 1]], axis=1)
        lo, hi = np.quantile(dist, min_distance_quantile), np.quantile(dist, max_distance_quantile)
        matches = matches[(dist >= lo) & (dist <= hi)]
    if direction_threshold != 0:
        v = b32[matches[:, 1]] - a32[matches[:, 0]]
        u = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-10)
        m = u.mean(axis=0)
        m = m / (np.linalg.norm(m) + 1e-10)
        matches = matches[np.degrees(np.arccos(np.clip(u @ m, -1.0, 1.0))) <= direction_threshold]
    if angle_threshold != 0 and a32.shape[1] == 2:
        v = b32[matches[:, 1]] - a32[matches[:, 0]]
        deg = np.degrees(np.arctan2(v[:, 1], v[:, 0]))
        hist, edges = np.histogram(deg, bins=np.linspace(-180, 180, 36))
        k = np.argmax(hist)
        matches = matches[np.abs(deg - (edges[k] + edges[k + 1]) / 2) <= angle_threshold]
    return matches


def match(points_a, points_b, k=5, weights=None, cost_threshold=0.9, max_ratio=None, cross_check=False, normalize=False):
    ea, eb = knn_edges(points_a, k), knn_edges(points_b, k)
    forward = solve_assignment(cost_matrix(points_a, ea, points_b, eb, weights, normalize), cost_threshold, max_ratio)
    if not cross_check:
        return forward
    backward = solve_assignment(cost_matrix(points_b, eb, points_a, ea, weights, normalize), cost_threshold, max_ratio)
    agreed = {(j, i) for i, j in backward}
    return np.array([[i, j] for i, j in forward if (i, j) in agreed], dtype=np.int32).reshape(-1, 2)
