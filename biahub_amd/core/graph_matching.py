"""Graph matching of bead positions — mirror of ``biahub/core/graph_matching.py``.

``Graph`` is a point set (2-D or 3-D) with directed neighbour edges and the local features the reference derives from them;
``GraphMatcher`` turns two graphs into a cost matrix, solves the padded assignment with scipy and filters the matches.

The expensive part of the reference is ``GraphMatcher._compute_edge_consistency_cost`` (:518-571): for every pair of nodes a
small table of ``|edge attribute - edge attribute|``, ``linear_sum_assignment`` on it, the mean of the matched entries.  Here
that loop is one kernel launch per attribute (``bh_edge_consistency_cost``, csrc/graphmatch.hip): each graph's
attribute rows are gathered on the host (O(N k)), the N x M problems are solved on the device.  ``edge_consistency_cost_host``
restates the loop with numpy and scipy; it runs when a node has more than 16 neighbours or when ``device="cpu"`` is asked for,
and it is what the tests hold the kernel to.  Everything else (``cdist``, the PCA and descriptor terms, the padded assignment,
the filters) is vectorised host code on at most a few hundred points.
"""

from __future__ import annotations

import ctypes as C
from functools import cached_property
from typing import Literal

import click
import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.spatial.distance import cdist

from .. import _lib

KMAX = _lib.GRAPH_KMAX


class Graph:
    """Points (N, D), D = 2 or 3, stored as float32, and directed edges (i, j) between them (graph_matching.py:38-234)."""

    def __init__(self, nodes, edges: list[tuple[int, int]]):
        self.nodes = np.asarray(nodes, dtype=np.float32)
        self._edges = edges
        if self.nodes.ndim != 2:
            raise ValueError(f"nodes must be 2D array, got shape {self.nodes.shape}")
        if self.dim not in (2, 3):
            raise ValueError(f"nodes must be 2D or 3D points, got dim={self.dim}")

    @classmethod
    def from_nodes(cls, nodes, mode: Literal["knn", "radius", "full"] = "knn", k: int = 5, radius: float = 30.0) -> "Graph":
        return cls(nodes, cls._build_edges(nodes, mode=mode, k=k, radius=radius))

    @staticmethod
    def _build_edges(points, mode: Literal["knn", "radius", "full"] = "knn", k: int = 5, radius: float = 30.0) -> list[tuple[int, int]]:
        """Edges in node order, each node's neighbours in the order the neighbour search returns them (:95-127).  ``knn`` asks for
        k + 1 neighbours and drops the node itself: where points coincide the search may return the twin instead of the node,
        and that node keeps k + 1 neighbours."""
        n = len(points)
        if n <= 1:
            return []
        if mode == "knn":
            from sklearn.neighbors import NearestNeighbors

            _, found = NearestNeighbors(n_neighbors=min(k + 1, n)).fit(points).kneighbors(points)
            return [(i, j) for i in range(n) for j in found[i] if i != j]
        if mode == "radius":
            from sklearn.neighbors import radius_neighbors_graph

            near = radius_neighbors_graph(points, radius=radius, mode="connectivity", include_self=False)
            if near.nnz == 0:
                return []
            return [(i, j) for i in range(n) for j in near[i].nonzero()[1]]
        if mode == "full":
            return [(i, j) for i in range(n) for j in range(n) if i != j]
        raise ValueError(f"Unknown mode: {mode}")

    @property
    def n_nodes(self) -> int:
        return len(self.nodes)

    @property
    def dim(self) -> int:
        return self.nodes.shape[1]

    @property
    def edges(self) -> list[tuple[int, int]]:
        return self._edges

    @cached_property
    def neighbor_map(self) -> dict[int, list[int]]:
        """node -> its neighbours in edge order; nodes without an edge have no entry."""
        out: dict[int, list[int]] = {}
        for i, j in self._edges:
            out.setdefault(i, []).append(j)
        return out

    @cached_property
    def edge_distances(self) -> dict[tuple[int, int], float]:
        """Length of every edge, under both orientations of its key (float32 arithmetic, as the nodes are stored)."""
        out = {}
        for i, j in self._edges:
            length = float(np.linalg.norm(self.nodes[j] - self.nodes[i]))
            out[(i, j)] = length
            out[(j, i)] = length
        return out

    @cached_property
    def edge_angles(self) -> dict[tuple[int, int], float]:
        """2-D only: atan2 of every edge's direction in radians, stored under BOTH orientations of the key (:159-170).  The later
        edge in iteration order overwrites the earlier, so where (j, i) is an edge too and comes later, the entry of (i, j)
        holds the angle of the reverse edge.  Kept as the reference has it: the cost matrix depends on it."""
        if self.dim != 2:
            return {}
        out = {}
        for i, j in self._edges:
            d = self.nodes[j] - self.nodes[i]
            angle = float(np.arctan2(d[1], d[0]))
            out[(i, j)] = angle
            out[(j, i)] = angle
        return out

    @cached_property
    def edge_descriptors(self) -> np.ndarray:
        """(N, 4) float32: mean and standard deviation of a node's edge lengths and, in 2-D, of its edge angles (:172-195)."""
        desc = np.zeros((self.n_nodes, 4), dtype=np.float32)
        for i, nbrs in self.neighbor_map.items():
            lengths = np.array([self.edge_distances[(i, j)] for j in nbrs])
            desc[i, 0], desc[i, 1] = np.mean(lengths), np.std(lengths)
            if self.dim == 2 and self.edge_angles:
                angles = np.array([self.edge_angles[(i, j)] for j in nbrs])
                desc[i, 2], desc[i, 3] = np.mean(angles), np.std(angles)
        return desc

    @cached_property
    def pca_features(self) -> tuple[np.ndarray, np.ndarray]:
        """(directions (N, D), anisotropy (N,)), float32, from the SVD of each node's centred neighbours (:197-227): the first
        right singular vector and S[0] / (S[-1] + 1e-5); NaN for a node without neighbours."""
        n, d = self.n_nodes, self.dim
        directions = np.zeros((n, d), dtype=np.float32)
        anisotropy = np.zeros(n, dtype=np.float32)
        for i in range(n):
            nbrs = self.neighbor_map.get(i, [])
            if not nbrs:
                directions[i], anisotropy[i] = np.nan, np.nan
                continue
            local = self.nodes[nbrs].copy()
            local -= local.mean(axis=0)
            _, S, Vt = np.linalg.svd(local, full_matrices=False)
            directions[i] = Vt[0] if Vt.shape[0] > 0 else np.zeros(d)
            anisotropy[i] = S[0] / (S[-1] + 1e-5) if len(S) >= 2 else 0.0
        return directions, anisotropy

    def get_neighbors(self, node_idx: int) -> list[int]:
        return self.neighbor_map.get(node_idx, [])

    def __repr__(self) -> str:
        return f"Graph(n_nodes={self.n_nodes}, n_edges={len(self.edges)}, dim={self.dim})"


# ---- the edge-consistency cost ----------------------------------------------------------------------------------------
def attribute_rows(graph: Graph, attr_type: str) -> list[np.ndarray] | None:
    """Per node the attributes of its edges (i, neighbour) in neighbour order, float64 arrays (empty for a node without
    neighbours); None when the graph has no such attribute (angles outside 2-D, or no edge at all)."""
    if attr_type == "distance":
        attrs = graph.edge_distances
    elif attr_type == "angle":
        attrs = graph.edge_angles
        if not attrs:
            return None
    else:
        raise ValueError(f"Unknown attr_type: {attr_type}")
    nbrs = graph.neighbor_map
    return [np.array([attrs[(i, j)] for j in nbrs.get(i, [])], dtype=np.float64) for i in range(graph.n_nodes)]


def edge_consistency_cost_host(rows_a, rows_b, default_cost: float) -> np.ndarray:
    """The reference's loop (:543-569) on gathered rows: per pair the float32 table of ``|a_p - b_q|``,
    ``linear_sum_assignment``, the float32 ``mean`` of the matched entries; ``default_cost`` where either node has no edge."""
    cost = np.full((len(rows_a), len(rows_b)), default_cost, dtype=np.float32)
    for i, a in enumerate(rows_a):
        if len(a) == 0:
            continue
        for j, b in enumerate(rows_b):
            if len(b) == 0:
                continue
            table = np.abs(a[:, None] - b[None, :]).astype(np.float32)
            p, q = linear_sum_assignment(table)
            cost[i, j] = table[p, q].mean()
    return cost


def pack_rows(rows, kmax: int) -> tuple[np.ndarray, np.ndarray]:
    """(len(rows), kmax) float32 and the int32 counts the kernel reads; the attributes are float32 values already (they come
    from float32 arithmetic on the nodes), so nothing is rounded here."""
    attr = np.zeros((len(rows), kmax), dtype=np.float32)
    cnt = np.zeros(len(rows), dtype=np.int32)
    for i, r in enumerate(rows):
        cnt[i] = len(r)
        attr[i, : len(r)] = r
    return attr, cnt


def edge_consistency_plan(n: int, m: int) -> tuple[int, int, int, int]:
    """(tile_n, tile_m, tiles, workgroups per compute unit) of ``bh_edge_consistency_cost`` for an n x m matrix: a workgroup takes
    tiles of tile_n x tile_m pairs, and the grid wraps when ``tiles`` exceeds the last figure times the card's compute units."""
    tn, tm, tiles, cap = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    _lib.check(_lib.load().bh_edge_consistency_plan(int(n), int(m), C.byref(tn), C.byref(tm), C.byref(tiles), C.byref(cap)))
    return int(tn.value), int(tm.value), int(tiles.value), int(cap.value)


def edge_consistency_cost_packed(attr_a, cnt_a, attr_b, cnt_b, default_cost: float, device="cuda"):
    """``bh_edge_consistency_cost`` on packed rows (host arrays or device tensors); returns the (n, m) float32 device tensor."""
    import torch

    from ..device import get_context, ptr, resolve_device

    dev = resolve_device(device)

    def on_device(x, dtype):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        return t.to(device=dev, dtype=dtype).contiguous()

    ta, tb = on_device(attr_a, torch.float32), on_device(attr_b, torch.float32)
    ca, cb = on_device(cnt_a, torch.int32), on_device(cnt_b, torch.int32)
    if ta.ndim != 2 or tb.ndim != 2 or ta.shape[1] != tb.shape[1]:
        raise ValueError(f"attribute rows must be (n, kmax) and (m, kmax), got {tuple(ta.shape)} and {tuple(tb.shape)}")
    n, m, kmax = int(ta.shape[0]), int(tb.shape[0]), int(ta.shape[1])
    if ca.shape != (n,) or cb.shape != (m,):
        raise ValueError("one count per attribute row")
    ctx = get_context(dev)
    with torch.cuda.device(dev):
        cost = torch.empty((n, m), dtype=torch.float32, device=dev)
        _lib.check(ctx.lib.bh_edge_consistency_cost(ctx.handle, ptr(ta), ptr(ca), n, ptr(tb), ptr(cb), m, kmax,
                                                    C.c_float(default_cost), ptr(cost)))
    return cost


def edge_consistency_cost_device(rows_a, rows_b, default_cost: float, device="cuda") -> np.ndarray:
    """The same matrix as ``edge_consistency_cost_host`` from the kernel (every row at most 16 attributes)."""
    kmax = max(1, max((len(r) for r in rows_a), default=0), max((len(r) for r in rows_b), default=0))
    if kmax > KMAX:
        raise ValueError(f"a node has {kmax} edge attributes; the kernel takes at most {KMAX}")
    if len(rows_a) == 0 or len(rows_b) == 0:
        return np.zeros((len(rows_a), len(rows_b)), dtype=np.float32)
    return edge_consistency_cost_packed(*pack_rows(rows_a, kmax), *pack_rows(rows_b, kmax), default_cost, device).cpu().numpy()


class GraphMatcher:
    """Correspondences between two graphs (graph_matching.py:242-768).  ``algorithm="hungarian"``: cost matrix from position
    distance and edge consistency, padded assignment, quantile / ratio tests, optional cross check.  ``"descriptor"`` needs
    ``skimage.feature.match_descriptors`` and is refused.  ``device``: where the edge-consistency loop runs ("cpu": the host
    restatement)."""

    DEFAULT_WEIGHTS = {"dist": 0.5, "edge_length": 1.0, "edge_angle": 1.0, "pca_dir": 0.0, "pca_aniso": 0.0, "edge_descriptor": 0.0}

    def __init__(self, algorithm: Literal["hungarian", "descriptor"] = "hungarian", weights: dict[str, float] | None = None,
                 distance_metric: str = "euclidean", normalize: bool = False, cost_threshold: float = 0.9, cross_check: bool = False,
                 max_ratio: float | None = None, metric: str = "euclidean", verbose: bool = False, device="cuda"):
        self.algorithm = algorithm
        self.weights = {**self.DEFAULT_WEIGHTS, **(weights or {})}
        self.distance_metric = distance_metric
        self.normalize = normalize
        self.cost_threshold = cost_threshold
        self.cross_check = cross_check
        self.max_ratio = max_ratio
        self.verbose = verbose
        self.metric = metric
        self.device = device

    def match(self, moving: Graph, reference: Graph, verbose: bool | None = None) -> np.ndarray:
        """(K, 2) int32 pairs [moving index, reference index]."""
        verbose = self.verbose if verbose is None else verbose
        if moving.dim != reference.dim:
            raise ValueError(f"Dimension mismatch: moving={moving.dim}D, reference={reference.dim}D")
        if moving.n_nodes == 0 or reference.n_nodes == 0:
            if verbose:
                click.echo("Warning: One or both graphs are empty")
            return np.zeros((0, 2), dtype=np.int32)
        if self.algorithm == "hungarian":
            return self._match_hungarian(moving, reference, verbose)
        if self.algorithm == "descriptor":
            raise NotImplementedError("GraphMatcher(algorithm='descriptor') calls skimage.feature.match_descriptors, which this "
                                      "package does not have; use algorithm='hungarian'")
        raise ValueError(f"Unknown algorithm: {self.algorithm}")

    def _match_hungarian(self, moving: Graph, reference: Graph, verbose: bool) -> np.ndarray:
        if not self.cross_check:
            return self._solve_assignment(self.compute_cost_matrix(moving, reference), verbose)
        forward = self._solve_assignment(self.compute_cost_matrix(moving, reference), False)
        backward = self._solve_assignment(self.compute_cost_matrix(reference, moving), False)
        confirmed = {(int(i), int(j)) for j, i in backward}
        matches = np.array([[i, j] for i, j in forward if (int(i), int(j)) in confirmed], dtype=np.int32).reshape(-1, 2)
        if verbose:
            click.echo(f"Forward: {len(forward)} matches, backward: {len(backward)}, cross-check: {len(matches)} symmetric matches")
        return matches

    def _edge_consistency_cost(self, moving: Graph, reference: Graph, attr_type: str, default_cost: float) -> np.ndarray:
        rows_a, rows_b = attribute_rows(moving, attr_type), attribute_rows(reference, attr_type)
        if rows_a is None or rows_b is None:
            return np.full((moving.n_nodes, reference.n_nodes), default_cost, dtype=np.float32)
        widest = max(max(len(r) for r in rows_a), max(len(r) for r in rows_b))
        if widest > KMAX or str(self.device) == "cpu":
            return edge_consistency_cost_host(rows_a, rows_b, default_cost)
        return edge_consistency_cost_device(rows_a, rows_b, default_cost, self.device)

    def compute_cost_matrix(self, moving: Graph, reference: Graph) -> np.ndarray:
        """(N, M) float32.  The terms are accumulated by the reference's own expressions, in its order (:451-516), so numpy
        rounds as it does there: ``total += w * term`` on the float32 ``total`` with a float64 term (cdist, the normalised
        angle term) is a float64 multiply-add rounded to float32; with a float32 term the product is float32 already."""
        n, m = moving.n_nodes, reference.n_nodes
        total = np.zeros((n, m), dtype=np.float32)
        w = self.weights

        def scaled(term):
            if self.normalize:
                top = term.max()
                if top > 0:
                    term = term / top
            return term

        if w["dist"] > 0:
            total += w["dist"] * scaled(cdist(moving.nodes, reference.nodes, metric=self.distance_metric))
        if w["edge_length"] > 0:
            total += w["edge_length"] * scaled(self._edge_consistency_cost(moving, reference, "distance", 1e6))
        if w["edge_angle"] > 0 and moving.dim == 2:
            term = self._edge_consistency_cost(moving, reference, "angle", np.pi)
            if self.normalize:
                term = term / np.pi
            total += w["edge_angle"] * term
        if w["pca_dir"] > 0 or w["pca_aniso"] > 0:
            mov_dirs, mov_aniso = moving.pca_features
            ref_dirs, ref_aniso = reference.pca_features
            if w["pca_dir"] > 0:
                total += w["pca_dir"] * scaled(1 - np.abs(np.clip(np.dot(mov_dirs, ref_dirs.T), -1.0, 1.0)))
            if w["pca_aniso"] > 0:
                total += w["pca_aniso"] * scaled(np.abs(mov_aniso[:, None] - ref_aniso[None, :]))
        if w["edge_descriptor"] > 0:
            total += w["edge_descriptor"] * scaled(cdist(moving.edge_descriptors, reference.edge_descriptors))
        return total

    def _solve_assignment(self, cost: np.ndarray, verbose: bool) -> np.ndarray:
        """Assignment on the matrix padded to a square with 1e6 (:573-615); a pair is kept when it is inside the matrix, its cost
        lies below the ``cost_threshold`` quantile of the whole matrix and, with ``max_ratio``, it is at most that fraction of the
        row's second smallest cost."""
        n_a, n_b = cost.shape
        side = max(n_a, n_b)
        padded = np.full((side, side), 1e6, dtype=np.float32)
        padded[:n_a, :n_b] = cost
        rows, cols = linear_sum_assignment(padded)
        limit = np.quantile(cost, self.cost_threshold)
        kept = []
        for i, j in zip(rows, cols):
            if i >= n_a or j >= n_b or cost[i, j] >= limit:
                continue
            if self.max_ratio is not None and n_b > 1:
                second = np.sort(cost[i, :])[1]
                if cost[i, j] / (second + 1e-10) > self.max_ratio:
                    continue
            kept.append((i, j))
        if verbose:
            click.echo(f"Found {len(kept)} matches (cost_threshold={limit:.3f})")
        return np.array(kept, dtype=np.int32).reshape(-1, 2)

    def filter_matches(self, matches, moving: Graph, reference: Graph, angle_threshold: float | None = 0,
                       direction_threshold: float | None = 0, min_distance_quantile: float = 0.01,
                       max_distance_quantile: float = 0.95, verbose: bool | None = None) -> np.ndarray:
        """Geometric consistency filters (:656-768), in the reference's order: displacement length inside two quantiles,
        direction within ``direction_threshold`` degrees of the mean unit displacement, and (2-D) angle within
        ``angle_threshold`` degrees of the fullest of 35 histogram bins.  A threshold of 0 switches its filter off."""
        verbose = self.verbose if verbose is None else verbose
        if len(matches) == 0:
            return matches
        if min_distance_quantile != 0 or max_distance_quantile != 0:
            length = np.linalg.norm(moving.nodes[matches[:, 0]] - reference.nodes[matches[:, 1]], axis=1)
            low, high = np.quantile(length, min_distance_quantile), np.quantile(length, max_distance_quantile)
            matches = matches[(length >= low) & (length <= high)]
            if verbose:
                click.echo(f"Distance range: [{low:.3f}, {high:.3f}]; matches after distance filtering: {len(matches)}")
        if direction_threshold != 0:
            shift = reference.nodes[matches[:, 1]] - moving.nodes[matches[:, 0]]
            unit = shift / (np.linalg.norm(shift, axis=1, keepdims=True) + 1e-10)
            mean = unit.mean(axis=0)
            mean = mean / (np.linalg.norm(mean) + 1e-10)
            off = np.degrees(np.arccos(np.clip(unit @ mean, -1.0, 1.0)))
            matches = matches[off <= direction_threshold]
            if verbose:
                click.echo(f"Dominant direction: {mean}; matches after direction filtering: {len(matches)}")
        if angle_threshold != 0 and moving.dim == 2:
            shift = reference.nodes[matches[:, 1]] - moving.nodes[matches[:, 0]]
            deg = np.degrees(np.arctan2(shift[:, 1], shift[:, 0]))
            hist, edges = np.histogram(deg, bins=np.linspace(-180, 180, 36))
            top = np.argmax(hist)
            dominant = (edges[top] + edges[top + 1]) / 2
            matches = matches[np.abs(deg - dominant) <= angle_threshold]
            if verbose:
                click.echo(f"Dominant angle: {dominant:.1f}; matches after 2D angle filtering: {len(matches)}")
        return matches
