"""CPU: the host side of bead registration — ``core/graph_matching.py`` against the restatement of tests/graph_match_ref.py bit
for bit, the point-set fits and the overlap score of ``registration/beads.py`` on hand-made inputs, the settings' defaults, and
the two CLI commands getting past their method checks.  The kernel itself is held in tests/test_gpu_graph_matching.py."""

import numpy as np
import pytest
from click.testing import CliRunner

import graph_match_ref as R
from biahub_amd.core.graph_matching import Graph, GraphMatcher, attribute_rows, edge_consistency_cost_host


def _points(n, dim, seed, duplicate=False, coincident=False):
    rng = np.random.default_rng(seed)
    box = np.array([64.0, 256.0, 256.0])[-dim:]
    pts = rng.uniform(0, 1, (n, dim)) * box
    if duplicate:
        pts[n // 2] = pts[1]
    if coincident:  # four points in one place: with k = 2 the search returns three twins for one of them, and not the node
        pts[3] = pts[5] = pts[7] = pts[1]
    return pts


CASES = {
    "3-D 14 x 11": (_points(14, 3, 1), _points(11, 3, 2), 5),
    "2-D 9 x 12": (_points(9, 2, 3), _points(12, 2, 4), 5),
    "3-D with a duplicate point": (_points(13, 3, 5, duplicate=True), _points(10, 3, 6), 4),
    "2-D with a duplicate point": (_points(10, 2, 7, duplicate=True), _points(10, 2, 8, duplicate=True), 3),
    "3-D four coincident points": (_points(9, 3, 13, coincident=True), _points(8, 3, 14), 2),
    "2-D four coincident points": (_points(9, 2, 15, coincident=True), _points(9, 2, 16, coincident=True), 2),
    "no more nodes than k": (_points(4, 3, 9), _points(5, 3, 10), 5),
    "one node against six": (_points(1, 3, 11), _points(6, 3, 12), 5),
}


@pytest.mark.parametrize("name", CASES)
def test_host_edge_consistency_equals_restatement(name):
    a, b, k = CASES[name]
    ga, gb = Graph.from_nodes(a, mode="knn", k=k), Graph.from_nodes(b, mode="knn", k=k)
    ea, eb = R.knn_edges(a, k), R.knn_edges(b, k)
    assert [tuple(map(int, e)) for e in ga.edges] == [tuple(map(int, e)) for e in ea]
    kinds = [("distance", 1e6)] + ([("angle", np.pi)] if a.shape[1] == 2 else [])
    for kind, default in kinds:
        rows_a, rows_b = attribute_rows(ga, kind), attribute_rows(gb, kind)
        want_rows = R.attribute_rows(a, ea, kind)
        assert len(rows_a) == len(want_rows) and all(np.array_equal(x, y) for x, y in zip(rows_a, want_rows))
        got = edge_consistency_cost_host(rows_a, rows_b, default)
        want = R.edge_cost(a, ea, b, eb, kind, default)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (name, kind)
    if len(a) == 1:  # a single node has no edge: the default everywhere
        assert np.all(got == np.float32(1e6))
    counts = [len(r) for r in attribute_rows(ga, "distance")]
    assert counts == [len(r) for r in R.attribute_rows(a, ea, "distance")] and max(counts, default=0) <= k + 1
    if "coincident" in name:  # twins stand in for the node itself in the search: that node keeps k + 1 neighbours
        assert max(counts) == k + 1, counts


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("cross_check", [False, True])
def test_host_matcher_equals_restatement(name, cross_check):
    a, b, k = CASES[name]
    ga, gb = Graph.from_nodes(a, mode="knn", k=k), Graph.from_nodes(b, mode="knn", k=k)
    for normalize in (False, True):
        m = GraphMatcher(cost_threshold=0.5, max_ratio=0.9, cross_check=cross_check, normalize=normalize, device="cpu")
        want_cost = R.cost_matrix(a, R.knn_edges(a, k), b, R.knn_edges(b, k), normalize=normalize)
        assert m.compute_cost_matrix(ga, gb).tobytes() == want_cost.tobytes(), (name, normalize)
        got = m.match(ga, gb)
        want = R.match(a, b, k=k, cost_threshold=0.5, max_ratio=0.9, cross_check=cross_check, normalize=normalize)
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, normalize)
    loose = GraphMatcher(cost_threshold=1.0, device="cpu")
    matches = loose.match(ga, gb)
    for kw in (dict(), dict(direction_threshold=50), dict(angle_threshold=30, min_distance_quantile=0, max_distance_quantile=0)):
        assert np.array_equal(loose.filter_matches(matches, ga, gb, **kw), R.filter_matches(matches, a, b, **kw)), (name, kw)


def test_angle_of_an_edge_is_overwritten_by_its_reverse():
    """Nodes 0 = (0, 0), 1 = (1, 0), 2 = (0, 1); edges (0, 1), (0, 2), (1, 0), (2, 1) in that order.  Edge (0, 1) points along +x
    (angle 0), but (1, 0), which comes later, writes its own angle pi under both keys: node 0's row holds pi, not 0.  Edge (0, 2)
    has no reverse and keeps pi / 2; (2, 1) points along (1, -1)."""
    nodes = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    g = Graph(nodes, [(0, 1), (0, 2), (1, 0), (2, 1)])
    pi32 = float(np.float32(np.pi))
    assert g.edge_angles[(0, 1)] == pi32 and g.edge_angles[(1, 0)] == pi32
    assert g.edge_angles[(0, 2)] == float(np.float32(np.pi / 2)) and g.edge_angles[(2, 0)] == float(np.float32(np.pi / 2))
    rows = attribute_rows(g, "angle")
    assert rows[0].tolist() == [pi32, float(np.float32(np.pi / 2))]
    assert rows[1].tolist() == [pi32]
    assert rows[2].tolist() == [float(np.arctan2(np.float32(-1), np.float32(1)))]
    assert g.edge_angles == R.edge_attributes(nodes.astype(np.float32), g.edges, "angle")
    # lengths have no such trap: both orientations are the same number
    assert g.edge_distances[(0, 1)] == 1.0 and g.edge_distances[(2, 1)] == float(np.float32(np.sqrt(np.float32(2))))
    assert Graph(np.zeros((3, 3)), []).edge_angles == {} and attribute_rows(Graph(np.zeros((3, 3)), [(0, 1)]), "angle") is None


def test_graph_modes_and_refusals():
    pts = _points(8, 3, 20)
    assert len(Graph.from_nodes(pts, mode="full").edges) == 8 * 7
    near = Graph.from_nodes(pts, mode="radius", radius=120.0)
    for i, j in near.edges:
        assert i != j and np.linalg.norm(pts[i] - pts[j]) <= 120.0
    assert Graph.from_nodes(pts[:1]).edges == [] and Graph.from_nodes(pts, mode="radius", radius=1e-3).edges == []
    with pytest.raises(ValueError, match="Unknown mode"):
        Graph.from_nodes(pts, mode="delaunay")
    with pytest.raises(ValueError, match="2D or 3D"):
        Graph(np.zeros((3, 4)), [])
    g = Graph.from_nodes(pts)
    with pytest.raises(NotImplementedError, match="match_descriptors"):
        GraphMatcher(algorithm="descriptor").match(g, g)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        GraphMatcher().match(g, Graph.from_nodes(pts[:, :2]))
    assert GraphMatcher().match(Graph(np.zeros((0, 3)), []), g).shape == (0, 2)
    d, a = g.pca_features
    assert d.shape == (8, 3) and a.shape == (8,) and g.edge_descriptors.shape == (8, 4)
    # more than 16 neighbours a node: the host loop, whatever the device
    full = Graph.from_nodes(_points(19, 3, 21), mode="full")
    got = GraphMatcher(device="cuda")._edge_consistency_cost(full, g, "distance", 1e6)
    assert got.tobytes() == edge_consistency_cost_host(attribute_rows(full, "distance"), attribute_rows(g, "distance"), 1e6).tobytes()


def _twelve(seed=3):
    return np.random.default_rng(seed).uniform(0, 200, (12, 3))


def _settings(kind):
    from biahub_amd.settings import AffineTransformSettings

    return AffineTransformSettings(transform_type=kind)


@pytest.mark.parametrize("kind,scale", [("euclidean", 1.0), ("similarity", 1.0), ("similarity", 1.37)])
def test_umeyama_recovers_rotation_translation_scale(kind, scale):
    """12 noiseless correspondences; every matrix entry within 1e-9."""
    from biahub_amd.registration.beads import transform_from_matches

    src = _twelve()
    az, ay = np.radians(25.0), np.radians(-8.0)
    Rz = np.array([[1, 0, 0], [0, np.cos(az), -np.sin(az)], [0, np.sin(az), np.cos(az)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    M = np.eye(4)
    M[:3, :3] = scale * (Rz @ Ry)
    M[:3, 3] = [3.5, -12.25, 40.0]
    dst = src @ M[:3, :3].T + M[:3, 3]
    order = np.random.default_rng(0).permutation(12)
    matches = np.stack([np.arange(12), np.argsort(order)], axis=1)  # dst is handed over shuffled: the matches undo it
    fwd, inv = transform_from_matches(matches, src, dst[order], _settings(kind), ndim=3)
    assert np.abs(fwd.matrix - M).max() < 1e-9, np.abs(fwd.matrix - M).max()
    assert np.abs(inv.matrix - np.linalg.inv(M)).max() < 1e-9


def test_affine_fit_recovers_a_3d_affine():
    from biahub_amd.registration.beads import transform_from_matches

    src = _twelve(5)
    M = np.array([[1.02, 0.03, -0.01, 4.0], [0.05, 0.97, 0.08, -7.5], [-0.02, 0.11, 1.1, 21.0], [0, 0, 0, 1.0]])
    dst = src @ M[:3, :3].T + M[:3, 3]
    matches = np.stack([np.arange(12), np.arange(12)], axis=1)
    fwd, inv = transform_from_matches(matches, src, dst, _settings("affine"), ndim=3)
    assert np.abs(fwd.matrix - M).max() < 1e-9, np.abs(fwd.matrix - M).max()
    assert np.abs(inv.matrix - np.linalg.inv(M)).max() < 1e-9
    with pytest.raises(ValueError, match="2D or 3D"):
        transform_from_matches(matches, src, dst, _settings("affine"), ndim=4)


def test_overlap_score_counts():
    from biahub_amd.registration.beads import overlap_score

    ref = np.array([[10, 10, 10], [10, 50, 50], [30, 90, 20], [5, 5, 90]], dtype=float)
    mov = np.array([[10, 10, 13], [10, 50, 57], [30, 90, 20], [31, 90, 20], [0, 0, 0]], dtype=float)
    # radius 6: ref 0 (3 away) and ref 2 (two movers, counted once) are covered, ref 1 (7 away) and ref 3 are not -> 2 / min(5, 4)
    assert overlap_score(mov, ref, radius=6) == 2 / 4
    assert overlap_score(mov, ref, radius=7) == 3 / 4     # the ball is closed: 7 away counts at radius 7
    assert overlap_score(mov[:1], ref, radius=6) == 1.0   # normalised by the smaller set
    assert np.isnan(overlap_score(np.zeros((0, 3)), ref))


def test_settings_defaults_equal_the_reference():
    """biahub/settings.py of the reference: DetectPeaksSettings :26-30, EdgeGraphSettings :130-148, CostMatrixSettings :151-160,
    HungarianMatchSettings :163-169, MatchDescriptorSettings :172-175, FilterMatchesSettings :178-182,
    QCBeadsRegistrationSettings :185-188, BeadsMatchSettings :191-202, AffineTransformSettings :240-245, and the validators that
    fill ``beads_match_settings`` in :284-292 and :312-315."""
    from biahub_amd import settings as S

    d = S.DetectPeaksSettings()
    assert (d.threshold_abs, d.nms_distance, d.min_distance, d.block_size) == (110, 16, 0, [8, 8, 8])
    e = S.EdgeGraphSettings()
    assert (e.method, e.k, e.radius) == ("knn", 5, None)
    e = S.EdgeGraphSettings(method="radius", k=7)
    assert (e.k, e.radius) == (None, 30.0)
    e = S.EdgeGraphSettings(method="full", k=7, radius=2.0)
    assert (e.k, e.radius) == (None, None)
    assert S.EdgeGraphSettings(k=9).k == 9
    c = S.CostMatrixSettings()
    assert c.weights == {"dist": 0.5, "edge_angle": 1.0, "edge_length": 1.0, "pca_dir": 0.0, "pca_aniso": 0.0, "edge_descriptor": 0.0}
    assert c.normalize is False
    h = S.HungarianMatchSettings()
    assert (h.distance_metric, h.cost_threshold, h.max_ratio, h.cross_check) == ("euclidean", 0.10, 0.8, False)
    assert h.edge_graph_settings == S.EdgeGraphSettings() and h.cost_matrix_settings == c
    m = S.MatchDescriptorSettings()
    assert (m.distance_metric, m.max_ratio, m.cross_check) == ("euclidean", 0.8, False)
    f = S.FilterMatchesSettings()
    assert (f.angle_threshold, f.direction_threshold, f.min_distance_quantile, f.max_distance_quantile) == (0, 0, 0.01, 0.95)
    q = S.QCBeadsRegistrationSettings()
    assert (q.iterations, q.score_threshold, q.score_centroid_mask_radius) == (2, 0.40, 6)
    b = S.BeadsMatchSettings()
    assert b.algorithm == "hungarian" and b.source_peaks_settings == d and b.target_peaks_settings == d
    assert (b.match_descriptor_settings, b.hungarian_match_settings, b.filter_matches_settings, b.qc_settings) == (m, h, f, q)
    a = S.AffineTransformSettings()
    assert (a.t_reference, a.transform_type, a.use_prev_t_transform, a.compute_approx_transform) == ("first", "euclidean", True, False)
    assert a.approx_transform == np.eye(4).tolist()
    with pytest.raises(ValueError):
        S.BeadsMatchSettings(algorithm="icp")
    with pytest.raises(ValueError):
        S.QCBeadsRegistrationSettings(iteration=3)  # unknown keys are rejected
    reg = S.EstimateRegistrationSettings(target_channel_name="a", source_channel_name="b", estimation_method="beads")
    assert reg.beads_match_settings == b
    assert S.EstimateRegistrationSettings(target_channel_name="a", source_channel_name="b", estimation_method="ants").beads_match_settings is None
    stab = S.EstimateStabilizationSettings(stabilization_estimation_channel="a", stabilization_channels=["a"], stabilization_type="xyz",
                                           stabilization_method="beads", beads_match_settings={"qc_settings": {"iterations": 1}})
    assert stab.beads_match_settings.qc_settings.iterations == 1 and stab.beads_match_settings.hungarian_match_settings == h


def test_approx_transform_and_loading(tmp_path):
    from biahub_amd.registration.utils import get_aprox_transform, load_transforms

    t = get_aprox_transform((10, 40, 60), (10, 60, 40), ref_voxel_size=(0.2, 0.1, 0.1), mov_voxel_size=(0.2, 0.1, 0.1))
    # equal voxel sizes: a quarter turn about z taking the moving centre (20, 30) to the reference centre (30, 20), inverted
    assert np.allclose(t.matrix @ np.array([5, 30, 20, 1.0]), [5, 20, 30, 1.0])
    assert np.allclose(t.matrix[:3, :3] @ t.matrix[:3, :3].T, np.eye(3))
    z2 = get_aprox_transform((10, 40, 40), (10, 40, 40), ref_voxel_size=(0.4, 0.1, 0.1), mov_voxel_size=(0.2, 0.1, 0.1))
    assert np.isclose(abs(np.linalg.det(z2.matrix[:3, :3])), 2.0)
    np.save(tmp_path / "0.npy", np.eye(4))
    np.save(tmp_path / "2.npy", 2 * np.eye(4))
    assert load_transforms(tmp_path, 3) == [np.eye(4).tolist(), None, (2 * np.eye(4)).tolist()]


def test_cli_no_longer_refuses_beads(tmp_path):
    """``detect_peaks`` has no host path, so without a GPU the commands cannot finish here: they must get past their method checks
    (the settings parse, ``xyz_transforms`` is made, which ``estimate_tczyx`` does before it touches a device) and then fail for
    another reason than the method: no GPU, or, on a GPU, the all-zero store in which no transform can be estimated."""
    from biahub_amd import io
    from biahub_amd.cli import cli

    io.create_empty_plate(tmp_path / "in.zarr", [("A", "1", "0")], ["ch0"], (2, 1, 4, 32, 40), scale=(1, 1, 0.2, 0.1, 0.1))
    pos = str(tmp_path / "in.zarr/A/1/0")
    cfg = tmp_path / "reg.yml"
    cfg.write_text("target_channel_name: ch0\nsource_channel_name: ch0\nestimation_method: beads\n"
                   "beads_match_settings:\n  qc_settings:\n    iterations: 1\n")
    res = CliRunner().invoke(cli, ["estimate-registration", "-s", pos, "-t", pos, "-o", str(tmp_path / "reg" / "out.yml"), "-c", str(cfg)])
    assert "is not available in biahub_amd (only" not in res.output
    assert (tmp_path / "reg" / "xyz_transforms").is_dir(), res.output
    assert res.exit_code != 0  # nothing to register in an empty store
    cfg.write_text("stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\nstabilization_type: xyz\n"
                   "stabilization_method: beads\n")
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", pos, "-o", str(tmp_path / "stab"), "-c", str(cfg)])
    assert "is not available in biahub_amd (only" not in res.output
    assert "Estimating xyz stabilization parameters with beads" in res.output and (tmp_path / "stab" / "xyz_transforms").is_dir()
    # what stays refused
    cfg.write_text("stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\nstabilization_type: xy\n"
                   "stabilization_method: beads\n")
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", pos, "-o", str(tmp_path / "stab2"), "-c", str(cfg)])
    assert res.exit_code != 0 and "not available" in res.output
    cfg.write_text("stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\nstabilization_type: xyz\n"
                   "stabilization_method: beads\neval_transform_settings:\n  validation_window_size: 3\n")
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", pos, "-o", str(tmp_path / "stab3"), "-c", str(cfg)])
    assert res.exit_code != 0 and "eval_transform_settings" in res.output
    cfg.write_text("stabilization_estimation_channel: ch0\nstabilization_channels: [ch0]\nstabilization_type: xyz\n"
                   "stabilization_method: beads\nbeads_match_settings:\n  algorithm: sift\n")
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", pos, "-o", str(tmp_path / "stab4"), "-c", str(cfg)])
    assert res.exit_code != 0
