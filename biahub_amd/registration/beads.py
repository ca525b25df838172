"""Bead-based registration — mirror of ``biahub/registration/beads.py``.

Beads are detected in the moving volume (warped by the current transform) and in the reference volume, matched as two
graphs, a transform is fitted to the matched pairs and composed with the current one, and the result is scored by how many
reference beads then have a moving bead within a few voxels.  ``estimate`` repeats that a few times per timepoint;
``estimate_tczyx`` runs it for every timepoint and writes ``xyz_transforms/<t>.npy``.

Everything that touches a volume runs on the GPU: the warp is the ITK-rule linear resample of ``csrc/affine.hip`` (the
reference's ``transform.to_ants().apply_to_image``, which pulls with the matrix itself: ``out(p) = mov(M p)``, the call
``registration/ants.py`` makes for the same purpose), the detection is ``detect_peaks`` (``bh_block_peaks``), and both take
device tensors: a timepoint's two volumes are uploaded once per ``estimate`` call and the warped volume never leaves the
device.  The matching is ``core/graph_matching.py`` (``bh_edge_consistency_cost``).  Conventions as in the reference:
coordinates are ZYX, "mov" is the volume being aligned, "ref" the fixed one, transforms are 4 x 4 and three-dimensional
(``detect_peaks`` and the ITK-rule warp are 3-D only here).
"""

from __future__ import annotations

from itertools import product
from pathlib import Path
from typing import Literal

import click
import numpy as np
from scipy.spatial import cKDTree

from .. import _lib
from ..array_ops import _check_nan_n_zeros
from ..characterize_psf import detect_peaks
from ..core.graph_matching import Graph, GraphMatcher
from ..core.transform import Transform
from ..settings import AffineTransformSettings, BeadsMatchSettings, DetectPeaksSettings
from .utils import get_aprox_transform, load_transforms


def _device_volume(vol, device):
    """float32 device tensor of a (Z, Y, X) array or tensor (a tensor on the device already is passed through)."""
    import torch

    from ..device import as_device_volume

    if isinstance(vol, torch.Tensor):
        return as_device_volume(vol.to(torch.float32), device)[0]
    return as_device_volume(np.asarray(vol).astype(np.float32), device)[0]


def _warp(transform: Transform, mov_t, out_shape):
    """``transform.to_ants().apply_to_image(mov, reference=ref)`` on the device: linear, ITK boundary rule, result on the device."""
    from ..register import affine_device

    return affine_device(mov_t, transform.matrix, tuple(int(s) for s in out_shape), "linear", _lib.BOUNDARY_ITK, 0.0, device=mov_t.device)


def overlap_score(mov_peaks, ref_peaks, radius: int = 6, verbose: bool = False) -> float:
    """Fraction of bead overlap (beads.py:238-295): the number of reference peaks with at least one moving peak within
    ``radius`` voxels, divided by the size of the smaller set; NaN when either set is empty."""
    if len(mov_peaks) == 0 or len(ref_peaks) == 0:
        click.echo("No peaks found, returning nan metrics")
        return np.nan
    near = cKDTree(mov_peaks).query_ball_point(np.asarray(ref_peaks), r=radius)
    covered = sum(1 for hits in near if len(hits) > 0)
    score = covered / max(min(len(mov_peaks), len(ref_peaks)), 1)
    if verbose:
        click.echo(f"Mov peaks: {len(mov_peaks)}; ref peaks: {len(ref_peaks)}; overlap count: {covered}; overlap fraction: {score}")
    return score


def peaks_from_beads(mov, ref, mov_peaks_settings: DetectPeaksSettings, ref_peaks_settings: DetectPeaksSettings, verbose: bool = False,
                     mask_path: Path = None, device="cuda"):
    """(mov_peaks, ref_peaks), each (N, 3) ZYX, from ``detect_peaks`` with the two settings (beads.py:561-638); arrays or device
    tensors.  Fewer than two peaks on either side gives ``(None, None)`` (the reference returns a bare ``None``, which its
    callers cannot unpack; they test both halves for ``None``).  ``mask_path``: an OME-Zarr position whose (t, c) = (0, 0) volume
    marks voxels to avoid; a reference peak is kept when its (y, x) column is inside the mask's plane and clear in every z."""

    def detect(vol, s, what):
        if verbose:
            click.echo(f"Detecting beads in {what} dataset")
        return detect_peaks(vol, block_size=s.block_size, threshold_abs=s.threshold_abs, nms_distance=s.nms_distance,
                            min_distance=s.min_distance, device=device, verbose=verbose)

    mov_peaks = detect(mov, mov_peaks_settings, "moving")
    ref_peaks = detect(ref, ref_peaks_settings, "reference")
    if verbose:
        click.echo(f"Total of peaks in moving dataset: {len(mov_peaks)}")
        click.echo(f"Total of peaks in reference dataset: {len(ref_peaks)}")
    if len(mov_peaks) < 2 or len(ref_peaks) < 2:
        click.echo("Not enough beads detected")
        return None, None
    if mask_path is not None:
        from ..io import open_ome_zarr

        click.echo("Filtering peaks with mask")
        with open_ome_zarr(mask_path) as mask_ds:
            mask = np.asarray(mask_ds.data[0, 0])
        kept = []
        for peak in ref_peaks:
            _, y, x = peak.astype(int)
            if 0 <= y < mask.shape[1] and 0 <= x < mask.shape[2] and not mask[:, y, x].any():
                kept.append(peak)
        ref_peaks = np.array(kept)
    return mov_peaks, ref_peaks


def matches_from_beads(mov_peaks, ref_peaks, beads_match_settings: BeadsMatchSettings, verbose: bool = False, device="cuda"):
    """(K, 2) index pairs [mov, ref] (beads.py:641-728): k-nearest-neighbour graphs of both peak sets, the Hungarian matcher with
    the settings' weights, thresholds and cross check, then the geometric filters.  ``algorithm: match_descriptor`` is refused:
    it is ``skimage.feature.match_descriptors``, which this package does not have."""
    if verbose:
        click.echo(f"Getting matches from beads with settings: {beads_match_settings}")
    if beads_match_settings.algorithm == "match_descriptor":
        raise NotImplementedError("beads_match_settings.algorithm 'match_descriptor' needs skimage.feature.match_descriptors, which is "
                                  "not available in biahub_amd; use 'hungarian' (the default)")
    if beads_match_settings.algorithm != "hungarian":
        raise ValueError(f"Unknown matching algorithm: {beads_match_settings.algorithm}")
    hs = beads_match_settings.hungarian_match_settings
    mov_graph = Graph.from_nodes(mov_peaks, mode="knn", k=hs.edge_graph_settings.k)
    ref_graph = Graph.from_nodes(ref_peaks, mode="knn", k=hs.edge_graph_settings.k)
    matcher = GraphMatcher(algorithm="hungarian", weights=hs.cost_matrix_settings.weights, cost_threshold=hs.cost_threshold,
                           cross_check=hs.cross_check, max_ratio=hs.max_ratio, verbose=verbose, device=device)
    matches = matcher.match(mov_graph, ref_graph)
    fs = beads_match_settings.filter_matches_settings
    matches = matcher.filter_matches(matches, mov_graph, ref_graph, angle_threshold=fs.angle_threshold,
                                     min_distance_quantile=fs.min_distance_quantile, max_distance_quantile=fs.max_distance_quantile,
                                     direction_threshold=fs.direction_threshold)
    if verbose:
        click.echo(f"Total of matches: {len(matches)}")
    return matches


# ---- point-set fits (skimage.transform's estimators, stated here because skimage is absent) --------------------------
def fit_umeyama(src, dst, with_scale: bool) -> np.ndarray:
    """Least-squares rotation (+ isotropic scale) + translation taking ``src`` to ``dst`` (both (N, D)), in float64: Umeyama,
    "Least-squares estimation of transformation parameters between two point patterns", PAMI 13(4), 1991, eqs. 34-43, with
    his rule for a rank-deficient covariance.  Returns the (D + 1) x (D + 1) homogeneous matrix; NaN when the covariance
    vanishes."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    count, dim = src.shape
    mu_s, mu_d = src.mean(axis=0), dst.mean(axis=0)
    cs, cd = src - mu_s, dst - mu_d
    cov = cd.T @ cs / count
    sign = np.ones(dim)
    if np.linalg.det(cov) < 0:
        sign[-1] = -1
    U, S, Vt = np.linalg.svd(cov)
    rank = np.linalg.matrix_rank(cov)
    out = np.eye(dim + 1)
    if rank == 0:
        return out * np.nan
    if rank == dim - 1:  # eq. 43: the reflection is decided by the two orthogonal factors, not by the covariance
        if np.linalg.det(U) * np.linalg.det(Vt) > 0:
            R = U @ Vt
        else:
            flipped = sign.copy()
            flipped[-1] = -1
            R = U @ np.diag(flipped) @ Vt
    else:
        R = U @ np.diag(sign) @ Vt
    scale = (S @ sign) / cs.var(axis=0).sum() if with_scale else 1.0
    out[:dim, :dim] = scale * R
    out[:dim, dim] = mu_d - scale * (R @ mu_s)
    return out


def fit_affine(src, dst) -> np.ndarray:
    """Affine map taking ``src`` to ``dst`` by homogeneous total least squares, as skimage's ``AffineTransform.estimate``
    does it: both sets are centred and scaled to a root-mean-square distance of sqrt(D) from the origin, the D * (D + 1)
    coefficients and one common homogeneous weight are the right singular vector of the smallest singular value of the
    stacked system ``[src 1] row_i - dst_i w = 0``, and the normalisations are undone."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    count, dim = src.shape

    def normaliser(pts):
        centre = pts.mean(axis=0)
        rms = np.sqrt(((pts - centre) ** 2).sum() / count)
        if rms == 0:
            return np.full((dim + 1, dim + 1), np.nan), np.full_like(pts, np.nan)
        s = np.sqrt(dim) / rms
        N = np.eye(dim + 1)
        N[:dim, :dim] *= s
        N[:dim, dim] = -s * centre
        return N, (pts - centre) * s

    Ns, s = normaliser(src)
    Nd, d = normaliser(dst)
    if not (np.all(np.isfinite(Ns)) and np.all(np.isfinite(Nd))):
        return np.full((dim + 1, dim + 1), np.nan)
    A = np.zeros((count * dim, dim * (dim + 1) + 1))
    for i in range(dim):
        block = slice(i * count, (i + 1) * count)
        A[block, i * (dim + 1): i * (dim + 1) + dim] = s
        A[block, i * (dim + 1) + dim] = 1.0
        A[block, -1] = -d[:, i]
    _, _, Vt = np.linalg.svd(A)
    if np.isclose(Vt[-1, -1], 0):
        return np.full((dim + 1, dim + 1), np.nan)
    H = np.eye(dim + 1)
    H[:dim, :] = (Vt[-1, :-1] / Vt[-1, -1]).reshape(dim, dim + 1)
    H = np.linalg.inv(Nd) @ H @ Ns
    return H / H[-1, -1]


def transform_from_matches(matches, mov_peaks, ref_peaks, affine_transform_settings: AffineTransformSettings, ndim: int = 3,
                           verbose: bool = False) -> tuple[Transform, Transform]:
    """(forward, inverse) transforms fitted to the matched peaks (beads.py:731-786): forward takes the moving peaks to the
    reference peaks.  ``transform_type``: euclidean and similarity are Umeyama's closed form, affine the total-least-squares fit."""
    if verbose:
        click.echo(f"Estimating transform with settings: {affine_transform_settings}")
    if ndim not in (2, 3):
        raise ValueError(f"Peaks must be 2D or 3D, got {ndim}D")
    src, dst = np.asarray(mov_peaks)[matches[:, 0]], np.asarray(ref_peaks)[matches[:, 1]]
    kind = affine_transform_settings.transform_type
    if kind == "affine":
        forward = fit_affine(src, dst)
    elif kind in ("euclidean", "similarity"):
        forward = fit_umeyama(src, dst, with_scale=kind == "similarity")
    else:
        raise ValueError(f"Unknown transform type: {kind}")
    return Transform(matrix=forward), Transform(matrix=np.linalg.inv(forward))


def optimize_transform(transform: Transform, mov, ref, beads_match_settings: BeadsMatchSettings,
                       affine_transform_settings: AffineTransformSettings, verbose: bool = False, debug: bool = False,
                       device="cuda") -> tuple[Transform, float]:
    """One refinement (beads.py:874-995): score ``transform`` by the overlap of the beads of the warped moving volume with the
    reference's, match the two peak sets, fit a correction, compose, score again; the better of the two transforms and its
    score come back, ``(None, -1)`` when there are too few peaks or fewer than three matches."""
    mov_t, ref_t = _device_volume(mov, device), _device_volume(ref, device)
    radius = beads_match_settings.qc_settings.score_centroid_mask_radius
    source, target = beads_match_settings.source_peaks_settings, beads_match_settings.target_peaks_settings

    mov_peaks, ref_peaks = peaks_from_beads(_warp(transform, mov_t, ref_t.shape), ref_t, source, target, verbose=debug, device=device)
    if mov_peaks is None or ref_peaks is None:
        return None, -1
    score_before = overlap_score(mov_peaks, ref_peaks, radius=radius, verbose=debug)

    matches = matches_from_beads(mov_peaks, ref_peaks, beads_match_settings, verbose=debug, device=device)
    if len(matches) < 3:
        click.echo("Not enough matches found, returning the current transform")
        return None, -1
    forward, inverse = transform_from_matches(matches, mov_peaks, ref_peaks, affine_transform_settings, ndim=mov_t.ndim, verbose=debug)
    composed = transform @ inverse

    new_mov_peaks, new_ref_peaks = peaks_from_beads(_warp(composed, mov_t, ref_t.shape), ref_t, source, target, verbose=debug,
                                                    device=device)
    if new_mov_peaks is None or new_ref_peaks is None:  # the correction lost the beads: keep what we had
        return transform, score_before
    score_after = overlap_score(new_mov_peaks, new_ref_peaks, radius=radius, verbose=debug)
    if debug:
        click.echo(f"Bead matches: {matches}\nForward transform: {forward}\nInverse transform: {inverse}\nComposed transform: {composed}")
    if verbose:
        click.echo(f"Quality score before beads matching: {score_before}")
        click.echo(f"Quality score after beads matching: {score_after}")
    if score_after >= score_before:
        return composed, score_after
    return transform, score_before


def estimate(mov, ref, beads_match_settings: BeadsMatchSettings, affine_transform_settings: AffineTransformSettings,
             verbose: bool = False, output_filepath: Path = None, user_transform=None, debug: bool = False, device="cuda") -> Transform:
    """Best transform of one pair of volumes (beads.py:998-1117).  ``qc_settings.iterations`` refinements starting from
    ``approx_transform``, each from the last one's result; on the first, ``user_transform`` (a 4 x 4 matrix, for instance the
    previous timepoint's result) is refined as well and takes over when it scores higher.  A score of exactly 1 ends the loop,
    and so does a refinement that found nothing to work with.  The best-scoring result is returned (``approx_transform``
    itself when no refinement produced one) and saved to ``output_filepath``.  All-NaN or all-zero data: ``None``, nothing
    saved."""
    if _check_nan_n_zeros(np.asarray(mov)) or _check_nan_n_zeros(np.asarray(ref)):
        click.echo("Skipping: moving or reference data contains only NaN/zeros.")
        return None
    mov_t, ref_t = _device_volume(mov, device), _device_volume(ref, device)  # the only uploads of this call
    initial = Transform(matrix=np.asarray(affine_transform_settings.approx_transform))
    kw = dict(mov=mov_t, ref=ref_t, beads_match_settings=beads_match_settings, affine_transform_settings=affine_transform_settings,
              verbose=verbose, debug=debug, device=device)
    iterations = beads_match_settings.qc_settings.iterations
    results = {}
    current = initial
    it = 0
    while it < iterations:
        click.echo(f"Iteration {it + 1}/{iterations}: optimizing transform via bead matching...")
        found, score = optimize_transform(transform=current, **kw)
        results[it] = (found, score)
        if score == 1:
            break
        current = found
        if user_transform is not None and it == 0:
            click.echo("Optimizing user transform:")
            found_user, score_user = optimize_transform(transform=Transform(matrix=np.asarray(user_transform)), **kw)
            if score < score_user:
                results[it] = (found_user, score_user)
                if score_user == 1:
                    break
                current = found_user
        if current is None:
            break
        it += 1
    best, best_score = max(results.values(), key=lambda r: r[1]) if results else (None, -1)
    if best is None:
        best = initial
    if verbose:
        click.echo(f"Best transform: {best}")
        click.echo(f"Best quality score: {best_score}")
    if output_filepath:
        click.echo(f"Saving transform to {output_filepath}")
        np.save(output_filepath, best.to_list())
    return best


def _reference_index(t_idx: int, T: int, t_reference: str) -> int:
    """Stabilization: which timepoint of the same channel is the fixed volume of ``t_idx`` (beads.py:840-850).  ``first``: 0.
    ``previous``: the reference rolls the stack by -1 and resets its first entry, so timepoint t > 0 is registered to
    (t + 1) mod T; restated as it is."""
    if t_reference == "first" or t_idx == 0:
        return 0
    if t_reference == "previous":
        return (t_idx + 1) % T
    raise ValueError("Invalid reference. Please use 'first' or 'previous' as reference.")


def estimate_tzyx(t_idx: int, mov_tzyx, ref_tzyx, beads_match_settings: BeadsMatchSettings,
                  affine_transform_settings: AffineTransformSettings, verbose: bool = False, output_folder_path: Path = None,
                  mode: Literal["registration", "stabilization"] = "registration", user_transform=None, device="cuda") -> Transform:
    """One timepoint (beads.py:789-871): ``registration`` pairs ``mov_tzyx[t]`` with ``ref_tzyx[t]``; ``stabilization`` ignores
    ``ref_tzyx`` and pairs it with another timepoint of ``mov_tzyx`` (``t_reference``).  Saves ``<output_folder_path>/<t>.npy``."""
    click.echo("........................................................................")
    click.echo(f"Processing timepoint: {t_idx}")
    T = int(mov_tzyx.shape[0])
    if mode == "stabilization":
        if affine_transform_settings.t_reference not in ("first", "previous"):
            raise ValueError("Invalid reference. Please use 'first' or 'previous' as reference.")
        ref_zyx = mov_tzyx[_reference_index(t_idx, T, affine_transform_settings.t_reference)]
    elif mode == "registration":
        ref_zyx = ref_tzyx[t_idx]
    else:
        raise ValueError(f"Unknown mode: {mode}")
    mov_zyx = np.asarray(mov_tzyx[t_idx]).astype(np.float32)
    ref_zyx = np.asarray(ref_zyx).astype(np.float32)
    output_filepath = None
    if output_folder_path:
        output_folder_path = Path(output_folder_path)
        output_folder_path.mkdir(parents=True, exist_ok=True)
        output_filepath = output_folder_path / f"{t_idx}.npy"
    return estimate(mov=mov_zyx, ref=ref_zyx, beads_match_settings=beads_match_settings,
                    affine_transform_settings=affine_transform_settings, verbose=verbose, output_filepath=output_filepath,
                    user_transform=user_transform, device=device)


def estimate_with_propagation(mov_tzyx, ref_tzyx, beads_match_settings: BeadsMatchSettings,
                              affine_transform_settings: AffineTransformSettings, verbose: bool = False, output_folder_path: Path = None,
                              mode: Literal["registration", "stabilization"] = "registration", device="cuda") -> None:
    """Timepoints in order, each starting from the previous one's result (beads.py:405-464): after a timepoint the settings'
    ``approx_transform`` is replaced by its transform (or reset to the initial one when it gave none), and the initial
    transform competes on every first iteration.  Stabilization skips timepoint 0; a timepoint whose moving or reference
    stack sums to zero is skipped too."""
    initial = affine_transform_settings.approx_transform
    for t in range(int(mov_tzyx.shape[0])):
        if mode == "stabilization" and t == 0:
            continue
        if np.sum(mov_tzyx[t]) == 0 or np.sum(ref_tzyx[t]) == 0:
            click.echo(f"Timepoint {t} has no data, skipping")
            continue
        found = estimate_tzyx(t_idx=t, mov_tzyx=mov_tzyx, ref_tzyx=ref_tzyx, beads_match_settings=beads_match_settings,
                              affine_transform_settings=affine_transform_settings, verbose=verbose,
                              output_folder_path=output_folder_path, mode=mode, user_transform=initial, device=device)
        affine_transform_settings.approx_transform = found.to_list() if found is not None else initial


def estimate_independently(mov_tzyx, ref_tzyx, beads_match_settings: BeadsMatchSettings,
                           affine_transform_settings: AffineTransformSettings, verbose: bool = False, output_folder_path: Path = None,
                           cluster: str = "local", sbatch_filepath: Path = None,
                           mode: Literal["registration", "stabilization"] = "registration", device="cuda") -> None:
    """Every timepoint from the same ``approx_transform`` (beads.py:467-558).  The reference submits one job per timepoint;
    nothing is submitted here: the timepoints of this rank run in-process on its GPU (dealt round-robin over the ranks under
    ``torchrun``), ``cluster`` and ``sbatch_filepath`` are accepted and unused."""
    from .. import parallel

    rank, world = parallel.init()
    for t in range(rank, int(mov_tzyx.shape[0]), world):
        estimate_tzyx(t_idx=t, mov_tzyx=mov_tzyx, ref_tzyx=ref_tzyx, beads_match_settings=beads_match_settings,
                      affine_transform_settings=affine_transform_settings, verbose=verbose, output_folder_path=output_folder_path,
                      mode=mode, device=device)
    parallel.barrier()


def estimate_tczyx(mov_tczyx, ref_tczyx, mov_channel_index: int, ref_channel_index: int = None,
                   beads_match_settings: BeadsMatchSettings = None, affine_transform_settings: AffineTransformSettings = None,
                   verbose: bool = False, cluster: bool = False, sbatch_filepath: Path = None, output_folder_path: Path = None,
                   ref_voxel_size: tuple[float, float, float] = (0.174, 0.1494, 0.1494),
                   mov_voxel_size: tuple[float, float, float] = (0.174, 0.1494, 0.1494),
                   mode: Literal["registration", "stabilization"] = "registration", device="cuda") -> list:
    """One 4 x 4 matrix (nested list) per timepoint, ``None`` where a timepoint gave none (beads.py:298-402): optionally the
    approximate transform from the shapes and voxel sizes, then the timepoints with propagation (``use_prev_t_transform``) or
    independently; the transforms are written to ``<output_folder_path>/xyz_transforms/<t>.npy`` and read back from there."""
    from .. import parallel

    mov_tzyx = _ChannelView(mov_tczyx, mov_channel_index)
    if mode == "stabilization":
        ref_tzyx = mov_tzyx
    elif mode == "registration":
        ref_tzyx = _ChannelView(ref_tczyx, ref_channel_index)
    else:
        raise ValueError(f"Unknown mode: {mode}")
    if beads_match_settings is None:
        beads_match_settings = BeadsMatchSettings()
    if affine_transform_settings is None:
        affine_transform_settings = AffineTransformSettings()
    transforms_path = Path(output_folder_path) / "xyz_transforms"
    transforms_path.mkdir(parents=True, exist_ok=True)

    if affine_transform_settings.compute_approx_transform:
        approx = get_aprox_transform(mov_shape=mov_tzyx.shape[-3:], ref_shape=ref_tzyx.shape[-3:], pre_affine_90degree_rotation=-1,
                                     pre_affine_fliplr=False, verbose=verbose, ref_voxel_size=ref_voxel_size, mov_voxel_size=mov_voxel_size)
        click.echo(f"Computed approx transform: {approx}")
        affine_transform_settings.approx_transform = approx.to_list()

    if affine_transform_settings.use_prev_t_transform:
        rank, _ = parallel.init()
        if rank == 0:  # a chain: one rank walks it, the others wait for the files
            estimate_with_propagation(mov_tzyx, ref_tzyx, beads_match_settings, affine_transform_settings, verbose=verbose,
                                      output_folder_path=transforms_path, mode=mode, device=device)
        parallel.barrier()
    else:
        estimate_independently(mov_tzyx, ref_tzyx, beads_match_settings, affine_transform_settings, verbose=verbose,
                               output_folder_path=transforms_path, cluster=cluster, sbatch_filepath=sbatch_filepath, mode=mode,
                               device=device)
    return load_transforms(transforms_path, int(mov_tzyx.shape[0]), verbose)


class _ChannelView:
    """``tczyx[:, c]`` of anything indexable by (t, c) — an OME-Zarr array, a numpy array — read one timepoint at a time."""

    def __init__(self, tczyx, channel: int):
        self._data, self._c = tczyx, int(channel)
        s = tuple(int(n) for n in tczyx.shape)
        self.shape = (s[0],) + s[2:]

    def __getitem__(self, t):
        return np.asarray(self._data[int(t), self._c])


def optimize_matches(mov, ref, approx_transform: Transform, beads_match_settings: BeadsMatchSettings,
                     affine_transform_settings: AffineTransformSettings, param_grid: dict = None, verbose: bool = False,
                     device="cuda") -> BeadsMatchSettings:
    """Grid search over matching and filter parameters (beads.py:57-235).  The peaks of the approximately registered moving
    volume and of the reference are detected once; every combination of ``param_grid`` (keys: min_distance_quantile,
    max_distance_quantile, direction_threshold, cost_threshold, max_ratio, k, weights_<name>) is matched, fitted, composed with
    ``approx_transform``, warped and scored, and the settings with the highest overlap score come back (the given ones when no
    combination could be scored)."""
    if param_grid is None:
        param_grid = {"min_distance_quantile": [0, 0.01], "max_distance_quantile": [0, 0.99], "direction_threshold": [0, 50], "k": [5, 10]}
    radius = beads_match_settings.qc_settings.score_centroid_mask_radius
    source, target = beads_match_settings.source_peaks_settings, beads_match_settings.target_peaks_settings
    mov_t, ref_t = _device_volume(mov, device), _device_volume(ref, device)
    click.echo("Detecting peaks in approximately registered space for grid search...")
    mov_peaks, ref_peaks = peaks_from_beads(_warp(approx_transform, mov_t, ref_t.shape), ref_t, source, target, device=device)
    if mov_peaks is None or ref_peaks is None or len(mov_peaks) < 2 or len(ref_peaks) < 2:
        click.echo("Not enough peaks detected for optimization, returning original settings.")
        return beads_match_settings
    keys = list(param_grid)
    click.echo(f"Starting grid search: {len(mov_peaks)} mov peaks, {len(ref_peaks)} ref peaks, "
               f"{int(np.prod([len(param_grid[k]) for k in keys]))} parameter combinations.")

    def with_params(params):
        trial = beads_match_settings.model_copy(deep=True)
        fm, hm = trial.filter_matches_settings, trial.hungarian_match_settings
        for key, value in params.items():
            if key in ("min_distance_quantile", "max_distance_quantile", "direction_threshold"):
                setattr(fm, key, value)
            elif key in ("cost_threshold", "max_ratio"):
                setattr(hm, key, value)
            elif key == "k":
                hm.edge_graph_settings.k = value
            elif key.startswith("weights_") and key[len("weights_"):] in GraphMatcher.DEFAULT_WEIGHTS:
                hm.cost_matrix_settings.weights[key[len("weights_"):]] = value
        return trial

    best_score, best = -1.0, beads_match_settings
    for combo in product(*(param_grid[k] for k in keys)):
        params = dict(zip(keys, combo))
        trial = with_params(params)
        try:
            matches = matches_from_beads(mov_peaks, ref_peaks, trial, device=device)
            if len(matches) < 3:
                continue
            _, inverse = transform_from_matches(matches, mov_peaks, ref_peaks, affine_transform_settings, ndim=mov_peaks.shape[1])
            new_mov, new_ref = peaks_from_beads(_warp(approx_transform @ inverse, mov_t, ref_t.shape), ref_t, source, target, device=device)
            if new_mov is None or new_ref is None:
                continue
            score = overlap_score(new_mov, new_ref, radius=radius)
            if np.isnan(score):
                continue
            if verbose:
                click.echo(f"  {params} -> matches={len(matches)}, score={score:.4f}")
            if score > best_score:
                best_score, best = score, trial
        except Exception as e:  # a combination that cannot be evaluated is skipped, as in the reference
            if verbose:
                click.echo(f"  {params} -> failed: {e}")
    if verbose:
        click.echo(f"Best score: {best_score:.4f}")
        click.echo(f"Best settings: {best}")
    return best
