"""Helpers shared by the registration estimators — the on-path part of ``biahub/registration/utils.py``."""

from __future__ import annotations

from pathlib import Path

import click
import numpy as np

from ..core.transform import Transform
from ..register import get_3D_fliplr_matrix, get_3D_rescaling_matrix, get_3D_rotation_matrix


def get_aprox_transform(mov_shape, ref_shape, pre_affine_90degree_rotation: int = -1, pre_affine_fliplr: bool = False,
                        verbose: bool = False, ref_voxel_size=(0.174, 0.1494, 0.1494), mov_voxel_size=(0.174, 0.1494, 0.1494)) -> Transform:
    """Starting transform from geometry alone (registration/utils.py:48-90): the inverse of scaling (ratio of the voxel sizes,
    about the reference's YX centre) after rotation by quarter turns about z (moving centre to reference centre) after an
    optional left-right flip."""
    scale_z = mov_voxel_size[-3] / ref_voxel_size[-3]
    scale_yx = mov_voxel_size[-1] / ref_voxel_size[-1]
    click.echo(f"Z scaling factor: {scale_z:.3f}; XY scaling factor: {scale_yx:.3f}\n")
    mov_shape, ref_shape = tuple(mov_shape), tuple(ref_shape)
    scaling = get_3D_rescaling_matrix(ref_shape, (scale_z, scale_yx, scale_yx), ref_shape)
    rotation = get_3D_rotation_matrix(mov_shape, 90 * pre_affine_90degree_rotation, ref_shape)
    flip = get_3D_fliplr_matrix(mov_shape, ref_shape) if pre_affine_fliplr else np.eye(4)
    return Transform(matrix=np.linalg.inv(scaling @ rotation @ flip))


def validate_transforms(transforms, shape_zyx, window_size: int = 10, tolerance: float = 100.0, verbose: bool = False) -> list:
    """Replace by ``None`` every transform that deviates beyond ``tolerance`` from the mean of the last ``window_size`` accepted
    ones (registration/utils.py:93-156).  The first ``window_size`` non-``None`` transforms are accepted unchecked; after that
    an accepted one is appended, the oldest popped, and the mean taken again, in that order.  Works on a copy of the list."""
    transforms = list(transforms)
    valid_transforms = []
    reference_transform = None
    for i, transform in enumerate(transforms):
        if transform is None:
            if verbose:
                click.echo(f"Transform at timepoint {i} is None and will be interpolated")
            continue
        if len(valid_transforms) < window_size:
            valid_transforms.append(transform)
            reference_transform = np.mean(valid_transforms, axis=0)
            if verbose:
                click.echo(f"[Bootstrap] Accepting transform at timepoint {i} (no validation)")
        elif check_transforms_difference(transform, reference_transform, shape_zyx, tolerance, verbose):
            valid_transforms.append(transform)
            if len(valid_transforms) > window_size:
                valid_transforms.pop(0)
            reference_transform = np.mean(valid_transforms, axis=0)
            if verbose:
                click.echo(f"Transform at timepoint {i} is valid")
        else:
            transforms[i] = None
            if verbose:
                click.echo(f"Transform at timepoint {i} is invalid and will be interpolated")
    return transforms


def interpolate_transforms(transforms, window_size: int = 3, interpolation_type: str = "linear", verbose: bool = False) -> list:
    """Fill the ``None`` entries by ``scipy.interpolate.interp1d`` over time on the whole 4 x 4 (registration/utils.py:159-244).
    ``window_size > 0``: per missing index the originally valid entries of ``[idx - w, idx + w]`` (one filled earlier in this
    call does not count); with fewer than two of them, the closest originally valid transform, the earlier one on a tie.
    ``window_size == 0``: one fit over all valid entries, linear whatever ``interpolation_type`` says.  Works on a copy of the
    list."""
    from scipy.interpolate import interp1d

    transforms = list(transforms)
    n = len(transforms)
    valid_transform_indices = [i for i, t in enumerate(transforms) if t is not None]
    valid_transforms = [np.array(transforms[i]) for i in valid_transform_indices]
    if len(valid_transform_indices) < 2:
        raise ValueError("At least two valid transforms are required for interpolation.")
    missing_indices = [i for i in range(n) if transforms[i] is None]
    if not missing_indices:
        return transforms
    if verbose:
        click.echo(f"Interpolating missing transforms at timepoints: {missing_indices}")
    if window_size > 0:
        valid = set(valid_transform_indices)
        for idx in missing_indices:
            local_x = [j for j in range(max(0, idx - window_size), min(n, idx + window_size + 1)) if j in valid]
            if len(local_x) < 2:
                closest_valid_idx = valid_transform_indices[np.argmin(np.abs(np.asarray(valid_transform_indices) - idx))]
                transforms[idx] = transforms[closest_valid_idx]
                if verbose:
                    click.echo(f"Not enough interpolation neighbors were found for timepoint {idx} using closest valid "
                               f"transform at timepoint {closest_valid_idx}")
                continue
            local_y = [np.array(transforms[j]) for j in local_x]
            f = interp1d(local_x, local_y, axis=0, kind=interpolation_type, fill_value="extrapolate")
            transforms[idx] = f(idx).tolist()
            if verbose:
                click.echo(f"Interpolated timepoint {idx} using neighbors: {local_x}")
    else:
        f = interp1d(valid_transform_indices, valid_transforms, axis=0, kind="linear", fill_value="extrapolate")
        transforms = [f(i).tolist() if transforms[i] is None else transforms[i] for i in range(n)]
    return transforms


def check_transforms_difference(tform1, tform2, shape_zyx, threshold: float = 5.0, verbose: bool = False):
    """Whether two 4 x 4 transforms move a 10 x 10 x 10 grid over the volume apart by no more than ``threshold`` on average
    (registration/utils.py:247-296).  The figure is the mean Euclidean distance of the grid points under the two matrices; the
    reference calls it MSE, and its echo line is kept."""
    tform1 = np.array(tform1)
    tform2 = np.array(tform2)
    Z, Y, X = shape_zyx
    zz, yy, xx = np.meshgrid(np.linspace(0, Z - 1, 10), np.linspace(0, Y - 1, 10), np.linspace(0, X - 1, 10))
    grid_points = np.vstack([zz.ravel(), yy.ravel(), xx.ravel(), np.ones(zz.size)]).T
    points_tform1 = np.dot(tform1, grid_points.T).T
    points_tform2 = np.dot(tform2, grid_points.T).T
    mse = np.mean(np.linalg.norm(points_tform1[:, :3] - points_tform2[:, :3], axis=1))
    if verbose:
        click.echo(f"MSE of transformed points: {mse:.2f}; threshold: {threshold:.2f}")
    return mse <= threshold


def evaluate_transforms(transforms, shape_zyx, validation_window_size: int = 10, validation_tolerance: float = 100.0,
                        interpolation_window_size: int = 3, interpolation_type: str = "linear", verbose: bool = False) -> list:
    """``validate_transforms`` then ``interpolate_transforms`` (registration/utils.py:299-367): a transform that jumps away from
    the rolling mean of its predecessors is dropped, the dropped and the missing ones are filled by interpolation over time.
    A list shorter than either window raises ``Warning``, as the reference does."""
    if not isinstance(transforms, list):
        transforms = transforms.tolist()
    if len(transforms) < validation_window_size:
        raise Warning(f"Not enough transforms for validation and interpolation. Required: {validation_window_size}, "
                      f"Provided: {len(transforms)}")
    transforms = validate_transforms(transforms=transforms, window_size=validation_window_size, tolerance=validation_tolerance,
                                     shape_zyx=shape_zyx, verbose=verbose)
    if len(transforms) < interpolation_window_size:
        raise Warning(f"Not enough transforms for interpolation. Required: {interpolation_window_size}, "
                      f"Provided: {len(transforms)}")
    return interpolate_transforms(transforms=transforms, window_size=interpolation_window_size,
                                  interpolation_type=interpolation_type, verbose=verbose)


def plot_translations(transforms_zyx, output_filepath: Path) -> None:
    """The z, x and y translations over time, one panel each in that order, as a png (registration/utils.py:425-464)."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    transforms_zyx = np.asarray(transforms_zyx)
    output_filepath = Path(output_filepath)
    output_filepath.parent.mkdir(parents=True, exist_ok=True)
    fig = Figure(figsize=(10, 10))
    FigureCanvasAgg(fig)  # no display, no pyplot state
    axs = fig.subplots(3, 1)
    for ax, row, title in zip(axs, (0, 2, 1), ("Z-Translation", "X-Translation", "Y-Translation")):
        ax.plot(transforms_zyx[:, row, 3])
        ax.set_title(title)
    fig.savefig(output_filepath, dpi=300, bbox_inches="tight")


def load_transforms(transforms_path: Path, T: int, verbose: bool = False) -> list:
    """``<transforms_path>/<t>.npy`` for t < T as nested lists, ``None`` for a timepoint without a file (:638-655)."""
    transforms = []
    for t in range(T):
        path = Path(transforms_path) / f"{t}.npy"
        if not path.exists():
            transforms.append(None)
            if verbose:
                click.echo(f"Transform for timepoint {t} not found.")
            continue
        matrix = np.load(path)
        transforms.append(matrix.tolist())
        if verbose:
            click.echo(f"Transform for timepoint {t}: {matrix}")
    return transforms
