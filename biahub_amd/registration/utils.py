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
