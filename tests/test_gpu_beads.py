"""GPU: bead registration end to end (``registration/beads.py``) on a synthetic bead slide, and the two CLI commands that use
it.

The fixture is a 48 x 160 x 160 volume of 40 Gaussian beads (sigma 1.5 voxels, 1000 counts on a background of 10) on a jittered
grid, and a second volume that is the first resampled through a known euclidean transform M (2 degrees about z, a shift of
(1.5, -3, 4) voxels): ``ref(p) = mov(M p)``, so the transform to find is M.  The acceptance radius is the reference's own:
``qc_settings.score_centroid_mask_radius`` (6 voxels).

Figures printed on an MI355X (``-s`` shows them):

    estimate: overlap score 0.575 at the identity, 1.000 at the estimate; bead centres land within 0.27 voxels (mean 0.20) of
        their partners; max |E - M| = 0.170 (a translation entry)
    estimate-stabilization: beads land within 0.27 (t = 1) and 0.13 (t = 2) voxels
"""

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

from biahub_amd import io
from biahub_amd.cli import cli

pytestmark = pytest.mark.gpu

SHAPE = (48, 160, 160)
PEAKS = {"threshold_abs": 100.0, "nms_distance": 8, "min_distance": 0, "block_size": [8, 8, 8]}


def _true_transform():
    t = np.radians(2.0)
    c, s = np.cos(t), np.sin(t)
    centre = (np.array(SHAPE) - 1) / 2
    M = np.eye(4)
    M[:3, :3] = [[1, 0, 0], [0, c, -s], [0, s, c]]
    M[:3, 3] = centre - M[:3, :3] @ centre + np.array([1.5, -3.0, 4.0])
    return M


def _bead_volume(seed=0):
    """40 of the 50 cells of a 2 x 5 x 5 grid (cells of 24 x 32 x 32) hold one bead, jittered by up to 4 voxels about the cell's
    centre: beads stay 16 voxels apart and 12 from every face."""
    rng = np.random.default_rng(seed)
    cells = [(z, y, x) for z in range(2) for y in range(5) for x in range(5)]
    chosen = rng.permutation(len(cells))[:40]
    centres = np.array([[12 + 24 * cells[i][0], 16 + 32 * cells[i][1], 16 + 32 * cells[i][2]] for i in chosen], dtype=np.float64)
    centres += rng.uniform(-4, 4, centres.shape)
    vol = np.full(SHAPE, 10.0, dtype=np.float32)
    r = 6
    for cz, cy, cx in centres:
        z0, y0, x0 = int(round(cz)), int(round(cy)), int(round(cx))
        zz, yy, xx = np.mgrid[z0 - r:z0 + r + 1, y0 - r:y0 + r + 1, x0 - r:x0 + r + 1]
        vol[z0 - r:z0 + r + 1, y0 - r:y0 + r + 1, x0 - r:x0 + r + 1] += (1000.0 * np.exp(
            -((zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 1.5 ** 2))).astype(np.float32)
    return vol, centres


@pytest.fixture(scope="module")
def slide(gpu):
    """(mov, ref, M, bead centres in mov); only read."""
    from biahub_amd.register import apply_affine_transform

    mov, centres = _bead_volume()
    M = _true_transform()
    ref = apply_affine_transform(mov, M, SHAPE)
    return mov, ref, M, centres


def _settings(iterations=2):
    from biahub_amd.settings import AffineTransformSettings, BeadsMatchSettings

    beads = BeadsMatchSettings(source_peaks_settings=PEAKS, target_peaks_settings=PEAKS, qc_settings={"iterations": iterations})
    return beads, AffineTransformSettings()


def _lands(E, where_fixed, where_moving):
    """Distances between E applied to the beads' places in the fixed volume and their places in the moving volume."""
    E = np.asarray(E, dtype=np.float64)
    return np.linalg.norm((E @ np.c_[where_fixed, np.ones(len(where_fixed))].T).T[:, :3] - where_moving, axis=1)


def _moved(M, centres):
    """Where beads at ``centres`` of a volume sit in the volume resampled through M (``out(p) = in(M p)``)."""
    return (np.linalg.inv(M) @ np.c_[centres, np.ones(len(centres))].T).T[:, :3]


RADIUS = 6  # qc_settings.score_centroid_mask_radius, the reference's acceptance radius


def _score(gpu, transform, mov, ref, beads):
    from biahub_amd.register import affine_device
    from biahub_amd.registration.beads import overlap_score, peaks_from_beads

    warped = affine_device(mov, transform, SHAPE, "linear", device=gpu)
    mp, rp = peaks_from_beads(warped, ref, beads.source_peaks_settings, beads.target_peaks_settings, device=gpu)
    return overlap_score(mp, rp, radius=beads.qc_settings.score_centroid_mask_radius)


def test_estimate_recovers_the_transform(gpu, slide, tmp_path):
    from biahub_amd.registration.beads import estimate

    mov, ref, M, centres = slide
    beads, affine = _settings()
    found = estimate(mov, ref, beads, affine, output_filepath=tmp_path / "0.npy", device=gpu)
    E = found.matrix
    before, after = _score(gpu, np.eye(4), mov, ref, beads), _score(gpu, E, mov, ref, beads)
    off = _lands(E, _moved(M, centres), centres)
    print(f"BEADS gpu estimate: overlap score {before:.3f} at the identity, {after:.3f} at the estimate; bead centres land "
          f"within {off.max():.2f} voxels (mean {off.mean():.2f}) of their partners; max |E - M| = {np.abs(E - M).max():.3f}")
    assert after >= before
    assert beads.qc_settings.score_centroid_mask_radius == RADIUS and off.max() <= RADIUS
    assert np.allclose(np.load(tmp_path / "0.npy"), E)


def test_empty_timepoints_are_skipped(gpu, slide, tmp_path):
    """T = 3 with an all-zero moving volume at t = 1: with propagation its sum is zero and it is passed over, independently
    ``estimate`` sees only zeros and returns nothing; either way no file is written for it and ``estimate_tczyx`` reports None."""
    from biahub_amd.registration.beads import estimate_tczyx

    mov, ref, M, centres = slide
    beads, affine = _settings(iterations=1)
    mov_t = np.stack([mov, np.zeros_like(mov), mov])[:, None]
    ref_t = np.stack([ref, ref, ref])[:, None]
    for name, propagate in (("chain", True), ("independent", False)):
        affine = affine.model_copy(update={"use_prev_t_transform": propagate, "approx_transform": np.eye(4).tolist()})
        out = estimate_tczyx(mov_t, ref_t, 0, 0, beads, affine, output_folder_path=tmp_path / name, device=gpu)
        assert len(out) == 3 and out[1] is None and not (tmp_path / name / "xyz_transforms" / "1.npy").exists()
        for t in (0, 2):
            assert _lands(out[t], _moved(M, centres), centres).max() <= RADIUS, (name, t)


def _write_config(path, text):
    peaks = "".join(f"    {k}: {v}\n" for k, v in PEAKS.items())
    path.write_text(text + "beads_match_settings:\n  source_peaks_settings:\n" + peaks + "  target_peaks_settings:\n" + peaks)


def test_cli_estimate_registration_with_beads_then_register(gpu, slide, tmp_path):
    mov, ref, M, centres = slide
    io.create_empty_plate(tmp_path / "in.zarr", [("A", "1", "0")], ["mov", "ref"], (1, 2) + SHAPE, scale=(1, 1, 0.2, 0.1, 0.1))
    data = io.open_ome_zarr(tmp_path / "in.zarr" / "A/1/0").data
    data[0, 0], data[0, 1] = mov, ref
    pos = str(tmp_path / "in.zarr/A/1/0")
    cfg = tmp_path / "est.yml"
    _write_config(cfg, "target_channel_name: ref\nsource_channel_name: mov\nestimation_method: beads\n")
    out_yml = tmp_path / "est" / "registration.yml"
    r = CliRunner()
    res = r.invoke(cli, ["estimate-registration", "-s", pos, "-t", pos, "-o", str(out_yml), "-c", str(cfg), "--local"])
    assert res.exit_code == 0, res.output
    est = yaml.safe_load(out_yml.read_text())
    assert est["source_channel_names"] == ["mov"] and est["target_channel_name"] == "ref"
    T = np.array(est["affine_transform_zyx"])
    assert _lands(T, _moved(M, centres), centres).max() <= RADIUS
    assert np.allclose(np.load(out_yml.parent / "xyz_transforms" / "0.npy"), T)
    est["keep_overhang"] = True
    out_yml.write_text(yaml.safe_dump(est))
    res = r.invoke(cli, ["register", "-s", pos, "-t", pos, "-c", str(out_yml), "-o", str(tmp_path / "reg.zarr"), "--local"])
    assert res.exit_code == 0, res.output
    got = np.asarray(io.open_ome_zarr(tmp_path / "reg.zarr" / "A/1/0").data[0, 0])
    inside = ref > 0  # where the resampled slide has data
    assert got.shape == SHAPE and np.corrcoef(got[inside], ref[inside])[0, 1] > 0.9


def test_cli_estimate_stabilization_with_beads(gpu, slide, tmp_path):
    """Three timepoints: the slide, the slide moved by M, the slide again.  ``xyz_stabilization_settings.yml`` holds three
    matrices: the identity for timepoint 0 (its own reference), one that takes the beads' places in the first volume to within the
    acceptance radius of their places in the moved one for timepoint 1 (``first(p) = moved(inv(M) p)``), and one that leaves them
    within it for timepoint 2."""
    mov, ref, M, centres = slide
    io.create_empty_plate(tmp_path / "in.zarr", [("A", "1", "0")], ["beads"], (3, 1) + SHAPE, scale=(1, 1, 0.2, 0.1, 0.1))
    data = io.open_ome_zarr(tmp_path / "in.zarr" / "A/1/0").data
    data[0, 0], data[1, 0], data[2, 0] = mov, ref, mov
    cfg = tmp_path / "stab.yml"
    _write_config(cfg, "stabilization_estimation_channel: beads\nstabilization_channels: [beads]\nstabilization_type: xyz\n"
                       "stabilization_method: beads\n")
    res = CliRunner().invoke(cli, ["estimate-stabilization", "-i", str(tmp_path / "in.zarr/A/1/0"), "-o", str(tmp_path / "out"), "-c",
                                   str(cfg), "--local"])
    assert res.exit_code == 0, res.output
    written = yaml.safe_load((tmp_path / "out" / "xyz_stabilization_settings.yml").read_text())
    assert written["stabilization_method"] == "beads" and written["stabilization_type"] == "xyz"
    mats = np.array(written["affine_transform_zyx_list"])
    assert mats.shape == (3, 4, 4) and np.array_equal(mats[0], np.eye(4))
    off1, off2 = _lands(mats[1], centres, _moved(M, centres)), _lands(mats[2], centres, centres)
    print(f"BEADS gpu estimate-stabilization: beads land within {off1.max():.2f} (t = 1) and {off2.max():.2f} (t = 2) voxels")
    assert off1.max() <= RADIUS and off2.max() <= RADIUS
