"""Every entry point whose kernels fold through csrc/reduce.hpp, on small seeded inputs: one line per output with the SHA-256 of
its bytes.  Run it once per library (BHCORE_LIB=/path/to/libbhcore.so selects one) and compare the outputs line for line: a
change of any fold's order shows up here as a changed digest (profiles/reduce_identity.txt).

Every input makes its kernels run at least two workgroups and a ragged last row or tail.

    python tools/reduce_identity.py [output file]
"""
import hashlib
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

LINES = []


def emit(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        h.update(np.ascontiguousarray(a).tobytes())
    LINES.append(f"{name} {h.hexdigest()}")
    print(LINES[-1], flush=True)


def beads(rng, shape, centres, sigma=(2.5, 1.8, 1.8)):
    g = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    v = np.full(shape, 110.0)
    for c in centres:
        v += 900.0 * np.exp(-0.5 * sum(((a - ci) / s) ** 2 for a, ci, s in zip(g, c, sigma)))
    return np.round(rng.poisson(v)).astype(np.float32)


def main():
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(20240607)
    from biahub_amd.estimate_bleaching import volume_moments

    f = (rng.standard_normal((5, 131, 301)) * 2.0 ** rng.uniform(-8, 8, (5, 131, 301))).astype(np.float32)
    f[1, 7, 5] = np.nan
    f[2, 9, :17] = 0.0
    for name, v in (("f32", f), ("u8", rng.integers(0, 256, f.shape).astype(np.uint8)), ("u16", rng.integers(0, 65536, f.shape).astype(np.uint16)),
                    ("i16", rng.integers(-32768, 32768, f.shape).astype(np.int16))):
        t = torch.from_numpy(v).to(dev)
        emit(f"bh_volume_moments {name}", volume_moments(t, dev, block_rows=16))
        emit(f"bh_volume_moments {name} view centre", volume_moments(t[:, 3:, 1:-2], dev, centre=1.5))

    from biahub_amd.focus import midband_power_and_sum

    stack = rng.integers(90, 4000, (7, 66, 130)).astype(np.uint16)
    power, total = midband_power_and_sum(stack, NA_det=1.35, lambda_ill=0.5, pixel_size=0.1494, device=dev, max_batch=3)
    emit("bh_focus_band_power uint16", power, np.float64(total))
    power, total = midband_power_and_sum(stack.astype(np.float32), NA_det=1.35, lambda_ill=0.5, pixel_size=0.1494, device=dev)
    emit("bh_focus_band_power float32", power, np.float64(total))

    from biahub_amd import estimate_stitch as S

    scene = rng.random((300, 420)).astype(np.float32)
    scene = (scene + np.roll(scene, 1, 0) + np.roll(scene, 1, 1)) * 1000 - 200  # negative values: the strip minimum is used
    tiles = [torch.from_numpy(np.ascontiguousarray(scene[y:y + 160, x:x + 200])).to(dev) for y, x in ((0, 0), (118, 3), (2, 158))]
    shifts, conf, prepared, corr = S.edge_shifts([tiles[0], tiles[0]], [tiles[1], tiles[2]], [S.BELOW, S.RIGHT], overlap=40, return_intermediates=True)
    emit("bh_stitch_edge_shifts", shifts, conf, *[t for p in prepared for t in p], *corr)

    from biahub_amd.deskew import fill_overhang

    vol = (rng.random((9, 37, 211)) * 50 + 1).astype(np.float32)
    vol[:, :, :30] = 0.0
    vol[:3, 20:, 150:] = 0.0
    emit("bh_overhang_fill mean", fill_overhang(torch.from_numpy(vol).to(dev), None, 3))
    emit("bh_overhang_fill mean cross", fill_overhang(torch.from_numpy(vol).to(dev), None, 2, connectivity=6))

    # the library reads its deskew switches on every call: the one-pass fill, then the mask pipeline behind either resampling kernel
    for label, env in (("one pass", {}), ("mask pipeline", {"BH_DESKEW_ONEPASS": "0"}), ("mask pipeline, tile kernel", {"BH_DESKEW_ONEPASS": "0", "BH_DESKEW_PERS": "0"})):
        os.environ.update(env)
        deskew(label)
        for k in env:
            del os.environ[k]

    from biahub_amd.deconvolve import transfer_function_device

    psf = np.exp(-0.5 * sum(((a - c) / s) ** 2 for a, c, s in zip(np.meshgrid(np.arange(9.), np.arange(11.), np.arange(13.), indexing="ij"), (4, 5, 6), (2, 1.5, 1.5))))
    emit("bh_transfer_function", transfer_function_device(torch.from_numpy(psf.astype(np.float32)).to(dev), (20, 36, 50), dev))

    from biahub_amd.estimate_stabilization import phase_cross_corr_device

    a = rng.random((12, 40, 50)).astype(np.float32)  # no power of two: the library transform, pcc_argmax_kernel finds the peak
    b = np.roll(a, (2, -3, 5), (0, 1, 2)) + 0.05 * rng.random(a.shape).astype(np.float32)
    for norm in (None, "magnitude"):
        shift, corr = phase_cross_corr_device(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), norm, dev, want_corr=True)
        emit(f"bh_phase_cross_corr {norm} shifted", shift, corr)
        shift, _ = phase_cross_corr_device(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), norm, dev, want_corr=False)
        emit(f"bh_phase_cross_corr {norm} peak", shift)

    from biahub_amd.registration import metric

    fixed = torch.from_numpy((rng.random((21, 45, 67)) * 900 + 50).astype(np.float32)).to(dev)
    moving = torch.from_numpy((fixed.cpu().numpy() * 0.8 + 60 * rng.random((21, 45, 67))).astype(np.float32)).to(dev)
    st = metric.image_stats(fixed)
    emit("bh_image_stats", np.float64([st["min"], st["max"], st["sum"]]), st["center_of_mass"])
    P = np.array([[1.01, 0.01, 0, 0.3], [0, 0.99, 0.02, -0.4], [0.01, 0, 1.0, 0.7]])
    val, grad, nv = metric.mattes_mi(fixed, moving, P, (50.0, 950.0, 40.0, 830.0), bins=32)
    emit("bh_mattes_mi value gradient", np.float64(val), grad, np.int64(nv))

    from biahub_amd.characterize_psf import fit_beads

    centres = [(7.3, 9.1, 8.6), (24.8, 8.2, 30.4), (8.9, 31.5, 29.7)]
    bv = torch.from_numpy(beads(rng, (34, 42, 42), centres)).to(dev)
    starts = [[int(c[0]) - 7, int(c[1]) - 8, int(c[2]) - 8] for c in centres]
    rows, guesses, status, iters = fit_beads(bv, starts, [[15, 17, 17]] * 3, (0.25, 0.1, 0.1), offset=100.0)
    emit("bh_psf_fit", rows, guesses, status, iters)

    from biahub_amd.apply_inverse_transfer_function import apply_inverse_transfer_function_zyx

    x = torch.from_numpy((rng.random((10, 30, 43)) * 100 + 10).astype(np.float32)).to(dev)
    H = torch.from_numpy((rng.random((14, 30, 43)) + 1j * rng.random((14, 30, 43))).astype(np.complex64)).to(dev)
    emit("bh_inverse_filter normalised", apply_inverse_transfer_function_zyx(x, H, 2, 1e-2, True))

    from biahub_amd.flat_field import flat_field_device

    stackf = rng.integers(100, 4000, (9, 50, 77)).astype(np.uint16)
    out, pattern = flat_field_device(torch.from_numpy(stackf).to(dev), dev, return_pattern=True)
    emit("bh_flat_field", out, pattern)

    from biahub_amd.estimate_crop import valid_mask_device

    m = (rng.random(70001) * 3).astype(np.float32)
    m[rng.random(m.size) < 0.3] = 0.0
    m[::997] = np.nan
    bits, count = valid_mask_device(torch.from_numpy(m).to(dev), dev)
    emit("bh_valid_mask", bits, np.int64(count))

    from biahub_amd.characterize_psf import block_peaks, recentre_beads
    from biahub_amd.estimate_psf import average_beads_device

    emit("bh_block_peaks", *block_peaks(bv, 3, (8, 9, 10)))
    margins = np.array([13.0, 15.0, 15.0])
    emit("bh_patch_peaks", recentre_beads(bv, np.round(centres) + 1, margins))
    emit("bh_average_patches", average_beads_device(bv, np.round(centres).astype(np.int64), margins)[0])

    from biahub_amd.process_data import _bin_reduce

    for mean in (False, True):
        out, lo, hi = _bin_reduce(torch.from_numpy(stackf).to(dev), _lib_code(stackf), (3, 5, 7), mean)
        emit(f"bh_bin_reduce mean {mean}", out, np.float32([lo, hi]))
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text("\n".join(LINES) + "\n")


def _lib_code(a):
    from biahub_amd.device import _NP_TO_DT

    return _NP_TO_DT[a.dtype]


def deskew(label):
    from biahub_amd.deskew import deskew_fill_path, fast_deskew_zyx

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    raw = rng.integers(100, 3000, (45, 70, 133)).astype(np.uint16)
    for name, v in (("uint16", raw), ("float32 with zeros", np.where(rng.random(raw.shape) < 0.001, 0, raw).astype(np.float32))):
        for avg in (1, 3):
            out = fast_deskew_zyx(torch.from_numpy(v).to(dev), 30.0, 0.35, True, avg, "mean")
            emit(f"bh_deskew mean fill {label} {name} average {avg} path {deskew_fill_path(dev)}", out)


if __name__ == "__main__":
    main()
