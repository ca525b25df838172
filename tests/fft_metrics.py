"""Error metrics of an FFT result against its float64 reference (``oracle/reference_f64.py``).

``conftest.rel_err`` is max|a - b| / max|b|: on camera-like data the beads set the maximum and the background, where almost
every voxel sits, can be wrong by a large fraction of a count without it noticing.  These metrics weigh every voxel:

    rms_rel   = ||got - ref||_2 / ||ref||_2
    voxel_rel = max |got - ref| / (|ref| + 0.01 rms(ref))     each voxel against its own magnitude (floored near zero)
    maxnorm   = max |got - ref| / max |ref|                   the old metric, for comparison

They run over slabs of whole planes (two passes: the floor needs rms(ref) first), so a volume of 2^31 voxels needs no
temporary of its size; ``got`` and ``ref`` may be numpy arrays or torch tensors on any device (planes are moved to ``ref``'s device).
"""

from __future__ import annotations

import math

import numpy as np
import torch

# Bounds of a float32 FFT result against float64: 10x the float32 oracle's own error on a bench-like volume (R-L, 10
# iterations, bench PSF); a ratio biased by 1e-4 on the dim voxels still fails them 20x (rms) and 8x (voxel)
# (tests/test_fft_reference.py).  The Tikhonov inverse filter rings through zero, where the per-voxel quotient measures the
# float32 rounding of the volume's scale: its voxel bound is 10x the oracle's own there (8.7e-5 at reg 1e-3).
RMS_TOL = 4e-6
VOXEL_TOL = 2e-5
TIK_VOXEL_TOL = 1e-3


SLAB_VOXELS = 1 << 24   # planes are taken in slabs of at most this many voxels (at least one plane)


def _slab(a, z0, z1, device):
    p = a[z0:z1] if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a[z0:z1]))
    return p.to(device=device, dtype=torch.float64)


def _scan(got, ref):
    if tuple(got.shape) != tuple(ref.shape):
        raise ValueError(f"shape {tuple(got.shape)} != reference shape {tuple(ref.shape)}")
    dev = ref.device if isinstance(ref, torch.Tensor) else torch.device("cpu")
    if len(ref.shape) < 3:
        got, ref = got[None], ref[None]
    Z = int(ref.shape[0])
    step = max(1, SLAB_VOXELS // max(1, math.prod(int(s) for s in ref.shape[1:])))
    ss_ref = ss_err = 0.0
    max_ref = max_err = 0.0
    for z0 in range(0, Z, step):
        r, g = _slab(ref, z0, z0 + step, dev), _slab(got, z0, z0 + step, dev)
        e = g - r
        ss_ref += float((r * r).sum())
        ss_err += float((e * e).sum())
        max_ref = max(max_ref, float(r.abs().max()))
        max_err = max(max_err, float(e.abs().max()))
    n = math.prod(int(s) for s in ref.shape)
    floor = max(0.01 * math.sqrt(ss_ref / n), 1e-300)
    worst = (-1.0, None, 0.0, 0.0)
    for z0 in range(0, Z, step):
        r, g = _slab(ref, z0, z0 + step, dev), _slab(got, z0, z0 + step, dev)
        q = (g - r).abs_().div_(r.abs().add_(floor))
        i = int(q.reshape(-1).nan_to_num(nan=math.inf).argmax())
        v = float(q.reshape(-1)[i])
        if not v <= worst[0]:   # NaN wins
            idx = tuple(int(k) for k in np.unravel_index(i, tuple(q.shape)))
            worst = (v, (z0 + idx[0],) + idx[1:], float(g.reshape(-1)[i]), float(r.reshape(-1)[i]))
    rms_rel = math.sqrt(ss_err) / max(math.sqrt(ss_ref), 1e-300)
    return rms_rel, worst[0], max_err / max(max_ref, 1e-300), worst[1:]


def fft_errors(got, ref64):
    """(rms_rel, voxel_rel, maxnorm) of ``got`` against the float64 reference ``ref64``."""
    rms_rel, voxel_rel, maxnorm, _ = _scan(got, ref64)
    return rms_rel, voxel_rel, maxnorm


def assert_fft_close(got, ref64, rms: float, voxel: float, what: str = ""):
    """Fail unless rms_rel <= rms and voxel_rel <= voxel (NaN fails); the message names the worst voxel.  Returns the errors."""
    rms_rel, voxel_rel, maxnorm, (idx, g, r) = _scan(got, ref64)
    ok = rms_rel <= rms and voxel_rel <= voxel
    assert ok, (f"{what}: rms_rel {rms_rel:.3e} (bound {rms:.1e}), voxel_rel {voxel_rel:.3e} (bound {voxel:.1e}), "
                f"maxnorm {maxnorm:.3e}; worst voxel {idx}: got {g!r}, float64 reference {r!r}")
    return rms_rel, voxel_rel, maxnorm
