#!/usr/bin/env python3
"""Mid-band power (bh_focus_band_power) of one (100, 800, 800) uint16 window, default optics, 0.1494-um pixel:
device ms per call (HIP events around the call, after warm-up; median of rounds in which the variants alternate), effective
GB/s of window bytes, and the same restatement in float32 with scipy.fft on 16 host threads.  Variants: the contiguous window
with the call's own chunking and with ``--max-batch`` caps, and the window read in place from a (100, 1024, 1024) volume.
Prints one JSON line; ``--out`` also writes it to a file.  BHCORE_LIB selects the library."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from biahub_amd.focus import midband_power_and_sum

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=[100, 800, 800])
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--max-batch", type=int, nargs="*", default=[0, 4, 8, 16, 32])
ap.add_argument("--host-threads", type=int, default=16)
ap.add_argument("--out", type=Path, default=None)
a = ap.parse_args()
Z, Y, X = a.shape
OPT = dict(NA_det=1.35, lambda_ill=0.5, pixel_size=0.1494)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(0)
host = rng.integers(100, 4000, (Z, Y, X)).astype(np.uint16)
win = torch.from_numpy(host).to(dev)
y0, x0 = 111, 113
host_vol = np.zeros((Z, Y + 224, X + 224), dtype=np.uint16)
host_vol[:, y0:y0 + Y, x0:x0 + X] = host
vol = torch.from_numpy(host_vol).to(dev)
del host_vol
view = vol[:, y0:y0 + Y, x0:x0 + X]

variants = {f"contiguous_max_batch_{b}": (win, b) for b in a.max_batch}
variants["in_place_max_batch_0"] = (view, 0)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
times = {k: [] for k in variants}
wall = {k: [] for k in variants}
ref, want_sum = None, float(host.sum(dtype=np.int64))
for r in range(a.rounds + 3):  # three warm-up rounds (plans, scratch, clocks)
    for k, (t, b) in variants.items():
        t0 = time.perf_counter()
        ev[0].record()
        power, total = midband_power_and_sum(t, max_batch=b, **OPT)
        ev[1].record()
        torch.cuda.synchronize()
        if ref is None:
            ref = power
        assert np.abs(power - ref).max() <= 1e-5 * ref.max() and total == want_sum
        if r >= 3:
            times[k].append(ev[0].elapsed_time(ev[1]))
            wall[k].append((time.perf_counter() - t0) * 1e3)
nbytes = host.nbytes
res = {"shape": a.shape, "dtype": "uint16", "rounds": a.rounds, "variants": {}}
for k in variants:
    ms = statistics.median(times[k])
    res["variants"][k] = {"device_ms": round(ms, 4), "min_ms": round(min(times[k]), 4), "wall_ms": round(statistics.median(wall[k]), 4),
                          "window_GBps": round(nbytes / ms / 1e6, 1)}

# the host: float32 / complex64 restatement with scipy.fft
import scipy.fft

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import focus_ref as R

mask = R.band_mask(Y, X, OPT["pixel_size"])
ht = []
for _ in range(3):
    t0 = time.perf_counter()
    spec = scipy.fft.fft2(host.astype(np.float32), axes=(-2, -1), workers=a.host_threads)
    p32 = np.abs(spec)[:, mask].sum(axis=1, dtype=np.float32)
    ht.append((time.perf_counter() - t0) * 1e3)
res["host_f32_scipy"] = {"threads": a.host_threads, "ms": round(min(ht), 2), "runs_ms": [round(v, 2) for v in ht]}
res["device_vs_host_f32_max_rel"] = float(np.abs(ref - p32.astype(np.float64)).max() / ref.max())
line = json.dumps(res)
print(line, flush=True)
if a.out:
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")
