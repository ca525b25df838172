#!/usr/bin/env python3
"""StackReg translation (bh_stackreg_translation) of 64 frames of 800 x 800 uint16 against frame 0: device ms
per call (HIP events around the call, which includes pyramids, prefilter, the descent and the read-back; three warm-up calls,
median of the rest), the same with the stack read in place from a (64, 1024, 1024) array, and the numpy restatement
(tests/stackreg_ref.py) on one pair on the host.  The frames are crops of one smooth random image at integer offsets (a random
walk of about a pixel per frame) with Poisson noise, so the true shifts are known.  Prints one JSON line; ``--out`` also writes
it to a file.  BHCORE_LIB selects the library."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch
from scipy import ndimage

from biahub_amd.stackreg import register_translation_pairs

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=[64, 800, 800])
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--out", type=Path, default=None)
a = ap.parse_args()
T, H, W = a.shape
M = 50  # margin of the base image around the frames: the offsets stay inside it
rng = np.random.default_rng(0)
base = ndimage.gaussian_filter(rng.random((H + 2 * M, W + 2 * M)), 2.0)
base = 100 + 4000 * (base - base.min()) / (base.max() - base.min())
offs = np.round(np.cumsum(rng.normal(0, 1.0, (T, 2)), axis=0)).astype(int).clip(-M + 10, M - 10)
offs[0] = 0
host = np.stack([rng.poisson(base[M + oy:M + H + oy, M + ox:M + W + ox]) for oy, ox in offs]).astype(np.uint16)
dev = torch.device("cuda", 0)
win = torch.from_numpy(host).to(dev)
host_big = np.zeros((T, H + 224, W + 224), dtype=np.uint16)
host_big[:, 111:111 + H, 113:113 + W] = host
big = torch.from_numpy(host_big).to(dev)
del host_big
variants = {"contiguous": win, "in_place": big[:, 111:111 + H, 113:113 + W]}
pairs = [(t, 0) for t in range(1, T)]
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
times = {k: [] for k in variants}
wall = {k: [] for k in variants}
first_ms, ref = None, None
for r in range(a.rounds + 3):
    for k, t in variants.items():
        t0 = time.perf_counter()
        ev[0].record()
        out = register_translation_pairs(t, pairs, max_frames=T)
        ev[1].record()
        torch.cuda.synchronize()
        if ref is None:
            ref, first_ms = out, ev[0].elapsed_time(ev[1])
        assert all(np.array_equal(x, y) for x, y in zip(out, ref))  # the same bits, every call and both variants
        if r >= 3:
            times[k].append(ev[0].elapsed_time(ev[1]))
            wall[k].append((time.perf_counter() - t0) * 1e3)
shift, mse, status, iters = ref
res = {"shape": a.shape, "dtype": "uint16", "pairs": len(pairs), "rounds": a.rounds, "first_call_ms": round(first_ms, 3), "variants": {},
       "status_counts": np.bincount(status, minlength=3).tolist(), "iterations_mean": round(float(iters.mean()), 2),
       "iterations_max": int(iters.max()), "max_abs_error_px": float(np.abs(shift + offs[1:]).max())}
for k in variants:
    res["variants"][k] = {"device_ms": round(statistics.median(times[k]), 4), "min_ms": round(min(times[k]), 4),
                          "wall_ms": round(statistics.median(wall[k]), 4)}

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
import stackreg_ref as R

ht = []
for _ in range(3):
    t0 = time.perf_counter()
    h_shift, _, h_status, _ = R.register_pairs(host[:2], [(1, 0)])
    ht.append(time.perf_counter() - t0)
res["host_restatement_one_pair"] = {"s": round(min(ht), 3), "runs_s": [round(v, 3) for v in ht],
                                    "device_minus_host_px": float(np.abs(h_shift[0] - shift[0]).max())}
line = json.dumps(res)
print(line, flush=True)
if a.out:
    a.out.parent.mkdir(parents=True, exist_ok=True)
    a.out.write_text(line + "\n")
