#!/usr/bin/env python3
"""bh_volume_moments on resident (512, 2048, 2048) volumes against torch's float64 sum of the same tensors, interleaved in one
process: uint16 (4.3 GB), then float32 (8.6 GB) about 0 and about the mean.  HIP-event times (slot T_MOMENTS for the library,
torch events for torch), REPS rounds after one warm-up round; prints the median, the spread and the read rate of each.
torch has no sum for uint16: its row is the same bytes viewed as int16.  BHCORE_LIB selects the library (A/B against a variant)."""
import statistics
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from biahub_amd import _lib
from biahub_amd.device import get_context
from biahub_amd.estimate_bleaching import volume_moments
REPS = 7
dev = torch.device("cuda", 0)
ctx = get_context(dev); ctx.set_timing(True)
shape = (512, 2048, 2048)
g = torch.Generator(device=dev).manual_seed(3)
f32 = torch.empty(shape, device=dev).normal_(1000.0, 40.0, generator=g)
u16 = f32.clamp(0, 65535).to(torch.uint16)
mean = float(f32.sum(dtype=torch.float64)) / f32.numel()
def lib(t, centre):
    rec = volume_moments(t, dev, centre=centre); return ctx.elapsed_ms(_lib.T_MOMENTS), rec
def torch_sum(t):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(); s = t.sum(dtype=torch.float64); ev[1].record(); torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), float(s)
rows = {"moments uint16": [], "torch sum int16 view": [], "moments float32 centre 0": [], "moments float32 centre mean": [], "torch sum float32": []}
for rep in range(REPS + 1):
    r = [lib(u16, 0.0), torch_sum(u16.view(torch.int16)), lib(f32, 0.0), lib(f32, mean), torch_sum(f32)]
    if rep:  # round 0 warms every shape up
        for k, v in zip(rows, r):
            rows[k].append(v[0])
    if rep == 1:
        got16, got32 = int(r[0][1]["isum"].sum()), float(r[2][1]["fsum"].sum())
        print(f"sums agree: uint16 {got16} vs torch {r[1][1]:.0f}; float32 {got32!r} vs torch {r[4][1]!r}", flush=True)
for k, ms in rows.items():
    nbytes = (u16 if "16" in k else f32).numel() * (2 if "16" in k else 4)
    med = statistics.median(ms)
    print(f"{k:28s} median {med:7.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {REPS} rounds)  {nbytes / med / 1e9:.2f} TB/s read", flush=True)
