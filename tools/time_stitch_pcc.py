#!/usr/bin/env python3
"""Time the pairwise registration of ``estimate-stitch --pcc-channel-name``: a 3 x 3 well of 2048 x 2048
uint16 planes at overlap 300, 12 edges.

    python tools/time_stitch_pcc.py [--reps 20] [--no-cpu]

GPU: one ``bh_stitch_edge_shifts`` call for the 12 edges, planes resident, HIP events around the call after a warm-up (plans
and workspace exist), ``--reps`` repetitions: min / median / max.  CPU: the float64 restatement (tests/stitch_pcc_ref.py
register_edge) over the same 12 edges on this machine's CPUs, once.  Prints one JSON line.  For the per-kernel split run it under
``rocprofv3 --kernel-trace --stats -- python tools/time_stitch_pcc.py --no-cpu`` (no counters in that run).
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

TILE, OVERLAP, GRID = (2048, 2048), 300, (3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import stitch_pcc_ref as R
    import torch

    from biahub_amd.estimate_stitch import edge_shifts, hilbert_edges

    rng = np.random.default_rng(3)
    errors = {(x, y): tuple(int(v) for v in rng.integers(-6, 7, 2)) for x in range(GRID[0]) for y in range(GRID[1]) if (x, y) != (0, 0)}
    tiles = R.well_tiles(17, GRID, TILE, OVERLAP, errors, "uint16")
    _, edges = hilbert_edges(list(tiles))
    want = []
    for a, b, rel in edges:
        nominal = (TILE[0] - OVERLAP, 0) if rel == R.BELOW else (0, TILE[1] - OVERLAP)
        ea, eb = errors.get(a, (0, 0)), errors.get(b, (0, 0))
        want.append([float(nominal[0] + eb[0] - ea[0]), float(nominal[1] + eb[1] - ea[1])])
    dev = torch.device("cuda", 0)
    planes = {c: torch.from_numpy(t).to(dev) for c, t in tiles.items()}
    ta, tb, rels = [planes[a] for a, _, _ in edges], [planes[b] for _, b, _ in edges], [r for _, _, r in edges]
    shifts, conf = edge_shifts(ta, tb, rels, overlap=OVERLAP)  # warm-up: plans, workspace
    ms, wall = [], []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        shifts, conf = edge_shifts(ta, tb, rels, overlap=OVERLAP)
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    out = {"workload": f"{GRID[0]}x{GRID[1]} well, {TILE[0]}x{TILE[1]} uint16, overlap {OVERLAP}, {len(edges)} edges", "reps": args.reps,
           "gpu_ms": {"min": min(ms), "median": statistics.median(ms), "max": max(ms)},
           "gpu_wall_ms": {"min": min(wall), "median": statistics.median(wall), "max": max(wall)},
           "shifts_equal_truth": shifts.tolist() == want, "confidence_min": float(conf.min())}
    if not args.no_cpu:
        t0 = time.perf_counter()
        ref = [R.register_edge(tiles[a], tiles[b], rel, OVERLAP) for a, b, rel in edges]
        out["cpu_restatement_s"] = time.perf_counter() - t0
        out["shifts_equal_restatement"] = shifts.tolist() == [[float(v) for v in r["shift"]] for r in ref]
        out["confidence_max_abs_diff"] = float(max(abs(c - r["confidence"]) for c, r in zip(conf, ref)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
