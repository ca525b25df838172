#!/usr/bin/env python3
"""Stitch timings on the GPU.

Kernel: a 3 x 3 well of (64, 2048, 2048) FOVs with 10 % overlap (steps of 1843 voxels: a (64, 5734, 5734) mosaic), uint16 in and
float16 out, then float32 in and out, timed with HIP events on the library's stream (torch's current stream, which the context
binds) around each of >= 20 launches after a warm-up.  Model bytes = every FOV voxel read once + every mosaic voxel written once;
the share is of the 8 TB/s HBM3E peak of an MI355X.
    python tools/time_stitch.py [--reps 20] [--fov 64 2048 2048] [--grid 3 3] [--overlap 0.1] [--exponent 1.0]

CPU baseline: wall time of the float64 numpy restatement (tests/stitch_ref.py) on one (t, c) of the same well.  --cpu-z planes
per FOV are run (the blend has no coupling along z, so the time is linear in Z) and the figure scaled to the well's Z is printed
next to the measured one.
    python tools/time_stitch.py --cpu [--cpu-z 8]
"""
import argparse, json, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--fov", type=int, nargs=3, default=[64, 2048, 2048])
ap.add_argument("--grid", type=int, nargs=2, default=[3, 3])
ap.add_argument("--overlap", type=float, default=0.1)
ap.add_argument("--exponent", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--cpu", action="store_true", help="time the numpy restatement instead")
ap.add_argument("--cpu-z", type=int, default=8)
args = ap.parse_args()
HBM_PEAK = 8.0e12

Z, Y, X = args.fov
sy, sx = round(Y * (1 - args.overlap)), round(X * (1 - args.overlap))
shifts = [(0, i * sy, j * sx) for i in range(args.grid[0]) for j in range(args.grid[1])]


def kernel_bench():
    import torch

    from biahub_amd.stitch import get_output_shape, stitch_fovs

    dev = torch.device("cuda", 0)
    mosaic = get_output_shape(shifts, (Z, Y, X))
    res = {"fov": [Z, Y, X], "grid": args.grid, "overlap": args.overlap, "mosaic": list(mosaic), "exponent": args.exponent, "rows": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for in_name, out_dt in (("uint16", torch.float16), ("float32", torch.float32)):
        if in_name == "uint16":
            fovs = [torch.randint(0, 4096, (Z, Y, X), generator=g, device=dev, dtype=torch.int16).view(torch.uint16) for _ in shifts]
        else:
            fovs = [torch.rand((Z, Y, X), generator=g, device=dev) * 1000 for _ in shifts]
        model = len(fovs) * fovs[0].numel() * fovs[0].element_size() + int(np.prod(mosaic)) * torch.empty(0, dtype=out_dt).element_size()
        run = lambda: stitch_fovs(fovs, shifts, args.exponent, out_dt)  # noqa: E731
        run()  # warm-up (code object load, allocations, workspace)
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(max(20, args.reps)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = run()
            e.record()
            e.synchronize()
            ms.append(s.elapsed_time(e))
            del out
        mm = float(np.median(ms))
        out_name = str(out_dt).replace("torch.", "")
        res["rows"].append({"in": in_name, "out": out_name, "ms_median": round(mm, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                            "launches": len(ms), "bytes": model, "TB_s": round(model / mm / 1e9, 3), "hbm_share": round(model / mm / 1e-3 / HBM_PEAK, 3)})
        print(f"{in_name:8s} -> {out_name:8s} {mm:8.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} launches)  "
              f"{model / 1e9:6.3f} GB by the model  {model / mm / 1e9:6.3f} TB/s  {100 * model / mm / 1e-3 / HBM_PEAK:5.1f} % of HBM peak", flush=True)
        del fovs
        torch.cuda.empty_cache()
    print(json.dumps(res))


def cpu_bench():
    from stitch_ref import stitch_ref

    z = min(args.cpu_z, Z)
    rng = np.random.default_rng(0)
    fovs = [rng.integers(0, 4096, (z, Y, X)).astype(np.uint16) for _ in shifts]
    t0 = time.perf_counter()
    out = stitch_ref(fovs, shifts, args.exponent)
    wall = time.perf_counter() - t0
    print(f"numpy restatement, {len(fovs)} FOVs of ({z}, {Y}, {X}) uint16 -> {out.shape} float64: {wall:.2f} s measured; "
          f"scaled to Z = {Z} (linear in Z): {wall * Z / z:.1f} s per (t, c)", flush=True)
    print(json.dumps({"cpu_z": z, "wall_s": round(wall, 3), "scaled_to_Z": Z, "scaled_wall_s": round(wall * Z / z, 2)}))


if args.cpu:
    cpu_bench()
else:
    kernel_bench()
