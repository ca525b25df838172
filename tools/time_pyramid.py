#!/usr/bin/env python3
"""Pyramid timings on the GPU.

Kernel: every method at (512, 2048, 2048) in float32 and uint16 with 4 levels (one launch of depth 3), timed with HIP events on
the library's stream (torch's current stream, which the context binds), beside a torch.Tensor.copy_ of the same volume in the same
process.  Model bytes = s * V * (1 + 1/8 + 1/64 + 1/512) (read level 0 once, write levels 1-3); the copy moves 2 * s * V.
    python tools/time_pyramid.py [--reps 10] [--shape 512 2048 2048]

CLI: one 537-MB uint16 position shaped like tools/zstd_read_bench.py's, as Blosc-zstd and as Blosc-lz4, run through the
``pyramid`` verb's per-position job with BH_PIPE_TIMING=1 (stages: read, upload, kernel, encode, write; seconds per position).
    python tools/time_pyramid.py --cli [--reps 3]
"""
import argparse, json, os, sys, tempfile, time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=[512, 2048, 2048])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--levels", type=int, default=4)
ap.add_argument("--cli", action="store_true", help="time the per-position job on Blosc-zstd and Blosc-lz4 stores instead")
ap.add_argument("--methods", nargs="*", default=["stride", "mean", "min", "max", "median", "mode"])
ap.add_argument("--dtypes", nargs="*", default=["float32", "uint16"], help="also float16, uint32, int16")
args = ap.parse_args()
dev = torch.device("cuda", 0)


def event_ms(fn, reps):
    fn()  # warm-up (code object load, allocations)
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def kernel_bench():
    from biahub_amd.pyramid import downsample_pyramid, level_shapes

    res = {"shape": args.shape, "levels": args.levels, "rows": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for dname in args.dtypes:
        dt = getattr(torch, dname)
        if dt == torch.float32:
            vol = torch.rand(args.shape, generator=g, device=dev) * 1000
        elif dt == torch.float16:  # positive finite bit patterns, subnormals included
            vol = torch.randint(0, 0x7BFF, args.shape, generator=g, device=dev, dtype=torch.int16).view(dt)
        elif dt == torch.uint32:  # a few labels
            vol = torch.randint(0, 5, args.shape, generator=g, device=dev, dtype=torch.int32).view(dt)
        else:
            vol = torch.randint(0, 4096, args.shape, generator=g, device=dev, dtype=torch.int16).view(dt)
        s = vol.element_size()
        V = vol.numel()
        model = s * sum(int(np.prod(sh)) for sh in level_shapes(args.shape, args.levels))
        dst = torch.empty_like(vol)
        copy = event_ms(lambda: dst.copy_(vol), args.reps)
        del dst
        cm = float(np.median(copy))
        res["rows"].append({"dtype": dname, "what": "copy_", "ms_median": round(cm, 3), "ms": [round(x, 3) for x in copy],
                            "bytes": 2 * s * V, "TB_s": round(2 * s * V / cm / 1e9, 3)})
        for m in args.methods:
            ms = event_ms(lambda: downsample_pyramid(vol, args.levels, m), args.reps)
            mm = float(np.median(ms))
            res["rows"].append({"dtype": dname, "what": m, "ms_median": round(mm, 3), "ms": [round(x, 3) for x in ms],
                                "bytes": model, "TB_s": round(model / mm / 1e9, 3), "vs_copy": round(mm / cm, 3)})
            print(f"{dname:8s} {m:7s} {mm:7.3f} ms  {model / mm / 1e9:6.2f} TB/s  {mm / cm:5.3f} x copy ({cm:.3f} ms)", flush=True)
        del vol
        torch.cuda.empty_cache()
    print(json.dumps(res))


def cli_bench():
    from contextlib import redirect_stderr
    from io import StringIO

    from biahub_amd import io

    Z, Y, X = 256, 1024, 1024
    rng = np.random.default_rng(0)
    vol = (rng.poisson(6, (Z, Y, X)) + 110 + (60 * np.sin(np.arange(X) / 50.0)).astype(np.int64)).astype(np.uint16)
    out = {"volume": f"uint16 {(Z, Y, X)} = {vol.nbytes / 1e6:.0f} MB, chunks (1,1,32,{Y},{X}), bit shuffle, levels {args.levels}"}
    tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=tmpdir) as tmp:
        for cname in ("zstd", "lz4"):
            comp = {"id": "blosc", "cname": cname, "clevel": 1, "shuffle": 2, "blocksize": 32768}
            p = Path(tmp) / cname
            io.create_empty_position(p, ["a"], (1, 1, Z, Y, X), chunks=(1, 1, 32, Y, X), dtype=np.uint16, version="0.4",
                                     compressor=comp)
            io.open_ome_zarr(p).data.write_volume(0, 0, vol)
            lines = []
            os.environ["BH_PIPE_TIMING"] = "1"  # compute_pyramid prints its stage seconds on stderr
            for r in range(args.reps + 1):  # in-process, the first run warms up; the GPU context and code objects stay loaded
                buf = StringIO()
                t0 = time.perf_counter()
                with redirect_stderr(buf):
                    io.open_ome_zarr(p).compute_pyramid(args.levels, "mean")
                torch.cuda.synchronize(dev)
                wall = time.perf_counter() - t0
                if r:
                    lines.append({"wall_s": round(wall, 3), "stages_s": buf.getvalue().strip().split(": ", 1)[-1]})
            out[f"blosc_{cname}"] = lines
            ref = io.open_ome_zarr(p)
            assert ref["3"].shape == (1, 1, 32, 128, 128)
    print(json.dumps(out, indent=1))


if args.cli:
    cli_bench()
else:
    kernel_bench()
