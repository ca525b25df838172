#!/usr/bin/env python3
"""Reading a Blosc-zstd store into HBM: host zstd (BH_ZSTD_DEVICE=0) against the device decoder (csrc/zstd.hip).
An iohub-style store — uint16 (256, 1024, 1024), chunks (1, 1, 32, 1024, 1024), Blosc zstd level 1, bit shuffle, 32-KiB
blocks as c-blosc picks them — is read with read_volume_device, the two settings alternating in one process.
    python tools/zstd_read_bench.py [--reps 5] [--device-only]"""
import argparse, json, os, sys, tempfile, time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np, torch
from biahub_amd import codecs, io

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=[256, 1024, 1024])
ap.add_argument("--zc", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device-only", action="store_true", help="only the device route (for a profiler run)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
Z, Y, X = args.shape
rng = np.random.default_rng(0)
vol = (rng.poisson(6, (Z, Y, X)) + 110 + (60 * np.sin(np.arange(X) / 50.0)).astype(np.int64)).astype(np.uint16)
dvol = torch.from_numpy(vol).to(dev)
out = {"volume": f"uint16 {tuple(args.shape)} = {vol.nbytes / 1e6:.0f} MB, chunks (1,1,{args.zc},{Y},{X}), blosc zstd-1 bitshuffle, "
                 "blocksize 32768"}


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
    return time.perf_counter() - t0, r


tmpdir = "/dev/shm" if os.path.isdir("/dev/shm") else None
with tempfile.TemporaryDirectory(dir=tmpdir) as tmp:
    comp = {"id": "blosc", "cname": "zstd", "clevel": 1, "shuffle": 2, "blocksize": 32768}
    p = Path(tmp) / "p"
    io.create_empty_position(p, ["a"], (1, 1, Z, Y, X), chunks=(1, 1, args.zc, Y, X), dtype=np.uint16, version="0.4", compressor=comp)
    arr = io.open_ome_zarr(p).data
    arr.write_volume(0, 0, vol)
    f = next(q for q in (p / "0").rglob("*") if q.is_file() and q.name != ".zarray" and not q.name.startswith("."))
    h = codecs.BloscHeader(f.read_bytes())
    out["stored_blocksize"] = h.blocksize
    out["frames"] = sum(len(codecs.blosc_stream_table(q.read_bytes(), codec="zstd")[2]) for q in (p / "0").rglob("*")
                        if q.is_file() and not q.name.startswith("."))
    modes = ("1",) if args.device_only else ("0", "1")
    times = {m: [] for m in modes}
    for m in modes:  # warm-up
        os.environ["BH_ZSTD_DEVICE"] = m
        assert torch.equal(arr.read_volume_device(0, 0, dev), dvol)
    for _ in range(args.reps):
        for m in modes:
            os.environ["BH_ZSTD_DEVICE"] = m
            t, r = timed(lambda: arr.read_volume_device(0, 0, dev))
            times[m].append(round(t, 4))
            del r
    for m in modes:
        out[f"read_volume_device_BH_ZSTD_DEVICE={m}_s"] = times[m]
        out[f"read_volume_device_BH_ZSTD_DEVICE={m}_median_s"] = float(np.median(times[m]))
print(json.dumps(out, indent=1))
