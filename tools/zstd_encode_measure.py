#!/usr/bin/env python3
"""The device zstd encoder (csrc/zstd_enc.hip) against the host route it can replace, on one GPU:

* ratio: device bytes over pyarrow's zstd level 1 for the same permuted 256-KiB blocks, per data kind of tests/zstd_corpus.py
  and for a camera-like uint16 volume written to a Blosc-zstd store both ways;
* time: the whole ``encode_volume_device(...)()`` call for that volume, BH_ZSTD_ENCODE_DEVICE=0 (libzstd on the I/O threads)
  against =1 (the GPU encoder), alternating in one process, after one warm-up call of each.

    python tools/zstd_encode_measure.py [--shape 512 1024 1024] [--pairs 5] [--out DIR]
writes zstd_encode_ratio.txt and zstd_encode_ab.txt into DIR (default: profiles/)."""
import argparse, os, statistics, sys, tempfile, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import numpy as np, torch
import zstd_corpus
from biahub_amd import codecs, io

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=[512, 1024, 1024])
ap.add_argument("--zc", type=int, default=32)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--out", default=str(ROOT / "profiles"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("no GPU: nothing is measured")
dev = torch.device("cuda", 0)
out = Path(args.out); out.mkdir(parents=True, exist_ok=True)
TS = dict(camera=2, float8=4, ramp=2, sparse=2, constant=2, alpha4=1, tile4=1, runs=1, zeros_tail=1)

# ---- ratio per data kind: one launch, frame k = kind k (one 256-KiB block, bit-shuffled for typesize 2 and 4)
kinds = zstd_corpus.data_kinds(262144)
perm = np.concatenate([codecs.filter_host(d, d.size, TS[k], 2) if TS[k] > 1 else d for k, d in kinds.items()])
packed, offs = codecs.blosc_zstd_compress_device(torch.from_numpy(perm).to(dev), len(kinds), 262144, 262144, 1, 0)
host = packed[: offs[-1]].cpu().numpy()
lines = ["# device zstd encoder (csrc/zstd_enc.hip) / pyarrow zstd level 1, same permuted bytes; MI355X",
         f"{'kind':12s} {'raw':>9s} {'device':>9s} {'zstd-1':>9s} {'lz4_raw':>9s} {'dev/zstd-1':>10s}"]
for i, (k, d) in enumerate(kinds.items()):
    p = perm[i * 262144:(i + 1) * 262144]
    _, _, csize, _, _ = codecs.blosc_stream_table(host[offs[i]: offs[i + 1]].tobytes(), codec="zstd")
    ref = len(codecs.zstd_compress(p, 1))
    lines.append(f"{k:12s} {p.size:9d} {int(csize[0]):9d} {ref:9d} {len(codecs.lz4_block_compress(p)):9d} {int(csize[0]) / ref:10.3f}")

# ---- the volume: camera-like uint16 (Poisson counts on an offset with a slow sine), made on the device
Z, Y, X = args.shape
g = torch.Generator(device=dev); g.manual_seed(0)
base = 110.0 + 60.0 * torch.sin(torch.arange(X, device=dev, dtype=torch.float32) / 50.0)
vol = torch.empty((Z, Y, X), dtype=torch.uint16, device=dev)
for z in range(Z):
    vol[z] = (torch.poisson(torch.full((Y, X), 6.0, device=dev), generator=g) + base).to(torch.uint16)
nbytes = vol.numel() * 2


def stored(p: Path, c: int) -> int:
    return sum(f.stat().st_size for f in (p / "0" / "0" / str(c)).rglob("*") if f.is_file())


with tempfile.TemporaryDirectory(dir="/dev/shm") as tmp:
    p = Path(tmp) / "p"
    io.create_empty_position(p, ["host", "device"], (1, 2, Z, Y, X), chunks=(1, 1, args.zc, Y, X), dtype=np.uint16, version="0.4",
                             compressor="blosc")
    arr = io.open_ome_zarr(p).data

    def call(route: int) -> float:
        os.environ["BH_ZSTD_ENCODE_DEVICE"] = str(route)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        arr.encode_volume_device(0, route, vol)()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    call(0); call(1)  # warm-up: code objects, scratch and pinned staging of both routes
    t = {0: [], 1: []}
    for _ in range(args.pairs):
        for route in (0, 1):
            t[route].append(call(route))
    b_host, b_dev = stored(p, 0), stored(p, 1)
    back = arr.read_volume_device(0, 1, dev)
    assert torch.equal(back, vol), "the device route's store does not read back"
    assert np.array_equal(arr.read_volume(0, 1)[:: max(1, Z // 4)], vol[:: max(1, Z // 4)].cpu().numpy())
lines.append(f"{'volume':12s} {nbytes:9d} {b_dev:9d} {b_host:9d} {'':>9s} {b_dev / b_host:10.3f}   # uint16 {Z}x{Y}x{X} camera-like, "
             f"chunks of {args.zc} planes, store bytes of each route")
(out / "zstd_encode_ratio.txt").write_text("\n".join(lines) + "\n")
ab = [f"# encode_volume_device(...)() of a uint16 {Z}x{Y}x{X} camera-like volume ({nbytes / 1e6:.0f} MB) into a Blosc-zstd store on /dev/shm,",
      f"# chunks of {args.zc} planes; {args.pairs} alternating pairs in one process after one warm-up call of each; seconds, wall clock",
      "# around the call and a device synchronise.  0: permute on the GPU, download raw, libzstd level 1 on the I/O threads.",
      "# 1: permute and zstd-encode on the GPU, download frames, I/O threads write.",
      "pair  route0_s  route1_s"]
ab += [f"{i:4d}  {a:8.3f}  {b:8.3f}" for i, (a, b) in enumerate(zip(t[0], t[1]))]
m0, m1 = statistics.median(t[0]), statistics.median(t[1])
ab.append(f"median {m0:7.3f}  {m1:8.3f}   spread (min..max) route0 {min(t[0]):.3f}..{max(t[0]):.3f}  route1 {min(t[1]):.3f}..{max(t[1]):.3f}")
ab.append(f"route1 / route0 = {m1 / m0:.3f}   ({nbytes / m0 / 1e9:.2f} GB/s -> {nbytes / m1 / 1e9:.2f} GB/s of volume bytes)")
ab.append(f"store bytes: route0 {b_host}  route1 {b_dev}  ({b_dev / b_host:.3f})")
(out / "zstd_encode_ab.txt").write_text("\n".join(ab) + "\n")
print("\n".join(lines)); print("\n".join(ab))
