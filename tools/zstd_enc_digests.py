#!/usr/bin/env python3
"""Record the zstd encoder's pinned output digests (tests/golden/zstd_enc_host_digests.json, zstd_enc_device_digests.json).
The tests compare against them, so a refactor cannot change a byte unnoticed; a DELIBERATE change to what the encoder emits
re-records them from the commit that makes it.

    python tools/zstd_enc_digests.py host|device --commit REV [--out FILE]      (device: needs the GPU)"""
import argparse, hashlib, json, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import zstd_corpus
from biahub_amd import codecs

ap = argparse.ArgumentParser()
ap.add_argument("which", choices=("host", "device"))
ap.add_argument("--commit", required=True, help="the commit whose build records (git rev-parse --short HEAD)")
ap.add_argument("--out")
args = ap.parse_args()
if args.which == "host":
    inputs = {**zstd_corpus.encoder_inputs(), **zstd_corpus.edge_inputs()}
    digests = {k: hashlib.sha256(codecs.zstd_compress_host(d)).hexdigest() for k, d in inputs.items()}
    what = "SHA-256 of codecs.zstd_compress_host(x) for zstd_corpus.encoder_inputs() and edge_inputs()"
else:
    import torch
    digests = zstd_corpus.device_encoder_digests(torch.device("cuda", 0))
    what = "SHA-256 of the frames of codecs.blosc_zstd_compress_device, zstd_corpus.device_encoder_digests()"
doc = {"what": what, "recorded_from": args.commit,
       "note": "a deliberate change to what the encoder emits re-records this file: tools/zstd_enc_digests.py", "digests": digests}
out = Path(args.out) if args.out else ROOT / "tests" / "golden" / f"zstd_enc_{args.which}_digests.json"
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(json.dumps(doc, indent=1) + "\n")
print(out, len(digests))
