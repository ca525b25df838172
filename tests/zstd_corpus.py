"""Inputs for the zstd frame tests: the data kinds and compression levels that together exercise every block, literals and
sequence mode of RFC 8878 that pyarrow's zstd writes (checked by ``tests/test_zstd_frames.py``'s header walker)."""
import numpy as np

LEVELS = (-5, 1, 3, 9, 19)
BLOCKS = (32768, 262144)


def data_kinds(nbytes: int = 262144, seed: int = 7) -> dict:
    """name -> uint8 array of ``nbytes``: camera-like uint16, float32 in 1/8-count steps, ramp, sparse and constant data."""
    rng = np.random.default_rng(seed)
    n16, n32 = nbytes // 2, nbytes // 4
    yy = np.arange(n16) % 512
    cam = (100 + 40 * np.sin(yy / 37.0) + rng.poisson(20, n16)).astype(np.uint16)
    f32 = (np.round(rng.normal(200, 30, n32) * 8) / 8).astype(np.float32)
    ramp = (np.arange(n16) // 3).astype(np.uint16)
    sparse = np.zeros(n16, np.uint16)
    idx = rng.choice(n16, n16 // 50, replace=False)
    sparse[idx] = rng.integers(1, 4000, idx.size)
    const = np.full(n16, 1234, np.uint16)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    alpha4 = rng.choice(acgt, nbytes)                                             # Huffman-4 and treeless literals
    tile4 = np.tile(rng.choice(acgt, 200), nbytes // 200 + 1)[:nbytes]            # Huffman-1 literals
    runs = np.repeat(rng.integers(0, 256, nbytes // 64).astype(np.uint8), 64)     # RLE and repeat sequence modes
    tail = np.concatenate([np.zeros(nbytes - nbytes // 4, np.uint8), rng.integers(0, 256, nbytes // 4).astype(np.uint8)])
    return {k: v.view(np.uint8).copy() for k, v in
            dict(camera=cam, float8=f32, ramp=ramp, sparse=sparse, constant=const, alpha4=alpha4, tile4=tile4, runs=runs,
                 zeros_tail=tail).items()}


def raw_frames():
    """(frame bytes, expected bytes) for every data kind x level x block size, one zstd frame per block."""
    from biahub_amd import codecs

    out = []
    for name, data in data_kinds().items():
        for level in LEVELS:
            for bs in BLOCKS:
                for o in range(0, data.size, bs):
                    blk = data[o:o + bs]
                    out.append((codecs.zstd_compress(blk, level), blk.tobytes()))
    return out


TYPESIZE = dict(camera=2, float8=4, ramp=2, sparse=2, constant=2, alpha4=1, tile4=1, runs=1, zeros_tail=1)
ENCODER_EDGE_SIZES = (1, 2, 3, 4, 12, 13, 127, 131071, 131072, 131073, 262143)  # 131073: a second zstd block of one byte
# frame header forms (content size in 1, 2 and 4 bytes: below 256, below 65792, above) and the 128-KiB zstd block edge
EDGE_LENGTHS = (1, 2, 3, 255, 256, 65791, 65792, 131071, 131072, 131073)


def encoder_inputs() -> dict:
    """name -> uint8 input of the host encoder's tests: every data kind at both block sizes, raw and as the store permutes it
    (bit-shuffled for typesize 2 and 4), camera prefixes of the edge sizes, and a block of noise in front of a block of zeros."""
    from biahub_amd import codecs

    out = {}
    for nbytes in BLOCKS:
        for kind, data in data_kinds(nbytes).items():
            out[f"{kind}/{nbytes}"] = data
            if TYPESIZE[kind] > 1:
                out[f"{kind}/{nbytes}/permuted"] = codecs.filter_host(data, 262144, TYPESIZE[kind], codecs.BLOSC_BITSHUFFLE)
    cam = data_kinds()["camera"]
    for n in ENCODER_EDGE_SIZES:
        out[f"camera[:{n}]"] = cam[:n]
    rng = np.random.default_rng(11)
    # a block of noise (Raw_Block) in front of a block of zeros (Compressed_Block): the frame shrinks, the first block cannot
    out["noise+zeros"] = np.concatenate([rng.integers(0, 256, 131072).astype(np.uint8), np.zeros(131072, np.uint8)])
    return out


def edge_inputs() -> dict:
    """name -> uint8 input at the lengths where the frame encoder takes another path (``EDGE_LENGTHS``), and 256 KiB + 3 bytes
    with one long run from byte 100000 to byte 200000: the match that covers it is cut at the 128-KiB block edge and its
    remainder carried into the next block."""
    cam = data_kinds(524288)["camera"]
    out = {f"edge/{n}": cam[:n] for n in EDGE_LENGTHS}
    carry = cam[:262144 + 3].copy()
    carry[100000:200000] = 0x5a
    out["edge/262147_run_over_block_edge"] = carry
    return out


def corrupt_cases():
    """(camera, cases): four good frames, and name -> (frame, expected bytes) of frames every decoder must refuse."""
    good = raw_frames()
    camera = [f for f in good if (b"\x28\xb5\x2f\xfd" == f[0][:4])][:4]
    frame, want = camera[1]
    # a one-block frame with 4-stream Huffman literals
    huf = next(fw for fw in good if len(fw[1]) == 32768 and ("literals", "huf4") in walk(fw[0]))
    did = 5 + (0 if (frame[4] >> 5) & 1 else 1)  # the dictionary ID field follows the window descriptor
    cases = {
        "truncated": (frame[: len(frame) // 2], want),
        "dictionary": (frame[:4] + bytes([frame[4] | 1]) + frame[5:did] + b"\x07" + frame[did:], want),
        "content_size": (frame, want + b"\0"),
        "offset": hand_frames()["offset_past_output"][0:1] + (bytes(7),),
    }
    # damaged Huffman tree description: the weights header byte of the first compressed block -> 255 weights of 15
    hb = bytearray(huf[0])
    fhd = hb[4]
    ip = 5 + (0 if (fhd >> 5) & 1 else 1) + ((1 if (fhd >> 5) & 1 else 0) if fhd >> 6 == 0 else 1 << (fhd >> 6))
    sf = (hb[ip + 3] >> 2) & 3
    q = ip + 3 + (3, 3, 4, 5)[sf]
    hb[q:q + 64] = b"\xff" * 64
    cases["huffman_header"] = (bytes(hb), huf[1])
    return camera, cases


def compressor_chunks(dtype: str) -> list:
    """Four chunks of 190000 elements for the device writers: camera-like, noise, zeros, runs and ramps."""
    rng = np.random.default_rng(12)
    ts = np.dtype(dtype).itemsize
    n_el = 190_000  # per chunk: 190 / 380 / 760 KB -> one to three 256-KiB blocks, the last one short
    x = np.arange(n_el)
    return [
        (300 + 200 * np.sin(x / 37.0) + rng.poisson(2, n_el)).astype(dtype),     # camera-like: compressible
        rng.integers(0, 256, n_el * ts, dtype=np.uint8).view(dtype),                # noise in every bit: incompressible
        np.zeros(n_el, dtype),                                                      # one long run
        np.where(x % 5000 < 4000, 1234, x % 251).astype(dtype),                     # runs and ramps
    ]


DEVICE_DIGEST_CASES = (("u2", 2), ("f4", 2), ("u2", 1), ("u1", 0))


def device_encoder_digests(gpu) -> dict:
    """name -> SHA-256 of the Blosc frames (each ``header.cbytes`` long, back to back, without the alignment gaps between them)
    that ``codecs.blosc_zstd_compress_device`` makes of the four ``compressor_chunks`` cases and of one chunk of two 256-KiB
    blocks and a third of 1000 bytes."""
    import hashlib

    import torch

    from biahub_amd import codecs

    def digest(filt, nframes, cbytes, bsz, ts, mode):
        packed, offs = codecs.blosc_zstd_compress_device(filt, nframes, cbytes, bsz, ts, mode)
        host = packed[: offs[-1]].cpu().numpy()
        h = hashlib.sha256()
        for i in range(nframes):
            n = int.from_bytes(host[offs[i] + 12: offs[i] + 16].tobytes(), "little")  # the header's cbytes
            assert offs[i] + n <= offs[i + 1]
            h.update(host[offs[i]: offs[i] + n].tobytes())
        return h.hexdigest()

    out = {}
    for dtype, mode in DEVICE_DIGEST_CASES:
        chunks = compressor_chunks(dtype)
        ts, cbytes = np.dtype(dtype).itemsize, chunks[0].nbytes
        bsz = codecs.default_blocksize(ts)
        src = torch.from_numpy(np.concatenate([c.view(np.uint8) for c in chunks])).to(gpu)
        filt = torch.empty_like(src)
        for i in range(len(chunks)):
            codecs.filter_device(src[i * cbytes:(i + 1) * cbytes], filt[i * cbytes:(i + 1) * cbytes], bsz, ts, mode)
        out[f"{dtype}/mode{mode}"] = digest(filt, len(chunks), cbytes, bsz, ts, mode)
    three = data_kinds(1 << 20)["camera"][: 2 * 262144 + 1000]  # the per-block stride and the short last block
    out["camera/2x256KiB+1000"] = digest(torch.from_numpy(three).to(gpu), 1, three.size, 262144, 1, 0)
    return out


def walk(frame: bytes) -> set:
    """The RFC 8878 features a zstd frame uses: ("block", raw|rle|compressed), ("literals", raw|rle|huf1|huf4|treeless) and
    ("seq", LL|OF|ML, predefined|rle|fse|repeat)."""
    b = bytes(frame)
    assert b[:4] == b"\x28\xb5\x2f\xfd"
    fhd = b[4]
    single, did, fcs = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    ip = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0) if fcs == 0 else 1 << fcs)
    out = set()
    while True:
        bh = int.from_bytes(b[ip:ip + 3], "little")
        ip += 3
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        out.add(("block", ("raw", "rle", "compressed")[btype]))
        if btype == 2:
            blk = b[ip:ip + size]
            lt, sf = blk[0] & 3, (blk[0] >> 2) & 3
            if lt <= 1:
                out.add(("literals", ("raw", "rle")[lt]))
                hb = (1, 2, 1, 3)[sf]
                regen = blk[0] >> 3 if hb == 1 else int.from_bytes(blk[:hb], "little") >> 4
                q = hb + (regen if lt == 0 else 1)
            else:
                hb = (3, 3, 4, 5)[sf]
                bits = (10, 10, 14, 18)[sf]
                csz = (int.from_bytes(blk[:hb], "little") >> (4 + bits)) & ((1 << bits) - 1)
                out.add(("literals", "treeless" if lt == 3 else ("huf1" if sf == 0 else "huf4")))
                q = hb + csz
            nseq = blk[q]
            q += 1 if nseq < 128 else (2 if nseq < 255 else 3)
            if nseq:
                m = blk[q]
                for name, sh in (("LL", 6), ("OF", 4), ("ML", 2)):
                    out.add(("seq", name, ("predefined", "rle", "fse", "repeat")[(m >> sh) & 3]))
        ip += 1 if btype == 1 else size
        if last:
            return out


def _frame(blocks, content_size: int) -> bytes:
    """A single-segment zstd frame (4-byte content size) of (type, size, payload) blocks."""
    out = bytearray(b"\x28\xb5\x2f\xfd" + bytes([0xa0]) + content_size.to_bytes(4, "little"))
    for i, (btype, size, payload) in enumerate(blocks):
        out += ((size << 3) | (btype << 1) | (i == len(blocks) - 1)).to_bytes(3, "little") + payload
    return bytes(out)


def _seq_block(ofcode: int) -> bytes:
    """Compressed block: raw literals b"abcd", one sequence (LL 4, ML 3) with RLE tables and offset code ``ofcode``."""
    bits = bytes([1 << ofcode])  # ofcode zero extra bits, then the end marker
    return bytes([4 << 3]) + b"abcd" + bytes([1, 0x54, 4, ofcode, 0]) + bits


def hand_frames():
    """name -> (frame, expected bytes or None when corrupt) for the cases the writers do not produce."""
    # compressed block, RLE literals (2-byte header: 300 x 0x5a), zero sequences
    blk = bytes([(300 << 4 & 0xf0) | (1 << 2) | 1, 300 >> 4, 0x5a, 0])
    seq = _seq_block(1)  # offset code 1 + LL != 0: repeat offset 2 = 4 -> "abcdabc"
    mixed = [(0, 5, b"hello"), (1, 7, b"z"), (2, len(blk), blk), (2, len(seq), seq)]
    return {
        "rle_literals": (_frame([(2, len(blk), blk)], 300), b"\x5a" * 300),
        "mixed_blocks": (_frame(mixed, 5 + 7 + 300 + 7), b"hello" + b"z" * 7 + b"\x5a" * 300 + b"abcdabc"),
        "offset_past_output": (_frame([(2, len(_seq_block(5)), _seq_block(5))], 7), None),
    }
