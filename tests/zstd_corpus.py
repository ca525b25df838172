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
