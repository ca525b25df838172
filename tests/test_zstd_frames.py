"""Blosc-zstd stream tables and the zstd frame corpus of the device decoder (csrc/zstd.hip) — host side, no GPU."""
import struct
from pathlib import Path

import numpy as np
import pytest

from biahub_amd import codecs

import zstd_corpus

GOLDEN = Path(__file__).parent / "golden"
MAGIC = b"\x28\xb5\x2f\xfd"


def _zstd_goldens():
    z = np.load(GOLDEN / "blosc_streams.npz")
    out = {}
    for k in sorted(z.files):
        if k.endswith("__blosc"):
            buf = z[k].tobytes()
            h = codecs.BloscHeader(buf)
            if h.codec == "zstd" and not h.memcpyed and h.nbytes > 0:
                out[k[: -len("__blosc")]] = buf
    return out


def test_zstd_stream_table_on_c_blosc_goldens():
    goldens = _zstd_goldens()
    assert len(goldens) >= 25
    stored = frames = 0
    for name, buf in goldens.items():
        h, soff, csize, doff, dlen = codecs.blosc_zstd_stream_table(buf)
        # the streams tile the chunk
        order = np.argsort(doff)
        assert int(doff[order[0]]) == 0, name
        assert np.array_equal(doff[order][1:], doff[order][:-1] + dlen[order][:-1].astype(np.uint64)), name
        assert int(doff[order[-1]]) + int(dlen[order[-1]]) == h.nbytes, name
        for so, cs, dl in zip(soff, csize, dlen):
            so, cs = int(so), int(cs)
            assert so + cs <= h.cbytes
            if cs == dl:
                stored += 1
            else:
                assert buf[so:so + 4] == MAGIC, name
                frames += 1
    assert stored == 3
    assert frames >= 40


def test_zstd_stream_table_rejects_corrupt_frames():
    buf = _zstd_goldens()["zstd1_u2_s2"]
    h, soff, csize, _, _ = codecs.blosc_zstd_stream_table(buf)
    with pytest.raises(ValueError):  # truncated: cbytes says more than there is
        codecs.blosc_zstd_stream_table(buf[: h.cbytes - 10])
    bad = bytearray(buf)
    struct.pack_into("<i", bad, 16, 8)  # bstart inside the header
    with pytest.raises(ValueError, match="corrupt blosc stream"):
        codecs.blosc_zstd_stream_table(bytes(bad))
    bad = bytearray(buf)
    struct.pack_into("<i", bad, int(soff[0]) - 4, h.cbytes)  # cb beyond the frame
    with pytest.raises(ValueError, match="corrupt blosc stream"):
        codecs.blosc_zstd_stream_table(bytes(bad))
    with pytest.raises(ValueError):  # another inner codec
        codecs.blosc_zstd_stream_table(codecs.blosc_compress(np.zeros(4096, np.uint8), 1, "lz4", 5))


def test_zstd_stream_table_always_split():
    """A frame written in always-split mode (no DONT_SPLIT flag): one stream per byte of the element."""
    raw = (np.arange(65536) % 251).astype(np.uint16).view(np.uint8)
    good = codecs.blosc_compress(raw, 2, "zstd", 1, codecs.BLOSC_SHUFFLE, 32768)
    h = codecs.BloscHeader(good)
    nb = -(-h.nbytes // h.blocksize)
    bstarts = struct.unpack_from(f"<{nb}i", good, 16)
    # rebuild it split: each block's two halves as separate zstd streams
    _, perm = codecs.blosc_decode_blocks(good)
    body, starts = bytearray(), []
    for b in range(nb):
        blk = perm[b * h.blocksize:(b + 1) * h.blocksize]
        starts.append(16 + 4 * nb + len(body))
        for j in range(2):
            s = codecs.zstd_compress(blk[j * blk.size // 2:(j + 1) * blk.size // 2], 1)
            body += struct.pack("<i", len(s)) + s
    hdr = bytearray(good[:16])
    hdr[2] &= ~0x10
    struct.pack_into("<I", hdr, 12, 16 + 4 * nb + len(body))
    split = bytes(hdr) + struct.pack(f"<{nb}i", *starts) + bytes(body)
    assert bstarts  # (the writer's own table had one stream per block)
    h2, soff, csize, doff, dlen = codecs.blosc_zstd_stream_table(split)
    assert len(csize) == 2 * nb and set(dlen.tolist()) == {h.blocksize // 2}
    assert np.array_equal(codecs.blosc_decode_blocks(split)[1], perm)


def test_zstd_corpus_covers_the_format():
    """The frames the GPU tests decode use every block type, literals type and sequence mode the decoder implements."""
    feats = set()
    for frame, _ in zstd_corpus.raw_frames():
        feats |= zstd_corpus.walk(frame)
    for frame, _ in zstd_corpus.hand_frames().values():
        feats |= zstd_corpus.walk(frame)
    for buf in _zstd_goldens().values():
        _, soff, csize, _, dlen = codecs.blosc_zstd_stream_table(buf)
        for so, cs, dl in zip(soff, csize, dlen):
            if cs != dl:
                feats |= zstd_corpus.walk(buf[int(so):int(so) + int(cs)])
    want = {("block", b) for b in ("raw", "rle", "compressed")}
    want |= {("literals", k) for k in ("raw", "rle", "huf1", "huf4", "treeless")}
    want |= {("seq", t, m) for t in ("LL", "OF", "ML") for m in ("predefined", "rle", "fse")}
    want |= {("seq", "LL", "repeat"), ("seq", "OF", "repeat")}
    assert want <= feats, sorted(want - feats)


def test_hand_built_frames_are_valid_zstd():
    for name, (frame, want) in zstd_corpus.hand_frames().items():
        if want is None:
            with pytest.raises(Exception):
                codecs.zstd_decompress(frame, 7)
        else:
            assert codecs.zstd_decompress(frame, len(want)).tobytes() == want, name
