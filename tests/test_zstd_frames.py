"""Blosc-zstd stream tables and the zstd frame corpus of the device decoder (csrc/zstd.hip) — host side, no GPU."""
import struct
from pathlib import Path

import numpy as np
import pytest

from biahub_amd import codecs

import zstd_corpus

GOLDEN = Path(__file__).parent / "golden"
MAGIC = b"\x28\xb5\x2f\xfd"


def _goldens(codec=None):
    """{name: (frame, raw)} of the compressed c-blosc streams, all of them or those of one inner codec."""
    z = np.load(GOLDEN / "blosc_streams.npz")
    out = {}
    for k in sorted(z.files):
        if k.endswith("__blosc"):
            buf = z[k].tobytes()
            h = codecs.BloscHeader(buf)
            if codec in (None, h.codec) and not h.memcpyed and h.nbytes > 0:
                out[k[: -len("__blosc")]] = (buf, z[k[: -len("__blosc")] + "__raw"])
    return out


def _zstd_goldens():
    return {k: buf for k, (buf, _) in _goldens("zstd").items()}


def _assert_tiles(name, h, soff, csize, doff, dlen):
    """The streams tile the chunk and every one of them ends inside the frame."""
    order = np.argsort(doff)
    assert int(doff[order[0]]) == 0, name
    assert np.array_equal(doff[order][1:], doff[order][:-1] + dlen[order][:-1].astype(np.uint64)), name
    assert int(doff[order[-1]]) + int(dlen[order[-1]]) == h.nbytes, name
    for so, cs in zip(soff, csize):
        assert int(so) + int(cs) <= h.cbytes, name


def test_zstd_stream_table_on_c_blosc_goldens():
    goldens = _zstd_goldens()
    assert len(goldens) >= 25
    stored = frames = 0
    for name, buf in goldens.items():
        h, soff, csize, doff, dlen = codecs.blosc_stream_table(buf, codec="zstd")
        _assert_tiles(name, h, soff, csize, doff, dlen)
        for so, cs, dl in zip(soff, csize, dlen):
            so, cs = int(so), int(cs)
            if cs == dl:
                stored += 1
            else:
                assert buf[so:so + 4] == MAGIC, name
                frames += 1
    assert stored == 3
    assert frames >= 40


def test_stream_table_tiles_every_c_blosc_golden():
    """The one walk on every compressed stream the real c-blosc wrote, whatever its inner codec and split mode."""
    goldens = _goldens()
    assert len(goldens) == 62
    split = 0
    for name, (buf, raw) in goldens.items():
        h, soff, csize, doff, dlen = codecs.blosc_stream_table(buf)
        assert [a.dtype for a in (soff, csize, doff, dlen)] == [np.uint64, np.uint32, np.uint64, np.uint32]
        _assert_tiles(name, h, soff, csize, doff, dlen)
        split += not h.flags & 0x10
        h2, perm = codecs.blosc_decode_blocks(buf)
        mode = codecs.BLOSC_NOSHUFFLE if h2.memcpyed else h2.shuffle_mode
        assert np.array_equal(codecs.unfilter(perm, h2.nbytes, h2.blocksize, h2.typesize, mode), raw.view(np.uint8).reshape(-1)), name
    assert split == 29


def _set(frame, offset, fmt, value, tail=b""):
    bad = bytearray(frame)
    struct.pack_into(fmt, bad, offset, value)
    return bytes(bad) + tail


def _corrupt_cases(frame):
    """{case: malformed copy of ``frame``}; every one must raise ValueError("corrupt blosc stream")."""
    h, soff, _, _, _ = codecs.blosc_stream_table(frame)
    cb0 = int(soff[0]) - 4  # where the first stream's length stands
    huge = _set(_set(frame, 4, "<I", 0xFFFFFFFF), 8, "<I", 1)
    return {
        "bstart_in_header": _set(frame, 16, "<i", 8),
        "bstart_negative": _set(frame, 16, "<i", -4),
        # one byte beyond cbytes, with bytes behind the frame: a check against len(buf) would pass
        "cb_beyond_cbytes": _set(frame, cb0, "<i", h.cbytes - int(soff[0]) + 1, tail=bytes(64)),
        "cb_zero": _set(frame, cb0, "<i", 0),
        "table_beyond_cbytes": huge,
        "blocksize_zero": _set(frame, 8, "<I", 0),
        "typesize_zero_split": _set(_set(frame, 2, "<B", frame[2] & ~0x10), 3, "<B", 0),
    }


_CORRUPT = ("bstart_in_header", "bstart_negative", "cb_beyond_cbytes", "cb_zero", "table_beyond_cbytes", "blocksize_zero",
            "typesize_zero_split")
_ENTRIES = {"table": codecs.blosc_stream_table, "decode_blocks": codecs.blosc_decode_blocks, "decompress": codecs.blosc_decompress}


@pytest.mark.parametrize("entry", sorted(_ENTRIES))
@pytest.mark.parametrize("case", _CORRUPT + ("cut_short",))
@pytest.mark.parametrize("golden,codec", [("lz4big_u2_s2", "lz4"), ("zstd1_u2_s2", "zstd")])
def test_corrupt_frames_raise(golden, codec, case, entry):
    """Every entry point that parses a frame refuses the same malformed frames: one walk, one idea of "corrupt"."""
    parse = _ENTRIES[entry]
    frame, _ = _goldens(codec)[golden]
    parse(frame)  # the frame itself is fine
    if case == "cut_short":  # cbytes says more than there is
        with pytest.raises(ValueError):
            parse(frame[: len(frame) - 10])
    else:
        with pytest.raises(ValueError, match="corrupt blosc stream"):
            parse(_corrupt_cases(frame)[case])


def test_zstd_stream_table_rejects_corrupt_frames():
    buf = _zstd_goldens()["zstd1_u2_s2"]
    h, soff, csize, _, _ = codecs.blosc_stream_table(buf, codec="zstd")
    with pytest.raises(ValueError):  # truncated: cbytes says more than there is
        codecs.blosc_stream_table(buf[: h.cbytes - 10], codec="zstd")
    bad = bytearray(buf)
    struct.pack_into("<i", bad, 16, 8)  # bstart inside the header
    with pytest.raises(ValueError, match="corrupt blosc stream"):
        codecs.blosc_stream_table(bytes(bad), codec="zstd")
    bad = bytearray(buf)
    struct.pack_into("<i", bad, int(soff[0]) - 4, h.cbytes)  # cb beyond the frame
    with pytest.raises(ValueError, match="corrupt blosc stream"):
        codecs.blosc_stream_table(bytes(bad), codec="zstd")
    with pytest.raises(ValueError):  # another inner codec
        codecs.blosc_stream_table(codecs.blosc_compress(np.zeros(4096, np.uint8), 1, "lz4", 5), codec="zstd")


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
    h2, soff, csize, doff, dlen = codecs.blosc_stream_table(split, codec="zstd")
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
        _, soff, csize, _, dlen = codecs.blosc_stream_table(buf, codec="zstd")
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
