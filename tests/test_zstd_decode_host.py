"""The library's own zstd frame decoder on the CPU (``bh_host_zstd_decompress``: the device decoder's source, csrc/zstd_frame.inc
and zstd_block.inc, compiled with one lane) — what ``tests/test_gpu_zstd.py`` asks of the kernel, asked where no GPU is: c-blosc
goldens, pyarrow's zstd across levels and data kinds, hand-built frames, corrupt frames, and the frames of the library's own
encoder with no other library in between."""
from pathlib import Path

import numpy as np
import pytest

import zstd_corpus
from biahub_amd import codecs
from test_zstd_encode_host import corpus_frames  # noqa: F401  (the fixture)

GOLDEN = Path(__file__).parent / "golden"


def _decode(frame, n: int) -> bytes:
    return codecs.zstd_decompress_host(frame, n).tobytes()


def test_decodes_c_blosc_goldens():
    z = np.load(GOLDEN / "blosc_streams.npz")
    done = 0
    for k in sorted(z.files):
        if not k.endswith("__blosc"):
            continue
        stream = z[k].tobytes()
        h = codecs.BloscHeader(stream)
        if h.codec != "zstd" or h.memcpyed or h.nbytes == 0:
            continue
        _, want = codecs.blosc_decode_blocks(stream)  # libzstd
        _, soff, csize, doff, dlen = codecs.blosc_stream_table(stream, codec="zstd")
        for so, cs, do, dl in zip(soff.tolist(), csize.tolist(), doff.tolist(), dlen.tolist()):
            assert _decode(stream[so:so + cs], dl) == want[do:do + dl].tobytes(), (k, do)
        done += 1
    assert done >= 25


def test_decodes_pyarrow_corpus_and_hand_built_frames():
    """Raw, RLE and compressed blocks, every literals type and sequence mode that pyarrow's zstd writes at five levels."""
    hf = zstd_corpus.hand_frames()
    for k, (frame, want) in enumerate(zstd_corpus.raw_frames() + [hf["rle_literals"], hf["mixed_blocks"]]):
        assert _decode(frame, len(want)) == want, k


def test_reports_corrupt_frames():
    camera, cases = zstd_corpus.corrupt_cases()
    assert set(cases) == {"truncated", "dictionary", "content_size", "offset", "huffman_header"}
    for name, (frame, want) in cases.items():
        with pytest.raises(ValueError, match="corrupt zstd stream"):
            _decode(frame, len(want))
        assert _decode(camera[0][0], len(camera[0][1])) == camera[0][1], name  # a good decode after every refusal
    # a stream as long as its output is a stored one: the bytes themselves
    stored = bytes(range(200))
    assert _decode(stored, len(stored)) == stored
    frame, want = camera[1]
    assert len(frame) != len(want) and _decode(frame, len(want)) == want


def test_encoder_to_decoder_without_a_library(corpus_frames):  # noqa: F811
    """zstd_decompress_host(zstd_compress_host(x)) == x over the encoder's corpus and at the lengths where the frame encoder
    takes another path: the content-size forms (below 256, below 65792, above), the 128-KiB block edge, and a match cut at
    that edge whose remainder is carried into the next block."""
    for name, (data, frame) in corpus_frames.items():
        assert _decode(frame, data.size) == data.tobytes(), name
    edges = zstd_corpus.edge_inputs()
    assert {int(k.split("/")[1].split("_")[0]) for k in edges} == {1, 2, 3, 255, 256, 65791, 65792, 131071, 131072, 131073, 262147}
    for name, data in edges.items():
        frame = codecs.zstd_compress_host(data)
        assert _decode(frame, data.size) == data.tobytes(), name
        if data.size >= 256:
            assert len(frame) < data.size, name  # a real frame, not the stored form
    carry = edges["edge/262147_run_over_block_edge"]
    frame = codecs.zstd_compress_host(carry)
    assert codecs.zstd_decompress(frame, carry.size).tobytes() == carry.tobytes()  # libzstd agrees
    assert len(frame) < carry.size - 90000  # the 100000-byte run across the edge went out as matches, not literals


def test_spread_agreement():
    """An encoder's FSE table is right only if its symbols are spread exactly as the decoder spreads them (fse_spread in
    csrc/zstd_format.inc serves both).  Frames from the host encoder whose sequences use the predefined LL, OF and ML
    distributions (each with "less than 1" symbols at the top of the table), tables fitted to the block, and FSE-compressed
    Huffman weights (bit-shuffled camera planes): libzstd and the host decoder both read them.  The encoder's own fitted tables
    give every present symbol at least one state (fse_normalize), so a FITTED table with "less than 1" symbols reaches the
    spread only from the decoder's side: the pyarrow corpus (levels 3 and up) in the test above."""
    values = np.random.default_rng(11).permutation(256)[:100].astype(np.uint8)
    kinds = zstd_corpus.data_kinds()
    sparse = codecs.filter_host(kinds["sparse"], 262144, 2, codecs.BLOSC_BITSHUFFLE)
    planes = codecs.filter_host(kinds["camera"], 262144, 2, codecs.BLOSC_BITSHUFFLE).reshape(16, -1)
    inputs = {"predefined": np.repeat(values[:50], 64), "rle": np.repeat(values, 64), "fse": sparse}
    inputs.update({f"plane{k}": planes[k] for k in range(16) if np.unique(planes[k]).size > 129})
    seen = set()
    for name, data in inputs.items():
        frame = codecs.zstd_compress_host(data)
        if len(frame) == data.size:
            continue
        seen |= zstd_corpus.walk(frame)
        assert codecs.zstd_decompress(frame, data.size).tobytes() == data.tobytes(), name
        assert _decode(frame, data.size) == data.tobytes(), name
    assert {("seq", t, m) for t in ("LL", "OF", "ML") for m in ("predefined", "fse")} <= seen
