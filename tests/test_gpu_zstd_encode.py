"""csrc/zstd_enc.hip on the GPU: Blosc frames with zstd inside, made on the device.  The judge of every zstd frame is pyarrow's
libzstd (``codecs.zstd_decompress``); the project's own decoders and, where the image has it, the real c-blosc read them too."""
import ctypes
import json
import os
from pathlib import Path

import numpy as np
import pytest

import zstd_corpus
from biahub_amd import codecs

torch = pytest.importorskip("torch")

EDGE_TAILS = (1, 2, 3, 4, 12, 13, 127)                 # as the short last block behind one full block (a chunk has >= 128 bytes)
EDGE_CHUNKS = (131071, 131072, 131073, 262143)         # 131073: a second zstd block of one byte
TYPESIZE = dict(camera=2, float8=4, ramp=2, sparse=2, constant=2, alpha4=1, tile4=1, runs=1, zeros_tail=1)


def _compress(gpu, permuted: np.ndarray, nframes: int, cbytes: int, bsz: int, ts: int, mode: int):
    """One launch over ``permuted``; the frames as host bytes."""
    packed, offs = codecs.blosc_zstd_compress_device(torch.from_numpy(permuted).to(gpu), nframes, cbytes, bsz, ts, mode)
    assert len(offs) == nframes + 1 and offs[-1] <= packed.numel()
    host = packed[: offs[-1]].cpu().numpy()
    frames = []
    for i in range(nframes):
        n = int(np.frombuffer(host[offs[i] + 12: offs[i] + 16].tobytes(), np.uint32)[0])
        assert offs[i] + n <= offs[i + 1]
        frames.append(host[offs[i]: offs[i] + n].tobytes())
    return frames


def _check_streams(frame: bytes, permuted: np.ndarray) -> list:
    """Every inner stream is stored, or a zstd frame that libzstd decodes to its block of ``permuted``; returns the sizes."""
    h, soff, csize, doff, dlen = codecs.blosc_stream_table(frame, codec="zstd")
    assert int(dlen.sum()) == permuted.size
    for so, cs, do, dl in zip(soff.tolist(), csize.tolist(), doff.tolist(), dlen.tolist()):
        want = permuted[do:do + dl]
        assert cs <= dl                                                   # never larger than stored
        if cs == dl:
            assert frame[so:so + cs] == want.tobytes()
        else:
            stream = frame[so:so + cs]
            assert codecs.zstd_frame_content_size(stream) == dl
            assert np.array_equal(codecs.zstd_decompress(stream, dl), want)
    return csize.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,mode", [("u2", 2), ("f4", 2), ("u2", 1), ("u1", 0)])
def test_zstd_device_compressor_frames(gpu, dtype, mode):
    """Permute -> zstd frames -> packed Blosc frames, all on the GPU: four chunks with a short last block, read back by libzstd
    stream by stream, by the host decoder, by the device decoder in one launch and by the real c-blosc."""
    ts = np.dtype(dtype).itemsize
    chunks = zstd_corpus.compressor_chunks(dtype)  # 190 / 380 / 760 KB each: one to three 256-KiB blocks, the last one short
    raw = np.concatenate([c.view(np.uint8) for c in chunks])
    cbytes = chunks[0].nbytes
    bsz = codecs.default_blocksize(ts)
    src = torch.from_numpy(raw).to(gpu)
    filt = torch.empty_like(src)
    for i in range(len(chunks)):
        codecs.filter_device(src[i * cbytes:(i + 1) * cbytes], filt[i * cbytes:(i + 1) * cbytes], bsz, ts, mode)
    packed, offs = codecs.blosc_zstd_compress_device(filt, len(chunks), cbytes, bsz, ts, mode)
    host = packed[: offs[-1]].cpu().numpy()
    permuted = filt.cpu().numpy()
    lib = ctypes.CDLL("/opt/conda/lib/libblosc.so.1") if os.path.exists("/opt/conda/lib/libblosc.so.1") else None
    if lib is not None:
        lib.blosc_decompress_ctx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    sizes, frames = [], []
    for i, c in enumerate(chunks):
        frame = host[offs[i]: offs[i + 1]]
        h = codecs.BloscHeader(frame.tobytes())
        assert (h.nbytes, h.blocksize, h.typesize, h.codec, h.shuffle_mode) == (cbytes, min(bsz, cbytes), ts, "zstd", mode if ts > 1 or mode != 1 else 0)
        stream = frame[: h.cbytes].tobytes()
        # the flags and versions of the host writer
        ref = codecs.blosc_compress(permuted[i * cbytes:(i + 1) * cbytes], ts, "zstd", 1, mode, bsz, prefiltered=True)
        assert stream[:12] == ref[:12], i
        _check_streams(stream, permuted[i * cbytes:(i + 1) * cbytes])                    # libzstd, stream by stream
        assert np.array_equal(codecs.blosc_decompress(stream), c.view(np.uint8)), i      # host decoder
        if lib is not None:                                                                 # the real library
            buf = np.frombuffer(stream, np.uint8).copy()
            back = np.empty(cbytes, np.uint8)
            assert lib.blosc_decompress_ctx(buf.ctypes.data, back.ctypes.data, back.size, 1) == cbytes, i
            assert np.array_equal(back, c.view(np.uint8)), i
        sizes.append(h.cbytes)
        frames.append(stream)
    # every frame of the "volume" in one upload and one launch (what read_volume_device does)
    allout = torch.zeros_like(filt)
    hs = codecs.blosc_decode_frames_device(frames, allout, [i * cbytes for i in range(len(chunks))])
    assert len(hs) == len(chunks) and torch.equal(allout, filt)
    nb = -(-cbytes // bsz)
    assert cbytes + 16 + 4 * nb <= sizes[1] <= cbytes + 16 + 8 * nb, sizes  # noise: every block stored
    assert all(s <= cbytes + 16 + 8 * nb for s in sizes), sizes               # no frame larger than stored
    assert sizes[2] < 0.001 * cbytes, sizes                                    # zeros: a few sequences per block


@pytest.mark.gpu
def test_zstd_device_encoder_bytes_are_pinned(gpu):
    """The device encoder resets its hash table per frame and its atomics only count, so its frames are a function of the input
    alone: the four cases of ``test_zstd_device_compressor_frames`` and a chunk of two 256-KiB blocks and a third of 1000 bytes,
    byte for byte against digests recorded on an MI355X before the encoder's source was last rearranged (the fixture names the
    commit).  A deliberate change to the encoder re-records the fixture."""
    assert [tuple(c) for c in zstd_corpus.DEVICE_DIGEST_CASES] == [("u2", 2), ("f4", 2), ("u2", 1), ("u1", 0)]
    pinned = json.loads((Path(__file__).parent / "golden" / "zstd_enc_device_digests.json").read_text())["digests"]
    assert zstd_corpus.device_encoder_digests(gpu) == pinned


@pytest.mark.gpu
def test_zstd_device_corpus_one_launch(gpu):
    """Every corpus kind at 262144 and 32768 bytes in ONE launch — frame k is kind k: a full block and a short one, permuted
    as the store permutes them — decoded by libzstd, with the size conditions of the format's entropy stage."""
    big, small = zstd_corpus.data_kinds(262144), zstd_corpus.data_kinds(32768)
    bsz, cbytes = 262144, 262144 + 32768
    parts = []
    for kind in big:
        ts = TYPESIZE[kind]
        for d in (big[kind], small[kind]):
            parts.append(codecs.filter_host(d, d.size, ts, codecs.BLOSC_BITSHUFFLE) if ts > 1 else d)
    permuted = np.concatenate(parts)
    frames = _compress(gpu, permuted, len(big), cbytes, bsz, 1, 0)
    for k, kind in enumerate(big):
        p = permuted[k * cbytes:(k + 1) * cbytes]
        csize = _check_streams(frames[k], p)
        print(kind, csize, len(codecs.zstd_compress(p[:bsz], 1)), len(codecs.lz4_block_compress(p[:bsz])))
        if kind in ("camera", "float8", "alpha4"):                        # the literal entropy coder: below an LZ-only codec
            assert csize[0] < len(codecs.lz4_block_compress(p[:bsz])), (kind, csize)
            assert csize[1] < len(codecs.lz4_block_compress(p[bsz:])), (kind, csize)
        if kind in ("constant", "tile4", "runs"):
            assert csize[0] < 0.05 * bsz and csize[1] < 0.05 * 32768, (kind, csize)


@pytest.mark.gpu
def test_zstd_device_edge_sizes(gpu):
    """Blocks of 1 to 127 bytes (the short last block of a chunk), chunks around the 128-KiB zstd block edge."""
    cam = zstd_corpus.data_kinds(524288)["camera"]
    bsz = 262144
    for tail in EDGE_TAILS:
        p = cam[: bsz + tail]
        (frame,) = _compress(gpu, p, 1, p.size, bsz, 1, 0)
        csize = _check_streams(frame, p)
        assert len(csize) == 2 and csize[1] <= tail
    for n in EDGE_CHUNKS:
        p = cam[:n]
        (frame,) = _compress(gpu, p, 1, n, bsz, 1, 0)
        csize = _check_streams(frame, p)
        assert len(csize) == 1 and csize[0] < n


@pytest.mark.gpu
@pytest.mark.parametrize("yx", [(96, 160), (256, 320)])
@pytest.mark.parametrize("version,shards_ratio,shuffle", [("0.4", None, 2), ("0.4", None, 1), ("0.5", None, 2), ("0.5", (1, 1, 2, 1, 1), 2)])
def test_zarr_device_volume_io_zstd_encoder(gpu, tmp_path, monkeypatch, version, shards_ratio, shuffle, yx):
    """With BH_ZSTD_ENCODE_DEVICE=1 a default (Blosc-zstd) store written from the device reads back through every reader, and
    without the variable the device encoder is not reached.  Planes of 96 x 160 are the shape of ``test_zarr_device_volume_io``:
    a chunk of 8 of them is smaller than one 256-KiB block, which the store has always handed to the host writer whole — so the
    variable changes nothing there; with planes of 256 x 320 (1.3-MB chunks, five blocks) the device encoder must be the one
    that wrote: one launch for the volume's three chunks, only compressed bytes across PCIe."""
    from biahub_amd import io

    Y, X = yx
    shape = (1, 2, 21, Y, X)  # 21 planes in chunks of 8: the last chunk overhangs
    comp = {"id": "blosc", "cname": "zstd", "clevel": 1, "shuffle": shuffle, "blocksize": 0}
    io.create_empty_position(tmp_path / "p", ["a", "b"], shape, chunks=(1, 1, 8, Y, X), dtype=np.uint16, version=version,
                             compressor=comp, shards_ratio=shards_ratio)
    arr = io.open_ome_zarr(tmp_path / "p").data
    rng = np.random.default_rng(2)
    v0 = (rng.poisson(4, shape[2:]) + 100).astype(np.uint16)
    v1 = (rng.poisson(9, shape[2:]) + 300).astype(np.uint16)
    calls = []
    real = codecs.blosc_zstd_compress_device

    def counted(*a, **k):
        calls.append(a[1])
        return real(*a, **k)

    monkeypatch.setattr(codecs, "blosc_zstd_compress_device", counted)
    monkeypatch.delenv("BH_ZSTD_ENCODE_DEVICE", raising=False)
    arr.write_volume_device(0, 1, torch.from_numpy(v1).to(gpu))   # the default route: libzstd on the I/O threads
    assert calls == []
    monkeypatch.setenv("BH_ZSTD_ENCODE_DEVICE", "1")
    arr.write_volume_device(0, 0, torch.from_numpy(v0).to(gpu))
    assert calls == ([3] if 8 * Y * X * 2 >= codecs.default_blocksize(2) else [])
    assert np.array_equal(arr.read_volume(0, 0), v0)              # host reader (libzstd)
    assert np.array_equal(arr.read_volume_device(0, 0, gpu).cpu().numpy(), v0)
    monkeypatch.setenv("BH_ZSTD_DEVICE", "0")
    assert np.array_equal(arr.read_volume_device(0, 0, gpu).cpu().numpy(), v0)
    monkeypatch.delenv("BH_ZSTD_DEVICE")
    assert np.array_equal(arr.read_volume_device(0, 1, gpu).cpu().numpy(), v1)
    f = tmp_path / "p" / "0" / ("c/0/0/0/0/0" if version == "0.5" else "0/0/0/0/0")
    assert f.stat().st_size < 8 * Y * X * 2 * (2 if shards_ratio else 1) // 2        # it really is compressed
