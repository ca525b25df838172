"""csrc/zstd.hip: Blosc-zstd chunks decoded on the GPU — c-blosc goldens, pyarrow's zstd across levels and data kinds, hand-built
frames, corrupt input, the store route and a full-size volume."""
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

from biahub_amd import codecs

import zstd_corpus

GOLDEN = Path(__file__).parent / "golden"


def _decode_raw_frames(frames, gpu):
    """zstd frames (one stream each) -> device, one launch; returns the host bytes per frame."""
    sizes = [len(w) for _, w in frames]
    src = np.frombuffer(b"".join(f for f, _ in frames), np.uint8)
    soff = np.cumsum([0] + [len(f) for f, _ in frames[:-1]]).astype(np.uint64)
    doff = np.cumsum([0] + sizes[:-1]).astype(np.uint64)
    csize = np.asarray([len(f) for f, _ in frames], np.uint32)
    dlen = np.asarray(sizes, np.uint32)
    out = torch.zeros(sum(sizes), dtype=torch.uint8, device=gpu)
    codecs._device_streams("bh_zstd_decompress_streams", torch.from_numpy(src.copy()).to(gpu), (soff, csize, doff, dlen), out)
    o = out.cpu().numpy()
    return [o[int(a):int(a) + n].tobytes() for a, n in zip(doff, sizes)]


@pytest.mark.gpu
def test_zstd_device_decodes_c_blosc_goldens(gpu):
    z = np.load(GOLDEN / "blosc_streams.npz")
    done = 0
    for k in sorted(z.files):
        if not k.endswith("__blosc"):
            continue
        stream = z[k].tobytes()
        h = codecs.BloscHeader(stream)
        if h.codec != "zstd" or h.memcpyed or h.nbytes == 0:
            continue
        _, want = codecs.blosc_decode_blocks(stream)
        out = torch.empty(h.nbytes, dtype=torch.uint8, device=gpu)
        codecs.blosc_decode_blocks_device(stream, out)
        assert np.array_equal(out.cpu().numpy(), want), k
        raw = torch.empty_like(out)
        codecs.unfilter_device(out, raw, h.blocksize, h.typesize, h.shuffle_mode)
        assert np.array_equal(raw.cpu().numpy(), z[k[: -len("__blosc")] + "__raw"]), k
        done += 1
    assert done >= 25


@pytest.mark.gpu
def test_zstd_device_decodes_pyarrow_corpus_in_one_launch(gpu):
    """Every data kind x level x block size through codecs.blosc_compress (pyarrow's zstd), all frames in one launch."""
    frames, want = [], []
    for data in zstd_corpus.data_kinds().values():
        for level in zstd_corpus.LEVELS:
            for bs in zstd_corpus.BLOCKS:
                fr = codecs.blosc_compress(data, 2, "zstd", level, codecs.BLOSC_BITSHUFFLE, bs)
                if codecs.BloscHeader(fr).memcpyed:
                    continue
                frames.append(fr)
                want.append(codecs.blosc_decode_blocks(fr)[1])
    offs = np.cumsum([0] + [w.size for w in want[:-1]]).tolist()
    out = torch.zeros(sum(w.size for w in want), dtype=torch.uint8, device=gpu)
    heads = codecs.blosc_decode_frames_device(frames, out, offs)
    assert len(heads) == len(frames) >= 80
    o = out.cpu().numpy()
    for k, (a, w) in enumerate(zip(offs, want)):
        assert np.array_equal(o[a:a + w.size], w), k
    # the same kinds as bare zstd frames (one per block): raw, RLE and compressed blocks, every literals type
    got = _decode_raw_frames(zstd_corpus.raw_frames(), gpu)
    for k, ((_, w), g) in enumerate(zip(zstd_corpus.raw_frames(), got)):
        assert g == w, k


@pytest.mark.gpu
def test_zstd_device_hand_built_frames(gpu):
    """RLE literals with zero sequences, and a frame mixing raw, RLE and compressed blocks (pyarrow accepts both)."""
    hf = zstd_corpus.hand_frames()
    cases = [hf["rle_literals"], hf["mixed_blocks"]]
    for (frame, want), got in zip(cases, _decode_raw_frames(cases, gpu)):
        assert got == want


def _expect_corrupt(frames, gpu, index):
    with pytest.raises(ValueError, match=f"corrupt zstd stream {index}"):
        _decode_raw_frames(frames, gpu)


@pytest.mark.gpu
def test_zstd_device_reports_corrupt_frames(gpu):
    camera, cases = zstd_corpus.corrupt_cases()
    assert set(cases) == {"truncated", "dictionary", "content_size", "offset", "huffman_header"}
    for bad in cases.values():
        _expect_corrupt([camera[0], bad, camera[2]], gpu, 1)
    # a good decode afterwards in the same process
    assert _decode_raw_frames(camera, gpu) == [w for _, w in camera]


@pytest.mark.gpu
def test_zstd_store_routes_are_bit_identical(gpu, tmp_path, monkeypatch):
    from biahub_amd import io

    shape = (1, 1, 21, 256, 320)  # the last chunk overhangs the array
    comp = {"id": "blosc", "cname": "zstd", "clevel": 1, "shuffle": 2, "blocksize": 0}
    io.create_empty_position(tmp_path / "p", ["a"], shape, chunks=(1, 1, 8, 256, 320), dtype=np.uint16, version="0.4", compressor=comp)
    arr = io.open_ome_zarr(tmp_path / "p").data
    rng = np.random.default_rng(3)
    v = (rng.poisson(6, shape[2:]) + 100).astype(np.uint16)
    arr.write_volume(0, 0, v)
    host = arr.read_volume(0, 0)
    assert np.array_equal(host, v)
    monkeypatch.setenv("BH_ZSTD_DEVICE", "1")
    staged = arr.stage_volume(0, 0)
    assert sorted(staged["frames"]) == list(range(len(staged["plan"])))
    assert staged["stage"] is None  # no raw-size pinned block
    dev1 = arr.upload_staged(staged, gpu).cpu().numpy()
    monkeypatch.setenv("BH_ZSTD_DEVICE", "0")
    staged0 = arr.stage_volume(0, 0)
    assert not staged0["frames"] and staged0["stage"] is not None
    dev0 = arr.read_volume_device(0, 0, gpu).cpu().numpy()
    assert np.array_equal(dev1, host) and np.array_equal(dev0, host)


@pytest.mark.gpu
def test_zstd_device_full_size_volume(gpu):
    """537 MB of uint16 in c-blosc's 32-KiB zstd blocks: ~16 K frames in one launch."""
    Z, Y, X = 256, 1024, 1024
    rng = np.random.default_rng(5)
    plane = (100 + rng.poisson(20, (Y, X))).astype(np.uint16)
    cz = 32
    frames, offs = [], []
    for z0 in range(0, Z, cz):
        chunk = np.roll(plane, z0, axis=1)[None].repeat(cz, 0) + np.arange(cz, dtype=np.uint16)[:, None, None]
        frames.append(codecs.blosc_compress(chunk.view(np.uint8).reshape(-1), 2, "zstd", 1, codecs.BLOSC_BITSHUFFLE, 32768))
        offs.append(z0 * Y * X * 2)
    h = codecs.BloscHeader(frames[0])
    nstreams = sum(len(codecs.blosc_stream_table(f, codec="zstd")[2]) for f in frames)
    assert nstreams >= 16000
    out = torch.empty(Z * Y * X * 2, dtype=torch.uint8, device=gpu)
    codecs.blosc_decode_frames_device(frames, out, offs)
    vol = torch.empty_like(out)
    cb = h.nbytes
    for k in range(len(frames)):
        codecs.unfilter_device(out[k * cb:(k + 1) * cb], vol[k * cb:(k + 1) * cb], h.blocksize, 2, h.shuffle_mode)
    got = vol.view(torch.int16).view(Z, Y, X).cpu().numpy().view(np.uint16)
    for z0 in range(0, Z, cz):
        want = np.roll(plane, z0, axis=1)[None].repeat(cz, 0) + np.arange(cz, dtype=np.uint16)[:, None, None]
        assert np.array_equal(got[z0:z0 + cz], want), z0


def _split_mode(frame):
    """``frame`` rewritten as c-blosc's always-split mode writes it: every full block as ``typesize`` zstd streams."""
    h, perm = codecs.blosc_decode_blocks(frame)
    nb = -(-h.nbytes // h.blocksize)
    body, starts = bytearray(), []
    for b in range(nb):
        blk = perm[b * h.blocksize:(b + 1) * h.blocksize]
        starts.append(16 + 4 * nb + len(body))
        for part in np.split(blk, h.typesize if blk.size == h.blocksize else 1):
            s = codecs.zstd_compress(part, 1)
            body += struct.pack("<i", len(s)) + s
    head = struct.pack("<BBBBIII", frame[0], frame[1], frame[2] & ~0x10, h.typesize, h.nbytes, h.blocksize, 16 + 4 * nb + len(body))
    return head + struct.pack(f"<{nb}i", *starts) + bytes(body)


@pytest.mark.gpu
def test_device_entry_mixed_codecs_in_one_batch(gpu):
    """lz4 and zstd frames interleaved in one call of blosc_decode_frames_device: multi-block frames with a short last block
    and frames with split blocks, into slots in reverse order with gaps between them; a malformed frame or a frame without a
    device decoder anywhere in the batch is refused on the host, before the device is touched."""
    z = np.load(GOLDEN / "blosc_streams.npz")
    goldens = [z[k].tobytes() for k in sorted(z.files) if k.endswith("__blosc")]
    heads = [codecs.BloscHeader(g) for g in goldens]

    def first(codec, split):
        return next(g for g, h in zip(goldens, heads) if h.codec == codec and not h.memcpyed and h.nbytes and bool(h.flags & 0x10) != split)

    data = (np.arange((2 * 4096 + 1000) // 2) // 7 % 300).astype(np.uint16)
    made = [codecs.blosc_compress(data, 2, c, 1, codecs.BLOSC_BITSHUFFLE, 4096) for c in ("lz4", "zstd")]
    # no zstd golden is written in split mode (c-blosc splits only its fast codecs): the first one, rewritten that way
    frames = [made[0], made[1], first("lz4", True), _split_mode(first("zstd", False))]
    tabs = [codecs.blosc_stream_table(f) for f in frames]
    assert [t[0].codec for t in tabs] == ["lz4", "zstd", "lz4", "zstd"]
    assert [len(t[1]) for t in tabs[:2]] == [3, 3] and all(int(t[4][-1]) == 1000 for t in tabs[:2])
    assert all(not t[0].flags & 0x10 and len(t[1]) > -(-t[0].nbytes // t[0].blocksize) for t in tabs[2:])
    want = [codecs.blosc_decode_blocks(f)[1] for f in frames]
    gap, offs, end = 48, [0] * len(frames), 48
    for k in reversed(range(len(frames))):
        offs[k] = end
        end += want[k].size + gap
    out = torch.full((end,), 0xA5, dtype=torch.uint8, device=gpu)
    got = codecs.blosc_decode_frames_device(frames, out, offs)
    assert [(h.codec, h.nbytes, h.cbytes) for h in got] == [(t[0].codec, t[0].nbytes, t[0].cbytes) for t in tabs]
    o = out.cpu().numpy()
    used = np.zeros(end, bool)
    for k, (a, w) in enumerate(zip(offs, want)):
        assert np.array_equal(o[a:a + w.size], w), k
        used[a:a + w.size] = True
    assert (~used).sum() == gap * (len(frames) + 1) and (o[~used] == 0xA5).all()
    # refused on the host: nothing is allocated, uploaded or launched, so the output keeps its fill
    out.fill_(0xA5)
    bad = bytearray(frames[1])
    struct.pack_into("<i", bad, 16, 8)
    zlib_frame = codecs.blosc_compress(data, 2, "zlib", 1, codecs.BLOSC_BITSHUFFLE, 4096)
    for batch in ([frames[0], bytes(bad)] + frames[2:], frames[:3] + [zlib_frame]):
        with pytest.raises(ValueError):
            codecs.blosc_decode_frames_device(batch, out, offs)
        assert bool((out == 0xA5).all())
