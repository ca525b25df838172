"""GPU: bh_pyramid_downsample for float16 and uint32 (csrc/pyramid.hip) against the numpy restatement
(tests/pyramid_dtypes_ref.py), every comparison on bit patterns: every method over awkward shapes and level counts, chained
launches against single steps, the four older dtypes unmoved, the store round trip on zarr v2 and sharded v3, and `stitch`
followed by `pyramid` from the command line."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

import pyramid_ref as base
from biahub_amd import io
from biahub_amd.pyramid import downsample_pyramid
from pyramid_dtypes_ref import WITNESS, WITNESS_MEAN_BITS, pyramid_ref
from pyramid_ref import METHODS, expected_datasets, level_shape

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((1, 1, 1), (1, 5, 7), (5, 7, 9), (17, 33, 65), (8, 64, 1001), (33, 130, 257))
LEVELS = (2, 3, 4, 5)  # launches of depth 1, 2, 3 and a chained 3 + 1
LABELS = np.array([0, 1, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1], np.uint32)  # ids float32 cannot hold, ids negative as int32
_UINT = {2: np.uint16, 4: np.uint32}
_INT = {torch.float16: torch.int16, torch.uint32: torch.int32, torch.uint16: torch.int16}


def _bits(a):
    """A numpy array as unsigned integers of its element size: the bit patterns."""
    return a.view(_UINT[a.dtype.itemsize])


def _tbits(t):
    """A tensor as signed integers of its element size (same bits): torch implements few operators for uint16 / uint32."""
    return t.view(_INT[t.dtype]) if t.dtype in _INT else t


def _finite_f16(rng, shape):
    """Random bit patterns over the whole finite float16 range: both signs, subnormals included, exponent field < 31; -0 -> +0."""
    b = rng.integers(0, 1 << 16, shape).astype(np.uint16)
    b[(b & 0x7C00) == 0x7C00] &= 0xBFFF  # inf / NaN patterns: clear one exponent bit
    b[b == 0x8000] = 0
    assert ((b & 0x7C00) != 0x7C00).all()
    return b.view(np.float16)


def _volume(shape, dtype, method, seed):
    rng = np.random.default_rng(seed)
    if dtype is np.float16:
        if method == "mode":  # few distinct values: ties and repeats in most blocks
            return (rng.integers(0, 4, shape) * 3 - 4).astype(np.float16) / np.float16(8)
        v = _finite_f16(rng, shape)
        if shape == (5, 7, 9):  # the double-rounding witness at an interior block and at the last whole block before the upper edges
            v[0:2, 2:4, 4:6] = WITNESS
            v[2:4, 4:6, 6:8] = WITNESS
        if shape == (17, 33, 65):  # and in a box wholly inside the source (the path without per-voxel tests)
            v[0:2, 0:2, 2:4] = WITNESS
        return v
    if method == "mode":
        return LABELS[rng.integers(0, len(LABELS), shape)]
    return rng.integers(0, 1 << 32, shape).astype(np.uint32)


def test_the_witness_sits_where_the_shape_says():
    v = _volume((5, 7, 9), np.float16, "mean", seed=2)
    lv = pyramid_ref(v, 2, "mean")[0]
    assert _bits(lv)[0, 1, 2] == WITNESS_MEAN_BITS and _bits(lv)[1, 2, 3] == WITNESS_MEAN_BITS


@pytest.mark.parametrize("dtype", [np.float16, np.uint32], ids=["float16", "uint32"])
@pytest.mark.parametrize("method", METHODS)
def test_bit_exact_against_restatement(gpu, method, dtype):
    for si, shape in enumerate(SHAPES):
        vol = _volume(shape, dtype, method, seed=si)
        ref = pyramid_ref(vol, max(LEVELS), method)
        dv = torch.from_numpy(vol).to(gpu)
        for levels in LEVELS:
            got = downsample_pyramid(dv, levels, method)
            assert len(got) == levels - 1
            for k, (g, r) in enumerate(zip(got, ref), start=1):
                assert g.dtype == dv.dtype and g.device == dv.device and tuple(g.shape) == level_shape(shape, k)
                h = g.cpu().numpy()
                assert h.dtype == r.dtype == np.dtype(dtype)
                if not np.array_equal(_bits(h), _bits(r)):
                    bad = np.argwhere(_bits(h) != _bits(r))
                    i = tuple(bad[0])
                    pytest.fail(f"{method} {np.dtype(dtype).name} {shape} levels={levels} level {k}: {len(bad)} voxels differ, "
                                f"first {i}: {int(_bits(h)[i]):#x} != {int(_bits(r)[i]):#x}")
        assert np.array_equal(_bits(dv.cpu().numpy()), _bits(vol))  # the input is only read
    if dtype is np.float16 and method == "mean":
        (lv,) = downsample_pyramid(torch.from_numpy(_volume((5, 7, 9), dtype, method, seed=2)).to(gpu), 2, method)
        got = _bits(lv.cpu().numpy())
        assert got[0, 1, 2] == WITNESS_MEAN_BITS and got[1, 2, 3] == WITNESS_MEAN_BITS
        (lv,) = downsample_pyramid(torch.from_numpy(_volume((17, 33, 65), dtype, method, seed=3)).to(gpu), 2, method)
        assert _bits(lv.cpu().numpy())[0, 0, 1] == WITNESS_MEAN_BITS


def test_float16_mean_of_tiny_values(gpu):
    """Exponent fields 0 and 1 only (|v| < 2^-13): most means are subnormal float16, many of them ties, so the float64 -> float16
    conversion is held on its subnormal side too (random patterns over the whole range almost never get there)."""
    shape = (17, 33, 65)
    bits = _bits(_finite_f16(np.random.default_rng(21), shape)) & 0x87FF
    bits[bits == 0x8000] = 0
    vol = bits.view(np.float16)
    ref = pyramid_ref(vol, 4, "mean")
    assert ((_bits(ref[0]) & 0x7C00) == 0).mean() > 0.5
    got = downsample_pyramid(torch.from_numpy(vol).to(gpu), 4, "mean")
    for k, (g, r) in enumerate(zip(got, ref), start=1):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(r)), k


@pytest.mark.parametrize("dtype,method", [(np.float16, "mean"), (np.uint32, "mode")], ids=["float16-mean", "uint32-mode"])
def test_chained_launches_equal_single_steps(gpu, dtype, method):
    vol = _volume((37, 70, 131), dtype, method, seed=7)
    dv = torch.from_numpy(vol).to(gpu)
    seven = downsample_pyramid(dv, 7, method)
    src, steps = dv, []
    for _ in range(6):
        before = _tbits(src).clone()
        (nxt,) = downsample_pyramid(src, 2, method)
        assert torch.equal(_tbits(src), before)  # the input is unchanged
        steps.append(nxt)
        src = nxt
    for a, b in zip(seven, steps):
        assert torch.equal(_tbits(a), _tbits(b))
    four = downsample_pyramid(dv, 4, method)
    more = downsample_pyramid(four[-1], 4, method)
    for a, b in zip(seven, four + more):
        assert torch.equal(_tbits(a), _tbits(b))
    for a, r in zip(seven, pyramid_ref(vol, 7, method)):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(r))
    assert np.array_equal(_bits(dv.cpu().numpy()), _bits(vol))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
def test_existing_dtypes_did_not_move(gpu, dtype):
    rng = np.random.default_rng(9)
    shape = (33, 130, 257)
    vol = rng.integers(0, 1 << 16, shape).astype(np.uint16) if dtype is np.uint16 else \
        (rng.standard_normal(shape) * 100).astype(np.float32)
    got = downsample_pyramid(torch.from_numpy(vol).to(gpu), 4, "mean")
    for g, r in zip(got, base.pyramid_ref(vol, 4, "mean")):
        h = g.cpu().numpy()
        assert h.dtype == r.dtype == np.dtype(dtype) and np.array_equal(_bits(h), _bits(r))


PLATES = {
    "ngff04_zstd": dict(version="0.4", compressor={"id": "blosc", "cname": "zstd", "clevel": 1, "shuffle": 2, "blocksize": 0},
                        shards_ratio=None),
    "ngff05_lz4_sharded": dict(version="0.5", compressor={"id": "blosc", "cname": "lz4", "clevel": 1, "shuffle": 2,
                                                          "blocksize": 0}, shards_ratio=(1, 1, 2, 1, 1)),
}


def _files(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


@pytest.mark.parametrize("dtype,method", [(np.float16, "mean"), (np.uint32, "mode")], ids=["float16-mean", "uint32-mode"])
@pytest.mark.parametrize("kind", list(PLATES))
def test_store_round_trip(gpu, tmp_path, kind, dtype, method):
    shape = (2, 2, 21, 77, 139)
    store = tmp_path / "plate.zarr"
    pos = store / "A" / "1" / "0"
    io.create_empty_plate(store, [("A", "1", "0")], ["a", "b"], shape, chunks=(1, 1, 4, shape[3], shape[4]),
                          scale=(1, 1, 2.0, 0.5, 0.5), dtype=dtype, **PLATES[kind])
    arr = io.open_ome_zarr(pos).data
    vols = {}
    for t in range(2):
        for c in range(2):
            vols[t, c] = _volume(shape[2:], dtype, method, seed=10 * t + c)
            arr.write_volume(t, c, vols[t, c])
    level0 = {k: v for k, v in _files(pos).items() if k.startswith("0/")}
    ds0 = io.open_ome_zarr(pos).zattrs["multiscales"][0]["datasets"][0]
    io.open_ome_zarr(pos).compute_pyramid(4, method)
    p = io.open_ome_zarr(pos)
    assert p.array_keys() == ["0", "1", "2", "3"]
    assert p.zattrs["multiscales"][0]["datasets"] == expected_datasets(ds0, 4)
    for (t, c), vol in vols.items():
        lv0 = p.data.read_volume(t, c)
        assert lv0.dtype == np.dtype(dtype) and np.array_equal(_bits(lv0), _bits(vol))
        ref = pyramid_ref(lv0, 4, method)
        for k in range(1, 4):
            got = p[str(k)].read_volume(t, c)
            assert got.dtype == np.dtype(dtype) and np.array_equal(_bits(got), _bits(ref[k - 1])), (t, c, k)
    dev = p["2"].read_volume_device(1, 1, gpu)  # the device read route serves the new levels, too
    assert dev.dtype == (torch.float16 if dtype is np.float16 else torch.uint32)
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(pyramid_ref(vols[1, 1], 3, method)[1]))
    assert {k: v for k, v in _files(pos).items() if k.startswith("0/")} == level0  # level 0 byte for byte


@pytest.mark.parametrize("dtype", [np.float16, np.uint32], ids=["float16", "uint32"])
def test_unwritten_volume_reads_as_fill_on_the_device(gpu, tmp_path, dtype):
    """The device read route fills chunks that have no file: torch has no fill for uint32, so the store layer must not need one."""
    pos = tmp_path / "p"
    io.create_empty_position(pos, ["a"], (1, 1, 8, 16, 24), chunks=(1, 1, 4, 16, 24), dtype=dtype, compressor="blosc")
    arr = io.open_ome_zarr(pos).data
    assert arr.stage_volume(0, 0) is not None  # plane-stack Blosc chunks: the device route
    dev = arr.read_volume_device(0, 0, gpu)
    assert dev.dtype == (torch.float16 if dtype is np.float16 else torch.uint32) and tuple(dev.shape) == (8, 16, 24)
    assert not dev.cpu().numpy().view(np.uint8).any()


def _run(tmp_path, *args):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    return subprocess.run([sys.executable, "-m", "biahub_amd", *args], env=env, cwd=tmp_path, capture_output=True, text=True, timeout=300)


def test_stitch_then_pyramid_from_the_command_line(gpu, tmp_path):
    shape = (1, 1, 3, 20, 24)
    shifts = {"A/1/0": [0, 0, 0], "A/1/1": [0, 0, 20], "A/1/2": [0, 16, 0], "A/1/3": [0, 16, 20]}  # 4 pixels of overlap
    keys = [tuple(k.split("/")) for k in shifts]
    store = tmp_path / "plate.zarr"
    io.create_empty_plate(store, keys, ["GFP"], shape, chunks=(1, 1, 3, 20, 24), scale=(1, 1, 2.0, 0.5, 0.5), dtype=np.uint16,
                          version="0.4", compressor="blosc")
    rng = np.random.default_rng(13)
    for k in keys:
        io.open_ome_zarr(store.joinpath(*k)).data.write_volume(0, 0, rng.integers(0, 60000, shape[2:]).astype(np.uint16))
    cfg = tmp_path / "stitch.yml"
    cfg.write_text(yaml.safe_dump({"total_translation": {k: [float(v) for v in s] for k, s in shifts.items()}}, sort_keys=False))
    out = tmp_path / "stitched.zarr"
    res = _run(tmp_path, "stitch", "-i", *[str(store.joinpath(*k)) for k in keys], "-c", str(cfg), "-o", str(out), "--local")
    assert res.returncode == 0, res.stdout + res.stderr
    mosaic = out / "A" / "1" / "0"
    lv0 = io.open_ome_zarr(mosaic).data.read_volume(0, 0)
    assert lv0.dtype == np.float16 and lv0.shape == (3, 36, 44) and lv0.any()
    res = _run(tmp_path, "pyramid", "-i", str(mosaic), "--levels", "3", "-m", "mean", "--local")
    assert res.returncode == 0, res.stdout + res.stderr
    p = io.open_ome_zarr(mosaic)
    assert p.array_keys() == ["0", "1", "2"]
    assert np.array_equal(_bits(p.data.read_volume(0, 0)), _bits(lv0))
    ref = pyramid_ref(lv0, 3, "mean")
    for k in (1, 2):
        got = p[str(k)].read_volume(0, 0)
        assert got.dtype == np.float16 and got.shape == level_shape(lv0.shape, k)
        assert np.array_equal(_bits(got), _bits(ref[k - 1])), k
