"""CPU: float16 and uint32 in the pyramid step — check_args accepts them however the dtype is given, the restatement
(tests/pyramid_dtypes_ref.py) keeps its own rules on hand-worked blocks (the float16 mean rounds once, the uint32 mean neither
overflows nor loses its ties-to-even), and initialize_pyramid creates level arrays of the input's dtype on zarr v2 and v3."""

import numpy as np
import pytest

from biahub_amd import io
from pyramid_dtypes_ref import (WITNESS, WITNESS_MEAN_BITS, WITNESS_TWICE_ROUNDED_BITS, pyramid_ref, reduce_level)
from pyramid_ref import METHODS, expected_datasets, level_shape


@pytest.mark.parametrize("method", METHODS)
def test_check_args_accepts_float16_and_uint32(method):
    import torch

    from biahub_amd.pyramid import DTYPES, check_args, level_shapes

    assert set(DTYPES) == {"uint8", "uint16", "int16", "float32", "float16", "uint32"}
    for dt in (np.float16, np.dtype("uint32"), torch.float16, torch.uint32, np.dtype("float16"), np.uint32):
        check_args(dt, 4, method)
    for dt, name in ((np.int32, "int32"), (np.int64, "int64"), (np.float64, "float64"), (bool, "bool"), (torch.int32, "int32"),
                     (torch.float64, "float64")):
        with pytest.raises(ValueError, match=name) as e:
            check_args(dt, 4, method)
        for ok in DTYPES:  # the message lists what is supported
            assert ok in str(e.value)
    assert level_shapes((21, 77, 139), 4) == [level_shape((21, 77, 139), k) for k in range(4)]


def test_float16_mean_rounds_once():
    assert WITNESS.dtype == np.float16 and WITNESS.astype(np.float64).sum() / 8 == 1 + 2.0 ** -11 + 2.0 ** -27
    got = reduce_level(WITNESS, "mean")
    assert got.dtype == np.float16 and got.shape == (1, 1, 1)
    assert got.view(np.uint16).item() == WITNESS_MEAN_BITS == 0x3C01
    twice = (WITNESS.astype(np.float64).sum() / 8).astype(np.float32).astype(np.float16)
    assert twice.view(np.uint16).item() == WITNESS_TWICE_ROUNDED_BITS == 0x3C00  # what the rule excludes
    # subnormal results of partial blocks (count 2), both ties, to even
    tiny = np.array([[[2.0 ** -24, 0, 2.0 ** -24, 2.0 ** -23]]], np.float16)
    assert reduce_level(tiny, "mean").view(np.uint16).ravel().tolist() == [0x0000, 0x0002]  # 2^-25 -> 0 (even); 1.5 * 2^-24 -> 2 * 2^-24
    for method in ("stride", "min", "max", "median", "mode"):
        assert reduce_level(WITNESS, method).dtype == np.float16
    assert reduce_level(WITNESS, "median").item() == 1 and reduce_level(WITNESS, "mode").item() == 1
    assert reduce_level(WITNESS, "max").item() == 2 and reduce_level(WITNESS, "min").item() == 0


def test_uint32_mean_holds_its_sum_and_its_ties():
    top = np.full((2, 2, 2), 0xFFFFFFFF, np.uint32)
    assert reduce_level(top, "mean").item() == 0xFFFFFFFF and reduce_level(top, "mean").dtype == np.uint32
    assert reduce_level(np.array([[[1, 2]]], np.uint32), "mean").item() == 2   # 1.5 -> 2
    assert reduce_level(np.array([[[2, 3]]], np.uint32), "mean").item() == 2   # 2.5 -> 2
    ids = np.array([2 ** 24 + 1, 2 ** 24 + 1, 2 ** 31, 2 ** 31, 2 ** 32 - 1, 0, 1, 2 ** 24], np.uint32).reshape(2, 2, 2)
    assert reduce_level(ids, "mode").item() == 2 ** 24 + 1  # two pairs: the smaller id, which float32 cannot hold
    assert reduce_level(ids, "max").item() == 2 ** 32 - 1 and reduce_level(ids, "median").item() == 2 ** 24 + 1
    assert [lv.dtype for lv in pyramid_ref(ids, 3, "mean")] == [np.uint32] * 2


STORES = {
    "ngff04": dict(version="0.4", compressor="blosc", shards_ratio=None),
    "ngff05_sharded": dict(version="0.5", compressor={"id": "blosc", "cname": "lz4", "clevel": 1, "shuffle": 2, "blocksize": 0},
                           shards_ratio=(1, 1, 2, 1, 1)),
}


def _files(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


@pytest.mark.parametrize("dtype", [np.float16, np.uint32], ids=["float16", "uint32"])
@pytest.mark.parametrize("kind", list(STORES))
def test_initialize_pyramid_keeps_the_dtype(tmp_path, kind, dtype):
    shape = (1, 2, 13, 37, 45)
    pos = tmp_path / "plate.zarr" / "A" / "1" / "0"
    io.create_empty_plate(tmp_path / "plate.zarr", [("A", "1", "0")], ["a", "b"], shape, chunks=(1, 1, 3, 37, 45),
                          scale=(1, 1, 2.0, 0.5, 0.25), dtype=dtype, **STORES[kind])
    p = io.open_ome_zarr(pos)
    vol = np.random.default_rng(2).integers(0, 2 ** 15, shape[2:]).astype(np.uint16).view(np.float16) if dtype is np.float16 else \
        np.random.default_rng(2).integers(0, 2 ** 32, shape[2:]).astype(np.uint32)
    p.data.write_volume(0, 1, vol)
    assert np.array_equal(io.open_ome_zarr(pos).data.read_volume(0, 1).view(np.uint8), vol.view(np.uint8))
    before = {k: v for k, v in _files(pos).items() if k.startswith("0/")}
    ds0 = p.zattrs["multiscales"][0]["datasets"][0]
    p.initialize_pyramid(4)
    p = io.open_ome_zarr(pos)
    assert p.array_keys() == ["0", "1", "2", "3"]
    for k in range(1, 4):
        a = p[str(k)]
        assert a.dtype == np.dtype(dtype) and a.shape == (1, 2) + level_shape(shape[2:], k)
        assert a.zarr_format == p.data.zarr_format and a.sharded == p.data.sharded and a.fill_value == 0
        assert a._plane_chunks() is not None  # the device codec route stays open
        empty = a.read_volume(0, 1)
        assert empty.dtype == np.dtype(dtype) and not empty.view(np.uint8).any()
    assert p.zattrs["multiscales"][0]["datasets"] == expected_datasets(ds0, 4)
    assert {k: v for k, v in _files(pos).items() if k.startswith("0/")} == before
