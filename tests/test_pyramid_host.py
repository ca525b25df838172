"""CPU: the pyramid semantics (tests/pyramid_ref.py against hand-worked blocks), the store layer's initialize_pyramid on NGFF 0.4,
0.5 and sharded 0.5 stores, the `pyramid` verb's host side, and bh_pyramid_downsample's argument checks."""

import ctypes as C
import json

import numpy as np
import pytest
from click.testing import CliRunner

from biahub_amd import io
from biahub_amd.cli import cli, expand_eat_all
from pyramid_ref import expected_datasets, level_shape, pyramid_ref, reduce_level


# ---- the restatement against hand-worked blocks -------------------------------------------------------------------------
def test_partial_blocks_of_1_2_4_8_elements():
    a = np.arange(1, 28, dtype=np.uint16).reshape(3, 3, 3)  # a[z, y, x] = 9z + 3y + x + 1; level 1 is (2, 2, 2)
    lv = reduce_level(a, "mean")
    assert lv.shape == (2, 2, 2)
    assert lv[0, 0, 0] == 8    # 8 elements: 1 2 4 5 10 11 13 14 = 60 -> 7.5 -> 8 (ties to even)
    assert lv[1, 0, 0] == 21   # 4 elements: 19 20 22 23 = 84 -> 21
    assert lv[1, 1, 0] == 26   # 2 elements: 25 26 -> 25.5 -> 26
    assert lv[1, 1, 1] == 27   # 1 element
    assert lv[0, 1, 1] == 14   # 2 elements, along z: 9 18 -> 13.5 -> 14
    assert reduce_level(a, "max")[1, 1, 0] == 26 and reduce_level(a, "min")[1, 1, 0] == 25
    assert reduce_level(a, "stride")[1, 1, 1] == 27


def test_integer_ties_to_even():
    u = np.array([[[2, 3, 3, 4]]], np.uint16)  # blocks of 2: 2.5 -> 2, 3.5 -> 4
    assert reduce_level(u, "mean").ravel().tolist() == [2, 4]
    s = np.array([[[-2, -3, -3, -4, -1, -2, 1, 2]]], np.int16)  # -2.5 -> -2, -3.5 -> -4, -1.5 -> -2, 1.5 -> 2
    assert reduce_level(s, "mean").ravel().tolist() == [-2, -4, -2, 2]
    eights = {(1, 0, 0, 0, 0, 0, 1, 1): 0,   # 3 / 8 = 0.375
              (1, 1, 1, 1, 1, 0, 0, 0): 1,   # 5 / 8 = 0.625
              (1, 1, 1, 1, 0, 0, 0, 0): 0,   # 4 / 8 = 0.5, to even
              (1, 2, 1, 2, 1, 2, 1, 2): 2}   # 12 / 8 = 1.5, to even
    for vals, want in eights.items():
        assert reduce_level(np.array(vals, np.uint8).reshape(2, 2, 2), "mean").item() == want, vals


def test_float_mean_sums_in_float64_in_order():
    v = np.array([1e8, 1, -1e8, 1, 3, 0.5, 0.25, 0.125], np.float32).reshape(2, 2, 2)
    want = np.float32((((((((0.0 + 1e8) + 1) + -1e8) + 1) + 3) + 0.5) + 0.25 + 0.125) / 8)
    assert reduce_level(v, "mean").item() == want
    assert reduce_level(v, "mean").dtype == np.float32


def test_lower_medians():
    assert reduce_level(np.array([[[5, 1]]], np.uint16), "median").item() == 1          # 2 elements: the lower
    assert reduce_level(np.array([[[4, 1], [3, 2]]], np.int16), "median").item() == 2    # 4: sorted[1]
    eight = np.array([8, 7, 6, 5, 4, 3, 2, 1], np.float32).reshape(2, 2, 2)
    assert reduce_level(eight, "median").item() == 4                                     # 8: sorted[3]
    assert reduce_level(np.array([[[9]]], np.uint8), "median").item() == 9


def test_mode_ties_take_the_smallest():
    assert reduce_level(np.array([3, 3, 1, 1, 2, 2, 5, 7], np.uint8).reshape(2, 2, 2), "mode").item() == 1
    assert reduce_level(np.array([9, 9, 9, 4, 4, 4, 7, 7], np.int16).reshape(2, 2, 2), "mode").item() == 4
    assert reduce_level(np.array([-5, 2, 2, -5, 2, 0, 0, 0], np.int16).reshape(2, 2, 2), "mode").item() == 0
    assert reduce_level(np.array([[[6, 5]]], np.uint16), "mode").item() == 5  # two singletons
    assert reduce_level(np.array([1.5, 2, 3, 4, 5, 6, 7, 1.5], np.float32).reshape(2, 2, 2), "mode").item() == 1.5


def test_stride_is_slicing():
    a = np.random.default_rng(0).integers(0, 1000, (13, 22, 37)).astype(np.uint16)
    for k, lv in enumerate(pyramid_ref(a, 6, "stride"), start=1):
        np.testing.assert_array_equal(lv, a[:: 2 ** k, :: 2 ** k, :: 2 ** k])
        assert lv.shape == level_shape(a.shape, k)


def test_cascade_differs_from_a_direct_mean():
    # seven 2x2x2 blocks sum to 4 (mean 0.5 -> 0), one to 12 (1.5 -> 2): the cascade gives mean(0 x 7, 2) = 0.25 -> 0,
    # while the 4x4x4 mean of level 0 is 40 / 64 = 0.625 -> 1
    a = np.zeros((4, 4, 4), np.uint8)
    for bz in range(2):
        for by in range(2):
            for bx in range(2):
                # the block's first z plane: four elements
                a[2 * bz, 2 * by:2 * by + 2, 2 * bx:2 * bx + 2] = 3 if (bz, by, bx) == (1, 1, 1) else 1
    blk = a[2:, 2:, 2:]
    assert a.sum() == 40 and blk.sum() == 12
    lv1, lv2 = pyramid_ref(a, 3, "mean")
    assert lv1.ravel().tolist() == [0] * 7 + [2]
    assert lv2.item() == 0 and round(a.sum() / 64) == 1


def test_axis_of_one_stays_one():
    a = np.arange(10, dtype=np.float32).reshape(1, 1, 10)
    shapes = [lv.shape for lv in pyramid_ref(a, 5, "max")]
    assert shapes == [(1, 1, 5), (1, 1, 3), (1, 1, 2), (1, 1, 1)]
    assert pyramid_ref(a, 5, "max")[-1].item() == 9


# ---- the store layer ------------------------------------------------------------------------------------------------------
STORES = {
    "ngff04": dict(version="0.4", compressor="blosc", shards_ratio=None),
    "ngff05": dict(version="0.5", compressor="blosc", shards_ratio=None),
    "ngff05_sharded": dict(version="0.5", compressor={"id": "blosc", "cname": "lz4", "clevel": 1, "shuffle": 2, "blocksize": 0},
                           shards_ratio=(1, 1, 2, 1, 1)),
}


def _files(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def _store(tmp_path, kind, shape=(2, 2, 13, 37, 45), dtype=np.uint16, zc=3):
    cfg = STORES[kind]
    pos = tmp_path / kind / "A" / "1" / "0"
    io.create_empty_plate(tmp_path / kind, [("A", "1", "0")], ["a", "b"], shape, chunks=(1, 1, zc, shape[3], shape[4]),
                          scale=(1, 1, 2.0, 0.5, 0.25), dtype=dtype, **cfg)
    p = io.open_ome_zarr(pos)
    ms = p.zattrs["multiscales"]
    ms[0]["datasets"][0]["coordinateTransformations"].append({"type": "translation", "translation": [0, 0, 1.5, -2.0, 3.0]})
    p.update_zattrs({"multiscales": ms})
    rng = np.random.default_rng(1)
    for t in range(shape[0]):
        for c in range(shape[1]):
            p.data.write_volume(t, c, rng.integers(0, 9, shape[2:]).astype(dtype))
    return pos


@pytest.mark.parametrize("kind", list(STORES))
def test_initialize_pyramid_metadata(tmp_path, kind):
    pos = _store(tmp_path, kind)
    before = {k: v for k, v in _files(pos).items() if k.startswith("0/")}
    attrs0 = io.open_ome_zarr(pos).zattrs
    p = io.open_ome_zarr(pos)
    p.initialize_pyramid(4)
    p = io.open_ome_zarr(pos)
    a0 = p.data
    assert p.array_keys() == ["0", "1", "2", "3"]
    for k in range(1, 4):
        a = p[str(k)]
        assert a.shape == (2, 2) + level_shape((13, 37, 45), k)
        assert a.inner == tuple(-(-c // 2 ** k) for c in a0.inner)
        assert [c // i for c, i in zip(a.chunks, a.inner)] == [c // i for c, i in zip(a0.chunks, a0.inner)]  # shards ratio
        assert a.dtype == a0.dtype and a.fill_value == 0 and a.zarr_format == a0.zarr_format
        assert a.sharded == a0.sharded
        assert [(c.kind, c.cfg) for c in a.codecs] == [(c.kind, c.cfg) for c in a0.codecs]
        assert a._plane_chunks() is not None  # plane-stack chunks: the device codec route stays open
        if a0.zarr_format == 2:
            m0 = json.loads((a0.path / ".zarray").read_text())
            m = json.loads((a.path / ".zarray").read_text())
            assert m["compressor"] == m0["compressor"]
        else:
            m0 = json.loads((a0.path / "zarr.json").read_text())
            m = json.loads((a.path / "zarr.json").read_text())
            strip = lambda cs: json.dumps(cs).replace(json.dumps(list(a0.inner)), "I").replace(json.dumps(list(a.inner)), "I")
            assert strip(m["codecs"]) == strip(m0["codecs"])
        assert not [f for f in a.path.rglob("*") if f.is_file() and f.name not in (".zarray", "zarr.json")]
    ds = p.zattrs["multiscales"][0]["datasets"]
    want = expected_datasets(attrs0["multiscales"][0]["datasets"][0], 4)
    assert ds == want
    assert ds[3]["coordinateTransformations"][0]["scale"] == [1, 1, 16.0, 4.0, 2.0]
    assert ds[2]["coordinateTransformations"][1] == {"type": "translation", "translation": [0, 0, 1.5, -2.0, 3.0]}
    rest = {k: v for k, v in p.zattrs.items() if k != "multiscales"}
    assert rest == {k: v for k, v in attrs0.items() if k != "multiscales"}
    assert {k: v for k, v in p.zattrs["multiscales"][0].items() if k != "datasets"} == \
        {k: v for k, v in attrs0["multiscales"][0].items() if k != "datasets"}
    assert {k: v for k, v in _files(pos).items() if k.startswith("0/")} == before  # level 0 byte for byte
    # a re-run with fewer levels deletes the arrays above and their dataset entries
    (p.path / "3" / "marker").write_bytes(b"x")
    p.initialize_pyramid(2)
    p = io.open_ome_zarr(pos)
    assert p.array_keys() == ["0", "1"] and not (pos / "2").exists() and not (pos / "3").exists()
    assert p.zattrs["multiscales"][0]["datasets"] == want[:2]
    assert {k: v for k, v in _files(pos).items() if k.startswith("0/")} == before


def test_pyramid_checks_before_any_device_work(tmp_path):
    import torch

    from biahub_amd.pyramid import check_args, downsample_pyramid

    with pytest.raises(ValueError, match="int32"):
        check_args(np.int32, 4, "mean")
    with pytest.raises(ValueError, match="float64"):
        downsample_pyramid(torch.zeros((2, 2, 2), dtype=torch.float64), 3, "mean")
    with pytest.raises(ValueError, match="method 'bilinear'"):
        check_args(np.uint16, 4, "bilinear")
    pos = tmp_path / "p"
    io.create_empty_position(pos, ["a"], (1, 1, 4, 4, 4), dtype=np.int32)
    files = _files(pos)
    with pytest.raises(ValueError, match="int32"):
        io.open_ome_zarr(pos).compute_pyramid(3, "mean")
    assert _files(pos) == files
    if not torch.cuda.is_available():  # no CPU path: the store is left alone
        pos = _store(tmp_path, "ngff04")
        files = _files(pos)
        with pytest.raises(RuntimeError, match="no GPU visible"):
            io.open_ome_zarr(pos).compute_pyramid(3, "mean")
        assert _files(pos) == files


# ---- the verb -------------------------------------------------------------------------------------------------------------
def test_cli_help_lists_the_verb_and_options():
    r = CliRunner()
    res = r.invoke(cli, ["--help"])
    assert res.exit_code == 0 and "pyramid" in res.output
    res = r.invoke(cli, ["pyramid", "--help"])
    assert res.exit_code == 0, res.output
    for opt in ("-i, --input-position-dirpaths", "-sb, --sbatch-filepath", "-l, --local", "-lv, --levels", "-m, --method",
                "stride|median|mode|mean|min|max", "default: 4", "default: mean"):
        assert opt in res.output, opt
    assert "--output-dirpath" not in res.output and "--monitor" not in res.output


def test_cli_levels_one_leaves_the_store_alone(tmp_path):
    pos = _store(tmp_path, "ngff04")
    files = _files(tmp_path)
    for lv in ("1", "0"):
        res = CliRunner().invoke(cli, expand_eat_all(["pyramid", "-i", str(pos), "--levels", lv]))
        assert res.exit_code == 0, res.output
        assert "No pyramid levels to create (levels must be > 1)." in res.output
        assert "RESOURCES:" not in res.output
    assert _files(tmp_path) == files


def test_cli_refuses_an_unknown_method(tmp_path):
    pos = _store(tmp_path, "ngff04")
    files = _files(tmp_path)
    res = CliRunner().invoke(cli, ["pyramid", "-i", str(pos), "-m", "bilinear"])
    assert res.exit_code == 2 and "Invalid value" in res.output and "bilinear" in res.output
    assert _files(tmp_path) == files


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_pyramid_abi_refuses_bad_arguments(lib_built):
    from biahub_amd import _lib

    lib = _lib.load()
    outs = (C.c_void_p * 3)()
    cases = [
        (dict(method=17), "method"),
        (dict(dtype=9), "dtype code 9"),
        (dict(n=0), "n = 0"),
        (dict(Z=0), "bad shape"),
        ({}, "null"),
    ]
    for kw, msg in cases:
        a = dict(dtype=_lib.DT_U16, Z=4, Y=4, X=4, method=_lib.DS_MEAN, n=2)
        a.update(kw)
        s = lib.bh_pyramid_downsample(None, None, a["dtype"], a["Z"], a["Y"], a["X"], a["method"], a["n"], outs)
        assert s == _lib.BH_ERR_INVALID, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
