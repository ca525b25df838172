"""GPU: bh_pyramid_downsample (csrc/pyramid.hip) bit-exact against the numpy restatement (tests/pyramid_ref.py) for every
method x dtype over awkward shapes and level counts (launches of depth 1, 2, 3 and chained launches), at full size through
aligned 8x8x8 source cubes, and the `pyramid` verb end to end on NGFF 0.4 Blosc-zstd and sharded 0.5 Blosc-lz4 plates."""

import json

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from biahub_amd import io
from biahub_amd.cli import cli, expand_eat_all
from biahub_amd.pyramid import downsample_pyramid
from pyramid_ref import METHODS, expected_datasets, level_shape, pyramid_ref

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16, np.int16, np.float32)
SHAPES = ((1, 1, 1), (1, 5, 7), (5, 7, 9), (17, 33, 65), (8, 64, 1001), (33, 130, 257))
LEVELS = (2, 3, 4, 5, 7)


def _bits(t):
    """uint16 tensors as int16 (same bits): torch implements few operators for uint16."""
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _volume(shape, dtype, method, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if method in ("mode", "median"):  # few distinct values: ties and repeats in most blocks
        v = rng.integers(0, 4, shape) * 3 - (4 if dt.kind == "i" else 0)
    elif dt.kind == "f":
        v = rng.standard_normal(shape) * 100
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, int(info.max) + 1, shape)
    return v.astype(dt)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
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
                if not np.array_equal(h, r):
                    bad = np.argwhere(h != r)
                    pytest.fail(f"{method} {np.dtype(dtype).name} {shape} levels={levels} level {k}: {len(bad)} voxels differ, "
                                f"first {tuple(bad[0])}: {h[tuple(bad[0])]} != {r[tuple(bad[0])]}")
        assert np.array_equal(dv.cpu().numpy(), vol)  # the input is only read


@pytest.mark.parametrize("method", ["mean", "median", "mode"])
def test_chained_launches_equal_single_steps(gpu, method):
    vol = _volume((37, 70, 131), np.uint16, method, seed=7)
    dv = torch.from_numpy(vol).to(gpu)
    seven = downsample_pyramid(dv, 7, method)
    src, steps = dv, []
    for _ in range(6):
        before = _bits(src).clone()
        (nxt,) = downsample_pyramid(src, 2, method)
        assert torch.equal(_bits(src), before)  # the input is unchanged
        steps.append(nxt)
        src = nxt
    for a, b in zip(seven, steps):
        assert torch.equal(_bits(a), _bits(b))
    four = downsample_pyramid(dv, 4, method)
    more = downsample_pyramid(four[-1], 4, method)
    for a, b in zip(seven, four + more):
        assert torch.equal(_bits(a), _bits(b))
    assert np.array_equal(dv.cpu().numpy(), vol)


def _edge_and_random_voxels(shape, n, seed):
    """Every corner and edge voxel of a (Z, Y, X) box, plus n random ones: (m, 3) int64."""
    Z, Y, X = shape
    pts = set()
    for z in (0, Z - 1):
        for y in (0, Y - 1):
            pts.update((z, y, x) for x in range(X))
        for x in (0, X - 1):
            pts.update((z, y, x) for y in range(Y))
    for y in (0, Y - 1):
        for x in (0, X - 1):
            pts.update((z, y, x) for z in range(Z))
    rng = np.random.default_rng(seed)
    pts.update(map(tuple, np.stack([rng.integers(0, s, n) for s in shape], 1).tolist()))
    return np.array(sorted(pts), np.int64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint16], ids=["float32", "uint16"])
def test_full_size_through_source_cubes(gpu, dtype):
    shape = (512, 2048, 2048)  # 2^31 voxels: offsets past 32 bits
    g = torch.Generator(device=gpu).manual_seed(5)
    if dtype == torch.float32:
        dv = torch.rand(shape, generator=g, device=gpu, dtype=torch.float32) * 1000
    else:
        dv = torch.randint(-32768, 32768, shape, generator=g, device=gpu, dtype=torch.int16).view(torch.uint16)
    pts = _edge_and_random_voxels(level_shape(shape, 3), 4096, seed=3)
    p = torch.from_numpy(pts).to(gpu)
    o = torch.arange(8, device=gpu)
    # the 8x8x8 source cube of every checked level-3 voxel (the volume's extents are multiples of 8: all cubes are whole)
    zi = (p[:, 0, None] * 8 + o)[:, :, None, None]
    yi = (p[:, 1, None] * 8 + o)[:, None, :, None]
    xi = (p[:, 2, None] * 8 + o)[:, None, None, :]
    np_dt = np.float32 if dtype == torch.float32 else np.uint16
    cubes = _bits(dv)[zi, yi, xi].cpu().numpy().view(np_dt)
    for method in ("mean", "median"):
        lv = downsample_pyramid(dv, 4, method)
        assert [tuple(t.shape) for t in lv] == [level_shape(shape, k) for k in (1, 2, 3)]
        got = _bits(lv[2])[p[:, 0], p[:, 1], p[:, 2]].cpu().numpy().view(np_dt)
        want = pyramid_ref(cubes, 4, method)[-1].reshape(-1)
        assert np.array_equal(got, want), (method, int((got != want).sum()))
        # level 1 and 2 at the far corner, too
        c1 = _bits(dv)[-2:, -2:, -2:].cpu().numpy().view(np_dt)
        assert _bits(lv[0])[-1:, -1:, -1:].cpu().numpy().view(np_dt).item() == pyramid_ref(c1, 2, method)[0].item()
        del lv
    torch.cuda.empty_cache()


PLATES = {
    "ngff04_zstd": dict(version="0.4", compressor={"id": "blosc", "cname": "zstd", "clevel": 1, "shuffle": 2, "blocksize": 0},
                        shards_ratio=None),
    "ngff05_lz4_sharded": dict(version="0.5", compressor={"id": "blosc", "cname": "lz4", "clevel": 1, "shuffle": 2,
                                                          "blocksize": 0}, shards_ratio=(1, 1, 2, 1, 1)),
}


def _files(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


@pytest.mark.parametrize("kind", list(PLATES))
def test_cli_end_to_end(gpu, tmp_path, kind):
    shape = (2, 2, 21, 77, 139)
    keys = [("A", "1", "0"), ("B", "2", "0")]
    store = tmp_path / "plate.zarr"
    io.create_empty_plate(store, keys, ["a", "b"], shape, chunks=(1, 1, 4, shape[3], shape[4]), scale=(1, 1, 2.0, 0.5, 0.5),
                          dtype=np.uint16, **PLATES[kind])
    rng = np.random.default_rng(11)
    positions = [store.joinpath(*k) for k in keys]
    for pos in positions:
        arr = io.open_ome_zarr(pos).data
        for t in range(2):
            for c in range(2):
                arr.write_volume(t, c, (rng.poisson(3, shape[2:]) + 100 * c).astype(np.uint16))
    level0 = {str(p): {k: v for k, v in _files(p).items() if k.startswith("0/")} for p in positions}
    attrs0 = {str(p): io.open_ome_zarr(p).zattrs for p in positions}
    for method in ("mean", "mode"):
        res = CliRunner().invoke(cli, expand_eat_all(["pyramid", "-i", *map(str, positions), "--levels", "4", "-m", method]))
        assert res.exit_code == 0, res.output
        assert "RESOURCES:" in res.output and res.output.count("Computing pyramid for FOV:") == 2
        for pos in positions:
            p = io.open_ome_zarr(pos)
            assert p.array_keys() == ["0", "1", "2", "3"]
            assert p.zattrs["multiscales"][0]["datasets"] == expected_datasets(attrs0[str(pos)]["multiscales"][0]["datasets"][0], 4)
            for t in range(2):
                for c in range(2):
                    ref = pyramid_ref(p.data.read_volume(t, c), 4, method)
                    for k in range(1, 4):
                        got = p[str(k)].read_volume(t, c)
                        assert got.dtype == np.uint16 and np.array_equal(got, ref[k - 1]), (method, str(pos), t, c, k)
            dev = p["2"].read_volume_device(1, 1, gpu)
            assert np.array_equal(dev.cpu().numpy(), pyramid_ref(p.data.read_volume(1, 1), 3, method)[1])
            assert {k: v for k, v in _files(pos).items() if k.startswith("0/")} == level0[str(pos)]
    log = json.dumps(sorted(x.name for x in tmp_path.iterdir()))
    assert "slurm_output" in log
