"""GPU: bh_stitch_blend (csrc/stitch.hip) against the float64 restatement of the reference's blend (tests/stitch_ref.py), voxel
by voxel, and the `estimate-stitch` / `stitch` verbs end to end.

Bound of the float32 output.  The kernel computes, per voxel, acc = fma(x_i, w_i, acc) and sw += w_i over the K covering FOVs
in list order, then acc / (sw + 1e-8f), with weights w_i = float32(d ** p) and inputs that float32 holds exactly.  Roundings:
numerator: 1 (the table weight) + K (the fused multiply-adds, the first one included); denominator: 1 (the table weight) +
K - 1 (the sum) + 1 (the + 1e-8); 1 for the division: 2K + 3 factors (1 + delta), |delta| <= u = 2^-24, acting on terms of one
sign pattern, so |got - ref| <= ((1 + u)^(2K + 3) - 1) * A with A = sum_i w_i |x_i| / (sum w + 1e-8).  That is below the
(2K + 4) * 2^-24 * A of a kernel that rounds the products separately.  The restatement's own float64 error, (2K + 4) * 2^-53 * A,
is added.  float16 output: |got - ref| <= 2^-11 * (|ref| + B) + B + 2^-25, B the float32 bound (one rounding to nearest of a
value within B of ref; 2^-25 is half the spacing of float16 subnormals).
"""

import json

import numpy as np
import pytest
import torch
import yaml
from click.testing import CliRunner

from biahub_amd import io
from biahub_amd.cli import cli, expand_eat_all
from biahub_amd.stitch import get_output_shape, stitch_fovs, stitch_well, tile_shape
from stitch_ref import distance_map, stitch_ref, stitch_ref_gathered

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _bound32(K, A):
    return ((1 + U) ** (2 * K + 3) - 1) * A + (2 * K + 4) * 2.0 ** -53 * A


def _bits(t):
    """uint16 tensors as int16 (same bits): torch implements few operators for uint16."""
    return t.view(torch.int16) if t.dtype == torch.uint16 else t


def _fovs(n, shape, dtype, seed, f16_safe=False):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return [(rng.standard_normal(shape) * 1000).astype(dt) for _ in range(n)]
    info = np.iinfo(dt)
    hi = min(int(info.max), 60000) if f16_safe else int(info.max)  # float16 holds up to 65504
    return [rng.integers(info.min, hi + 1, shape).astype(dt) for _ in range(n)]


def _check(gpu, fovs, shifts, exponent, f16=True, what=""):
    """One case: float32 and float16 mosaics against the restatement, exact zeros, inputs untouched."""
    dev = [torch.from_numpy(f).to(gpu) for f in fovs]
    ref, K, A = stitch_ref(fovs, shifts, exponent, with_bound=True)
    got = stitch_fovs(dev, shifts, exponent)
    assert got.dtype == torch.float32 and got.device == dev[0].device and tuple(got.shape) == ref.shape
    g = got.cpu().numpy().astype(np.float64)
    B = _bound32(K, A)
    err = np.abs(g - ref)
    worst = float((err / np.maximum(B, 1e-300)).max()) if (B > 0).any() else 0.0
    print(f"{what}: float32 max |err| {err.max():.3e}, max err / bound {worst:.3f}, K up to {int(K.max())}")
    assert (err <= B).all(), (what, float(err.max()), worst)
    assert (g[ref == 0] == 0).all(), what  # uncovered and border-only voxels are exactly 0
    if f16:
        h = stitch_fovs(dev, shifts, exponent, torch.float16)
        assert h.dtype == torch.float16 and tuple(h.shape) == ref.shape
        h64 = h.cpu().numpy().astype(np.float64)
        err16 = np.abs(h64 - ref)
        B16 = 2.0 ** -11 * (np.abs(ref) + B) + B + 2.0 ** -25
        print(f"{what}: float16 max err / bound {float((err16 / B16).max()):.3f}")
        assert (err16 <= B16).all(), (what, float((err16 / B16).max()))
        assert (h64[ref == 0] == 0).all(), what
        # the float16 value is the float32 result rounded to nearest even
        assert np.array_equal(h.cpu().numpy().view(np.uint16), got.cpu().numpy().astype(np.float16).view(np.uint16)), what
    for d, f in zip(dev, fovs):
        assert np.array_equal(d.cpu().numpy(), f), what  # the inputs are only read
    return got


GRID = [(0, 0.4, 1.75), (1, 0.0, 13.5), (0, 9.25, 0.0), (1, 10.9, 12.01)]  # 2 x 2 with overlap, fractional shifts, a z shift


@pytest.mark.parametrize("exponent", [0, 1, 2.5])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.float32], ids=lambda d: np.dtype(d).name)
def test_grid_every_dtype_and_exponent(gpu, dtype, exponent):
    fovs = _fovs(4, (3, 16, 20), dtype, seed=1, f16_safe=True)
    if np.dtype(dtype) == np.int16:
        assert min(f.min() for f in fovs) < 0
    _check(gpu, fovs, GRID, exponent, what=f"grid {np.dtype(dtype).name} p={exponent}")


LAYOUTS = {
    "single": ((3, 16, 20), [(0, 0, 0)]),
    "grid_integer_shifts": ((3, 16, 20), [(0, 0, 0), (0, 0, 15), (0, 12, 0), (0, 12, 15)]),
    "identical_shifts": ((2, 9, 11), [(0, 1.5, 2), (0, 1.5, 2)]),
    "gap": ((2, 7, 9), [(0, 0, 0), (0, 12, 0), (0, 0, 14), (1, 13, 15)]),
    "twelve_one_voxel_apart": ((2, 30, 40), [(i % 2, i, i) for i in range(12)]),
    "taller_than_wide": ((2, 70, 24), [(0, 0, 0), (0, 3, 17), (1, 50.5, 9)]),  # dy exceeds every dx: the weight table ends at (X - 1) / 2
    "wider_than_tall": ((2, 9, 300), [(0, 0, 0), (0, 5, 131), (1, 2, 277)]),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layouts(gpu, name):
    shape, shifts = LAYOUTS[name]
    fovs = _fovs(len(shifts), shape, np.uint16, seed=2, f16_safe=True)
    got = _check(gpu, fovs, shifts, 1.0, what=name)
    if name == "gap":
        assert (got[:, 8:11, 10:13] == 0).all()
    if name == "twelve_one_voxel_apart":
        assert stitch_ref(fovs, shifts, 1.0, with_bound=True)[1].max() == 12


@pytest.mark.parametrize("shape", [(2, 2, 9), (2, 9, 1), (1, 2, 1), (3, 1, 30)], ids=str)
def test_fovs_without_interior_give_zeros(gpu, shape):
    fovs = _fovs(2, shape, np.uint16, seed=3)
    for out_dtype in (torch.float32, torch.float16):
        got = stitch_fovs([torch.from_numpy(f).to(gpu) for f in fovs], [(0, 0, 0), (0, 1, 0)], 1.0, out_dtype)
        assert tuple(got.shape) == get_output_shape([(0, 0, 0), (0, 1, 0)], shape) and not got.any()
    assert not stitch_ref(fovs, [(0, 0, 0), (0, 1, 0)], 1.0).any()


@pytest.mark.parametrize("X", [1, 5, 67, 130])
def test_vector_heads_and_tails(gpu, X):
    """Odd x offsets and widths that are no multiple of the lane's vector: rows of the mosaic start at every phase of the
    16-byte store grid, FOV rows at every phase of the load."""
    for dtype in (np.uint16, np.float32, np.uint8):
        fovs = _fovs(3, (2, 7, X), dtype, seed=X, f16_safe=True)
        _check(gpu, fovs, [(0, 0, 1), (0, 3, 0), (1, 1, 3 + X // 2 * 2)], 2.5, what=f"X={X} {np.dtype(dtype).name}")


def test_tile_edges(gpu):
    """A mosaic of more than 3 launch tiles in y and 3 in x, FOV edges on a tile edge and one voxel either side of it."""
    ty, tx = tile_shape()
    Y, X = ty + 2, tx + 8
    shifts = [(0, 0, 0), (0, ty - 1, tx), (0, ty, tx - 1), (1, ty + 1, tx + 1), (0, 2 * ty, 2 * tx - X), (0, 2 * ty - 1, 2 * tx - X + 1),
              (0, 2 * ty - Y, 2 * tx - X - 1), (1, 3 * ty - Y + 1, tx - X + 8)]
    fovs = _fovs(len(shifts), (2, Y, X), np.uint16, seed=5, f16_safe=True)
    mosaic = get_output_shape(shifts, (2, Y, X))
    assert mosaic[1] > 3 * ty and mosaic[2] > 2 * tx
    _check(gpu, fovs, shifts, 1.0, what="tile edges")


def test_regions_equal_one_launch_bit_for_bit(gpu):
    ty, tx = tile_shape()
    shape = (3, ty + 5, tx // 2 + 3)
    shifts = [(0, 0, 0), (0, 3.5, tx // 2 - 20), (1, ty - 2, 7), (0, ty + 1, tx // 2 + 1), (2, 2 * ty - 9, tx - 60)]
    fovs = [torch.from_numpy(f).to(gpu) for f in _fovs(len(shifts), shape, np.uint16, seed=6, f16_safe=True)]
    mz, my, mx = get_output_shape(shifts, shape)
    for out_dtype in (torch.float32, torch.float16):
        whole = stitch_fovs(fovs, shifts, 2.5, out_dtype)
        # y bands of unequal heights that split FOVs
        cuts = [0, 1, 8, ty - 1, ty + 6, 2 * ty + 1, my]
        bands = torch.cat([stitch_fovs(fovs, shifts, 2.5, out_dtype, region=((0, a, 0), (mz, b - a, mx))) for a, b in zip(cuts, cuts[1:])], 1)
        assert torch.equal(bands, whole)
        # boxes with odd corners in every axis
        for origin, extent in (((1, 5, 3), (2, 11, 70)), ((0, ty - 1, tx // 2 - 1), (mz, 3, mx - tx // 2 + 1)), ((2, 0, 17), (3, my, 1)),
                               ((mz - 1, my - 1, mx - 1), (1, 1, 1))):
            part = stitch_fovs(fovs, shifts, 2.5, out_dtype, region=(origin, extent))
            sl = tuple(slice(o, o + e) for o, e in zip(origin, extent))
            assert torch.equal(part, whole[sl]), (origin, extent)
    with pytest.raises(ValueError, match="negative shift"):
        stitch_fovs(fovs, [(0, 0, -1)] * len(fovs))


def _well(tmp_path, n, shape5, shifts, dtype=np.uint16, version="0.4", compressor="blosc", seed=7):
    store = tmp_path / "well_in.zarr"
    keys = [("A", "1", str(i)) for i in range(n)]
    io.create_empty_plate(store, keys, [f"c{i}" for i in range(shape5[1])], shape5, chunks=(1, 1, shape5[2], shape5[3], shape5[4]),
                          dtype=dtype, version=version, compressor=compressor)
    rng = np.random.default_rng(seed)
    data = {}
    for k in keys:
        arr = io.open_ome_zarr(store.joinpath(*k)).data
        for t in range(shape5[0]):
            for c in range(shape5[1]):
                data[k[2], t, c] = rng.integers(0, 60000, shape5[2:]).astype(dtype)
                arr.write_volume(t, c, data[k[2], t, c])
    return store, [store.joinpath(*k) for k in keys], data


def test_stitch_well_bands_equal_one_launch(gpu, tmp_path):
    shape5 = (1, 2, 3, 20, 24)
    shifts = [(0, 0, 0), (0, 0.5, 20), (0, 17, 1), (1, 20.5, 21.25), (0, 35, 3)]  # no row meets more than 3 FOVs
    _, paths, data = _well(tmp_path, 5, shape5, shifts)
    mosaic = get_output_shape(shifts, shape5)
    outs = {}
    for name, budget in (("whole", None), ("banded", 3 * 3 * 20 * 24 * 2 + mosaic[0] * 6 * mosaic[2] * 2)):
        store = tmp_path / f"{name}.zarr"
        io.create_empty_plate(store, [("A", "1", "0")], ["c1"], (1, 1, *mosaic), chunks=(1, 1, 10, 20, 24), dtype=np.float16,
                              compressor="blosc")
        info = stitch_well(paths, shifts, store / "A" / "1" / "0", channel_indices=[1], blending_exponent=2.0, max_device_bytes=budget)
        assert info["mosaic"] == mosaic and (info["bands"] == 1) == (budget is None)
        if budget is not None:
            assert info["bands"] >= 3
        outs[name] = io.open_ome_zarr(store / "A" / "1" / "0").data.read_volume(0, 0)
    assert outs["whole"].dtype == np.float16 and outs["whole"].any()
    assert np.array_equal(outs["whole"].view(np.uint16), outs["banded"].view(np.uint16))  # bit for bit
    direct = stitch_fovs([torch.from_numpy(data[str(i), 0, 1]).to(gpu) for i in range(5)], shifts, 2.0, torch.float16)
    assert np.array_equal(direct.cpu().numpy().view(np.uint16), outs["whole"].view(np.uint16))


def test_past_32_bits(gpu):
    """Two (260, 2048, 2048) uint16 FOVs, the second shifted by x = 2000: the float32 mosaic has more than 2^31 voxels.  Every corner
    and edge voxel, the seam columns and 4096 random voxels against the restatement evaluated on the gathered inputs."""
    Z, Y, X = 260, 2048, 2048
    shifts = [(0, 0, 0), (0, 0, 2000)]
    g = torch.Generator(device=gpu).manual_seed(9)
    fovs = [torch.randint(-32768, 32768, (Z, Y, X), generator=g, device=gpu, dtype=torch.int16).view(torch.uint16) for _ in range(2)]
    mz, my, mx = get_output_shape(shifts, (Z, Y, X))
    assert mz * my * mx > 2 ** 31
    pts = set()
    for z in (0, mz - 1):
        for y in (0, my - 1):
            pts.update((z, y, x) for x in range(mx))
        for x in (0, mx - 1):
            pts.update((z, y, x) for y in range(my))
    for y in (0, my - 1):
        for x in (0, mx - 1):
            pts.update((z, y, x) for z in range(mz))
    for x in (1999, 2000, 2001, 2002, 2045, 2046, 2047, 2048):  # the second FOV's first columns, the first FOV's last ones
        for z in (0, 131, mz - 1):
            pts.update((z, y, x) for y in range(0, my, 3))
    rng = np.random.default_rng(4)
    pts.update(map(tuple, np.stack([rng.integers(0, s, 4096) for s in (mz, my, mx)], 1).tolist()))
    p = np.array(sorted(pts), np.int64)
    dmap = distance_map(Y, X).astype(np.int64)
    vals, dists = np.zeros((len(p), 2)), np.full((len(p), 2), -1, np.int64)
    for i, (oz, oy, ox) in enumerate(shifts):
        q = p - np.array([oz, oy, ox])
        cov = ((q >= 0) & (q < np.array([Z, Y, X]))).all(axis=1)
        qc = torch.from_numpy(q[cov]).to(gpu)
        vals[cov, i] = _bits(fovs[i])[qc[:, 0], qc[:, 1], qc[:, 2]].cpu().numpy().view(np.uint16)
        dists[cov, i] = dmap[q[cov, 1], q[cov, 2]]
    pd = torch.from_numpy(p).to(gpu)
    for exponent in (1.0, 2.5):
        ref, A, K = stitch_ref_gathered(vals, dists, exponent)
        out = stitch_fovs(fovs, shifts, exponent)
        assert tuple(out.shape) == (mz, my, mx)
        got = out[pd[:, 0], pd[:, 1], pd[:, 2]].cpu().numpy().astype(np.float64)
        del out
        err, B = np.abs(got - ref), _bound32(K, A)
        print(f"past 32 bits p={exponent}: {len(p)} voxels, max |err| {err.max():.3e}, max err / bound "
              f"{float((err / np.maximum(B, 1e-300)).max()):.3f}")
        assert (err <= B).all() and (got[ref == 0] == 0).all()
        # both FOVs blend somewhere, and at least the seam voxels off the y border (8 columns x 3 planes x 682 rows) carry data
        assert (K == 2).any() and (ref != 0).sum() >= 8 * 3 * 682
    del fovs
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
def test_cli_end_to_end(gpu, tmp_path, kind, monkeypatch):
    shape = (2, 3, 5, 33, 47)
    scale = (1, 1, 2.0, 0.5, 0.25)
    channels = ["GFP", "Phase", "RFP"]
    wells = {"A/1": [(0, 0, 0), (0, 0, 40), (0, 29, 0), (0, 29, 40)],  # stage steps in pixels; each well its own layout
             "B/2": [(0, 0, 0), (1, 2.5, 41.25), (2, 27.75, 3), (3, 30, 44.5)]}
    keys = [(*w.split("/"), str(f)) for w in wells for f in range(4)]
    store = tmp_path / "plate.zarr"
    io.create_empty_plate(store, keys, channels, shape, chunks=(1, 1, 5, 33, 47), scale=scale, dtype=np.uint16, **PLATES[kind])
    rng = np.random.default_rng(12)
    entries, data = [], {}
    for k in keys:
        well, f = f"{k[0]}/{k[1]}", int(k[2])
        sz, sy, sx = wells[well][f]
        label = f"{k[0]}{k[1]}-Site_{f}"
        entries.append({"Label": label, "DefaultXYStage": "XY", "DefaultZStage": "Z", "XY": [500.0 + sx * scale[4], -20.0 + sy * scale[3]],
                        "Z": 7.0 + sz * scale[2]})
        pos = io.open_ome_zarr(store.joinpath(*k))
        pos.update_zattrs({"omero": {**pos.zattrs["omero"], "name": label}})
        for t in range(shape[0]):
            for c in range(shape[1]):
                data["/".join(k), t, c] = rng.integers(0, 60000, shape[2:]).astype(np.uint16)
                pos.data.write_volume(t, c, data["/".join(k), t, c])
    attrs = io._read_group_attrs(store)
    attrs["Summary"] = {"StagePositions": entries}
    io._write_group(store, io._group_format(store), attrs, PLATES[kind]["version"])
    before = _files(store)
    positions = [store.joinpath(*k) for k in keys]
    cfg = tmp_path / "stitch.yml"
    res = CliRunner().invoke(cli, expand_eat_all(["estimate-stitch", "-i", *map(str, positions), "-o", str(cfg)]))
    assert res.exit_code == 0, res.output
    raw = yaml.safe_load(cfg.read_text())
    assert raw["total_translation"] == {"/".join(k): [float(v) for v in wells[f"{k[0]}/{k[1]}"][int(k[2])]] for k in keys}
    raw["channels"] = ["RFP", "GFP"]  # a subset that is no prefix, in another order
    cfg.write_text(yaml.safe_dump(raw, sort_keys=False))
    if kind == "ngff05_lz4_sharded":
        monkeypatch.setenv("BH_ZARR_COMPRESSOR", "blosc-lz4")
    out = tmp_path / "stitched.zarr"
    res = CliRunner().invoke(cli, expand_eat_all(["stitch", "-i", *map(str, positions), "-c", str(cfg), "-o", str(out), "-b", "2", "-v"]))
    assert res.exit_code == 0, res.output
    assert "RESOURCES:" in res.output and res.output.count("Stitch complete:") == 2
    assert (tmp_path / "slurm_output" / "submitit_jobs_ids.log").read_text().split("\n") == ["stitch-0", "stitch-1"]
    shapes = set()
    for well, shifts in wells.items():
        pos = io.open_ome_zarr(out / well / "0")
        mosaic = get_output_shape(shifts, shape)
        shapes.add(mosaic)
        arr = pos.data
        assert arr.dtype == np.float16 and arr.shape == (2, 2, *mosaic)
        assert (arr.inner if arr.sharded else arr.chunks) == (1, 1, 10, 33, 47)
        assert pos.scale == [float(s) for s in scale] and pos.channel_names == ["RFP", "GFP"] and pos.version == PLATES[kind]["version"]
        assert arr.codecs and arr.codecs[0].cfg.get("cname") == ("lz4" if kind == "ngff05_lz4_sharded" else "zstd")
        for t in range(2):
            for k, c in enumerate((2, 0)):
                fovs = [data[f"{well}/{f}", t, c] for f in range(4)]
                ref, K, A = stitch_ref(fovs, shifts, 2.0, with_bound=True)
                got = arr.read_volume(t, k)
                assert got.dtype == np.float16
                B = _bound32(K, A)
                assert (np.abs(got.astype(np.float64) - ref) <= 2.0 ** -11 * (np.abs(ref) + B) + B + 2.0 ** -25).all(), (well, t, k)
                assert (got[ref == 0] == 0).all() and got.any()
                dev = arr.read_volume_device(t, k, gpu)
                assert dev.dtype == torch.float16 and np.array_equal(dev.cpu().numpy().view(np.uint16), got.view(np.uint16))
    assert len(shapes) == 2  # each well has its own mosaic
    assert _files(store) == before  # the input store is unchanged byte for byte
    meta = json.loads((out / ("zarr.json" if kind == "ngff05_lz4_sharded" else ".zattrs")).read_text())
    plate = meta["attributes"]["ome"]["plate"] if kind == "ngff05_lz4_sharded" else meta["plate"]
    assert [w["path"] for w in plate["wells"]] == ["A/1", "B/2"]
