"""CPU: the host side of the stitch step.  The float64 restatement (tests/stitch_ref.py) against the reference's own output
(tests/golden/stitch.npz, made by tests/golden/make_stitch_golden.py), the mosaic shape and stage-position helpers against their
goldens, StitchSettings, the kernel's tile lists against brute force, the verbs' errors, estimate-stitch end to end, the C-ABI's
argument checks, and float16 arrays in the store layer."""

import ctypes as C
import json

import numpy as np
import pytest
import yaml
from click.testing import CliRunner

from conftest import GOLDEN
from stitch_ref import output_shape, seeded_fovs, stitch_ref


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "stitch.npz"), json.loads((GOLDEN / "stitch.json").read_text())


def test_restatement_equals_reference_exactly(golden):
    arrays, meta = golden
    names = [c["name"] for c in meta["cases"]]
    for want in ("grid_int_p0", "grid_int_p1", "grid_int_p2.5", "grid_frac_p0", "grid_frac_p1", "grid_frac_p2.5", "single", "identical",
                 "gap", "y2", "float32"):
        assert want in names
    for case in meta["cases"]:
        fovs = seeded_fovs(case["seed"], len(case["shifts"]), case["shape"], case["dtype"])
        got = stitch_ref(fovs, case["shifts"], case["exponent"])
        ref = arrays[case["name"]]
        assert got.dtype == np.float64 and got.shape == ref.shape == (case["shape"][0], *case["mosaic"])
        assert np.array_equal(got, ref), (case["name"], float(np.abs(got - ref).max()))
    assert not arrays["y2"].any()  # a FOV without an interior weighs nothing
    assert (arrays["gap"] == 0).any() and (arrays["gap"] != 0).any()


def test_output_shape_and_stage_positions_equal_goldens(golden):
    from biahub_amd.stitch import extract_stage_position, get_output_shape

    _, meta = golden
    for row in meta["output_shapes"]:
        assert list(get_output_shape(row["shifts"], row["tile_shape"])) == row["expected"]
        assert list(get_output_shape(list(row["shifts"].values()), row["tile_shape"])) == row["expected"]
        assert list(output_shape(row["shifts"].values(), row["tile_shape"])) == row["expected"]
    assert set(meta["stage_positions"]) == {"device_positions", "direct_keys"}
    for layout in meta["stage_positions"].values():
        attrs = {"Summary": {"StagePositions": layout["entries"]}}
        for label, want in layout["expected"].items():
            assert [float(v) for v in extract_stage_position(attrs, label)] == want, label


def test_stitch_settings(tmp_path):
    from pydantic import ValidationError

    from biahub_amd.settings import StitchSettings
    from biahub_amd.utils.config import model_to_yaml, yaml_to_model

    s = StitchSettings(total_translation={"A/1/0": [1.5, 2.25], "A/1/1": [3, 4.5, 6]})
    assert s.total_translation == {"A/1/0": [0.0, 1.5, 2.25], "A/1/1": [3.0, 4.5, 6.0]}
    assert s.channels is None and s.affine_transform is None and s.output_ome_zarr_version is None
    with pytest.raises(ValueError, match="Either affine_transform or total_translation must be provided"):
        StitchSettings(channels=["a"])
    with pytest.raises(ValueError, match="Either affine_transform"):
        StitchSettings(total_translation={}, affine_transform=None)
    assert StitchSettings(affine_transform={"A/1/0": [[1, 0], [0, 1]]}).total_translation is None
    with pytest.raises(ValidationError):
        StitchSettings(total_translation={"A/1/0": [1, 2, 3, 4]})
    with pytest.raises(ValidationError):
        StitchSettings(total_translation={"A/1/0": [1, 2]}, output_ome_zarr_version="0.3")
    with pytest.raises(ValidationError):
        StitchSettings(total_translation={"A/1/0": [1, 2]}, unknown_key=1)
    full = StitchSettings(channels=["GFP", "Phase"], total_translation={"B/2/0": [0, 0, 0], "B/2/1": [0.0, 10.25, 1843.2]},
                          output_ome_zarr_version="0.5")
    model_to_yaml(full, tmp_path / "s.yml")
    assert yaml_to_model(tmp_path / "s.yml", StitchSettings) == full
    assert "affine_transform" not in yaml.safe_load((tmp_path / "s.yml").read_text())


def _brute_lists(off, fov, origin, extent, tile, apron, grid):
    """Per tile, the FOVs (in order) with a voxel in the tile: rows [ty * tile_y, ...), columns [tx * tile_x - apron, ...) of the
    region, clipped to it; FOVs whose z range misses the region are in no list."""
    Z, Y, X = fov
    lists = []
    for ty in range(grid[0]):
        for tx in range(grid[1]):
            y0, y1 = origin[1] + ty * tile[0], origin[1] + min((ty + 1) * tile[0], extent[1])
            x0, x1 = origin[2] + max(tx * tile[1] - apron, 0), origin[2] + min((tx + 1) * tile[1], extent[2])
            lists.append([i for i, (oz, oy, ox) in enumerate(off)
                          if oz < origin[0] + extent[0] and oz + Z > origin[0] and oy < y1 and oy + Y > y0 and ox < x1 and ox + X > x0])
    return lists


def test_tile_lists_on_random_layouts(lib_built):
    from biahub_amd.stitch import build_tile_lists, get_output_shape, tile_shape

    ty, tx = tile_shape()
    rng = np.random.default_rng(42)
    seen_long = seen_empty = 0
    for trial in range(60):
        n = int(rng.integers(1, 14))
        fov = (int(rng.integers(1, 4)), int(rng.integers(1, 3 * ty)), int(rng.integers(1, 2 * tx + 40)))
        off = np.stack([rng.integers(0, 3, n), rng.integers(0, 4 * ty, n), rng.integers(0, 3 * tx, n)], 1)
        if trial % 3 == 0:  # edges on tile edges and one voxel either side
            off[:, 1] = rng.choice([0, ty - 1, ty, ty + 1, 2 * ty], n)
            off[:, 2] = rng.choice([0, tx - 1, tx, tx + 1, max(0, tx - fov[2]), max(0, tx - fov[2] + 1)], n)
        mosaic = get_output_shape(off, fov)
        if trial % 2:
            origin = tuple(int(rng.integers(0, m)) for m in mosaic)
            extent = tuple(int(rng.integers(1, m - o + 1)) for m, o in zip(mosaic, origin))
        else:
            origin, extent = (0, 0, 0), mosaic
        r = build_tile_lists(off, fov, origin, extent)
        assert r["tile"] == (ty, tx)
        grid = (-(-extent[1] // ty), -(-(extent[2] + r["apron_x"]) // tx))
        assert r["grid"] == grid and len(r["tile_off"]) == grid[0] * grid[1] + 1 and r["tile_off"][0] == 0
        want = _brute_lists(off.tolist(), fov, origin, extent, (ty, tx), r["apron_x"], grid)
        got = [r["tile_fov"][a:b].tolist() for a, b in zip(r["tile_off"][:-1], r["tile_off"][1:])]
        assert got == want, (trial, fov, off.tolist(), origin, extent)  # exactly the FOVs that meet the tile, in FOV order
        seen_long += any(len(g) > 4 for g in got)
        seen_empty += any(len(g) == 0 for g in got)
    assert seen_long and seen_empty


def test_abi_refuses_bad_arguments(lib_built):
    from biahub_amd import _lib

    lib = _lib.load()
    I3 = C.c_int64 * 3
    one = (C.c_void_p * 1)(8)
    ok = dict(n=1, fov=one, off=I3(0, 0, 0), dt=_lib.DT_U16, Z=2, Y=4, X=4, p=1.0, r0=I3(0, 0, 0), R=I3(2, 4, 4), odt=_lib.DT_F16,
              out=C.c_void_p(16))

    def call(**kw):
        a = {**ok, **kw}
        return lib.bh_stitch_blend(C.c_void_p(8), a["n"], a["fov"], a["off"], a["dt"], a["Z"], a["Y"], a["X"], a["p"], a["r0"], a["R"],
                                   a["odt"], a["out"])

    bad = [call(n=0), call(fov=None), call(fov=(C.c_void_p * 1)(None)), call(off=None), call(out=None), call(r0=None), call(R=None),
           call(Z=0), call(X=-1), call(R=I3(2, 0, 4)), call(off=I3(0, -1, 0)), call(r0=I3(0, 0, -2)), call(dt=_lib.DT_F16), call(dt=9),
           call(odt=_lib.DT_U16), call(odt=7), call(p=-0.5), call(p=float("nan")), call(p=1e6, Y=9, X=9),
           lib.bh_stitch_blend(None, 1, one, I3(0, 0, 0), _lib.DT_U16, 2, 4, 4, 1.0, I3(0, 0, 0), I3(2, 4, 4), _lib.DT_F32, C.c_void_p(16))]
    assert all(s == _lib.BH_ERR_INVALID for s in bad), bad  # every one before any device call: there is no GPU here
    assert "bh_stitch_blend" in _lib.last_error()


def test_stitch_fovs_checks_and_fails_loudly_without_gpu(lib_built):
    import torch

    from biahub_amd.stitch import placements, plan_bands, stitch_fovs

    vols = [torch.zeros((2, 4, 5), dtype=torch.uint16) for _ in range(2)]
    with pytest.raises(ValueError, match="negative shift"):
        stitch_fovs(vols, [(0, 0, 0), (0, -0.5, 3)])
    with pytest.raises(ValueError, match="2 FOVs for 1 shifts"):
        stitch_fovs(vols, [(0, 0, 0)])
    with pytest.raises(ValueError, match="blending_exponent"):
        stitch_fovs(vols, [(0, 0, 0), (0, 1, 1)], blending_exponent=-1)
    with pytest.raises(ValueError, match="share one shape"):
        stitch_fovs([vols[0], torch.zeros((2, 4, 6), dtype=torch.uint16)], [(0, 0, 0), (0, 1, 1)])
    assert placements([(0.99, 1.0, 2.5)]).tolist() == [[0, 1, 2]]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path|no GPU visible"):
            stitch_fovs(vols, [(0, 0, 0), (0, 1, 1)])
    # bands: FOVs of 100 B in two rows of a 2 x 2 grid; the whole job is 400 + mosaic
    off, fov = [(0, 0, 0), (0, 0, 8), (0, 8, 0), (0, 8, 8)], (1, 10, 10)
    assert plan_bands(off, fov, 100, 2, None) == [(0, 18)]
    assert plan_bands(off, fov, 100, 2, 400 + 18 * 18 * 2) == [(0, 18)]
    bands = plan_bands(off, fov, 100, 2, 4 * 100 + 4 * 18 * 2)  # rows 8 and 9 need all four FOVs: room for them and four mosaic rows
    assert len(bands) >= 3 and bands[0][0] == 0 and bands[-1][1] == 18 and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
    assert all(sum(o[1] < y1 and o[1] + 10 > y0 for o in off) * 100 + (y1 - y0) * 18 * 2 <= 544 for y0, y1 in bands)
    with pytest.raises(MemoryError):
        plan_bands(off, fov, 100, 2, 150)


def _stage_plate(tmp_path, version="0.4", dtype=np.uint16, shape=(1, 2, 3, 8, 10), scale=(1, 1, 2.0, 0.5, 0.25)):
    """2 wells x 2 x 2 FOVs with micro-manager stage metadata; returns (store, position paths, stage positions by FOV name)."""
    from biahub_amd import io

    store = tmp_path / "in.zarr"
    keys = [(r, c, str(f)) for r, c in (("A", "1"), ("B", "2")) for f in range(4)]
    io.create_empty_plate(store, keys, ["GFP", "Phase", "RFP"][: shape[1]], shape, chunks=(1, 1, shape[2], shape[3], shape[4]),
                          scale=scale, dtype=dtype, version=version)
    stage, entries = {}, []
    for i, k in enumerate(keys):
        f, well = i % 4, i // 4
        # (x, y) in micrometres: a 2 x 2 grid; well B is laid out wider; z differs in well B
        x = 1000.0 + (f % 2) * (2.0 + 0.5 * well) - 50 * well
        y = -300.0 + (f // 2) * (3.0 + well)
        z = 10.0 + (2.0 * f if well else 0.0)
        label = f"{k[0]}{k[1]}-Site_{f}"
        stage["/".join(k)] = (z, y, x)
        entries.append({"Label": label, "DefaultXYStage": "XY", "DefaultZStage": "Z", "XY": [x, y], "Z": z} if well else
                       {"Label": label, "DefaultXYStage": "XY", "DevicePositions": [{"Device": "XY", "Position_um": [x, y]},
                                                                                    {"Device": "Z", "Position_um": [z]}]})
        pos = io.open_ome_zarr(store.joinpath(*k))
        pos.update_zattrs({"omero": {**pos.zattrs["omero"], "name": label}})
    attrs = io._read_group_attrs(store)
    attrs["Summary"] = {"StagePositions": entries}
    io._write_group(store, io._group_format(store), attrs, version)
    return store, [store.joinpath(*k) for k in keys], stage


def _expected_translations(stage, scale_zyx, fliplr=False, flipud=False, flipxy=False):
    out = {}
    for well in sorted({k.rsplit("/", 1)[0] for k in stage}):
        names = [k for k in stage if k.startswith(well + "/")]
        a = np.array([stage[k] for k in names], np.float64)
        a = (a - a.min(axis=0)) / np.asarray(scale_zyx)
        if fliplr:
            a[:, 2] = -a[:, 2]
        if flipud:
            a[:, 1] = -a[:, 1]
        if flipxy:
            a = a[:, [0, 2, 1]]
        a = a - np.minimum(a.min(axis=0), 0)
        out.update({k: [float(v) for v in np.round(a[i], 2)] for i, k in enumerate(names)})
    return out


@pytest.mark.parametrize("version", ["0.4", "0.5"])
def test_estimate_stitch_from_stage_metadata(tmp_path, version):
    from biahub_amd.cli import cli, expand_eat_all
    from biahub_amd.settings import StitchSettings
    from biahub_amd.utils.config import yaml_to_model

    store, positions, stage = _stage_plate(tmp_path, version)
    for flags in ([], ["--fliplr"], ["--flipud", "--flipxy"], ["--fliplr", "--flipud", "--flipxy"]):
        out = tmp_path / "stitch.yml"
        res = CliRunner().invoke(cli, expand_eat_all(["estimate-stitch", "-i", *map(str, positions), "-o", str(out), *flags]))
        assert res.exit_code == 0, res.output
        raw = yaml.safe_load(out.read_text())
        assert list(raw) == ["total_translation"]
        want = _expected_translations(stage, (2.0, 0.5, 0.25), **{f[2:]: True for f in flags})
        assert raw["total_translation"] == want, flags
        assert all(v >= 0 for t in want.values() for v in t) and any(t[0] > 0 for t in want.values())
        assert yaml_to_model(out, StitchSettings).total_translation == want
    no_flip = _expected_translations(stage, (2.0, 0.5, 0.25))
    assert no_flip["A/1/3"] == [0.0, 6.0, 8.0] and no_flip["B/2/3"] == [3.0, 8.0, 10.0]


def test_verbs_refuse_what_they_do_not_do(tmp_path):
    from biahub_amd.cli import cli, expand_eat_all

    run = lambda *a: CliRunner().invoke(cli, expand_eat_all([str(x) for x in a]))  # noqa: E731
    for verb in ("stitch", "estimate-stitch"):
        res = run(verb, "--help")
        assert res.exit_code == 0 and "--input-position-dirpaths" in res.output
    assert "--blending-exponent" in run("stitch", "--help").output and "--fliplr" in run("estimate-stitch", "--help").output
    store, positions, _ = _stage_plate(tmp_path)
    res = run("estimate-stitch", "-i", *positions, "-o", tmp_path / "s.yml", "--pcc-channel-name", "GFP")
    assert res.exit_code == 2 and "reference biahub package" in res.output and not (tmp_path / "s.yml").exists()
    cfg = tmp_path / "neg.yml"
    cfg.write_text(yaml.safe_dump({"total_translation": {"A/1/0": [0, 0, 0], "A/1/1": [0, -1.5, 4]}}))
    res = run("stitch", "-i", *positions, "-c", cfg, "-o", tmp_path / "out.zarr")
    assert res.exit_code == 2 and "negative shift" in res.output and not (tmp_path / "out.zarr").exists()
    cfg = tmp_path / "affine.yml"
    cfg.write_text(yaml.safe_dump({"affine_transform": {"A/1/0": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]}}))
    res = run("stitch", "-i", *positions, "-c", cfg, "-o", tmp_path / "out.zarr")
    assert res.exit_code == 2 and "total_translation" in res.output and not (tmp_path / "out.zarr").exists()
    cfg = tmp_path / "chan.yml"
    cfg.write_text(yaml.safe_dump({"channels": ["nope"], "total_translation": {"A/1/0": [0, 0, 0]}}))
    res = run("stitch", "-i", *positions, "-c", cfg, "-o", tmp_path / "out.zarr")
    assert res.exit_code == 2 and "Invalid channel" in res.output
    cfg = tmp_path / "empty.yml"
    cfg.write_text(yaml.safe_dump({"channels": ["GFP"]}))
    res = run("stitch", "-i", *positions, "-c", cfg, "-o", tmp_path / "out.zarr")
    assert res.exit_code != 0 and "Either affine_transform or total_translation" in str(res.exception)


FLOAT16_STORES = {
    "v2_blosc_zstd": dict(version="0.4", compressor={"id": "blosc", "cname": "zstd", "clevel": 1, "shuffle": 2, "blocksize": 0},
                          shards_ratio=None),
    "v3_sharded_blosc_lz4": dict(version="0.5", compressor={"id": "blosc", "cname": "lz4", "clevel": 1, "shuffle": 2, "blocksize": 0},
                                 shards_ratio=(1, 1, 2, 1, 2)),
}


@pytest.mark.parametrize("kind", list(FLOAT16_STORES))
def test_float16_host_round_trip(tmp_path, kind):
    from biahub_amd import io

    shape = (2, 2, 13, 33, 47)
    rng = np.random.default_rng(3)
    vols = {(t, c): (rng.standard_normal(shape[2:]) * 10.0 ** rng.integers(-6, 5, shape[2:])).astype(np.float16) for t in range(2)
            for c in range(2)}
    vols[0, 0][0, 0, :6] = [np.inf, -np.inf, 0.0, -0.0, 6e-8, 65504.0]
    io.create_empty_plate(tmp_path / "p.zarr", [("A", "1", "0")], ["a", "b"], shape, chunks=(1, 1, 10, 16, 20), dtype=np.float16,
                          **FLOAT16_STORES[kind])
    arr = io.open_ome_zarr(tmp_path / "p.zarr" / "A" / "1" / "0").data
    assert arr.dtype == np.float16 and arr.chunks == (1, 1, 10, 16, 20) if not arr.sharded else arr.inner == (1, 1, 10, 16, 20)
    for (t, c), v in vols.items():
        arr.write_volume(t, c, v)
    back = io.open_ome_zarr(tmp_path / "p.zarr" / "A" / "1" / "0").data
    meta = json.loads((back.path / (".zarray" if kind.startswith("v2") else "zarr.json")).read_text())
    assert meta.get("dtype", meta.get("data_type")) in ("<f2", "float16")
    for (t, c), v in vols.items():
        got = back.read_volume(t, c)
        assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), v.view(np.uint16)), (t, c)  # bit for bit
    assert io._torch_dtype(np.float16) is not None
