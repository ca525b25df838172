"""GPU: ``bh_volume_moments`` (csrc/moments.hip) against the exact restatement of tests/bleaching_ref.py, and estimate-bleaching
end to end through the store's device read paths.

Integer dtypes: every record equal, ``mean_std`` equal bit for bit to the once-rounded exact rational.  float32: each sum within
``(N + 4) * 2^-53 * sum |term|`` of the correctly rounded value, N the voxels of the call — a bound every order of float64
summation meets (N - 1 additions of relative error 2^-53 each, three roundings to form a term (x - centre)^2, one to spare) and
a float32 accumulator does not (``test_float32_bound_has_teeth``).  The wrap cases are sized from the card's compute-unit count
so that workgroups of the items kernel take a second trip through their grid-stride loop, and assert that they do.

Figures printed on an MI355X (256 compute units; got / allowed of the last slice that set the case's worst, ``-s`` shows
them).  About 0 every float32 sum came out equal to the correctly rounded value (got 0.0e+00: the values carry 24 bits and
their partial sums fit float64 exactly); about the mean:

    float32 (1, 1, 1)                    sum 0.0e+00 / 0.0e+00   sumsq 0.0e+00 / 0.0e+00
    float32 (1, 1, 67)                   sum 3.4e-12 / 4.0e-10   sumsq 0.0e+00 / 3.9e-07
    float32 (3, 5, 7)                    sum 1.8e-12 / 3.2e-10   sumsq 3.7e-09 / 3.7e-07
    float32 view big[:, 3:20, 5:72]      sum 8.4e-11 / 4.6e-07   sumsq 2.4e-07 / 4.7e-04
    float32 Z = 1, sz = 1 (1, 9, 40)     sum 2.3e-11 / 1.1e-08   sumsq 6.0e-08 / 1.1e-05
    float32 wrap (3, 2751, 67)           sum 6.3e-09 / 8.9e-03   sumsq 0.0e+00 / 9.0e+00
    float32 1000 + U(0, 100), (3, 160, 200): volume sum 0.0e+00 / 1.1e-03; N * float32 np.mean is off by 1.2e+01
    integers: every record and every mean_std equal; numpy's float64 np.mean off by 0, np.std by at most 7.3e-12
"""

import math
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import bleaching_ref as R
from biahub_amd.estimate_bleaching import mean_std, moments_plan, volume_moments

pytestmark = pytest.mark.gpu

WRAP_BLOCK_ROWS = 4
U = 2.0 ** -53


def _names(d):
    return np.dtype(d).name


def _wrap_shape(gpu):
    """(3, Y, 67) with 4-row items: Y from the card so that the 3 ceil(Y / 4) items exceed the capped grid by a few."""
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    cap = moments_plan(8, 67, WRAP_BLOCK_ROWS)[2] * cus
    return (3, WRAP_BLOCK_ROWS * (cap // 3 + 5) + 3, 67), cap


def _cases(gpu, dtype):
    """name -> (host array the view's values equal, device tensor or view, block_rows)."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    out = {}
    for shape in ((1, 1, 1), (1, 1, 67), (3, 5, 7)):
        v = R.volume(shape, dtype, seed=sum(shape))
        out[str(shape)] = (v, dev(v), 0)
    big = R.volume((4, 32, 80), dtype, seed=9)
    out["view big[:, 3:20, 5:72]"] = (big[:, 3:20, 5:72], dev(big)[:, 3:20, 5:72], 0)
    flat = R.volume((1, 9, 40), dtype, seed=8)
    out["Z = 1, sz = 1"] = (flat, torch.as_strided(dev(flat), (1, 9, 40), (1, 40, 1)), 0)
    wshape, _ = _wrap_shape(gpu)
    w = R.volume(wshape, dtype, seed=10)
    out["wrap"] = (w, dev(w), WRAP_BLOCK_ROWS)
    return out


def _hold(name, got, host, centre, n_call):
    """Records of one call against the restatement; returns the worst (got, allowed) of the two float sums."""
    want = R.exact_records(host, centre)
    is_float = host.dtype.kind == "f"
    worst = {"fsum": (0.0, 0.0), "fsumsq": (0.0, 0.0)}
    assert len(got) == len(want)
    for z, (g, w) in enumerate(zip(got, want)):
        assert (int(g["n_nan"]), int(g["n_zero"])) == (w["n_nan"], w["n_zero"]), (name, z)
        assert (float(g["min"]), float(g["max"])) == (w["min"], w["max"]), (name, z)
        if not is_float:
            assert (int(g["isum"]), int(g["isumsq"])) == (w["sum"], w["sumsq"]), (name, z)
            assert (float(g["fsum"]), float(g["fsumsq"])) == (0.0, 0.0)
            continue
        assert (int(g["isum"]), int(g["isumsq"])) == (0, 0)
        for field, key in (("fsum", "sum"), ("fsumsq", "sumsq")):
            value, mass = w[key]
            if math.isnan(value):
                assert math.isnan(float(g[field])), (name, z, field)
                continue
            err, allowed = abs(float(g[field]) - value), (n_call + 4) * U * mass
            if err >= worst[field][0]:
                worst[field] = (err, allowed)
            assert err <= allowed, (name, z, field, err, allowed)
    return worst


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_names)
def test_records_vs_restatement(gpu, dtype):
    """(1, 1, 1); one row of 67; (3, 5, 7) with x neither a vector multiple nor aligned; a strided view; Z = 1 with a plane
    stride of 1; and the wrap case.  float32 about 0 and about the mean."""
    wshape, cap = _wrap_shape(gpu)
    rows, blocks, _ = moments_plan(wshape[1], wshape[2], WRAP_BLOCK_ROWS)
    assert rows == WRAP_BLOCK_ROWS and cap < wshape[0] * blocks < 2 * cap, (
        f"{wshape}: {wshape[0] * blocks} items do not wrap a grid of {cap} workgroups once: size the case for this card")
    for name, (host, t, block_rows) in _cases(gpu, dtype).items():
        got = volume_moments(t, gpu, block_rows=block_rows)
        worst = _hold(name, got, host, 0.0, host.size)
        again = volume_moments(t, gpu, block_rows=block_rows)
        assert got.tobytes() == again.tobytes(), name
        line = f"MOMENTS gpu {_names(dtype)} {name} {host.shape}:"
        if host.dtype.kind == "f":
            m = float(np.mean(host, dtype=np.float64))
            centred = volume_moments(t, gpu, centre=m, block_rows=block_rows)
            wc = _hold(name, centred, host, m, host.size)
            assert centred.tobytes() == volume_moments(t, gpu, centre=m, block_rows=block_rows).tobytes(), name
            line += (f" sum {worst['fsum'][0]:.1e} / {worst['fsum'][1]:.1e}, sumsq {worst['fsumsq'][0]:.1e} / {worst['fsumsq'][1]:.1e};"
                     f" about the mean: sum {wc['fsum'][0]:.1e} / {wc['fsum'][1]:.1e}, sumsq {wc['fsumsq'][0]:.1e} / {wc['fsumsq'][1]:.1e}")
        else:
            exact = R.exact_mean_std(host)
            assert mean_std(t, gpu) == exact, name
            line += f" exact; np.mean off by {abs(float(np.mean(host)) - exact[0]):.1e}, np.std by {abs(float(np.std(host)) - exact[1]):.1e}"
        print(line)


def test_uploaded_numpy_equals_the_device_tensor(gpu):
    v = R.volume((3, 5, 7), np.uint16, seed=2)
    assert volume_moments(v, gpu).tobytes() == volume_moments(torch.from_numpy(v).to(gpu), gpu).tobytes()
    f = R.volume((3, 5, 7), np.float32, seed=2)
    assert volume_moments(f.astype(np.float16), gpu).tobytes() == volume_moments(f.astype(np.float16).astype(np.float32), gpu).tobytes()
    with pytest.raises(ValueError, match="not exactly representable"):
        volume_moments(torch.zeros((2, 2, 2), dtype=torch.int32, device=gpu), gpu)


@pytest.mark.parametrize("dtype,value", [(np.uint16, 65535), (np.int16, -32768), (np.uint8, 255)], ids=["uint16 max", "int16 min", "uint8 max"])
def test_overflow_edges(gpu, dtype, value):
    """(3, 160, 200) of the extreme value: 96 000 voxels, the 16-bit sums beyond 2^32 and every 16-bit square beyond 2^31."""
    v = np.full((3, 160, 200), value, dtype=dtype)
    got = volume_moments(v, gpu)
    n = 160 * 200
    for g in got:
        assert (int(g["isum"]), int(g["isumsq"]), int(g["n_zero"]), float(g["min"]), float(g["max"])) == (n * value, n * value * value, 0, value, value)
    if np.dtype(dtype).itemsize == 2:
        assert abs(3 * n * value) > 2 ** 31 and value * value > 2 ** 29 and n * value * value > 2 ** 32
    assert mean_std(v, gpu) == (float(value), 0.0) == R.exact_mean_std(v)


def test_float32_bound_has_teeth(gpu):
    """1000 + U(0, 100), 96 000 voxels: the kernel's sums are inside the bound, float32 accumulation (what np.mean does on a
    float32 array) is outside it."""
    rng = np.random.default_rng(12)
    v = (1000.0 + 100.0 * rng.random((3, 160, 200))).astype(np.float32)
    got = volume_moments(v, gpu)
    worst = _hold("teeth", got, v, 0.0, v.size)
    (value, mass), _ = R.fsum_centred(v, 0.0)
    allowed = (v.size + 4) * U * mass
    total = math.fsum(float(x) for x in got["fsum"])
    assert v.dtype == np.float32 and np.mean(v).dtype == np.float32
    f32 = abs(float(np.mean(v)) * v.size - value)  # float32 pairwise accumulation, then one float32 division
    print(f"MOMENTS gpu float32 1000 + U(0, 100) {v.shape}: slice sum {worst['fsum'][0]:.1e} / {worst['fsum'][1]:.1e}, "
          f"volume sum {abs(total - value):.1e} / {allowed:.1e}; N * float32 np.mean is off by {f32:.1e}")
    assert abs(total - value) <= allowed < f32
    m, s = mean_std(v, gpu)
    centred = R.fsum_centred(v, m)
    assert m == pytest.approx(value / v.size, rel=1e-14)
    assert s == pytest.approx(math.sqrt((centred[1][0] - centred[0][0] ** 2 / v.size) / v.size), rel=1e-13)


def test_nan_in_one_slice(gpu):
    v = R.volume((4, 17, 67), np.float32, seed=21)
    clean = volume_moments(v, gpu)
    v[2, 5, 33] = np.nan
    v[2, 16, 66] = np.nan
    got = volume_moments(v, gpu)
    _hold("nan", got, v, 0.0, v.size)
    assert int(got["n_nan"][2]) == 2 and math.isnan(got["fsum"][2]) and math.isnan(got["fsumsq"][2])
    assert math.isfinite(got["min"][2]) and math.isfinite(got["max"][2])
    keep = [0, 1, 3]
    assert got[keep].tobytes() == clean[keep].tobytes()
    allnan = np.full((2, 3, 5), np.nan, dtype=np.float32)
    rec = volume_moments(allnan, gpu)
    assert list(rec["n_nan"]) == [15, 15] and np.all(rec["min"] == np.inf) and np.all(rec["max"] == -np.inf)
    assert all(math.isnan(x) for x in mean_std(v, gpu))


def test_arguments_refused(gpu):
    from biahub_amd import _lib
    from biahub_amd.device import get_context, ptr

    ctx = get_context(gpu)
    t = torch.zeros((2, 4, 8), dtype=torch.uint16, device=gpu)
    out = np.zeros(2, dtype=volume_moments(t, gpu).dtype)
    call = lambda *a: ctx.lib.bh_volume_moments(ctx.handle, *a, out.ctypes.data)  # noqa: E731
    assert call(ptr(t), _lib.DT_U16, 2, 4, 8, 32, 4, 0.0, 0) == _lib.BH_ERR_INVALID          # row stride below X
    assert call(ptr(t), _lib.DT_U16, 2, 4, 8, 16, 8, 0.0, 0) == _lib.BH_ERR_INVALID          # planes overlap
    assert call(ptr(t), _lib.DT_F16, 2, 4, 8, 32, 8, 0.0, 0) == _lib.BH_ERR_INVALID          # dtype
    assert call(ptr(t), _lib.DT_U16, 1 << 20, 1 << 10, 1 << 10, 1 << 20, 1 << 10, 0.0, 0) == _lib.BH_ERR_INVALID  # 2^40 voxels
    assert "2**32" in _lib.last_error()
    assert call(ptr(t), _lib.DT_F32, 2, 4, 8, 32, 8, math.nan, 0) == _lib.BH_ERR_INVALID
    assert call(ptr(t), _lib.DT_U16, 2, 4, 8, 32, 8, 0.0, 0) == _lib.BH_OK


def test_get_empty_frame_indices_on_a_device_tensor(gpu):
    from biahub_amd.array_ops import get_empty_frame_indices

    v = R.empty_frames_case()
    assert get_empty_frame_indices(torch.from_numpy(v).to(gpu)) == R.empty_frames_loop(v) == [1, 2, 3, 4]
    u = R.volume((5, 4, 6), np.uint16, seed=2)
    u[u == 0] = 1
    u[[0, 3]] = 0
    assert get_empty_frame_indices(torch.from_numpy(u).to(gpu)) == get_empty_frame_indices(u, device=gpu) == [0, 3]


@pytest.fixture(scope="module")
def plate():
    return R.plate_data()


@pytest.mark.parametrize("codec", list(R.COMPRESSORS))
def test_cli_end_to_end(gpu, tmp_path, monkeypatch, plate, codec):
    """2 positions, T = 6, C = 2, (4, 32, 48) uint16 with planted decays, stored raw, Blosc-lz4 and Blosc-zstd: the Blosc stores
    reach the reduction through the device decoders.  CSV means and stds equal the exact values, the lifetimes equal curve_fit on
    those, the SVG parses."""
    from biahub_amd import io
    from biahub_amd.cli import cli, expand_eat_all

    monkeypatch.delenv("BH_BLEACHING_DEVICE", raising=False)
    uploads = []
    real = io.ZarrArray.upload_staged
    monkeypatch.setattr(io.ZarrArray, "upload_staged", lambda self, staged, device=None: (uploads.append(1), real(self, staged, device))[1])
    store = R.write_plate(tmp_path / "in.zarr", plate, R.COMPRESSORS[codec])
    out = tmp_path / "bleaching-curves"
    res = CliRunner().invoke(cli, expand_eat_all(["estimate-bleaching", "-i", *[str(store / "/".join(k)) for k in plate], "-o", str(out)]))
    assert res.exit_code == 0, res.output
    T, C = R.PLATE_SHAPE[:2]
    assert len(uploads) == (0 if codec == "raw" else len(plate) * T * C)
    for key, vol in plate.items():
        _, _, fits = R.check_position_outputs(out.joinpath(*key), vol)
        for name, (a, b, c) in R.PLATE_CURVES.items():
            assert fits[name]["fit_ok"] == "1" and abs(float(fits[name]["lifetime_minutes"]) - b) < 0.1 * b
        assert ET.parse(out.joinpath(*key) / "bleaching.svg").getroot().tag.endswith("svg")
