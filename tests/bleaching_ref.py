"""Cases and the exact restatement for the per-slice moments and estimate-bleaching.

Integer truth: ``np.sum(dtype=np.int64)`` per slice and Python ints across slices, so sums, mean and variance are exact
rationals; ``exact_mean_std`` rounds each once.  float32 truth: ``math.fsum`` (correctly rounded sum) over float64 terms.  The
terms of sum(x) are the float64 conversions, exact.  The terms (x - m)^2 are formed in x87 extended precision (64-bit
significand: their error is 2^-11 of a float64 rounding) and handed to fsum as two float64 pieces each.
"""

import math
import warnings

import numpy as np

DTYPES = (np.uint8, np.uint16, np.int16, np.float32)


def volume(shape, dtype, seed=0):
    """Seeded values over the dtype's whole range (float32: 1000 + U(0, 100) with signs mixed in), a few exact zeros."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        v = (1000.0 + 100.0 * rng.random(shape)).astype(np.float32)
        v[rng.random(shape) < 0.25] *= -1
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=np.int64).astype(dt)
    v[rng.random(shape) < 0.05] = 0
    return v


def exact_records(v, centre=0.0):
    """Per slice: n_nan, n_zero, min, max, and the two sums — Python ints for integer dtypes, ``(value, sum of |terms|)`` pairs
    from math.fsum for float32 (NaN when the slice holds one)."""
    v = np.asarray(v)
    out = []
    for s in v.reshape(v.shape[0], -1):
        r = {"n_zero": int(np.count_nonzero(s == 0)), "n_nan": 0}
        if v.dtype.kind == "f":
            nan = np.isnan(s)
            r["n_nan"] = int(nan.sum())
            ok = s[~nan]
            r["min"], r["max"] = (float(ok.min()), float(ok.max())) if ok.size else (math.inf, -math.inf)
            if r["n_nan"]:
                r["sum"] = r["sumsq"] = (math.nan, math.nan)
            else:
                r["sum"], r["sumsq"] = fsum_centred(s, centre)
        else:
            r["min"], r["max"] = float(s.min()), float(s.max())
            w = s.astype(np.int64)
            r["sum"] = int(np.sum(w, dtype=np.int64))
            r["sumsq"] = int(np.sum((w * w).astype(np.uint64), dtype=np.uint64))  # below 2^64 for fewer than 2^32 voxels
        out.append(r)
    return out


def fsum_centred(x, centre):
    """``((sum d, sum |d|), (sum d^2, sum d^2))`` for d = x - centre over a float32 array, correctly rounded."""
    assert np.finfo(np.longdouble).nmant >= 63, "this restatement needs x87 extended precision"
    # exact while x's last bit and the centre's are fewer than 64 bits from the larger one's first (a centre near the mean)
    d = np.asarray(x, dtype=np.float32).ravel().astype(np.longdouble) - np.longdouble(centre)

    def parts(a):
        hi = a.astype(np.float64)
        return list(hi) + list((a - hi).astype(np.float64))

    sq = d * d
    return (math.fsum(parts(d)), math.fsum(parts(np.abs(d)))), (math.fsum(parts(sq)), math.fsum(parts(sq)))


def exact_mean_std(v):
    """Integer volume: mean = S / N and std = sqrt((N Q - S^2) / N^2), each quotient rounded once (Python int division)."""
    v = np.asarray(v)
    assert v.dtype.kind in "iu"
    w = v.astype(np.int64).ravel()
    N = w.size
    S = int(np.sum(w, dtype=np.int64))
    assert N < 2 ** 32
    Q = int(np.sum((w * w).astype(np.uint64), dtype=np.uint64))
    return S / N, math.sqrt((N * Q - S * S) / (N * N))


def empty_frames_loop(v):
    """The reference's loop (biahub/utils/array_ops.py:93-99) in numpy."""
    v = np.asarray(v)
    return [z for z in range(v.shape[0]) if bool(np.all(np.isnan(v[z])) or np.all(v[z] == 0))]


def empty_frames_case():
    """(7, 5, 9) float32: slice 1 all NaN, 2 all +0, 3 all -0.0, 4 zeros and -0.0 mixed, 5 NaN and zero mixed (not empty), 6 one NaN."""
    v = volume((7, 5, 9), np.float32, seed=11)
    v[v == 0] = 1.0
    v[1] = np.nan
    v[2] = 0.0
    v[3] = -0.0
    v[4] = 0.0
    v[4, ::2] = -0.0
    v[5] = 0.0
    v[5, 2, 3:] = np.nan
    v[6, 0, 0] = np.nan
    return v


# ---- the end-to-end plate
PLATE_KEYS = (("A", "1", "0"), ("B", "2", "0"))
PLATE_SHAPE = (6, 2, 4, 32, 48)
PLATE_INTERVAL_MS = 90000
PLATE_CURVES = {"ch0": (900.0, 6.0, 400.0), "ch1": (3000.0, 3.0, 1500.0)}  # a, b (minutes), c
COMPRESSORS = {"raw": None, "lz4": {"id": "blosc", "cname": "lz4", "clevel": 1, "shuffle": 2, "blocksize": 0},
               "zstd": {"id": "blosc", "cname": "zstd", "clevel": 1, "shuffle": 2, "blocksize": 0}}


def plate_data(seed=5):
    """{position key: uint16 (T, C, Z, Y, X)}: a exp(-t / b) + c per channel plus seeded noise of sigma 40."""
    rng = np.random.default_rng(seed)
    T, C, Z, Y, X = PLATE_SHAPE
    times = np.arange(T) * (PLATE_INTERVAL_MS / 60000)
    data = {}
    for key in PLATE_KEYS:
        vol = np.empty(PLATE_SHAPE, dtype=np.uint16)
        for c, (a, b, c0) in enumerate(PLATE_CURVES.values()):
            for t in range(T):
                vol[t, c] = np.clip(np.rint(a * np.exp(-times[t] / b) + c0 + 40.0 * rng.standard_normal((Z, Y, X))), 0, 65535).astype(np.uint16)
        data[key] = vol
    return data


def write_plate(store, data, compressor=None, interval_ms=PLATE_INTERVAL_MS, dtype=np.uint16):
    """An HCS plate holding ``data``; ``Summary.Interval_ms`` in the plate attributes unless ``interval_ms`` is None."""
    from biahub_amd import io

    shape = next(iter(data.values())).shape
    io.create_empty_plate(store, list(data), list(PLATE_CURVES)[: shape[1]], shape, chunks=(1, 1) + tuple(shape[2:]), dtype=dtype, compressor=compressor)
    for key, vol in data.items():
        arr = io.open_ome_zarr(store / "/".join(key)).data
        for t in range(shape[0]):
            for c in range(shape[1]):
                arr.write_volume(t, c, vol[t, c])
    if interval_ms is not None:
        attrs = io._read_group_attrs(store)
        attrs["Summary"] = {"Interval_ms": interval_ms}
        io._write_group(store, 2, attrs, "0.4")
    return store


def read_csv(path):
    import csv

    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def check_position_outputs(out_dir, vol, interval_ms=PLATE_INTERVAL_MS):
    """The three files of one position against the exact statistics of ``vol`` (T, C, Z, Y, X integers) and a direct curve_fit."""
    import xml.etree.ElementTree as ET

    from scipy.optimize import curve_fit

    T, C = vol.shape[:2]
    names = list(PLATE_CURVES)[:C]
    times = np.arange(T) * float(np.float32(interval_ms / 60000)) if interval_ms is not None else np.arange(T) * 1.0
    rows = read_csv(out_dir / "bleaching.csv")
    assert [tuple(r) for r in rows[:1]] == [("t", "time_minutes", "channel", "mean", "std")]
    assert len(rows) == T * C
    means, stds = np.zeros((T, C)), np.zeros((T, C))
    for r in rows:
        t, c = int(r["t"]), names.index(r["channel"])
        assert float(r["time_minutes"]) == times[t]
        means[t, c], stds[t, c] = float(r["mean"]), float(r["std"])
    for t in range(T):
        for c in range(C):
            assert (means[t, c], stds[t, c]) == exact_mean_std(vol[t, c]), (t, c)
    fits = {r["channel"]: r for r in read_csv(out_dir / "bleaching_fit.csv")}
    for c, name in enumerate(names):
        y, e = means[:, c], stds[:, c]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")  # a standard deviation of 0 divides by zero inside curve_fit
            try:
                popt, _ = curve_fit(lambda x, a, b, c0: a * np.exp(-x / b) + c0, times, y, sigma=e, p0=(np.max(y) - np.min(y), 100, np.min(y)),
                                    maxfev=5000)
            except Exception:  # noqa: BLE001
                popt = None
            if popt is not None and not np.all(np.isfinite((popt[0] * np.exp(-times / popt[1]) + popt[2] - y) / e)):
                popt = None  # MINPACK returned p0 at once, which is no fit
        if popt is None:
            assert fits[name]["fit_ok"] == "0"
        else:
            assert fits[name]["fit_ok"] == "1"
            assert (float(fits[name]["a"]), float(fits[name]["lifetime_minutes"]), float(fits[name]["c"])) == tuple(float(p) for p in popt)
    root = ET.parse(out_dir / "bleaching.svg").getroot()
    assert root.tag.endswith("svg")
    return means, stds, fits
