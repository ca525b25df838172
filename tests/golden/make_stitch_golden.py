#!/usr/bin/env python3
"""Generate the stitch fixtures by running the *reference* (biahub/stitch.py write_output_chunk, get_output_shape;
biahub/estimate_stitch.py extract_stage_position).  Run only where the reference is mounted:

    python tests/golden/make_stitch_golden.py

Writes stitch.npz (float64 mosaics) and stitch.json (shifts, seeds, exponents, shapes, stage positions) next to this script.
Inputs are not stored: tests/stitch_ref.py seeded_fovs regenerates them.

write_output_chunk is called on duck-typed plates ({name: SimpleNamespace(data=ndarray)}, {"0": ndarray}) with one chunk
covering the mosaic and channel_idx = np.asarray([0]).  The reference module's ``np.power(..., where=d > 0)`` has no ``out=``:
where d == 0 the weight is uninitialised memory.  The module's ``np`` is wrapped here so that ``where=`` gets a zeroed ``out``
(the intent: w(0) = 0).
"""

from __future__ import annotations

import json
import sys
import types
from pathlib import Path
from types import SimpleNamespace

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from oracle.ref_import import _StubModule, load_reference, reference_available  # noqa: E402
from stitch_ref import seeded_fovs  # noqa: E402

GRID_INT = [[0, 0, 0], [0, 0, 8], [0, 6, 0], [0, 6, 8]]
GRID_FRAC = [[0, 0.4, 1.75], [1, 0.0, 9.5], [0, 6.25, 0.0], [1, 7.9, 8.01]]
CASES = [
    *[dict(name=f"grid_int_p{p}", seed=1, shifts=GRID_INT, shape=[2, 3, 16, 20], dtype="uint16", exponent=p) for p in (0, 1, 2.5)],
    *[dict(name=f"grid_frac_p{p}", seed=2, shifts=GRID_FRAC, shape=[2, 3, 16, 20], dtype="uint16", exponent=p) for p in (0, 1, 2.5)],
    dict(name="single", seed=3, shifts=[[0, 0, 0]], shape=[1, 2, 6, 7], dtype="uint16", exponent=1),
    dict(name="identical", seed=4, shifts=[[0, 1.5, 2], [0, 1.5, 2]], shape=[1, 2, 6, 7], dtype="uint16", exponent=2.5),
    dict(name="gap", seed=5, shifts=[[0, 0, 0], [0, 8, 0], [0, 0, 11]], shape=[1, 1, 5, 6], dtype="uint16", exponent=1),
    dict(name="y2", seed=6, shifts=[[0, 0, 0], [0, 1, 3]], shape=[1, 2, 2, 9], dtype="uint16", exponent=1),
    dict(name="float32", seed=7, shifts=[[0, 0, 0], [0, 2.5, 4]], shape=[1, 2, 7, 9], dtype="float32", exponent=2.5),
]

STAGE = {  # the two layouts of Summary.StagePositions entries extract_stage_position reads
    "device_positions": [
        {"Label": "A1-Site_0", "DefaultXYStage": "XYStage", "DefaultZStage": "ZDrive", "DevicePositions": [
            {"Device": "XYStage", "Position_um": [1200.5, -340.25]}, {"Device": "ZDrive", "Position_um": [15.5]},
            {"Device": "PiezoZ", "Position_um": [2.25]}]},
        {"Label": "A1-Site_1", "DefaultXYStage": "XYStage", "DevicePositions": [
            {"Device": "ZDrive", "Position_um": [7.0]}, {"Device": "XYStage", "Position_um": [-10.0, 20.0]}]},
        {"Label": "A1-Site_2", "DefaultXYStage": "", "DevicePositions": [{"Device": "ZDrive", "Position_um": [3.0]}]},
    ],
    "direct_keys": [
        {"Label": "B2-Site_0", "DefaultXYStage": "XY", "DefaultZStage": "Z", "XY": [100.0, 250.5], "Z": 12.5},
        {"Label": "B2-Site_1", "DefaultXYStage": "XY", "XY": [0.0, -3.5]},
        {"Label": "B2-Site_2", "DefaultZStage": "Z", "Z": -4.0},
    ],
}

SHAPES = [
    dict(shifts={"A/1/0": [0, 0, 0], "A/1/1": [0.0, 1843.2, 10.99], "A/1/2": [2.7, 0.5, 1843.9]}, tile_shape=[3, 2, 64, 2048, 2048]),
    dict(shifts={"B/3/7": [0, 5.5, 7.25]}, tile_shape=[16, 20, 30]),
]


class _ZeroedPower:
    """numpy, except that np.power(..., where=...) without out= starts from zeros."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def power(a, b, *args, **kw):
        if "where" in kw and "out" not in kw and not args:
            kw["out"] = np.zeros_like(np.asarray(a), dtype=np.float64)
        return np.power(a, b, *args, **kw)


def main():
    if not reference_available():
        sys.exit("the reference is not mounted here: nothing written")
    load_reference()
    for n in ("iohub.ngff.nodes", "biahub.cli.monitor", "biahub.utils.ngff"):
        if n not in sys.modules:
            m = _StubModule(n)
            m.__path__ = []
            sys.modules[n] = m
    import biahub.estimate_stitch as E
    import biahub.stitch as S

    S.np = _ZeroedPower()
    arrays, meta = {}, {"cases": [], "stage_positions": {}, "output_shapes": []}
    for case in CASES:
        T, Z, Y, X = case["shape"]
        fovs = seeded_fovs(case["seed"], len(case["shifts"]), (T, Z, Y, X), case["dtype"])
        names = [f"A/1/{i}" for i in range(len(fovs))]
        shifts = {n: tuple(s) for n, s in zip(names, case["shifts"])}
        plate = {n: SimpleNamespace(data=f[:, None]) for n, f in zip(names, fovs)}
        mosaic = S.get_output_shape(shifts, (T, 1, Z, Y, X))
        out = {"0": np.full((T, 1, *mosaic), np.nan)}
        S.write_output_chunk(tuple(slice(0, m) for m in mosaic), shifts, np.asarray([0]), plate, (T, 1, Z, Y, X), out, False,
                             blending_exponent=case["exponent"])
        res = out["0"][:, 0]
        assert res.dtype == np.float64 and not np.isnan(res).any()
        arrays[case["name"]] = res
        meta["cases"].append({**case, "mosaic": [int(m) for m in mosaic]})
    for layout, entries in STAGE.items():
        plate = SimpleNamespace(zattrs={"Summary": {"StagePositions": entries}})
        meta["stage_positions"][layout] = {"entries": entries, "expected": {
            e["Label"]: [float(v) for v in E.extract_stage_position(plate, e["Label"])] for e in entries}}
    for row in SHAPES:
        meta["output_shapes"].append({**row, "expected": [int(v) for v in S.get_output_shape(row["shifts"], tuple(row["tile_shape"]))]})
    np.savez_compressed(HERE / "stitch.npz", **arrays)
    (HERE / "stitch.json").write_text(json.dumps(meta, indent=1))
    print({p.name: p.stat().st_size for p in (HERE / "stitch.npz", HERE / "stitch.json")})


if __name__ == "__main__":
    main()
