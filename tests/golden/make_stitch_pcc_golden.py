#!/usr/bin/env python3
"""Generate the fixtures of the estimate-stitch refinement by running the *reference* (biahub/vendor/stitch: tile.py offset and
optimal_positions, _dexp_shim.py register_translation_nd, graph.py hilbert_over_points and connectivity).  Run only where the
reference is mounted:

    python tests/golden/make_stitch_pcc_golden.py

Writes stitch_pcc.json and stitch_pcc.npz next to this script.  Inputs are not stored: tests/stitch_pcc_ref.py regenerates them
from the seeds recorded here.  Per edge case the file holds the reference's shift and confidence, and the deviation of the
reference's float32 pipeline from the float64 restatement (prepared strips and shifted correlation: max |ref - restatement| /
max |restatement|; confidence: absolute), which is what the GPU tests scale their margins from.  Every case written has a peak
margin (stitch_pcc_ref.peak_margin) of at least 0.6 and, unless it is a zero-confidence case, a reference shift equal to its
displacement; a seed that falls short is replaced by the next one.

Square tiles go through ``offset``; the two non-square ones through ``register_translation_nd`` on the strips, with the nominal
offset of the right axis added here (``offset`` swaps the two extents: DESIGN.md §3.7).
"""

from __future__ import annotations

import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import scipy

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import stitch_pcc_ref as R  # noqa: E402
from oracle.ref_import import load_reference, reference_available  # noqa: E402

MIN_MARGIN = 0.6
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def _edge_specs():
    """(tile, overlap, disp, relation, zero): the table of the issue, each row for both relations.  The zero-confidence rows put
    the peak within the mask's half width of the crop's edge along one axis of the BELOW strip (48 x 64); their RIGHT twins are
    the transposed displacements on the (64 x 48) strip."""
    rows = []
    for disp in ((0, 0), (3, -5), (-4, 7), (9, 2)):
        rows.append(((64, 64), 48, disp))
    for disp in ((0, 0), (3, -5), (-4, 7)):
        rows.append(((96, 96), 32, disp))
    rows += [((75, 64), 48, (3, -5)), ((64, 75), 48, (3, -5)), ((96, 96), 33, (2, 4)), ((320, 320), 300, (5, -7)),
             ((320, 320), 300, (-6, 11))]
    specs = [(t, o, d, rel, False) for t, o, d in rows for rel in (R.BELOW, R.RIGHT)]
    for disp in ((0, -24), (-14, 0), (-16, 3)):
        specs.append(((64, 64), 48, disp, R.BELOW, True))
        specs.append(((64, 64), 48, (disp[1], disp[0]), R.RIGHT, True))
    return specs


GRAPHS = {
    "2x2": [(x, y) for x in range(2) for y in range(2)],
    "3x3": [(x, y) for x in range(3) for y in range(3)],
    "4x3": [(x, y) for x in range(4) for y in range(3)],
    "5x5": [(x, y) for x in range(5) for y in range(5)],
    "L": [(0, 0), (0, 1), (0, 2), (1, 2), (2, 2)],
    "from_001002": [(x, y) for x in range(1, 4) for y in range(2, 4)],
}

# (graph, pitch (i, j), seed of the per-tile integer errors, outlier: (edge index, (di, dj)) or None)
SOLVES = [("2x2", (20, 20), 1, None), ("3x3", (64, 64), 2, None), ("3x3", (64, 64), 3, (4, (37, -21))), ("4x3", (48, 60), 4, None),
          ("L", (30, 30), 5, None), ("from_001002", (64, 64), 6, (2, (-15, 9)))]


def main():
    if not reference_available():
        sys.exit("the reference is not mounted here: nothing written")
    load_reference()
    import torch

    from biahub.vendor.stitch import _dexp_shim as D
    from biahub.vendor.stitch import graph as G
    from biahub.vendor.stitch import tile as T

    def non_negative(roi):  # what ``offset`` does to a strip before it registers it
        roi = np.ascontiguousarray(roi)
        return roi - roi.min() if roi.min() < 0 else roi

    def ref_intermediates(sa, sb):
        pre = [D._preprocess(non_negative(r)) for r in (sa, sb)]
        win = D._hanning_window(pre[0].shape, torch.device("cpu")).numpy()
        corr = D._phase_correlation(torch.as_tensor(pre[0]), torch.as_tensor(pre[1])).numpy()
        return [p * win for p in pre], corr

    def rel_dev(got, ref):
        return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())

    meta = {"scipy_version": scipy.__version__, "numpy_version": np.__version__, "min_margin": MIN_MARGIN, "edge_cases": [],
            "graphs": {}, "solves": []}
    arrays = {}
    stored = 0
    for k, (tile, overlap, disp, rel, zero) in enumerate(_edge_specs()):
        row = k // 2  # both relations of a row share dtype and flips, so that one batch call can mix them
        dtype = ("uint16", "float32")[row % 2]
        flipud, fliplr = FLIPS[(row // 2) % 4]
        seed = 1000 + 10 * k
        while True:
            a, b = R.cut_pair(seed, tile, rel, overlap, disp, dtype, flipud, fliplr)
            rest = R.register_edge(a, b, rel, overlap, flipud, fliplr)
            fa, fb = (T.augment_tile(t, flipud=flipud, fliplr=fliplr, rot90=0) for t in (a, b))
            if tile[0] == tile[1]:
                model = T.offset(fa, fb, (0, -1) if rel == R.BELOW else (-1, 0), overlap)
                shift, conf = [int(v) for v in model.shift_vector], float(model.confidence)
            else:
                sa, sb = R.strips(a, b, rel, overlap, flipud, fliplr)
                model = D.register_translation_nd(non_negative(sa), non_negative(sb))
                nominal = (tile[0] - overlap, 0) if rel == R.BELOW else (0, tile[1] - overlap)
                shift = [int(model.shift_vector[0]) + nominal[0], int(model.shift_vector[1]) + nominal[1]]
                conf = float(model.confidence)
            margin = R.peak_margin(rest["corr"])
            nominal = (tile[0] - overlap, 0) if rel == R.BELOW else (0, tile[1] - overlap)
            right_shift = shift == [nominal[0] + disp[0], nominal[1] + disp[1]]
            if margin >= MIN_MARGIN and right_shift and (conf == 0.0) == zero and shift == list(rest["shift"]):
                break
            seed += 1
            assert seed < 1000 + 10 * k + 10, f"no seed for case {k}"
        sa, sb = R.strips(a, b, rel, overlap, flipud, fliplr)
        ref_prep, ref_corr = ref_intermediates(sa, sb)
        name = f"{tile[0]}x{tile[1]}_o{overlap}_{'below' if rel == R.BELOW else 'right'}_{disp[0]}_{disp[1]}"
        case = {"name": name, "tile": list(tile), "overlap": overlap, "disp": list(disp), "relation": rel, "dtype": dtype,
                "flipud": flipud, "fliplr": fliplr, "seed": seed, "zero_confidence": zero, "shift": shift, "confidence": conf,
                "margin": margin,
                "deviation": {"prepared": max(rel_dev(ref_prep[i], rest["prepared"][i]) for i in (0, 1)),
                              "corr": rel_dev(ref_corr, rest["corr"]), "confidence": abs(conf - rest["confidence"])},
                "stored": False}
        if tile == (64, 64) and overlap == 48 and not zero and disp != (0, 0) and stored < 2 and rel == stored:
            case["stored"] = True
            stored += 1
            arrays[name + "/prepared_a"], arrays[name + "/prepared_b"] = (p.astype(np.float32) for p in ref_prep)
            arrays[name + "/corr"] = ref_corr.astype(np.float32)
        meta["edge_cases"].append(case)
        print(name, dtype, flipud, fliplr, seed, shift, f"{conf:.4f}", f"{margin:.3f}", case["deviation"])

    for gname, cells in GRAPHS.items():
        order = G.hilbert_over_points(np.asarray(cells))
        edges = G.connectivity(order)
        meta["graphs"][gname] = {"cells": [list(c) for c in cells], "order": [[int(v) for v in p] for p in order],
                                 "edges": [[[int(v) for v in a], [int(v) for v in b]] for a, b in edges.values()]}
    for gname, pitch, seed, outlier in SOLVES:
        cells = GRAPHS[gname]
        g = meta["graphs"][gname]
        names = [f"{x:03d}{y:03d}" for x, y in cells]
        rng = np.random.default_rng(seed)
        x0, y0 = min(c[0] for c in cells), min(c[1] for c in cells)
        nominal = np.array([[(y - y0) * pitch[0], (x - x0) * pitch[1]] for x, y in cells], np.float64)
        truth = nominal + rng.integers(-4, 5, nominal.shape)
        index = {tuple(c): k for k, c in enumerate(cells)}
        shifts = [truth[index[tuple(b)]] - truth[index[tuple(a)]] for a, b in g["edges"]]
        if outlier is not None:
            shifts[outlier[0]] = shifts[outlier[0]] + np.asarray(outlier[1], np.float64)
        edge_objs = [SimpleNamespace(tile_a=names[index[tuple(a)]], tile_b=names[index[tuple(b)]],
                                     model=SimpleNamespace(shift_vector=np.asarray(s, np.float32)))
                     for (a, b), s in zip(g["edges"], shifts)]
        lut = {n: k for k, n in enumerate(names)}
        res = T.optimal_positions(edge_objs, lut, "A/1", tile_size=(pitch[0], pitch[1]),
                                  initial_guess={"A/1": {"i": nominal[:, 0].copy(), "j": nominal[:, 1].copy()}})
        meta["solves"].append({"graph": gname, "pitch": list(pitch), "seed": seed, "outlier": outlier is not None,
                               "edges": [[index[tuple(a)], index[tuple(b)], [float(v) for v in s]] for (a, b), s in zip(g["edges"], shifts)],
                               "guess_i": nominal[:, 0].tolist(), "guess_j": nominal[:, 1].tolist(),
                               "truth": (truth - truth.min(axis=0)).tolist(),
                               "positions": [res[f"A/1/{n}"] for n in names]})
    np.savez_compressed(HERE / "stitch_pcc.npz", **arrays)
    (HERE / "stitch_pcc.json").write_text(json.dumps(meta, indent=1))
    print({p.name: p.stat().st_size for p in (HERE / "stitch_pcc.npz", HERE / "stitch_pcc.json")})


if __name__ == "__main__":
    main()
