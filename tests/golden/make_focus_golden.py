"""Writes tests/golden/focus_cases.json: the windows of tests/test_focus_host.py and tests/test_gpu_focus.py (generated from
their seeds by tests/focus_ref.py, not stored) and, per case, how far the float32 evaluation of the restatement (scipy.fft,
complex64 — the stand-in for the reference's complex64 torch pipeline) is from the float64 one:
``f32_dev = max |P32 - P64| / max P64``.  The GPU is held to a multiple of that figure (tests/test_gpu_focus.py).

Every case must be decidable by the float64 restatement alone: the top-two margin (P1 - P2) / P1 of its powers is at least
1e-3, and no bin of its plane lies within 1e-9 (relative) of either band edge.  Run from the repository root:
``python tests/golden/make_focus_golden.py``.
"""

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import focus_ref as R  # noqa: E402

CASES = [
    {"name": "min16_f32", "shape": [5, 16, 16], "dtype": "float32", "z0": 2, "pixel_size": 0.1494, "seed": 11},
    {"name": "u16_64x96", "shape": [9, 64, 96], "dtype": "uint16", "z0": 4, "pixel_size": 0.1494, "seed": 12},
    {"name": "f32_50x36", "shape": [7, 50, 36], "dtype": "float32", "z0": 3, "pixel_size": 0.25, "seed": 13},
    {"name": "i16_200x120_first", "shape": [12, 200, 120], "dtype": "int16", "z0": 0, "pixel_size": 0.1494, "seed": 14},
    {"name": "u8_96x64_last", "shape": [6, 96, 64], "dtype": "uint8", "z0": 5, "pixel_size": 0.25, "seed": 15},
    {"name": "u16_200x200", "shape": [11, 200, 200], "dtype": "uint16", "z0": 5, "pixel_size": 0.1494, "seed": 16},
    {"name": "u16_z2", "shape": [2, 32, 48], "dtype": "uint16", "z0": 1, "pixel_size": 0.2, "seed": 17},
]
MIN_MARGIN = 1e-3
EDGE_CLEARANCE = 1e-9


def main():
    out = []
    for c in CASES:
        v = R.case_window(c)
        _, Y, X = c["shape"]
        p64 = R.midband_power(v, c["pixel_size"])
        p32 = R.midband_power_f32(v, c["pixel_size"]).astype(np.float64)
        top = np.sort(p64)[::-1]
        margin = float((top[0] - top[1]) / top[0])
        frr = R.band_radius(Y, X, c["pixel_size"])
        clearance = min(float(np.abs(frr / e - 1.0).min()) for e in R.band_edges())
        focus = R.focus_index(p64)
        assert focus == c["z0"], (c["name"], focus)
        assert margin >= MIN_MARGIN, (c["name"], margin)
        assert clearance > EDGE_CLEARANCE, (c["name"], clearance)
        assert R.focus_index(p32) == focus, c["name"]
        rec = dict(c, focus=focus, n_bins=int(R.band_mask(Y, X, c["pixel_size"]).sum()), margin=margin, edge_clearance=clearance,
                   f32_dev=float(np.abs(p32 - p64).max() / p64.max()))
        print(rec)
        out.append(rec)
    (HERE / "focus_cases.json").write_text(json.dumps({"NA_det": R.NA_DET, "lambda_ill": R.LAMBDA_ILL, "midband_fractions": list(R.FRACTIONS),
                                                       "cases": out}, indent=1) + "\n")


if __name__ == "__main__":
    main()
