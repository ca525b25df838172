#!/usr/bin/env python3
"""Generate the fixtures of transform validation and interpolation over time by running the *reference*
(biahub/registration/utils.py: evaluate_transforms, validate_transforms, interpolate_transforms).  Run only where the reference
is mounted:

    python tests/golden/make_eval_transforms_golden.py

Writes eval_transforms.json next to this script.  Per case the file holds the function called, its inputs (``null`` for a
timepoint without a transform), and either the reference's output or, for a case that fails, the exception's type and message.
Cases that go through ``evaluate_transforms`` also hold what ``validate_transforms`` alone returns on the same input, so that
the flagged timepoints are pinned and not only the filled list.  The reference mutates the list it is given: every call here
gets a fresh copy.
"""

from __future__ import annotations

import copy
import json
import sys
from pathlib import Path

import numpy as np
import scipy

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from oracle.ref_import import load_reference, reference_available  # noqa: E402


def translation(z=0.0, y=0.0, x=0.0):
    m = np.eye(4)
    m[:3, 3] = (z, y, x)
    return m.tolist()


def drift(T, per_t):
    return [translation(*(c * t for c in per_t)) for t in range(T)]


def similarity(t, a=None):
    """A slow rotation about z (``a`` radians when given) with a slow isotropic scale and a drift, about the origin."""
    a, s = 0.002 * t if a is None else a, 1.0 + 0.001 * t
    m = np.eye(4)
    m[1:3, 1:3] = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    m[:3, 3] = (0.0, 0.3 * t, -0.2 * t)
    return m


def cases():
    """name -> (function, kwargs).  Translations are (z, y, x)."""
    out = {}
    ev = dict(validation_window_size=3, interpolation_window_size=3, interpolation_type="linear")
    # 1. clean drift
    out["clean_drift"] = ("evaluate", dict(transforms=drift(8, (0.1, 0.5, -0.3)), shape_zyx=(16, 32, 40), validation_tolerance=3.5, **ev))
    # 2. outlier after the bootstrap window
    out["outlier_after_bootstrap"] = ("evaluate", dict(transforms=[translation(y=v) for v in (0, 1, 2, 3, 4, -9, 6, 7)],
                                                       shape_zyx=(16, 32, 40), validation_tolerance=3.5, **ev))
    # 3. an outlier at t = 5, None at t = 6; the lagging mean flags t = 7 too
    t3 = drift(8, (0.1, 0.5, -0.3))
    t3[5] = translation(0.5, 2.5 + 20.0, -1.5)
    t3[6] = None
    out["outlier_and_none"] = ("evaluate", dict(transforms=t3, shape_zyx=(16, 32, 40), validation_tolerance=2.0, **ev))
    # 4. an outlier inside the bootstrap window
    t4 = drift(10, (0.0, 0.5, 0.0))
    t4[1] = translation(y=0.5 + 12.0)
    out["outlier_in_bootstrap"] = ("evaluate", dict(transforms=t4, shape_zyx=(16, 32, 40), validation_tolerance=2.0, **ev))
    # 5. a run of None longer than the window
    t5 = drift(10, (0.0, 1.0, 0.5))
    for t in range(2, 7):
        t5[t] = None
    out["long_gap_window_1"] = ("interpolate", dict(transforms=t5, window_size=1, interpolation_type="linear"))
    # 6, 7. quadratic z drift, cubic locally against the global fit, which is linear
    t6 = [translation(z=0.01 * t * t) for t in range(12)]
    t6[6] = None
    out["cubic_local"] = ("interpolate", dict(transforms=t6, window_size=3, interpolation_type="cubic"))
    out["cubic_global_is_linear"] = ("interpolate", dict(transforms=t6, window_size=0, interpolation_type="cubic"))
    # 8. cubic with three local points
    t8 = [translation(z=0.01 * t * t) for t in range(12)]
    t8[5] = t8[6] = None
    out["cubic_three_points"] = ("interpolate", dict(transforms=t8, window_size=2, interpolation_type="cubic"))
    # 9. fewer than two valid transforms
    out["one_valid"] = ("interpolate", dict(transforms=[None, translation(y=1.0), None, None], window_size=3, interpolation_type="linear"))
    out["none_valid"] = ("interpolate", dict(transforms=[None, None, None], window_size=0, interpolation_type="linear"))
    # 10. an ndarray goes in, a list of lists comes out
    t10 = np.asarray([translation(y=v) for v in (0, 1, 2, 3, 4, -9, 6, 7)])
    out["ndarray_input"] = ("evaluate", dict(transforms=t10, shape_zyx=(16, 32, 40), validation_tolerance=3.5, **ev))
    # 11. rotation and scale on one plane: the same list, flagged or not by the extent the grid spans
    t11 = [similarity(t) for t in range(10)]
    t11[6] = similarity(6, a=0.1)  # the drift of its timepoint: only the far corners of a large plane move
    t11 = [m.tolist() for m in t11]
    out["similarity_one_plane"] = ("evaluate", dict(transforms=t11, shape_zyx=(1, 64, 48), validation_tolerance=3.0, **ev))
    out["similarity_one_plane_small"] = ("evaluate", dict(transforms=t11, shape_zyx=(1, 8, 6), validation_tolerance=3.0, **ev))
    # 12. T below a window
    out["short_for_validation"] = ("evaluate", dict(transforms=drift(2, (0.0, 1.0, 0.0)), shape_zyx=(16, 32, 40), validation_window_size=3,
                                                    validation_tolerance=100.0, interpolation_window_size=3, interpolation_type="linear"))
    out["short_for_interpolation"] = ("evaluate", dict(transforms=drift(3, (0.0, 1.0, 0.0)), shape_zyx=(16, 32, 40), validation_window_size=2,
                                                       validation_tolerance=100.0, interpolation_window_size=5, interpolation_type="linear"))
    return out


def as_json(v):
    if isinstance(v, np.ndarray):
        return {"ndarray": v.tolist()}
    return v


def main():
    if not reference_available():
        sys.exit("the reference is not mounted here: nothing written")
    load_reference()
    from biahub.registration import utils as U

    functions = {"evaluate": U.evaluate_transforms, "interpolate": U.interpolate_transforms}
    meta = {"scipy_version": scipy.__version__, "numpy_version": np.__version__, "cases": []}
    for name, (function, kwargs) in cases().items():
        case = {"name": name, "function": function, "kwargs": {k: as_json(v) for k, v in kwargs.items()}}
        try:
            out = functions[function](**copy.deepcopy(kwargs))
            assert isinstance(out, list) and all(isinstance(m, list) for m in out), name
            case["output"] = out
        except Exception as e:  # Warning is one
            case["raises"] = {"type": type(e).__name__, "message": str(e)}
        if function == "evaluate" and "output" in case:
            k = copy.deepcopy(kwargs)
            t = k["transforms"].tolist() if isinstance(k["transforms"], np.ndarray) else k["transforms"]
            validated = U.validate_transforms(transforms=t, shape_zyx=k["shape_zyx"], window_size=k["validation_window_size"],
                                              tolerance=k["validation_tolerance"])
            case["validated"] = validated
            case["flagged"] = [i for i, (a, b) in enumerate(zip(kwargs["transforms"], validated)) if a is not None and b is None]
        meta["cases"].append(case)
        print(name, case.get("flagged"), case.get("raises", ""))
    path = HERE / "eval_transforms.json"
    path.write_text(json.dumps(meta, indent=None, separators=(",", ":")))
    print(path.name, path.stat().st_size)


if __name__ == "__main__":
    main()
