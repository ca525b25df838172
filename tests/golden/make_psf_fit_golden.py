"""Writes tests/golden/psf_fit_cases.json: the bead cases of tests/test_psf_fit_host.py and tests/test_gpu_psf_fit.py
(settings and seeds only -- tests/psf_fit_ref.py regenerates the voxels) and, per case and fit, what the REFERENCE's
``PSF(...).analyze()`` (vendor/napari_psf_analysis, scipy curve_fit with a finite-difference Jacobian at MINPACK's default
tolerances) returns next to the TRUTH: the same model solved with the analytic Jacobian to convergence (psf_fit_ref.fit).

    ref_dev     = max_p |p_ref - p_truth| / sde_truth        how far the reference itself stops from the optimum
    ref_sde_dev = max_p |sde_ref - sde_truth| / sde_truth

The GPU is held to the largest of each per fit kind, with no extra factor (tests/test_gpu_psf_fit.py).

A case is only recorded if the restatement alone decides it: the reference raised nothing, the truth's gradient is at
rounding level, ref_dev <= 1e-2, the fitted covariance is positive definite, a truth fit started from the reference's answer
agrees with the one started from the initial guess to 1e-8 standard errors, and the restated initial guesses equal the
reference's estimators'.  Where MINPACK with the analytic Jacobian and tolerances of 1e-15 stops is printed next to it (within
1e-6 standard errors of the truth on all cases but one bead of the batch, where it leaves the basin; not asserted).

Needs the reference checkout (oracle/ref_import.py); skimage is absent, so ``skimage.measure.centroid`` is set to the
restated centroid before the reference's modules are imported.  Run from the repository root:
``python tests/golden/make_psf_fit_golden.py``.
"""

import json
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))

import psf_fit_ref as R  # noqa: E402

SP_A, SP_B = [0.25, 0.15, 0.15], [0.4, 0.2, 0.2]
BASE = {"bg": 100.0, "amp": 2000.0, "offset": 0.0, "gain": 1.0, "tilt_zx": 0.0, "tilt_yx": 0.0, "dtype": "uint16"}
CASES = [
    dict(BASE, name="p7", patch=[7, 7, 7], spacing=SP_A, sigmas=[0.28, 0.17, 0.17], seed=101),
    dict(BASE, name="p9x11x13_tilt+0.3", patch=[9, 11, 13], spacing=SP_A, sigmas=[0.4, 0.25, 0.3], tilt_zx=0.3, seed=102),
    dict(BASE, name="p8x10x12_even_f32_tilt-0.5", patch=[8, 10, 12], spacing=SP_A, sigmas=[0.35, 0.22, 0.27], tilt_zx=-0.5,
         dtype="float32", seed=103),
    dict(BASE, name="p15x18x18", patch=[15, 18, 18], spacing=SP_A, sigmas=[0.6, 0.28, 0.28], seed=104),
    dict(BASE, name="p15x18x18_f32_tilt+0.6_spB", patch=[15, 18, 18], spacing=SP_B, sigmas=[0.9, 0.35, 0.4], tilt_zx=0.6,
         dtype="float32", seed=105),
    dict(BASE, name="p17x23x29_tilts_spB", patch=[17, 23, 29], spacing=SP_B, sigmas=[1.0, 0.6, 0.8], tilt_zx=0.3, tilt_yx=0.4,
         seed=106),
    dict(BASE, name="p15x18x18_offset-100_gain0.5", patch=[15, 18, 18], spacing=SP_A, sigmas=[0.6, 0.28, 0.28], offset=-100.0,
         gain=0.5, seed=107),
    dict(BASE, name="p15x18x18_f32_offset_gain", patch=[15, 18, 18], spacing=SP_A, sigmas=[0.55, 0.3, 0.26], offset=-100.25,
         gain=0.37, tilt_yx=-0.3, dtype="float32", seed=108),
    dict(BASE, name="p15x18x18_truncated", patch=[15, 18, 18], spacing=SP_A, sigmas=[0.5, 0.28, 0.28], truncate=[3, 2, 2],
         seed=109),
]
BATCH = dict(BASE, name="batch37", volume=[48, 96, 96], patch=[15, 18, 18], slots=[2, 4, 5], count=37, spacing=SP_A,
             sigmas=[0.55, 0.27, 0.27], amp_range=[800.0, 3000.0], seed=200)
MAX_REF_DEV, START_AGREEMENT, GRAD_LEVEL = 1e-2, 1e-8, 1e-10


def load_reference():
    from oracle.ref_import import load_reference as _load

    _load()
    sys.modules["skimage.measure"].centroid = R.centroid
    from biahub.vendor.napari_psf_analysis import PSF, Calibrated3DImage
    from biahub.vendor.napari_psf_analysis.psf_analysis.fit import fitter

    return PSF, Calibrated3DImage, fitter


def reference_guess(fitter, image, kind):
    f = {"z": fitter.ZFitter, "yx": fitter.YXFitter, "zyx": fitter.ZYXFitter}[kind](image=image)
    e = f._estimator
    if kind == "z":
        return [e.get_background(), e.get_amplitude(), e.get_centroid(), e.get_sigma()]
    s = [v**2 for v in e.get_sigmas()]
    if kind == "yx":
        return [e.get_background(), e.get_amplitude(), *e.get_centroid(), s[0], 0, s[1]]
    return [e.get_background(), e.get_amplitude(), *e.get_centroid(), s[0], 0, 0, s[1], 0, s[2]]


def one_bead(ref, sample, spacing, label):
    PSF, Image, fitter = ref
    image = Image(data=sample, spacing=tuple(spacing))
    psf = PSF(image=image)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        psf.analyze()  # must not raise
    summary = psf.get_summary_dict()
    assert list(summary) == R.COLUMNS, label
    fits = {}
    for kind in R.KINDS:
        rec = np.array([summary[c] for c in R.COLS[kind]], dtype=np.float64)
        ref_p, ref_sde = rec[R.PAR_COLS[kind]], rec[R.SDE_COLS[kind]]
        p0 = R.initial_guess(sample, spacing, kind)
        g_ref = np.array(reference_guess(fitter, image, kind), dtype=np.float64)
        assert np.allclose(p0, g_ref, rtol=1e-12, atol=0), (label, kind, p0, g_ref)
        t = R.fit(kind, sample, spacing, p0)
        t2 = R.fit(kind, sample, spacing, ref_p)
        assert t["ok"] and t2["ok"], (label, kind)
        if kind == "z":  # the record keeps |sigma|; the model is even in sigma
            t["p"][3], t2["p"][3] = abs(t["p"][3]), abs(t2["p"][3])
        start_dev = float(np.max(np.abs(t["p"] - t2["p"]) / t["sde"]))
        minpack_dev = float(np.max(np.abs(R.scipy_fit(kind, sample, spacing, p0) - t["p"]) / t["sde"]))
        n = len(ref_sde)
        ref_dev = float(np.max(np.abs(ref_p - t["p"]) / t["sde"]))
        ref_sde_dev = float(np.max(np.abs(ref_sde - t["sde"][:n]) / t["sde"][:n]))
        if kind != "z":
            assert np.all(np.linalg.eigvalsh(R._cov_of(kind, t["p"])) > 0), (label, kind)
        assert np.all(R.record(kind, t["p"], t["sde"])[[R.COLS[kind].index(c) for c in R.COLS[kind] if c in R.NON_NEGATIVE]] >= 0)
        assert t["grad"] <= GRAD_LEVEL, (label, kind, t["grad"])
        assert ref_dev <= MAX_REF_DEV, (label, kind, ref_dev)
        assert start_dev <= START_AGREEMENT, (label, kind, start_dev)
        print(f"{label:36s} {kind:3s} ref_dev {ref_dev:.2e} ref_sde_dev {ref_sde_dev:.2e} starts {start_dev:.1e} minpack "
              f"{minpack_dev:.1e} grad {t['grad']:.1e} iters {t['iters']}")
        fits[kind] = dict(ref_p=ref_p.tolist(), ref_sde=ref_sde.tolist(), truth_p=t["p"].tolist(), truth_sde=t["sde"].tolist(),
                          guess=p0.tolist(), ref_dev=ref_dev, ref_sde_dev=ref_sde_dev, truth_iters=t["iters"])
    return fits


def main():
    ref = load_reference()
    cases = []
    for c in CASES:
        vol, starts, shapes = R.make_case_volume(c)
        sample = R.to_sample(R.crop(vol, starts[0], shapes[0]), c["offset"], c["gain"])
        cases.append(dict(c, crop=[int(v) for v in shapes[0]], sample_sum=int(sample.sum(dtype=np.int64)),
                          fits=one_bead(ref, sample, c["spacing"], c["name"])))
    vol, starts, shapes = R.make_batch_volume(BATCH)
    beads = []
    for i, (st, sh) in enumerate(zip(starts, shapes)):
        sample = R.to_sample(R.crop(vol, st, sh), 0.0, 1.0)
        beads.append(dict(fits=one_bead(ref, sample, BATCH["spacing"], f"batch37[{i}]")))
    # the all-zero patch of the isolation test: what does the reference do with it?
    PSF, Image, _ = ref
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            psf = PSF(image=Image(data=np.zeros(BATCH["patch"], dtype=np.int32), spacing=tuple(BATCH["spacing"])))
            psf.analyze()
            dropped = bool(np.any(np.isnan(np.array(list(psf.get_summary_dict().values()), dtype=np.float64))))
    except Exception as e:  # analyze_psf catches it, the summary becomes {} and dropna() removes the bead
        print("all-zero patch: the reference raises", type(e).__name__)
        dropped = True
    batch = dict(BATCH, volume_sum=int(vol.astype(np.int64).sum()), beads=beads, zero_patch_dropped=dropped)
    every = [c["fits"] for c in cases] + [b["fits"] for b in beads]
    bounds = {k: dict(ref_dev=max(f[k]["ref_dev"] for f in every), ref_sde_dev=max(f[k]["ref_sde_dev"] for f in every),
                      min_ref_dev=min(f[k]["ref_dev"] for f in every)) for k in R.KINDS}
    print(bounds, "zero patch dropped:", dropped)
    (HERE / "psf_fit_cases.json").write_text(json.dumps({"columns": R.COLUMNS, "bounds": bounds, "cases": cases, "batch": batch},
                                                        indent=1) + "\n")


if __name__ == "__main__":
    main()
