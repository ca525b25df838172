"""Float64 restatement of the bead fits of ``characterize-psf`` -- test infrastructure, NumPy/SciPy only.

What the reference does per bead (biahub/characterize_psf.py:236-246 -> vendor/napari_psf_analysis): the sample is
``np.clip((patch + offset) * gain, 0, None).astype(np.int32)``; three Gaussians are fitted with ``scipy.optimize.curve_fit``
(MINPACK, finite-difference Jacobian, tolerances 1.49e-8) from initial guesses formed in ``fit/estimator.py``.  Here:

* ``make_case_volume`` / ``make_batch_volume``: the seeded bead generator (Poisson noise on bg + amp exp(-d' C^-1 d / 2), with
  sub-voxel centre offsets).  Fixtures keep only settings and seeds; the voxels are regenerated, and ``sample_sum`` pins them.
* ``initial_guess``: the reference's guesses (``skimage.measure.centroid`` is sum(i w) / sum(w)).
* ``fit``: the TRUTH -- the same models, solved with the ANALYTIC Jacobian by a plain NumPy Levenberg-Marquardt until the
  undamped Gauss-Newton step is below 1e-9 standard errors.  The fixture's maker cross-checks it against
  ``scipy.optimize.least_squares(method="lm", jac=analytic, xtol=ftol=gtol=1e-15)`` and against a second start.
* ``record``: a fit's columns in the order of the reference's ``get_summary_dict()``.
"""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "psf_fit_cases.json"
KINDS = ("z", "yx", "zyx")
NPAR = {"z": 4, "yx": 7, "zyx": 11}
FWHM = 2 * np.sqrt(2 * np.log(2))

Z_COLS = ["z_bg", "z_amp", "z_mu", "z_sigma", "z_fwhm", "z_bg_sde", "z_amp_sde", "z_mu_sde", "z_sigma_sde"]
YX_COLS = ["yx_bg", "yx_amp", "y_mu", "x_mu", "yx_cyy", "yx_cyx", "yx_cxx", "y_fwhm", "x_fwhm", "yx_pc1_fwhm", "yx_pc2_fwhm",
           "yx_bg_sde", "yx_amp_sde", "y_mu_sde", "x_mu_sde", "yx_cyy_sde", "yx_cyx_sde", "yx_cxx_sde"]
ZYX_COLS = ["zyx_bg", "zyx_amp", "zyx_z_mu", "zyx_y_mu", "zyx_x_mu", "zyx_czz", "zyx_czy", "zyx_czx", "zyx_cyy", "zyx_cyx",
            "zyx_cxx", "zyx_z_fwhm", "zyx_y_fwhm", "zyx_x_fwhm", "zyx_pc1_fwhm", "zyx_pc2_fwhm", "zyx_pc3_fwhm", "zyx_bg_sde",
            "zyx_amp_sde", "zyx_z_mu_sde", "zyx_y_mu_sde", "zyx_x_mu_sde", "zyx_czz_sde", "zyx_czy_sde", "zyx_czx_sde",
            "zyx_cyy_sde", "zyx_cyx_sde", "zyx_cxx_sde"]
COLS = {"z": Z_COLS, "yx": YX_COLS, "zyx": ZYX_COLS}
COLUMNS = Z_COLS + YX_COLS + ZYX_COLS
COL0 = {"z": 0, "yx": 9, "zyx": 27}
# where a fit's parameters and their standard errors sit inside its record; the yx record has no error of cxx (its last
# column repeats the error of cyx, as the reference writes it)
PAR_COLS = {"z": list(range(4)), "yx": list(range(7)), "zyx": list(range(11))}
SDE_COLS = {"z": list(range(5, 9)), "yx": list(range(11, 17)), "zyx": list(range(17, 28))}
GUESS0 = {"z": 0, "yx": 4, "zyx": 11}


def load_golden():
    return json.loads(GOLDEN.read_text())


# ------------------------------------------------------------------------------------------------------------ generator
def gaussian(shape, spacing, bg, amp, centre_um, cov):
    """bg + amp exp(-d' C^-1 d / 2) on the grid index * spacing (float64)."""
    grids = np.meshgrid(*[np.arange(n) * s for n, s in zip(shape, spacing)], indexing="ij")
    d = np.stack([g - c for g, c in zip(grids, centre_um)], -1)
    q = np.linalg.inv(np.asarray(cov, dtype=np.float64))
    return bg + amp * np.exp(-0.5 * np.einsum("...i,ij,...j->...", d, q, d))


def bead_covariance(sigmas_um, tilt_zx=0.0, tilt_yx=0.0):
    """Covariance (um^2) with the given standard deviations and correlation coefficients czx, cyx."""
    sz, sy, sx = sigmas_um
    return [[sz * sz, 0.0, tilt_zx * sz * sx], [0.0, sy * sy, tilt_yx * sy * sx], [tilt_zx * sz * sx, tilt_yx * sy * sx, sx * sx]]


def make_bead(c, shape=None, seed=None):
    """One noisy bead patch of a case (raw store units, float64 counts): Poisson(bg + Gaussian) / gain - offset, so that
    the reference's (patch + offset) * gain lands back near the counts."""
    shape = tuple(c["patch"]) if shape is None else tuple(shape)
    rng = np.random.default_rng(c["seed"] if seed is None else seed)
    sp = c["spacing"]
    sub = rng.uniform(-0.5, 0.5, 3)
    centre = [(n // 2 + o) * s for n, o, s in zip(c["patch"], sub, sp)]
    clean = gaussian(shape, sp, c["bg"], c["amp"], centre, bead_covariance(c["sigmas"], c.get("tilt_zx", 0.0), c.get("tilt_yx", 0.0)))
    counts = rng.poisson(clean).astype(np.float64)
    return counts / c["gain"] - c["offset"]


def _store(raw, dtype):
    if dtype == "float32":
        return raw.astype(np.float32)
    return np.clip(np.rint(raw), 0, np.iinfo(dtype).max).astype(dtype)


def make_case_volume(c):
    """(volume, starts (1, 3), shapes (1, 3)) of a single-bead case.  ``volume`` is the patch itself, or -- with ``truncate`` --
    a volume whose far border cuts the nominal patch short (NumPy slicing semantics, as the reference's crops)."""
    nominal = tuple(c["patch"])
    if c.get("truncate"):
        cut = tuple(c["truncate"])  # voxels missing at the far border
        shape = tuple(n - k for n, k in zip(nominal, cut))
        rng = np.random.default_rng(c["seed"] + 1)
        pad = (3, 4, 5)
        vol = rng.poisson(c["bg"], tuple(p + s for p, s in zip(pad, shape))).astype(np.float64) / c["gain"] - c["offset"]
        vol[pad[0]:, pad[1]:, pad[2]:] = make_bead(c, shape=shape)
        return _store(vol, c["dtype"]), np.array([pad], dtype=np.int32), np.array([shape], dtype=np.int32)
    vol = _store(make_bead(c), c["dtype"])
    return vol, np.zeros((1, 3), dtype=np.int32), np.array([nominal], dtype=np.int32)


def make_batch_volume(b):
    """The batch case: ``count`` beads scattered in one volume, one per slot of a regular grid, jittered inside the slot."""
    rng = np.random.default_rng(b["seed"])
    shape, patch, slots = tuple(b["volume"]), tuple(b["patch"]), tuple(b["slots"])
    vol = rng.poisson(b["bg"], shape).astype(np.float64)
    cell = [s // n for s, n in zip(shape, slots)]
    order = rng.permutation(int(np.prod(slots)))[: b["count"]]
    starts = []
    for i, slot in enumerate(order):
        iz, iy, ix = np.unravel_index(slot, slots)
        st = [k * c + int(rng.integers(0, c - p + 1)) for k, c, p in zip((iz, iy, ix), cell, patch)]
        c = dict(b, amp=float(rng.uniform(*b["amp_range"])), sigmas=[float(s * rng.uniform(0.85, 1.15)) for s in b["sigmas"]],
                 tilt_zx=float(rng.uniform(-0.5, 0.5)), gain=1.0, offset=0.0)
        vol[st[0]:st[0] + patch[0], st[1]:st[1] + patch[1], st[2]:st[2] + patch[2]] = make_bead(c, seed=b["seed"] + 1 + i)
        starts.append(st)
    starts = np.array(starts, dtype=np.int32)
    return _store(vol, b["dtype"]), starts, np.tile(np.array(patch, dtype=np.int32), (len(starts), 1))


def to_sample(patch, offset, gain):
    """The reference's int32 sample of a raw patch (truncation, not rounding).  NumPy keeps float32 for a float32 patch."""
    p = (np.asarray(patch) + offset) * gain
    return np.clip(p, 0, None).astype(np.int32)


def crop(vol, start, shape):
    return vol[tuple(slice(int(s), int(s) + int(n)) for s, n in zip(start, shape))]


# ----------------------------------------------------------------------------------------------------- initial guesses
def centroid(image):
    """skimage.measure.centroid: sum(i w) / sum(w) per axis."""
    image = np.asarray(image)
    w = image.astype(np.float64)
    total = w.sum()
    grids = np.meshgrid(*[np.arange(n) for n in image.shape], indexing="ij")
    return np.array([(g * w).sum() / total for g in grids])


def sub_sample(sample, kind):
    sz, sy, sx = sample.shape
    return {"z": sample[:, sy // 2, sx // 2], "yx": sample[sz // 2], "zyx": sample}[kind]


def kind_spacing(spacing, kind):
    return {"z": spacing[:1], "yx": spacing[1:], "zyx": spacing}[kind]


def coordinates(shape, spacing):
    grids = np.meshgrid(*[np.arange(n) * s for n, s in zip(shape, spacing)], indexing="ij")
    return np.stack([g.ravel() for g in grids], -1)


def initial_guess(sample, spacing, kind):
    """fit/estimator.py + fit/fitter.py: uint16 median of the WHOLE patch, max - median, weighted centroid of the raw
    sub-sample, diagonal of np.cov(coords, fweights=sample), off-diagonals 0."""
    sub, sp = sub_sample(sample, kind), tuple(kind_spacing(tuple(spacing), kind))
    with np.errstate(all="ignore"):
        bg = np.median(sample).astype(np.uint16)
        amp = sub.max() - bg
        mu = centroid(sub) * np.array(sp)
        cov = np.atleast_2d(np.cov(coordinates(sub.shape, sp).T, fweights=sub.ravel()))
        var = np.abs(np.sqrt(np.diag(cov))) ** 2
        if kind == "z":
            return np.array([bg, amp, mu[0], np.abs(np.sqrt(cov[0, 0]))], dtype=np.float64)
        if kind == "yx":
            return np.array([bg, amp, mu[0], mu[1], var[0], 0, var[1]], dtype=np.float64)
        return np.array([bg, amp, mu[0], mu[1], mu[2], var[0], 0, 0, var[1], 0, var[2]], dtype=np.float64)


# -------------------------------------------------------------------------------------------------------------- models
def _cov_of(kind, p):
    if kind == "yx":
        return np.array([[p[4], p[5]], [p[5], p[6]]])
    return np.array([[p[5], p[6], p[7]], [p[6], p[8], p[9]], [p[7], p[9], p[10]]])


def model_jac(kind, p, coords):
    """(f, J) at the (M, D) coordinates: the reference's models (fit_1d/2d/3d.py), analytic Jacobian."""
    p = np.asarray(p, dtype=np.float64)
    if kind == "z":
        d = coords[:, 0] - p[2]
        e = np.exp(-(d**2) / (2 * p[3] ** 2))
        J = np.stack([np.ones_like(e), e, p[1] * e * d / p[3] ** 2, p[1] * e * d**2 / p[3] ** 3], -1)
        return p[1] * e + p[0], J
    D = 2 if kind == "yx" else 3
    d = coords - p[2:2 + D]
    u = d @ np.linalg.inv(_cov_of(kind, p))
    e = np.exp(-0.5 * (d * u).sum(-1))
    ae = p[1] * e
    cols = [np.ones_like(e), e] + [ae * u[:, i] for i in range(D)]
    for i in range(D):
        for j in range(i, D):
            cols.append(ae * u[:, i] * u[:, j] * (0.5 if i == j else 1.0))
    return ae + p[0], np.stack(cols, -1)


def fit(kind, sample, spacing, p0, max_iter=400):
    """Levenberg-Marquardt with Marquardt's scaling from p0 until the undamped Gauss-Newton step is <= 1e-9 standard
    errors in every parameter (rounding leaves about 1e-10 on these cases).  Returns dict(p, sde, ok, iters, grad) -- grad = max_i |J_i . r| / (|J_i| |r|) at the end."""
    sub = sub_sample(sample, kind)
    coords = coordinates(sub.shape, kind_spacing(tuple(spacing), kind))
    y = sub.ravel().astype(np.float64)
    P, M = NPAR[kind], y.size
    nan = dict(p=np.full(P, np.nan), sde=np.full(P, np.nan), ok=False, iters=0, grad=np.nan)
    p = np.asarray(p0, dtype=np.float64).copy()
    if M <= P or not np.all(np.isfinite(p)):
        return nan

    def normal(q):
        with np.errstate(all="ignore"):
            f, J = model_jac(kind, q, coords)
            r = y - f
            return J.T @ J, J.T @ r, float(r @ r)

    A, g, ssr = normal(p)
    if not np.isfinite(ssr):
        return nan
    lam = 1e-3
    for it in range(1, max_iter + 1):
        d = np.sqrt(np.diag(A))
        if not (np.all(d > 0) and np.all(np.isfinite(d))):
            return nan
        As = A / np.outer(d, d)
        try:
            step = np.linalg.solve(As + lam * np.eye(P), g / d) / d
        except np.linalg.LinAlgError:
            return nan
        At, gt, ssrt = normal(p + step)
        if np.isfinite(ssrt) and ssrt <= ssr * (1 + 1e-13):  # r.r resolves a step only down to ~1e-7 sde: rounding-level rises pass
            rel = (ssr - ssrt) / ssr if ssr > 0 else 0.0
            p, A, g, ssr, lam = p + step, At, gt, ssrt, max(lam * 0.1, 1e-12)
        else:
            rel = (ssr - ssrt) / ssr if np.isfinite(ssrt) and ssr > 0 else np.inf
            lam = min(lam * 10, 1e16)
        if abs(rel) <= 1e-12:
            d = np.sqrt(np.diag(A))
            try:
                gn = np.linalg.solve(A / np.outer(d, d), g / d)
            except np.linalg.LinAlgError:
                continue
            if np.abs(gn).max() <= 1e-9 * np.sqrt(ssr / (M - P)) or np.linalg.norm(gn) <= 1e-12 * np.linalg.norm(p * d):
                break
    else:
        return nan
    for _ in range(2):  # the Gauss-Newton step is good far below what r.r can judge: take it down to rounding
        p = p + gn / d
        A, g, ssr = normal(p)
        d = np.sqrt(np.diag(A))
        gn = np.linalg.solve(A / np.outer(d, d), g / d)
    with np.errstate(all="ignore"):
        cov =np.linalg.inv(A / np.outer(d, d)) / np.outer(d, d) * ssr / (M - P)
        f, J = model_jac(kind, p, coords)
        r = y - f
        grad = float(np.max(np.abs(J.T @ r) / (np.linalg.norm(J, axis=0) * np.linalg.norm(r)))) if ssr > 0 else 0.0
    return dict(p=p, sde=np.sqrt(np.diag(cov)), ok=True, iters=it, grad=grad)


def scipy_fit(kind, sample, spacing, p0):
    """The same optimum through MINPACK with the analytic Jacobian at the tightest tolerances (cross-check of ``fit``)."""
    from scipy.optimize import least_squares

    sub = sub_sample(sample, kind)
    coords = coordinates(sub.shape, kind_spacing(tuple(spacing), kind))
    y = sub.ravel().astype(np.float64)
    res = least_squares(lambda q: model_jac(kind, q, coords)[0] - y, p0, jac=lambda q: model_jac(kind, q, coords)[1], method="lm",
                        xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return res.x


# ------------------------------------------------------------------------------------------------------------- records
def record(kind, p, sde):
    """The fit's columns as the reference's fitter writes them (fit/fitter.py), in ``COLS[kind]`` order."""
    p, sde = np.asarray(p, dtype=np.float64), np.asarray(sde, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == "z":
            return np.array([p[0], p[1], p[2], abs(p[3]), FWHM * abs(p[3]), *sde])
        pcs = np.sort(np.abs(np.sqrt(np.linalg.eigvalsh(_cov_of(kind, p)))))[::-1]
        if kind == "yx":
            return np.array([*p, FWHM * np.sqrt(p[4]), FWHM * np.sqrt(p[6]), *(FWHM * pcs), *sde[:6], sde[5]])
        return np.array([*p, FWHM * np.sqrt(p[5]), FWHM * np.sqrt(p[8]), FWHM * np.sqrt(p[10]), *(FWHM * pcs), *sde])


# the reference's records are pydantic models: these fields are NonNegativeFloat, a negative (or NaN) one raises, the bead's
# summary becomes {} and dropna() removes the bead (records.py; characterize_psf.py:241-246, 264)
NON_NEGATIVE = [c for c in COLUMNS if c not in ("yx_cyy", "yx_cyx", "yx_cxx", "zyx_czz", "zyx_czy", "zyx_czx", "zyx_cyy",
                                                "zyx_cyx", "zyx_cxx")]


def analyze(sample, spacing):
    """One bead on the host: (row of len(COLUMNS), kept) -- kept is False where the reference would drop the bead."""
    row, kept = [], True
    for kind in KINDS:
        r = fit(kind, sample, spacing, initial_guess(sample, spacing, kind))
        kept &= r["ok"]
        row.extend(record(kind, r["p"], r["sde"]))
    row = np.array(row)
    nn = row[[COLUMNS.index(c) for c in NON_NEGATIVE]]
    kept = bool(kept and np.all(np.isfinite(row)) and np.all(nn >= 0))
    return row, kept
