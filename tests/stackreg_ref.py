"""Float64 numpy restatement of the StackReg translation estimator and the synthetic scenes its tests use.

It shares no code with the library: the constants below mirror ``BH_STACKREG_*`` of ``include/bhcore.h`` (a host test holds the
two to each other), everything else is written out here.

The algorithm, per (moving, reference) pair:

* pyramid: level 0 is the frame clipped below at 0; while min(H, W) of the last level is >= MIN_SIDE_FOR_NEXT a level is
  appended: [1, 4, 6, 4, 1] / 16 along x, then along y, whole-sample mirror boundaries, even indices kept;
* every level gets cubic B-spline coefficients (pole sqrt(3) - 2, mirror boundaries, axis 0 first);
* cost at a displacement d: E = sum r^2 / count over Omega(d), r = M(x + d) - R(x), M from the moving level's coefficients
  (the taps start at floor(d), the weights come from d - floor(d); at an integer d the moving level's values are read
  instead, so identical frames give exactly 0), R the reference level's values;
* descent: g = sum r grad R, H = sum grad R grad R^T over Omega(d), grad R the central difference of the reference's
  coefficients; u = (H + lambda diag H)^-1 g, attempt d - u, accepted when E falls strictly (lambda / 4), else lambda * 4; the
  level ends after the iteration whose |u| < EPS or after MAX_ITER; d doubles to the next finer level;
* a pair is degenerate (shift 0, status 2) when the level-0 gradient matrix of either frame is flat against its energy
  (min(Hyy, Hxx) <= FLAT_REL * sum v^2), not finite, or ill-conditioned (det <= COND_REL * Hyy * Hxx), or when an H of the
  descent is.
"""

from __future__ import annotations

import math

import numpy as np

MIN_SIDE_FOR_NEXT = 24
EPS = 1e-3
MAX_ITER = 20
LAMBDA0 = 1.0
LAMBDA_FACTOR = 4.0
FLAT_REL = 1e-20
COND_REL = 1e-10
POLE = math.sqrt(3.0) - 2.0
CONVERGED, ITERCAP, DEGENERATE = 0, 1, 2


def mirror(i, n):
    """Whole-sample mirror index (-1 -> 1, n -> n - 2), then clamped: one reflection is all an in-range pixel's taps need."""
    i = np.abs(np.asarray(i))
    i = np.where(i > n - 1, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def clip_to_f64(frame):
    v = np.asarray(frame).astype(np.float64)
    return np.where(v > 0, v, 0.0)


def reduce_level(v):
    k = (0.0625, 0.25, 0.375, 0.25, 0.0625)
    H, W = v.shape
    xs, ys = 2 * np.arange((W + 1) // 2), 2 * np.arange((H + 1) // 2)
    t = sum(k[b] * v[:, mirror(xs + b - 2, W)] for b in range(5))
    return sum(k[a] * t[mirror(ys + a - 2, H), :] for a in range(5))


def pyramid(frame):
    levels = [clip_to_f64(frame)]
    while min(levels[-1].shape) >= MIN_SIDE_FOR_NEXT:
        levels.append(reduce_level(levels[-1]))
    return levels


def _prefilter_axis0(c):
    c = c * ((1.0 - POLE) * (1.0 - 1.0 / POLE))
    n = c.shape[0]
    zn1 = POLE ** (n - 1)
    c0 = c[0] + zn1 * c[n - 1]
    zi = POLE
    for i in range(1, n - 1):
        c0 = c0 + zi * (c[i] + zn1 * c[n - 1 - i])
        zi *= POLE
    c[0] = c0 / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[i] += POLE * c[i - 1]
    c[n - 1] = (POLE * c[n - 2] + c[n - 1]) * POLE / (POLE * POLE - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = POLE * (c[i + 1] - c[i])
    return c


def spline_coefficients(v):
    """``scipy.ndimage.spline_filter(v, order=3, mode="mirror")``, written out."""
    return _prefilter_axis0(_prefilter_axis0(np.array(v, dtype=np.float64)).T.copy()).T.copy()


def tap_weights(f):
    return np.array([(1 - f) ** 3 / 6, (3 * f**3 - 6 * f**2 + 4) / 6, (-3 * f**3 + 3 * f**2 + 3 * f + 1) / 6, f**3 / 6])


def evaluate(v_mov, c_mov, v_ref, c_ref, d):
    """The seven sums over Omega(d): count, r.r, r.gy, r.gx, gy.gy, gy.gx, gx.gx.  At an integer d the moving level's values
    are read in place of its coefficients: the spline interpolates them."""
    H, W = v_ref.shape
    dy, dx = float(d[0]), float(d[1])
    iy0, ix0 = math.floor(dy), math.floor(dx)
    wy, wx = tap_weights(dy - iy0), tap_weights(dx - ix0)
    if dy == iy0 and dx == ix0:
        c_mov, wy, wx = v_mov, np.array([0.0, 1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0, 0.0])
    ys, xs = np.arange(H), np.arange(W)
    yok = (ys + dy >= 0) & (ys + dy <= H - 1)
    xok = (xs + dx >= 0) & (xs + dx <= W - 1)
    rowf = sum(wx[l] * c_mov[:, mirror(xs + ix0 + l - 1, W)] for l in range(4))
    M = sum(wy[k] * rowf[mirror(ys + iy0 + k - 1, H), :] for k in range(4))
    r = M - v_ref
    gy = 0.5 * (c_ref[mirror(ys + 1, H), :] - c_ref[mirror(ys - 1, H), :])
    gx = 0.5 * (c_ref[:, mirror(xs + 1, W)] - c_ref[:, mirror(xs - 1, W)])
    m = yok[:, None] & xok[None, :]
    r, gy, gx = r[m], gy[m], gx[m]
    return np.array([m.sum(), (r * r).sum(), (r * gy).sum(), (r * gx).sum(), (gy * gy).sum(), (gy * gx).sum(), (gx * gx).sum()])


def usable(hyy, hyx, hxx):
    with np.errstate(all="ignore"):
        return bool(np.isfinite(hyy + hyx + hxx) and hyy > 0 and hxx > 0 and hyy * hxx - hyx * hyx > COND_REL * hyy * hxx)


def frame_is_flat(v0, c0):
    """Level 0 of a frame carries no usable gradient: its matrix over the whole level against the frame's energy."""
    H, W = v0.shape
    ys, xs = np.arange(H), np.arange(W)
    gy = 0.5 * (c0[mirror(ys + 1, H), :] - c0[mirror(ys - 1, H), :])
    gx = 0.5 * (c0[:, mirror(xs + 1, W)] - c0[:, mirror(xs - 1, W)])
    with np.errstate(all="ignore"):
        hyy, hyx, hxx, e = (gy * gy).sum(), (gy * gx).sum(), (gx * gx).sum(), (v0 * v0).sum()
        return not (usable(hyy, hyx, hxx) and np.isfinite(e) and min(hyy, hxx) > FLAT_REL * e)


def solve_step(s, lam):
    a, b, c = s[4] * (1 + lam), s[5], s[6] * (1 + lam)
    det = a * c - b * b
    return np.array([(c * s[2] - b * s[3]) / det, (a * s[3] - b * s[2]) / det])


class Prepared:
    def __init__(self, frame):
        self.values = pyramid(frame)
        self.coefs = [spline_coefficients(v) for v in self.values]
        self.flat = frame_is_flat(self.values[0], self.coefs[0])


def register_pair(mov: Prepared, ref: Prepared, trace=None):
    """``(shift_yx, mse, status, iterations)`` of one pair."""
    if mov.flat or ref.flat:
        return np.zeros(2), 0.0, DEGENERATE, 0
    d = np.zeros(2)
    iterations, capped = 0, False
    for level in range(len(ref.values) - 1, -1, -1):
        vm, cm, vr, cr = mov.values[level], mov.coefs[level], ref.values[level], ref.coefs[level]
        lam = LAMBDA0
        cur = evaluate(vm, cm, vr, cr, d)
        if cur[0] == 0 or not np.isfinite(cur).all() or not usable(cur[4], cur[5], cur[6]):
            return np.zeros(2), 0.0, DEGENERATE, iterations
        capped = True
        for _ in range(MAX_ITER):
            u = solve_step(cur, lam)
            trial = evaluate(vm, cm, vr, cr, d - u)
            iterations += 1
            ok = trial[0] > 0 and np.isfinite(trial).all() and trial[1] / trial[0] < cur[1] / cur[0]
            if ok and not usable(trial[4], trial[5], trial[6]):
                return np.zeros(2), 0.0, DEGENERATE, iterations
            if ok:
                d, cur, lam = d - u, trial, lam / LAMBDA_FACTOR
            else:
                lam *= LAMBDA_FACTOR
            if trace is not None:
                trace.append((level, iterations, ok, float(np.hypot(*u))))
            if math.hypot(u[0], u[1]) < EPS:
                capped = False
                break
        if level > 0:
            d = 2.0 * d
    return d, float(cur[1] / cur[0]), (ITERCAP if capped else CONVERGED), iterations


def register_pairs(tyx, pairs):
    prepared = {}
    for t in sorted({int(t) for p in pairs for t in p}):
        prepared[t] = Prepared(tyx[t])
    out = [register_pair(prepared[int(m)], prepared[int(r)]) for m, r in pairs]
    return (np.array([o[0] for o in out]).reshape(-1, 2), np.array([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32),
            np.array([o[3] for o in out], dtype=np.int32))


# --------------------------------------------------------------------------------------------------------------- scenes
BACKGROUND = 100.0


def blobs(H, W, seed):
    """Blob centres, amplitudes and sigmas (1.5 to 3.5 px) of a scene; one blob per 128 pixels (denser scenes leave the coarsest level of 96 x 128 no structure to lock on)."""
    rng = np.random.default_rng(seed)
    n = max(6, H * W // 128)
    return rng.uniform(0, H - 1, n), rng.uniform(0, W - 1, n), rng.uniform(200.0, 1000.0, n), rng.uniform(1.5, 3.5, n)


def render(H, W, scene, shift_yx=(0.0, 0.0), noise_seed=None, dtype=np.float32):
    """The scene with its content displaced by ``shift_yx`` (what sits at x in the unshifted frame sits at x + s), evaluated
    analytically; optional Poisson noise; integer dtypes are rounded."""
    cy, cx, amp, sig = scene
    y = np.arange(H, dtype=np.float64)[:, None, None] - (cy + shift_yx[0])
    x = np.arange(W, dtype=np.float64)[None, :, None] - (cx + shift_yx[1])
    img = BACKGROUND + (amp * np.exp(-(y * y + x * x) / (2.0 * sig * sig))).sum(axis=-1)
    if noise_seed is not None:
        img = np.random.default_rng(noise_seed).poisson(img).astype(np.float64)
    if np.issubdtype(np.dtype(dtype), np.integer):
        img = np.rint(img)
    return img.astype(dtype)


def focus_volume(Z, H, W, scene, focus, shift_yx=(0.0, 0.0), defocus=1.5, dtype=np.uint16):
    """A (Z, H, W) stack of the scene displaced by ``shift_yx``: plane z is the scene blurred by a Gaussian of sigma
    ``defocus * |z - focus|`` (analytically: the blobs widen, their integrals stay), so plane ``focus`` is the sharpest."""
    cy, cx, amp, sig = scene
    planes = []
    for z in range(Z):
        wide = np.sqrt(sig * sig + (defocus * (z - focus)) ** 2)
        planes.append(render(H, W, (cy, cx, amp * sig * sig / (wide * wide), wide), shift_yx, dtype=dtype))
    return np.stack(planes)


# (name, H, W, true shift (y, x)): one level; two; odd halving; 50 x 70; zero and mixed-sign shifts up to 1/8 of the short side
CASES = (
    ("20x23", 20, 23, (1.3, -0.7)),
    ("24x47", 24, 47, (-2.6, 2.2)),
    ("49x63", 49, 63, (3.4, -5.8)),
    ("50x70", 50, 70, (-6.2, 4.3)),
    ("64x64-zero", 64, 64, (0.0, 0.0)),
    ("64x64", 64, 64, (7.6, 5.1)),
    ("96x128", 96, 128, (-11.3, 9.8)),
)


def case_pair(case, noise: bool, dtype):
    """``tyx`` of two frames: the reference (frame 0) and the moving frame (frame 1) displaced by the case's shift."""
    name, H, W, shift = case
    scene = blobs(H, W, seed=1000 + H * W)
    ref = render(H, W, scene, (0.0, 0.0), noise_seed=11 if noise else None, dtype=dtype)
    mov = render(H, W, scene, shift, noise_seed=12 if noise else None, dtype=dtype)
    return np.stack([ref, mov])


# The restatement's own worst error (max over y and x) on CASES, as float32 and as uint16: the recovery bounds of the tests.
RECOVERY_BOUND_NOISELESS = 0.012  # measured 0.0118 px (20x23, uint16); two or more levels: <= 0.0050 px (64x64)
RECOVERY_BOUND_NOISY = 0.030  # measured 0.0294 px (64x64, Poisson noise)

_REFERENCE = {}


def reference_result(index: int, noise: bool, dtype_name: str):
    """``(tyx, shift_yx (2,), mse, status, iterations)`` of CASES[index] (moving frame 1 against frame 0), computed once."""
    key = (index, bool(noise), dtype_name)
    if key not in _REFERENCE:
        tyx = case_pair(CASES[index], noise, np.dtype(dtype_name))
        shift, mse, status, iterations = register_pairs(tyx, [(1, 0)])
        _REFERENCE[key] = (tyx, shift[0], float(mse[0]), int(status[0]), int(iterations[0]))
    return _REFERENCE[key]
