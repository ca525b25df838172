"""Inputs of the inverse-filter tests (tests/test_invtf_reference.py on the CPU, tests/test_gpu_invtf_f64.py on the GPU): the
transfer functions of each case, the shapes, and a float32 restatement of the operator.

The transfer functions have no symmetry on purpose: only the Hermitian part of conj(H) / (|H|^2 + reg) acts on a real volume,
so the staged filter mixes H(k) and H(-k), and a slip in the mirror index or in the sign of an imaginary part changes the result
(with a real even H — every Tikhonov and ``deconvolve`` test — it cannot).
"""

import numpy as np
import torch

from test_gpu_f64_parity import FAMILIES, camera_volume

# case -> (transfer function kind, regularisation, normalize)
CASES = {
    "complex": ("complex", 1e-2, True),
    "complex_offset": ("complex_offset", 1e-3, False),
    "real": ("real", 1e-3, False),
}
BF16_CASE = ("complex_offset", 1e-3, False)

# odd radix on all three axes at once, tile X rows of 3 * 64 and 5 * 64: the engine families test_gpu_f64_parity.FAMILIES lacks
ALL_ODD_RADIX = [((24, 96, 192), "radix 3 on z, y and x"), ((40, 160, 320), "radix 5 on z, y and x")]

# (shape, z_padding, bf16 too, note): z padding on the engine
PADDED = [
    ((20, 96, 192), 2, True, "padded Z 24"),
    ((30, 160, 320), 5, True, "padded Z 40"),
    ((6, 64, 512), 1, True, "padded Z 8, wave-private rows: the normalisation cannot fuse"),
    ((4, 32, 64), 6, True, "pad >= Z: zero planes"),
    ((380, 32, 64), 2, False, "padded Z 384: the colz3 Z pass (float32 only)"),
]

# rows the wave-private X passes take: normalize=True rides in their load (fftconv_xw.inc, fftconv_x3.inc)
WAVE_PRIVATE_X = (512, 1024, 2048, 1536, 3072)


LIBRARY = [((15, 21, 25), 0, {}), ((9, 14, 31), 2, {}), ((10, 20, 50), 3, {}), ((24, 96, 192), 0, {"BH_FFT_BACKEND": "hipfft"})]
NO_REG = [(24, 96, 192), (8, 64, 1024), (15, 21, 25)]   # reg = 0, |H| in [0.5, 1.5]: the exact inverse


def engine_families():
    """(shape, switches, what) of every FAMILIES entry the engine takes, one per distinct (shape, switches), and the two
    all-odd-radix boxes."""
    seen, out = set(), []
    for shape, _, env, backend, what in FAMILIES:
        key = (shape, tuple(sorted(env.items())))
        if backend == "engine" and key not in seen:
            seen.add(key)
            out.append((shape, env, what))
    return out + [(shape, {}, what) for shape, what in ALL_ODD_RADIX]


ENGINE = engine_families()
WAVE_PRIVATE = [f for f in ENGINE if f[0][2] in WAVE_PRIVATE_X and "BH_FC_XW" not in f[1]]


def float32_inputs():
    """Every (shape, z_padding, kind, reg, normalize) the GPU tests run in float32 storage, grouped by (shape, z_padding)."""
    out = {}

    def add(shape, pad, kind, reg, normalize):
        cases = out.setdefault((tuple(shape), pad), [])
        if (kind, reg, normalize) not in cases:
            cases.append((kind, reg, normalize))

    for shape, _, _ in ENGINE:
        for case in CASES.values():
            add(shape, 0, *case)
    for shape, _, _ in WAVE_PRIVATE:
        for name in ("complex", "complex_offset"):
            add(shape, 0, CASES[name][0], CASES[name][1], True)
    for shape, pad, _, _ in PADDED:
        for normalize in (False, True):
            add(shape, pad, CASES["complex_offset"][0], CASES["complex_offset"][1], normalize)
    for shape, pad, _ in LIBRARY:
        for case in CASES.values():
            add(shape, pad, *case)
    for shape in NO_REG:
        for normalize in (False, True):
            add(shape, 0, "unit", 0.0, normalize)
    return out


def bf16_inputs():
    """Every (shape, z_padding, normalize) the GPU tests run with the bfloat16 filter (BF16_CASE's H and reg)."""
    out = [(shape, 0, BF16_CASE[2]) for shape in dict.fromkeys(f[0] for f in ENGINE)]
    return out + [(shape, pad, n) for shape, pad, bf16, _ in PADDED if bf16 for n in (False, True)]


def transfer_function(kind, tshape, seed):
    """complex: 0.3 (N + iN); complex_offset: 1 + 0.3 (N + iN) (complex64); real: 0.5 N (float32); real_even: the magnitude
    spectrum of a Gaussian (float32); unit: |H| in [0.5, 1.5] with random phase (complex64).  None of the first three has any symmetry."""
    rng = np.random.default_rng(seed)
    if kind in ("complex", "complex_offset"):
        H = 0.3 * (rng.standard_normal(tshape) + 1j * rng.standard_normal(tshape))
        return (H + (1.0 if kind == "complex_offset" else 0.0)).astype(np.complex64)
    if kind == "real":
        return (0.5 * rng.standard_normal(tshape)).astype(np.float32)
    if kind == "unit":
        return ((0.5 + rng.random(tshape)) * np.exp(2j * np.pi * rng.random(tshape))).astype(np.complex64)
    if kind == "real_even":
        g = [np.exp(-0.5 * (np.fft.fftfreq(n) * n / 1.2) ** 2) for n in tshape]
        psf = g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
        return np.abs(np.fft.fftn(psf / psf.sum())).astype(np.float32)
    raise ValueError(kind)


def case_volume(shape):
    """The camera-like volume of a shape (offset 110, noise, beads on the faces too), the same in the CPU and the GPU tests."""
    return camera_volume(shape, seed=sum(shape))


def case_transfer_function(kind, tshape):
    return transfer_function(kind, tshape, 1000 + sum(tshape))   # not the volume's seed: the two must not share a stream


def inverse_filter_c64(vol, H, z_padding=0, reg=1e-3, normalize=False, mean_f32_running_sum=False):
    """The operator restated in float32 / complex64 on the CPU (torch's FFTs): what a float32 implementation of the definition
    gives, the yardstick of the float32 bounds.  ``mean_f32_running_sum``: a planted defect, the mean of the normalisation from
    a sequential float32 sum."""
    x = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32))
    if normalize:
        if mean_f32_running_sum:
            mean = float(np.cumsum(np.asarray(vol, np.float32).ravel(), dtype=np.float32)[-1]) / x.numel()
        else:
            mean = float(x.double().mean())
        x = x * np.float32(1.0 / mean) - 1.0
    pad, Z = int(z_padding), x.shape[0]
    if pad:
        xp = torch.zeros((Z + 2 * pad,) + tuple(x.shape[1:]), dtype=torch.float32)
        xp[pad:pad + Z] = x
        if pad < Z:
            xp[:pad] = x[:pad].flip(0)
            xp[pad + Z:] = x[Z - pad:].flip(0)
        x = xp
    H = torch.from_numpy(np.ascontiguousarray(H))
    H = H.to(torch.complex64) if H.is_complex() else H.to(torch.float32)
    filt = H.conj() / (H.abs() ** 2 + np.float32(reg))
    out = torch.fft.ifftn(torch.fft.fftn(x.to(torch.complex64)) * filt).real
    return (out[pad:pad + Z] if pad else out).contiguous()
