"""StackReg translation on MI355X — ``pystackreg``'s ``StackReg(StackReg.TRANSLATION).register_stack`` as the reference calls
it (``biahub/estimate_stabilization.py:755-756``).

pystackreg is not a dependency of this package: TurboReg's translation mode is restated as a
cubic-spline pyramid with a Marquardt-Levenberg descent on the mean squared difference, every pair of a call in one batched
float64 solve on the device (``bh_stackreg_translation``, csrc/stackreg.hip).  The rigid, affine and bilinear modes are not
available.
"""

from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib
from .device import _TORCH_TO_DT, get_context, ptr, resolve_device, upload, volume_pool

WORKING_BYTES = 1 << 30  # device working memory a call may take for its pyramids (16 * 4/3 * H * W bytes per frame)


def default_max_frames(H: int, W: int) -> int:
    return max(2, int(WORKING_BYTES // (16 * 4 * H * W // 3 + 1)))


def _chunks(pairs: np.ndarray, max_frames: int):
    """Consecutive runs of pairs that name at most ``max_frames`` distinct frames: ``(first, last + 1, sorted frames)``."""
    start, frames = 0, set()
    for i, (m, r) in enumerate(pairs):
        new = frames | {int(m), int(r)}
        if len(new) > max_frames and i > start:
            yield start, i, sorted(frames)
            start, new = i, {int(m), int(r)}
        frames = new
    if len(pairs) > start:
        yield start, len(pairs), sorted(frames)


def _frames_on_device(tyx, frames, dev):
    """The listed frames as a device tensor the kernel can read in place, and the dtype code.  A device tensor whose listed
    frames are a contiguous run with unit stride along x and rows and planes that do not overlap is viewed, not copied."""
    if isinstance(tyx, torch.Tensor) and tyx.is_cuda:
        t = tyx if tyx.dtype in _TORCH_TO_DT else tyx.to(torch.float32)
        if frames == list(range(frames[0], frames[-1] + 1)):
            t = t[frames[0]:frames[-1] + 1]
        else:
            with volume_pool(dev):
                picked = torch.empty((len(frames),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            for i, f in enumerate(frames):
                picked[i].copy_(t[f])
            t = picked
        _, H, W = t.shape
        st, sy, sx = t.stride()
        if not (sx == 1 and sy >= W and (t.shape[0] == 1 or st >= (H - 1) * sy + W)):
            t = t.contiguous()
        return t, _TORCH_TO_DT[t.dtype]
    host = tyx.numpy() if isinstance(tyx, torch.Tensor) else np.asarray(tyx)
    return upload(host[frames], dev)


def register_translation_pairs(tyx, pairs, device="cuda", max_frames: int | None = None):
    """Translation of every ``(moving, reference)`` pair of frame indices of the stack ``tyx`` (numpy array, uploaded frame by
    needed frame; or a device tensor, which may be a strided window of a larger resident array and is then read in place).

    Returns ``(shift_yx float64 (n, 2), mse float64 (n,), status int32 (n,), iterations int32 (n,))``: the moving frame's
    content sits at ``x + shift`` where the reference's sits at ``x``; status 0 converged, 1 iteration cap at the finest level,
    2 degenerate (a frame without usable gradients: shift 0).  Values below 0 are read as 0.  Pairs are solved in runs that
    name at most ``max_frames`` frames (default: what fits ``WORKING_BYTES``); a pair's result does not depend on the runs."""
    if len(tyx.shape) != 3:
        raise ValueError(f"expected a (T, Y, X) stack, got shape {tuple(tyx.shape)}")
    T, H, W = (int(n) for n in tyx.shape)
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    if pairs.size and (pairs.min() < 0 or pairs.max() >= T):
        raise ValueError(f"pairs name frames outside 0..{T - 1}")
    n = len(pairs)
    shift, mse = np.zeros((n, 2), dtype=np.float64), np.zeros(n, dtype=np.float64)
    status, iterations = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    if n == 0:
        return shift, mse, status, iterations
    dev = resolve_device(tyx.device if isinstance(tyx, torch.Tensor) and tyx.is_cuda else device)
    ctx = get_context(dev)
    max_frames = default_max_frames(H, W) if max_frames is None else max(2, int(max_frames))
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for lo, hi, frames in _chunks(pairs, max_frames):
        t, code = _frames_on_device(tyx, frames, dev)
        local = np.ascontiguousarray(np.searchsorted(frames, pairs[lo:hi]).astype(np.int32))
        st, sy, _ = t.stride()
        if t.shape[0] == 1:
            st = max(st, (H - 1) * sy + W)
        sh, ms = np.empty((hi - lo, 2), dtype=np.float64), np.empty(hi - lo, dtype=np.float64)
        stt, it = np.empty(hi - lo, dtype=np.int32), np.empty(hi - lo, dtype=np.int32)
        with torch.cuda.device(dev):
            _lib.check(ctx.lib.bh_stackreg_translation(ctx.handle, ptr(t), code, len(frames), H, W, int(st), int(sy),
                                                       local.ctypes.data_as(pi), hi - lo, sh.ctypes.data_as(pd), ms.ctypes.data_as(pd),
                                                       stt.ctypes.data_as(pi), it.ctypes.data_as(pi)))
        shift[lo:hi], mse[lo:hi], status[lo:hi], iterations[lo:hi] = sh, ms, stt, it
    return shift, mse, status, iterations


def matrices_from_shifts(shift_yx, reference: str) -> np.ndarray:
    """pystackreg's ``(T, 3, 3)`` translation matrices (output -> input: ``[0, 2]`` the x shift, ``[1, 2]`` the y shift) from the
    T - 1 shifts of frames 1 ... T - 1; with ``"previous"`` the pairwise shifts are accumulated in that order."""
    shift_yx = np.asarray(shift_yx, dtype=np.float64).reshape(-1, 2)
    out = np.tile(np.eye(3), (len(shift_yx) + 1, 1, 1))
    total = np.zeros(2)
    for t, s in enumerate(shift_yx, start=1):
        total = total + s if reference == "previous" else s
        out[t, 0, 2], out[t, 1, 2] = total[1], total[0]
    return out


def register_stack(tyx, reference: str = "first", device="cuda", max_frames: int | None = None) -> np.ndarray:
    """``StackReg(StackReg.TRANSLATION).register_stack(tyx, reference=reference, axis=0)``: ``(T, 3, 3)`` float64 matrices,
    frame 0 the identity.  ``"first"`` registers every frame against frame 0, ``"previous"`` against its predecessor and
    accumulates.  If frame t's content sits at ``x + s`` where the reference's sits at ``x`` the entry is ``+s``."""
    if reference not in ("first", "previous"):
        raise ValueError(f"reference must be 'first' or 'previous', got {reference!r} (pystackreg's 'mean' is not available in biahub_amd)")
    T = int(tyx.shape[0])
    pairs = [(t, 0 if reference == "first" else t - 1) for t in range(1, T)]
    shift, _, status, _ = register_translation_pairs(tyx, pairs, device=device, max_frames=max_frames)
    bad = [t for t, s in enumerate(status, start=1) if s != _lib.STACKREG_CONVERGED]
    if bad:
        names = {_lib.STACKREG_ITERCAP: "iteration cap", _lib.STACKREG_DEGENERATE: "no usable gradients, shift 0"}
        warnings.warn("stackreg: frames " + ", ".join(f"{t} ({names[int(status[t - 1])]})" for t in bad) + " did not converge",
                      stacklevel=2)
    return matrices_from_shifts(shift, reference)
