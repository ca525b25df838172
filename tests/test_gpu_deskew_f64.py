"""GPU: the deskew (bh_deskew_rows: csrc/deskew.hip, csrc/deskew_rows.inc, csrc/fill.hip) on every kernel path against the float64
reference (oracle/reference_f64.py: deskew_f64), per voxel.

``|got - V| <= (N + 3) 2^-24 M`` at every voxel, exact zeros where M == 0, the fill rule inside the reference's mask: the bound is
derived at the head of tests/deskew_cases.py, which also holds the inputs (beads of 3 000 .. 60 000 counts on a background of
110) and the geometries; tests/test_deskew_reference.py shows on the CPU that the restated launch rules select the configuration
each case names, that the float32 oracle and the host deskew sit under the bound at every input here, and that the bound bites.

What runs here and nowhere else under a comparison: tile configurations 2, 3 and 4 (``TX = 32`` register staging, vector and
scalar; the ``J = 1`` compute loop), the > 64 KiB LDS attribute branch, the generic-N kernels of every configuration, and the
persistent kernel walking three and more tiles per workgroup — buffer flips, runs of overhang tiles, the reused interpolation
plan, the loaders' ``emit`` cursor — in its three fill modes.  Every case prints one ``F64 deskew ...`` line (``-s`` shows them).
"""

import functools

import numpy as np
import pytest
import torch

import deskew_cases as D
from oracle import reference_f64 as R

pytestmark = pytest.mark.gpu

SWITCHES = ("BH_DESKEW_CFG", "BH_DESKEW_PERS", "BH_DESKEW_ONEPASS", "BH_DESKEW_ROWS_KERNEL")


@functools.lru_cache(maxsize=4)
def _input(shape, dtype, zb):
    """(the operator's input on the GPU, the same values as float32 for the reference: every input type widens exactly)"""
    vol = D.bead_volume(shape)
    vol = np.array(D.as_dtype(D.zero_block(vol) if zb else vol, dtype))
    return torch.from_numpy(vol).cuda(), torch.from_numpy(vol.astype(np.float32)).cuda()


@functools.lru_cache(maxsize=3)
def _reference(shape, angle, ratio, N, keep, dtype, zb):
    """deskew_f64 on the GPU with the mean fill: (V, M, mask, mean); computed once per input and left unchanged."""
    return R.deskew_f64(_input(shape, dtype, zb)[1], angle, ratio, keep, N, "mean")


def reference(case, fill, dtype="f32", zb=False):
    shape, angle, ratio, N, keep = case
    V, M, mask, mean = _reference(shape, angle, ratio, N, keep, dtype, zb)
    if fill == 0 or mask is None:
        return V, M, None, None
    return V, M, mask, (mean if fill == "mean" else float(fill))


def run(gpu, monkeypatch, case, fill, dtype="f32", zb=False, row_sums=None, **switches):
    """One call of the operator under the given BH_DESKEW_* switches (all others unset); returns (result, fill path)."""
    from biahub_amd.deskew import deskew_fill_path, fast_deskew_zyx

    shape, angle, ratio, N, keep = case
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in switches.items():
        monkeypatch.setenv("BH_DESKEW_" + name, str(value))
    out = fast_deskew_zyx(_input(shape, dtype, zb)[0], angle, ratio, keep, N, fill, row_sums=row_sums)
    path = deskew_fill_path(gpu)
    for name in switches:
        monkeypatch.delenv("BH_DESKEW_" + name)
    return out, path


def check(name, got, case, fill, dtype="f32", zb=False):
    worst = D.assert_deskew_close(got, reference(case, fill, dtype, zb), case[3], name, fill=fill)
    print(f"F64 deskew {name} {case[0]} N{case[3]} {dtype} fill {fill}: {worst:.2f} u M (bound {case[3] + 3})")


def outside_fill(case, fill, dtype="f32", zb=False):
    """Where two paths must agree bit for bit: everywhere, or with a mean fill (summed in another order) outside the mask."""
    mask = reference(case, fill, dtype, zb)[2]
    return slice(None) if mask is None or fill != "mean" else ~mask


# ----------------------------------------------------------------------------- natural selection
@pytest.mark.parametrize("dtype", ["f32", "u16"])
@pytest.mark.parametrize("shape,angle,ratio,N,cfg", D.NATURAL, ids=[f"cfg {c[4]}" for c in D.NATURAL])
def test_deskew_selected_configuration_vs_float64(gpu, monkeypatch, shape, angle, ratio, N, cfg, dtype):
    """The five geometries at which ``launch_deskew`` itself selects configurations 0 .. 4 (the one-pass fill, whose order starts
    at 1, takes 1 at the first): without a fill, with the one-pass mean and constant fill, and with the mask prologue."""
    case = (shape, angle, ratio, N, True)
    assert D.selected_cfg(shape, angle, ratio, N)[0] == cfg and D.persistent(shape, angle, ratio, N) is None
    got, path = run(gpu, monkeypatch, case, 0, dtype)
    assert path == 0
    check(f"cfg {cfg} selected", got, case, 0, dtype)
    for fill in ("mean", 321.5):
        got, path = run(gpu, monkeypatch, case, fill, dtype)
        assert path == 1, (shape, fill)
        check(f"cfg {max(cfg, 1)} selected, one pass", got, case, fill, dtype)
        old, path = run(gpu, monkeypatch, case, fill, dtype, ONEPASS=0)
        assert path == 0, (shape, fill)
        check(f"cfg {cfg} selected, mask prologue", old, case, fill, dtype)
        keep = outside_fill(case, fill, dtype)
        assert torch.equal(got[keep], old[keep]), (shape, fill)


# ----------------------------------------------------------------------------- forced configurations
@pytest.mark.parametrize("g,N,dtype,fill", D.forced_cases(), ids=str)
def test_deskew_forced_configurations_vs_float64(gpu, monkeypatch, g, N, dtype, fill):
    """BH_DESKEW_CFG = 0 .. 4 on the tile kernel (BH_DESKEW_PERS=0: whole-tile float32 volumes would go to the persistent kernel
    with the mask prologue): each against float64, and all five bit-identical to each other — the arithmetic per output is the
    same (with the mask prologue's mean, summed per workgroup, outside the fill).  Which (geometry, N, dtype, fill) run:
    ``deskew_cases.forced_cases``."""
    case = D.FORCED_GEOMETRIES[g] + (N, True)
    first = {}
    for cfg in range(5):
        for onepass in ((1, 0) if fill != 0 else (1,)):
            got, path = run(gpu, monkeypatch, case, fill, dtype, CFG=cfg, PERS=0, ONEPASS=onepass)
            assert path == (1 if fill != 0 and onepass else 0), (cfg, onepass)
            check(f"cfg {cfg} forced{'' if onepass else ', mask prologue'}", got, case, fill, dtype)
            keep = outside_fill(case, fill, dtype) if not onepass else slice(None)
            if onepass not in first:
                first[onepass] = got
            assert torch.equal(got[keep], first[onepass][keep]), (cfg, onepass)


def test_deskew_oversized_tile_is_refused(gpu, monkeypatch):
    """Configuration 0 forced where it needs 387 KB of LDS: the launch is refused on the host, nothing runs."""
    shape, angle, ratio, N, cfg = D.NATURAL[4]
    assert D.cfg_lds(shape, D.geometry(shape, angle, ratio, N), N, 0) > D.LDS_MAX
    with pytest.raises((ValueError, RuntimeError), match="exceeds 160 KiB"):
        run(gpu, monkeypatch, (shape, angle, ratio, N, True), 0, CFG=0)
    monkeypatch.delenv("BH_DESKEW_CFG")
    got, _ = run(gpu, monkeypatch, (shape, angle, ratio, N, True), 0)      # and the context is as good as before
    check("after the refusal", got, (shape, angle, ratio, N, True), 0)


def test_deskew_unknown_dtype_code_is_refused(gpu, monkeypatch):
    """A dtype code that is none of the four, without a fill and with a mean fill: BH_ERR_INVALID and the message naming the
    code, nothing is launched (the output buffer keeps its marker), and the next valid call on the context is as good as before."""
    from biahub_amd import _lib
    from biahub_amd.deskew import get_deskewed_data_shape
    from biahub_amd.device import get_context, ptr

    shape, angle, ratio, N, keep, _ = D.EDGES[0]
    vol = _input(shape, "f32", False)[0]
    out = torch.full(get_deskewed_data_shape(shape, angle, ratio, keep, N)[0], -7.0, dtype=torch.float32, device=gpu)
    ctx = get_context(gpu)
    for mode in (_lib.FILL_NONE, _lib.FILL_MEAN):
        with torch.cuda.device(gpu):
            status = ctx.lib.bh_deskew(ctx.handle, ptr(vol), 99, *shape, angle, ratio, int(keep), N, mode, 0.0, ptr(out), None)
        assert status == _lib.BH_ERR_INVALID and _lib.last_error() == "unsupported input dtype code 99", mode
        torch.cuda.synchronize(gpu)
        assert bool((out == -7.0).all()), mode
    for fill in (0, "mean"):
        got, _ = run(gpu, monkeypatch, (shape, angle, ratio, N, keep), fill)
        check("after the refusal", got, (shape, angle, ratio, N, keep), fill)


# ----------------------------------------------------------------------------- the persistent kernel
PERS_MODES = {
    # what: (fill, switches of the persistent run, switches of the tile-kernel run, expected fill path)
    "no fill": (0, dict(PERS=1), dict(PERS=0), 0),
    "mask prologue": ("mean", dict(PERS=1, ONEPASS=0), dict(PERS=0, ONEPASS=0), 0),
    "one pass": ("mean", dict(ROWS_KERNEL="pers"), dict(), 1),
}


def _assert_walk(gpu, shape, angle, ratio, N, ntiles):
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    got = D.persistent(shape, angle, ratio, N)
    assert got is not None and got[0] == ntiles
    assert -(-ntiles // cus) >= 3, (ntiles, cus)        # consecutive tiles of every workgroup that gets any
    if ntiles >= 3 * D.CUS:
        assert ntiles >= 3 * cus, (ntiles, cus)


@pytest.mark.parametrize("mode", list(PERS_MODES))
@pytest.mark.parametrize("shape,angle,ratio,N,ntiles", D.PERSISTENT, ids=[str(c[0]) for c in D.PERSISTENT])
def test_deskew_persistent_walk_vs_float64(gpu, monkeypatch, shape, angle, ratio, N, ntiles, mode):
    """Three and more tiles per workgroup, a good part of them overhang: the persistent kernel without a fill, as the mask
    prologue and in its one-pass form — against float64, and bit-identical to the tile kernel outside the fill.
    ``ntiles >= 3 x multi_processor_count`` is asserted at (48, 400, 128), (24, 576, 128), (24, 575, 128) and the N = 2 and N = 4
    rows.  (24, 402, 128) and
    (24, 401, 128) have 536 tiles, fewer than 3 x 256: a workgroup walks ``ceil(ntiles / grid)`` = 3 consecutive tiles there (the
    179 workgroups that get any), which is what ``_assert_walk`` holds them to — deliberately, not by oversight."""
    _assert_walk(gpu, shape, angle, ratio, N, ntiles)
    case = (shape, angle, ratio, N, True)
    fill, pers_env, tile_env, want_path = PERS_MODES[mode]
    new, path = run(gpu, monkeypatch, case, fill, **pers_env)
    assert path == want_path
    check(f"persistent, {mode}", new, case, fill)
    old, path = run(gpu, monkeypatch, case, fill, **tile_env)
    assert path == want_path
    keep = outside_fill(case, fill) if mode == "mask prologue" else slice(None)
    assert torch.equal(new[keep], old[keep]), (shape, mode)


@pytest.mark.parametrize("shape,angle,ratio,N,ntiles", D.PERSISTENT, ids=[str(c[0]) for c in D.PERSISTENT])
def test_deskew_persistent_walk_with_data_zeros(gpu, monkeypatch, shape, angle, ratio, N, ntiles):
    """A block of exact zeros in the data: the one-pass kernel (tile or persistent) raises its flag and the mask pipeline queued
    behind it — the persistent kernel as the conditional mask prologue — redoes the volume: path 2, and the reference's result."""
    case = (shape, angle, ratio, N, True)
    for fill, env in (("mean", {}), ("mean", dict(ROWS_KERNEL="pers")), (321.5, {}), ("mean", dict(PERS=0))):
        got, path = run(gpu, monkeypatch, case, fill, zb=True, **env)
        assert path == 2, (shape, fill, env)
        check(f"data zeros {env or ''}", got, case, fill, zb=True)
    got, path = run(gpu, monkeypatch, case, "mean")     # the flag is re-armed per call
    assert path == 1


def test_deskew_persistent_kernel_declines_for_lds(gpu, monkeypatch):
    """Two tile buffers of 242 KB: BH_DESKEW_PERS=1 falls back to the tile kernel (configuration 3), same result."""
    case = D.PERSISTENT_DECLINED + (True,)
    assert D.persistent(*D.PERSISTENT_DECLINED) is None and D.selected_cfg(*D.PERSISTENT_DECLINED)[0] == 3
    for fill, env in ((0, dict(PERS=1)), ("mean", dict(PERS=1, ONEPASS=0)), ("mean", dict(ROWS_KERNEL="pers"))):
        got, path = run(gpu, monkeypatch, case, fill, **env)
        check(f"persistent declined {env}", got, case, fill)
        ref, _ = run(gpu, monkeypatch, case, fill, **{**env, "PERS": 0})
        keep = outside_fill(case, fill) if "ONEPASS" in env else slice(None)
        assert torch.equal(got[keep], ref[keep])


# ----------------------------------------------------------------------------- edges
@pytest.mark.parametrize("shape,angle,ratio,N,keep,what", D.EDGES, ids=[e[5].split(":")[0] for e in D.EDGES])
def test_deskew_edges_vs_float64(gpu, monkeypatch, shape, angle, ratio, N, keep, what):
    """The smallest volume, Y < N, keep_overhang=False, Xp = 256 and Xp = 257 (the persistent kernel's 16-byte stores, whole and
    ragged): the default path and every switch, each against float64."""
    case = (shape, angle, ratio, N, keep)
    runs = [(0, {}), (0, dict(PERS=1)), (0, dict(PERS=0))]
    if keep:
        runs += [("mean", {}), ("mean", dict(ROWS_KERNEL="pers")), ("mean", dict(ONEPASS=0)), ("mean", dict(ONEPASS=0, PERS=0)),
                 (321.5, {}), (321.5, dict(ONEPASS=0))]
    for fill, env in runs:
        got, path = run(gpu, monkeypatch, case, fill, **env)
        assert path == (1 if fill != 0 and "ONEPASS" not in env else 0)
        check(f"edge [{what}] {env or ''}", got, case, fill)
    if not keep:   # never fills (reference :538)
        assert torch.equal(run(gpu, monkeypatch, case, "mean")[0], run(gpu, monkeypatch, case, 0)[0])


@pytest.mark.parametrize("shape,angle,ratio,N", [D.NATURAL[0][:4], D.EDGES[4][:4], D.PERSISTENT[1][:4]], ids=str)
def test_deskew_row_sums_handed_in_vs_float64(gpu, monkeypatch, shape, angle, ratio, N):
    """The mean fill from row sums the caller hands in and from row sums the operator reduces itself: both against float64."""
    case = (shape, angle, ratio, N, True)
    rs = _input(shape, "f32", False)[1].to(torch.float64).sum(dim=2).contiguous()
    for env in ({}, dict(ROWS_KERNEL="pers")):
        for row_sums in (None, rs):
            got, path = run(gpu, monkeypatch, case, "mean", row_sums=row_sums, **env)
            assert path == 1
            check(f"row sums {'handed in' if row_sums is not None else 'reduced'} {env or ''}", got, case, "mean")
