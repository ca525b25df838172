"""The stabilisation estimate on MI355X — mirror of ``biahub/estimate_stabilization.py``.

Three of the reference's estimators run here, each around one device primitive:

* ``phase-cross-corr`` (``stabilization_type: xyz``; :129-310, :444-693): ``bh_phase_cross_corr`` — two R2C transforms, the
  fused normalised conjugate product, C2R, |.| + first-occurrence argmax on device — under the
  reference's call chain ``phase_cross_corr_padding``, ``get_tform_from_pcc``, ``estimate_xyz_stabilization_pcc[_per_position]``.
* ``focus-finding`` (``stabilization_type: z``, the reference's default method; :900-1220): ``bh_focus_band_power`` — the
  mid-band power of every z-slice of the centre window (``biahub_amd/focus.py``) — under
  ``estimate_z_focus_per_position``, ``get_mean_z_positions`` and ``estimate_z_stabilization``.
* StackReg translation (``stabilization_type: xy`` and ``xyz`` with ``focus-finding``; :696-897): ``bh_stackreg_translation`` —
  the in-focus plane of every timepoint registered against the first or the previous one in one batched solve
  (``biahub_amd/stackreg.py``) — under ``estimate_xy_stabilization[_per_position]``.

Either way ``estimate-stabilization`` writes the per-timepoint 4x4 matrices ``stabilize`` consumes.  Bead matching lives in
``registration/beads.py``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .device import as_device_volume, get_context, ptr, resolve_device, to_host


def phase_cross_corr_device(ref_img, mov_img, normalization=None, device="cuda", want_corr: bool = True):
    """Device-level correlation: ``(shift float32[3], corr tensor or None)``.  With ``want_corr=False`` the correlation
    volume is neither written nor copied (a 1-GB volume costs ~80 ms to bring to the host; the shift costs nothing)."""
    if normalization not in _lib.PCC_NORM:
        raise ValueError(f"unknown normalization {normalization!r}")
    dev = resolve_device(device if not isinstance(ref_img, torch.Tensor) else ref_img.device)
    a, _, _ = as_device_volume(ref_img, dev)
    b, _, _ = as_device_volume(mov_img, dev)
    a, b = a.to(torch.float32), b.to(torch.float32)
    if a.ndim != 3 or a.shape != b.shape:
        raise ValueError(f"expected two 3-D images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    Z, Y, X = (int(s) for s in a.shape)
    ctx = get_context(dev)
    shift = (C.c_float * 3)()
    with torch.cuda.device(dev):
        # irfftn without a shape: an odd last axis comes back one shorter (the reference's behaviour, kept)
        corr = torch.empty((Z, Y, X - (X & 1)), dtype=torch.float32, device=dev) if want_corr else None
        _lib.check(ctx.lib.bh_phase_cross_corr(ctx.handle, ptr(a), ptr(b), Z, Y, X, _lib.PCC_NORM[normalization],
                                               shift, ptr(corr) if want_corr else None))
    return np.array(list(shift), dtype=np.float32), corr


class PreparedPhaseCrossCorr:
    """``phase_cross_corr`` with ONE of the two images fixed (``bh_phase_cross_corr_create``): its spectrum is computed once, a
    call transforms the other image only.  The stabilisation estimate correlates every timepoint with the first one — or, with
    ``roll=True``, with its predecessor: the image of a call then becomes the stored one, its spectrum a by-product of the
    call's own Z pass (estimate_stabilization.py:505-520).  ``fixed_is_second``: the stored image is ``phase_cross_corr``'s
    second argument (``mov_img``), as in ``get_tform_from_pcc``, which passes the varying timepoint first."""

    def __init__(self, fixed_img, fixed_is_second: bool = False, device="cuda"):
        self.device = resolve_device(device if not isinstance(fixed_img, torch.Tensor) else fixed_img.device)
        a, _, _ = as_device_volume(fixed_img, self.device)
        a = a.to(torch.float32)
        if a.ndim != 3:
            raise ValueError(f"expected a 3-D image, got shape {tuple(a.shape)}")
        self.shape = tuple(int(n) for n in a.shape)
        self.fixed_is_second = bool(fixed_is_second)
        self._ctx = get_context(self.device)
        self._handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._ctx.lib.bh_phase_cross_corr_create(self._ctx.handle, ptr(a), *self.shape, int(self.fixed_is_second),
                                                                C.byref(self._handle)))
            torch.cuda.current_stream(self.device).synchronize()  # the image may be dropped by the caller from here on

    def __call__(self, img, normalization=None, want_corr: bool = False, roll: bool = False):
        """``(shift float32[3], fftshift(|corr|) tensor or None)`` of ``phase_cross_corr(fixed, img)`` — of
        ``phase_cross_corr(img, fixed)`` when ``fixed_is_second``."""
        if normalization not in _lib.PCC_NORM:
            raise ValueError(f"unknown normalization {normalization!r}")
        b, _, _ = as_device_volume(img, self.device)
        b = b.to(torch.float32)
        if tuple(b.shape) != self.shape:
            raise ValueError(f"image shape {tuple(b.shape)} != the shape this handle was prepared for {self.shape}")
        Z, Y, X = self.shape
        shift = (C.c_float * 3)()
        with torch.cuda.device(self.device):
            corr = torch.empty((Z, Y, X - (X & 1)), dtype=torch.float32, device=self.device) if want_corr else None
            _lib.check(self._ctx.lib.bh_phase_cross_corr_apply(self._ctx.handle, self._handle, ptr(b), _lib.PCC_NORM[normalization],
                                                               int(bool(roll)), shift, ptr(corr) if want_corr else None))
        return np.array(list(shift), dtype=np.float32), corr

    def close(self) -> None:
        if self._handle:
            torch.cuda.synchronize(self.device)
            _lib.check(self._ctx.lib.bh_phase_cross_corr_destroy(self._handle))
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def phase_cross_corr(ref_img, mov_img, normalization=None, output_path=None, verbose: bool = False, device="cuda"):
    """Translation between two equally shaped 3-D images: ``(shift, corr_shifted)`` like the reference.

    ``shift`` is a float32 array (the signed location of max |corr|), ``corr_shifted = fftshift(|corr|)``.
    ``normalization`` is ``None``, ``"magnitude"`` or ``"classic"`` (estimate_stabilization.py:233-238).
    """
    shift, corr = phase_cross_corr_device(ref_img, mov_img, normalization, device, want_corr=True)
    return shift, to_host(corr)


# ----------------------------------------------------------------------------- padding variant and the per-position chain
def pad_to_shape(arr, shape, mode: str, **kwargs):
    """``registration/utils.py:856-896``: centred ``np.pad`` up to ``shape``."""
    assert arr.ndim == len(shape)
    dif = tuple(s - a for s, a in zip(shape, arr.shape))
    assert all(d >= 0 for d in dif)
    return np.pad(arr, pad_width=[[s // 2, s - s // 2] for s in dif], mode=mode, **kwargs)


def center_crop(arr, shape):
    """``registration/utils.py:899-924``."""
    assert arr.ndim == len(shape)
    starts = tuple((cur - s) // 2 for cur, s in zip(arr.shape, shape))
    assert all(s >= 0 for s in starts)
    return arr[tuple(slice(s, s + d) for s, d in zip(starts, shape))]


def match_shape(img, shape):
    """``registration/utils.py:927-958``: reflect-pad the short axes, centre-crop the long ones."""
    if np.any(np.asarray(shape) > np.asarray(img.shape)):
        img = pad_to_shape(img, tuple(np.maximum(img.shape, shape)), mode="reflect")
    if np.any(np.asarray(shape) < np.asarray(img.shape)):
        img = center_crop(img, shape)
    return img


def phase_cross_corr_padding(ref_img, mov_img, maximum_shift: float = 1.2, normalization=None, output_path=None,
                             verbose: bool = False, device="cuda"):
    """``estimate_stabilization.py:129-196``: both images padded / cropped to ``next_fast_len(max(s) * maximum_shift)``, then
    the same correlation; returns ``(peak, fftshift(|corr|))`` with ``peak = s // 2 - argmax`` (note the sign convention
    differs from ``phase_cross_corr``)."""
    from scipy.fftpack import next_fast_len  # 5-smooth sizes, as the reference imports it

    ref_img, mov_img = np.asarray(ref_img), np.asarray(mov_img)
    shape = tuple(int(next_fast_len(int(max(s1, s2) * maximum_shift))) for s1, s2 in zip(ref_img.shape, mov_img.shape))
    if verbose:
        print(f"phase cross corr. fft shape of {shape} for arrays of shape {ref_img.shape} and {mov_img.shape} "
              f"with maximum shift of {maximum_shift}")
    ref_img = np.ascontiguousarray(match_shape(ref_img, shape))
    mov_img = np.ascontiguousarray(match_shape(mov_img, shape))
    shift, corr = phase_cross_corr(ref_img, mov_img, normalization=normalization, device=device)
    # argmax position m of |corr| (signed shift folded back), seen through fftshift: p = (m + s // 2) % s
    peak = tuple(int(s // 2 - ((int(sh) % s) + s // 2) % s) for s, sh in zip(corr.shape, shift))
    if verbose:
        print(f"phase cross corr. peak at {peak}")
    return peak, corr


def get_tform_from_pcc(t: int, source_channel_tzyx, target_channel_tzyx, function_type: str = "custom", normalization=None,
                       output_path=None, verbose: bool = False, device="cuda", want_corr: bool = True):
    """``estimate_stabilization.py:259-310``, kept as written: the image named ``target`` is read from the *source* stack
    and vice versa, and the shift lands as ``transform[0, 3] = dx, [1, 3] = dy, [2, 3] = dz``."""
    target = np.asarray(source_channel_tzyx[t]).astype(np.float32)
    source = np.asarray(target_channel_tzyx[t]).astype(np.float32)
    if function_type == "custom_padding":
        shift, corr = phase_cross_corr_padding(target, source, normalization=normalization, device=device)
    elif function_type == "custom":
        if want_corr:
            shift, corr = phase_cross_corr(target, source, normalization=normalization, device=device)
        else:  # the per-position loop only reads the correlation volume for its verbose statistics
            shift, corr = phase_cross_corr_device(target, source, normalization, device, want_corr=False)
    else:
        raise ValueError(f"unknown function_type {function_type!r}")
    if verbose:
        print(f"Time {t}: shift (dz,dy,dx) = {shift[0]}, {shift[1]}, {shift[2]}")
    dz, dy, dx = shift
    transform = np.eye(4)
    transform[0, 3] = dx
    transform[1, 3] = dy
    transform[2, 3] = dz
    return transform, shift, corr


def remove_beads_fov_from_path_list(position_dirpaths, skip_beads_fov: str):
    """``estimate_stabilization.py:50-74``."""
    if skip_beads_fov != "0":
        print(f"Removing beads FOV {skip_beads_fov} from input data paths")
        position_dirpaths = [p for p in position_dirpaths if skip_beads_fov not in str(p)]
    return position_dirpaths


def _axis_slice(spec, n):
    return slice(0, n) if spec == "all" else slice(spec[0], spec[1])


def estimate_xyz_stabilization_pcc_per_position(input_position_dirpath, output_folder_path, output_shifts_path,
                                                channel_index: int, phase_cross_corr_settings, verbose: bool = False,
                                                device="cuda"):
    """``estimate_stabilization.py:444-587``: one transform per timepoint against the first or the previous timepoint;
    saves ``<row>_<col>_<fov>.npy`` (float32) and, when verbose, the shifts as csv.  Plots are not produced."""
    from pathlib import Path

    from .io import open_ome_zarr

    s = phase_cross_corr_settings
    input_position_dirpath = Path(input_position_dirpath)
    data = open_ome_zarr(input_position_dirpath).data
    T, _, Z, Y, X = data.shape
    # the reference computes a centre crop first and then overrides it with the X/Y slices (:476-496); same here
    x_idx, y_idx, z_idx = _axis_slice(s.X_slice, X), _axis_slice(s.Y_slice, Y), _axis_slice(s.Z_slice, Z)
    if verbose:
        print(f"x_idx: {x_idx}, y_idx: {y_idx}, z_idx: {z_idx}")
    vols = [np.asarray(data[t, channel_index][z_idx, y_idx, x_idx]) for t in range(T)]
    source = vols
    target = [vols[0]] * T if s.t_reference == "first" else [vols[0]] + vols[:-1]
    name = "_".join(input_position_dirpath.parts[-3:])
    transforms, shifts = [], []
    # function_type "custom": get_tform_from_pcc calls phase_cross_corr(source[t], target[t]) — the varying timepoint first, the
    # reference timepoint as the conjugated factor.  The reference image's spectrum is computed once ("first") or falls out of
    # the previous call ("previous": roll) instead of being rebuilt for every timepoint; same shifts (tests/test_io_cli.py).
    prepared = None
    if s.function_type == "custom" and T > 1:
        prepared = PreparedPhaseCrossCorr(vols[0].astype(np.float32), fixed_is_second=True, device=device)
    for t in range(T):
        if t == 0:
            transforms.append(np.eye(4).tolist())
            shifts.append((t, 0, 0, 0))
            continue
        if prepared is not None:
            shift, _ = prepared(vols[t].astype(np.float32), s.normalization, want_corr=False, roll=s.t_reference == "previous")
            if verbose:
                print(f"Time {t}: shift (dz,dy,dx) = {shift[0]}, {shift[1]}, {shift[2]}")
            transform = np.eye(4)
            transform[0, 3], transform[1, 3], transform[2, 3] = shift[2], shift[1], shift[0]
        else:
            transform, shift, _corr = get_tform_from_pcc(t, source, target, function_type=s.function_type,
                                                         normalization=s.normalization, verbose=verbose, device=device,
                                                         want_corr=False)
        transforms.append(transform)
        shifts.append((t, *[float(v) for v in shift]))
    if prepared is not None:
        prepared.close()
    output_folder_path = Path(output_folder_path)
    output_folder_path.mkdir(parents=True, exist_ok=True)
    np.save(output_folder_path / f"{name}.npy", np.array(transforms, dtype=np.float32))
    if verbose:
        Path(output_shifts_path).mkdir(parents=True, exist_ok=True)
        with open(Path(output_shifts_path) / f"{name}.csv", "w") as f:
            f.write("TimepointID,ShiftZ,ShiftY,ShiftX\n")
            for row in shifts:
                f.write(",".join(str(v) for v in row) + "\n")
    return transforms


def estimate_xyz_stabilization_pcc(input_position_dirpaths, output_folder_path, phase_cross_corr_settings,
                                   channel_index: int = 0, sbatch_filepath=None, cluster: str = "local",
                                   verbose: bool = False, device="cuda") -> dict:
    """``estimate_stabilization.py:590-693``: every position (sharded over ranks instead of submitit jobs), then the
    per-position ``.npy`` files are gathered into ``{fov_name: transforms}`` and the temporary folder is removed."""
    import shutil
    from pathlib import Path

    from . import parallel

    input_position_dirpaths = remove_beads_fov_from_path_list(list(input_position_dirpaths),
                                                              phase_cross_corr_settings.skip_beads_fov)
    output_folder_path = Path(output_folder_path)
    transforms_out = output_folder_path / "transforms_per_position"
    shifts_out = output_folder_path / "shifts_per_position"
    transforms_out.mkdir(parents=True, exist_ok=True)
    rank, world = parallel.init()  # binds this rank to GPU LOCAL_RANK before any device call
    for p in parallel.shard_positions(input_position_dirpaths, rank, world):
        estimate_xyz_stabilization_pcc_per_position(p, transforms_out, shifts_out, channel_index,
                                                    phase_cross_corr_settings, verbose=verbose, device=device)
    parallel.barrier()
    fov_transforms = {f.stem: np.load(f).tolist() for f in sorted(transforms_out.glob("*.npy"))}
    parallel.barrier()
    if rank == 0:
        shutil.rmtree(transforms_out)
    return fov_transforms


# ----------------------------------------------------------------------------- focus finding: the z chain (:900-1220)
NA_DET = 1.35
LAMBDA_ILL = 0.5
FOCUS_CSV_COLUMNS = ("position", "time_idx", "channel", "focus_idx")


def _write_focus_csv(path, rows) -> None:
    import csv

    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(FOCUS_CSV_COLUMNS)
        w.writerows(rows)


def _read_focus_csv(path) -> list[tuple]:
    """Rows ``(position, time_idx int, channel, focus_idx)``; ``focus_idx`` is an int where the file holds one, a float (NaN
    for an empty field) otherwise."""
    import csv

    def num(x):
        if x == "":
            return float("nan")
        try:
            return int(x)
        except ValueError:
            return float(x)

    with open(path, newline="") as f:
        return [(r["position"], int(r["time_idx"]), r["channel"], num(r["focus_idx"])) for r in csv.DictReader(f)]


def z_transforms_from_focus(focus_idx) -> np.ndarray:
    """``estimate_stabilization.py:980-993``: ``[eye] + [eye with [0, 3] = f - f_ref for f in focus_idx[1:]]``, ``f_ref`` the
    first index that is neither 0 (an empty FOV, a failed estimate) nor NaN."""
    z_ref = next((v for v in focus_idx if v != 0 and not np.isnan(v)), None)
    if z_ref is None:
        raise ValueError("Z index of focus reference is None, focus_idx contains only zeros")
    out = [np.eye(4)]
    for v in list(focus_idx)[1:]:
        shift = np.eye(4)
        shift[0, 3] = v - z_ref
        out.append(shift)
    return np.array(out)


def merge_focus_rows(new_rows, old_rows=()) -> list[tuple]:
    """``estimate_stabilization.py:1160-1168``: new rows first, an existing file's rows after them, duplicates on
    ``(position, time_idx)`` dropped keeping the first, sorted by ``(position, time_idx)`` (stable)."""
    seen, merged = set(), []
    for r in list(new_rows) + list(old_rows):
        key = (r[0], r[1])
        if key not in seen:
            seen.add(key)
            merged.append(tuple(r))
    return sorted(merged, key=lambda r: (r[0], r[1]))


def centre_window(Y: int, X: int, center_crop_xy) -> tuple[slice, slice]:
    """The reference's window ``[Y//2 - cy//2 : Y//2 + cy//2, X//2 - cx//2 : X//2 + cx//2]`` for ``center_crop_xy = [cx, cy]``
    (:938-942).  A crop larger than the FOV is refused: the reference's slice then starts at a negative index, which numpy
    counts from the end, and the window it cuts is off-centre (or the whole FOV, once the crop is twice the FOV)."""
    cx, cy = (int(v) for v in center_crop_xy)
    if cx < 2 or cy < 2 or cx > X or cy > Y:
        raise ValueError(f"center_crop_xy {[cx, cy]} does not fit the FOV (Y, X) = ({Y}, {X}): the reference's slice would wrap to "
                         "an off-centre window, which is not available in biahub_amd; set focus_finding_settings.center_crop_xy "
                         "to at most the FOV")
    return slice(Y // 2 - cy // 2, Y // 2 + cy // 2), slice(X // 2 - cx // 2, X // 2 + cx // 2)


def estimate_z_focus_per_position(input_position_dirpath, input_channel_indices, center_crop_xy, output_path_focus_csv,
                                  output_path_transform, verbose: bool = False, device="cuda") -> None:
    """``estimate_stabilization.py:900-1000``: the focus slice of every (timepoint, channel) from the centre window
    (``centre_window``); only the window is uploaded.
    An empty window (sum 0) gets index 0.  Writes ``<row>_<col>_<fov>.csv`` and the z-shift matrices ``<row>_<col>_<fov>.npy``."""
    import itertools
    from pathlib import Path

    from .focus import focus_from_power, midband_power_and_sum
    from .io import open_ome_zarr

    input_position_dirpath = Path(input_position_dirpath)
    position = str(Path(*input_position_dirpath.parts[-3:]))
    rows = []
    with open_ome_zarr(input_position_dirpath) as dataset:
        channel_names = dataset.channel_names
        T, _, Z, Y, X = dataset.data.shape
        pixel_size = float(dataset.scale[-1])
        ys, xs = centre_window(Y, X, center_crop_xy)
        for t, c in itertools.product(range(T), input_channel_indices):
            window = np.asarray(dataset.data[t, c][:, ys, xs])
            if Z == 1:
                z_idx = 0
            else:
                power, total = midband_power_and_sum(window, NA_DET, LAMBDA_ILL, pixel_size, device=device)
                if total == 0:  # an empty FOV: the focal plane is 0
                    z_idx = 0
                else:
                    z_idx = focus_from_power(power)
                    print(f"Estimating focus for timepoint {t} and channel {c}: {z_idx}")
            rows.append((position, t, channel_names[c], z_idx))
    output_path_focus_csv = Path(output_path_focus_csv)
    output_path_focus_csv.mkdir(parents=True, exist_ok=True)
    if verbose:
        print(f"Saving focus finding results to {output_path_focus_csv}")
    name = position.replace("/", "_")
    _write_focus_csv(output_path_focus_csv / f"{name}.csv", rows)
    transform = z_transforms_from_focus([r[3] for r in rows])
    output_path_transform = Path(output_path_transform)
    output_path_transform.mkdir(parents=True, exist_ok=True)
    np.save(output_path_transform / f"{name}.npy", transform)
    if verbose:
        print(f"Saved Z transform matrices to {output_path_transform}")


def get_mean_z_positions(dataframe_path, verbose: bool = False, method: str = "mean") -> np.ndarray:
    """``estimate_stabilization.py:1003-1049`` without the plot: rows sorted by ``time_idx``, a focus index of 0 read as NaN,
    then the NaN-skipping mean or median of every ``time_idx`` (NaN where a timepoint has no estimate)."""
    if method not in ("mean", "median"):
        raise ValueError(f"unknown method {method!r}")
    rows = sorted(_read_focus_csv(dataframe_path), key=lambda r: r[1])
    groups: dict = {}
    for _, t, _, f in rows:
        groups.setdefault(t, []).append(np.nan if f == 0 else float(f))
    out = []
    for t in sorted(groups):
        v = np.array([x for x in groups[t] if not np.isnan(x)], dtype=np.float64)
        out.append(np.nan if v.size == 0 else float(np.mean(v) if method == "mean" else np.median(v)))
    return np.array(out, dtype=np.float64)


def estimate_z_stabilization(input_position_dirpaths, output_folder_path, focus_finding_settings, channel_index: int,
                             sbatch_filepath=None, cluster: str = "local", verbose: bool = False, estimate_z_index: bool = False,
                             device="cuda"):
    """``estimate_stabilization.py:1052-1220``: every position (sharded over ranks instead of submitit jobs); rank 0 merges
    the per-position tables into ``positions_focus.csv`` and every rank returns ``{"average": transforms}`` with
    ``average_across_wells``, else ``{<row>_<col>_<fov>: transforms}``; ``None`` with ``estimate_z_index``.
    ``focus_finding_settings``: a ``FocusFindingSettings``, a dict of its fields, or ``None`` for the defaults."""
    import shutil
    from pathlib import Path

    from . import parallel
    from .settings import FocusFindingSettings

    s = focus_finding_settings
    if s is None:
        s = FocusFindingSettings()
    elif isinstance(s, dict):
        s = FocusFindingSettings(**s)
    input_position_dirpaths = remove_beads_fov_from_path_list(list(input_position_dirpaths), s.skip_beads_fov)
    output_folder_path = Path(output_folder_path)
    focus_out = output_folder_path / "z_focus_positions"
    transforms_out = output_folder_path / "z_transforms"
    focus_out.mkdir(parents=True, exist_ok=True)
    transforms_out.mkdir(parents=True, exist_ok=True)
    rank, world = parallel.init()  # binds this rank to GPU LOCAL_RANK before any device call
    for p in parallel.shard_positions(input_position_dirpaths, rank, world):
        estimate_z_focus_per_position(p, (channel_index,), s.center_crop_xy, focus_out, transforms_out, verbose=verbose, device=device)
    parallel.barrier()
    merged_path = output_folder_path / "positions_focus.csv"
    if rank == 0:
        csvs = sorted(focus_out.glob("*.csv"))
        if len(csvs) != len(input_position_dirpaths):
            print(f"Warning: {len(csvs)} focus CSV files found for {len(input_position_dirpaths)} input data paths.")
        new_rows = [r for f in csvs for r in _read_focus_csv(f)]
        old_rows = []
        if merged_path.exists():
            print("Using existing focus CSV file.")
            old_rows = _read_focus_csv(merged_path)
        _write_focus_csv(merged_path, merge_focus_rows(new_rows, old_rows))
    parallel.barrier()
    result = None
    if not estimate_z_index:
        if s.average_across_wells:
            offsets = get_mean_z_positions(merged_path, method=s.average_across_wells_method, verbose=verbose)
            try:
                result = {"average": z_transforms_from_focus(offsets).tolist()}
            except ValueError:
                raise ValueError("Z index of focus reference is None; no valid (non-zero, non-NaN) z-index found in "
                                 "z_drift_offsets") from None
            if verbose and rank == 0:
                print(f"Saving z focus shift matrices to {output_folder_path}")
                np.save(output_folder_path / "z_focus_shift.npy", result["average"])
        else:
            result = {f.stem: np.load(f).tolist() for f in sorted(transforms_out.glob("*.npy"))}
    parallel.barrier()
    if rank == 0:
        shutil.rmtree(focus_out)
        shutil.rmtree(transforms_out)
    return result


# ----------------------------------------------------------------------------- StackReg: the xy chain (:696-897)
def fill_focus_indices(focus_idx) -> list[int]:
    """``estimate_stabilization.py:739-742``: ``focus_idx.replace(0, nan).ffill().fillna(focus_idx.mean()).astype(int)``.  A 0
    (an empty FOV, a failed estimate) takes the last estimate before it; what is still missing — the timepoints before the
    first estimate — takes the mean, which the reference takes over the column as read: zeros count, NaN does not."""
    v = np.asarray(list(focus_idx), dtype=np.float64)
    mean = float(np.mean(v[~np.isnan(v)])) if (~np.isnan(v)).any() else np.nan
    w = np.where(v == 0, np.nan, v)
    last = np.nan
    for i in range(len(w)):
        if np.isnan(w[i]):
            w[i] = last
        else:
            last = w[i]
    w = np.where(np.isnan(w), mean, w)
    if np.isnan(w).any():
        raise ValueError("focus_idx holds no estimate to fill the missing timepoints from")
    return [int(x) for x in w]


def xy_transforms_from_stackreg(T_stackreg) -> np.ndarray:
    """``estimate_stabilization.py:758-764``: the translations swapped (x, y) -> (y, x) and the 3 x 3 matrices embedded into
    ``[1:4, 1:4]`` of 4 x 4 ZYX matrices: ``[1, 3]`` is the y shift, ``[2, 3]`` the x shift."""
    m = np.array(T_stackreg, dtype=np.float64)
    m[:, [0, 1], 2] = m[:, [1, 0], 2]
    transform = np.zeros((m.shape[0], 4, 4))
    transform[:, 1:4, 1:4] = m
    transform[:, 0, 0] = 1
    return transform


def estimate_xy_stabilization_per_position(input_position_dirpath, output_folder_path, df_z_focus_path, channel_index: int,
                                           center_crop_xy, t_reference: str = "previous", verbose: bool = False, device="cuda"):
    """``estimate_stabilization.py:696-771``: one plane per timepoint, at its focus slice (``fill_focus_indices`` of the
    position's rows of the focus table) and in the centre window, clipped below at 0 and registered by ``register_stack``;
    saves ``<row>_<col>_<fov>.npy`` (float32) and returns the float64 matrices."""
    from pathlib import Path

    from .io import open_ome_zarr
    from .stackreg import register_stack

    input_position_dirpath = Path(input_position_dirpath)
    position = str(Path(*input_position_dirpath.parts[-3:]))
    with open_ome_zarr(input_position_dirpath) as dataset:
        T, _, Z, Y, X = dataset.data.shape
        ys, xs = centre_window(Y, X, center_crop_xy)
        if verbose:
            print(f"Reading focus index from {df_z_focus_path}")
        z_idx = fill_focus_indices([r[3] for r in _read_focus_csv(df_z_focus_path) if r[0] == position])
        if len(z_idx) != T:
            raise ValueError(f"{df_z_focus_path} holds {len(z_idx)} focus indices for {position}, the position has {T} timepoints")
        if min(z_idx) < 0 or max(z_idx) >= Z:
            raise ValueError(f"{df_z_focus_path}: focus indices {z_idx} of {position} leave the {Z} slices of the position")
        if verbose:
            print("Calculating xy stabilization...")
        tyx = np.stack([np.asarray(dataset.data[t, channel_index, z, ys, xs]) for t, z in zip(range(T), z_idx)])
    T_stackreg = register_stack(tyx, reference=t_reference, device=device)  # the kernel reads values below 0 as 0 (:753)
    transform = xy_transforms_from_stackreg(T_stackreg)
    output_folder_path = Path(output_folder_path)
    output_folder_path.mkdir(parents=True, exist_ok=True)
    np.save(output_folder_path / f"{position.replace('/', '_')}.npy", transform.astype(np.float32))
    return transform


def estimate_xy_stabilization(input_position_dirpaths, output_folder_path, stack_reg_settings, channel_index: int = 0,
                              sbatch_filepath=None, cluster: str = "local", verbose: bool = False, device="cuda") -> dict:
    """``estimate_stabilization.py:774-897``: ``positions_focus.csv`` of the output folder is reused when it exists, otherwise
    written by ``estimate_z_stabilization(estimate_z_index=True)`` with the nested focus settings; then every position (sharded
    over ranks instead of submitit jobs); returns ``{<row>_<col>_<fov>: transforms}``.
    ``stack_reg_settings``: a ``StackRegSettings``, a dict of its fields, or ``None`` for the defaults."""
    import shutil
    from pathlib import Path

    from . import parallel
    from .settings import StackRegSettings

    s = stack_reg_settings
    if s is None:
        s = StackRegSettings()
    elif isinstance(s, dict):
        s = StackRegSettings(**s)
    input_position_dirpaths = remove_beads_fov_from_path_list(list(input_position_dirpaths), s.skip_beads_fov)
    output_folder_path = Path(output_folder_path)
    output_folder_path.mkdir(parents=True, exist_ok=True)
    df_focus_path = output_folder_path / "positions_focus.csv"
    rank, world = parallel.init()  # binds this rank to GPU LOCAL_RANK before any device call
    if df_focus_path.exists():
        print("Using existing Z focus index file.")
    else:
        print("Estimating Z focus positions...")
        estimate_z_stabilization(input_position_dirpaths, output_folder_path, s.focus_finding_settings, channel_index,
                                 sbatch_filepath=sbatch_filepath, cluster=cluster, verbose=verbose, estimate_z_index=True,
                                 device=device)
    parallel.barrier()
    transforms_out = output_folder_path / "xy_transforms"
    transforms_out.mkdir(parents=True, exist_ok=True)
    for p in parallel.shard_positions(input_position_dirpaths, rank, world):
        estimate_xy_stabilization_per_position(p, transforms_out, df_focus_path, channel_index, s.center_crop_xy,
                                               t_reference=s.t_reference, verbose=verbose, device=device)
    parallel.barrier()
    fov_transforms = {f.stem: np.load(f).tolist() for f in sorted(transforms_out.glob("*.npy"))}
    parallel.barrier()
    if rank == 0:
        shutil.rmtree(transforms_out)
    return fov_transforms


def save_transforms(model, transforms, output_filepath_settings, output_filepath_plot=None, verbose: bool = False):
    """``registration/utils.py:370-422``: the settings file, and with ``verbose`` and a plot path the translations over time as
    a png."""
    from pathlib import Path

    from .registration.utils import plot_translations
    from .utils.config import model_to_yaml

    if transforms is None or len(transforms) == 0:
        raise ValueError("Transforms are empty")
    if not isinstance(transforms, list):
        transforms = transforms.tolist()
    model.affine_transform_zyx_list = transforms
    output_filepath_settings = Path(output_filepath_settings)
    if output_filepath_settings.suffix not in [".yml", ".yaml"]:
        output_filepath_settings = output_filepath_settings.with_suffix(".yml")
    output_filepath_settings.parent.mkdir(parents=True, exist_ok=True)
    model_to_yaml(model, output_filepath_settings)
    if verbose and output_filepath_plot is not None:
        output_filepath_plot = Path(output_filepath_plot)
        if output_filepath_plot.suffix not in [".png"]:
            output_filepath_plot = output_filepath_plot.with_suffix(".png")
        output_filepath_plot.parent.mkdir(parents=True, exist_ok=True)
        plot_translations(np.asarray(transforms), output_filepath_plot)
