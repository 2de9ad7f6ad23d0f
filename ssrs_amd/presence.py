"""Presence density (K3'/K4) host side, behind the reference's function names
(/root/reference/ssrs/movmodel.py:410-439) plus the normalisation ladder of
Simulator.plot_presence_map (simulator.py:520-546)."""

import math

import numpy as np
import torch

from . import _native as nat
from ._device import device, stream_ptr, to_dev, is_tensor, like_input


def _scratch(dev):
    return torch.zeros(8, dtype=torch.uint8, device=dev)


def compute_presence_counts(tracks, gridshape):
    """movmodel.py:410-419.  `tracks`: list of int16 (n_i, 2) arrays (numpy) or
    one CUDA int16 (N, 2) tensor of concatenated points.  Returns an int32
    raster holding uint32 counts (the reference's int16 wraps above 32767)."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    if is_tensor(tracks):
        pts = to_dev(tracks, torch.int16).reshape(-1, 2)
        as_numpy = False
    else:
        as_numpy = True
        tracks = [np.asarray(t, dtype=np.int16).reshape(-1, 2) for t in tracks]
        flat = np.concatenate(tracks) if tracks else np.zeros((0, 2), dtype=np.int16)
        pts = to_dev(flat, torch.int16)
    hist = torch.zeros((rows, cols), dtype=torch.int32, device=device())
    nat.check(nat.lib().ssrs_presence_count(
        nat.ptr(pts), int(pts.shape[0]), nat.ptr(hist), rows, cols,
        nat.ptr(_scratch(hist.device)), stream_ptr()))
    return hist.cpu().numpy() if as_numpy else hist


MAX_OCCUPANCY_PLANES = nat.SSRS_OCCUPANCY_MAX_PLANES


def occupancy_workspace(gridshape, planes):
    """A zeroed workspace of ssrs_track_occupancy for `planes` rasters of `gridshape`: a call leaves it zero, so one
    serves any number of calls."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    nbytes = nat.lib().ssrs_track_occupancy_workspace_bytes(rows, cols, int(planes))
    return torch.zeros(nbytes, dtype=torch.uint8, device=device())


def occupancy_planes(ntracks, gridshape):
    """min(8, ceil(ntracks / 32), the planes that fit in 1/8 of the free device memory), at least 1."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    fit = (torch.cuda.mem_get_info()[0] // 8) // (rows * cols * 4)
    return int(max(1, min(MAX_OCCUPANCY_PLANES, -(-int(ntracks) // 32), fit)))


def compute_track_occupancy(tracks, gridshape, *, offsets=None, counts=None, cells_per_track=False, planes=None,
                            workspace=None):
    """How many DISTINCT tracks passed through each cell (K13, ssrs_track_occupancy): +1 in cell (r, c) for every track
    with at least one point (r, c); points outside the raster are ignored.
    `tracks`: a list of int16 (n_i, 2) host arrays, or a device int16 (points, 2) tensor with `offsets` int64
    (ntracks + 1) as movmodel.simulate_tracks / TrackBatch.iter_device_chunks() give them (`offsets` may be a slice of a
    longer vector: its first entry need not be 0).  Returns the int32 raster holding the uint32 counts, numpy for host
    input and a tensor for device input like compute_presence_counts; with cells_per_track=True also the int32 (ntracks)
    vector of each track's distinct in-raster cells (their sum is the raster's sum).
    counts: an int32 device raster that is ADDED to (chunks and sub-batches accumulate in one raster) and returned.
    planes: 1..8 mask rasters of the workspace, 32 tracks each per round (None: occupancy_planes); the result does not
    depend on it.  workspace: of occupancy_workspace(gridshape, planes), trusted to be zero and left zero (it is
    re-zeroed here if the library call raises); None allocates one."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    if planes is not None and not 1 <= int(planes) <= MAX_OCCUPANCY_PLANES:
        raise ValueError(f'compute_track_occupancy: planes = {planes!r}, expected 1 to {MAX_OCCUPANCY_PLANES}')
    as_numpy = not is_tensor(tracks)
    if as_numpy:
        if offsets is not None:
            raise ValueError('compute_track_occupancy: offsets goes with a device tensor of points, not with a list of tracks')
        tracks = [np.asarray(t) for t in tracks]
        for k, t in enumerate(tracks):
            if t.dtype != np.int16 or t.ndim != 2 or t.shape[1] != 2:
                raise ValueError(f'compute_track_occupancy: track {k} is {t.dtype} {t.shape}, expected int16 (n, 2)')
        flat = np.concatenate(tracks) if tracks else np.zeros((0, 2), dtype=np.int16)
        offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    else:
        if offsets is None:
            raise ValueError('compute_track_occupancy: a tensor of points needs offsets= (int64, ntracks + 1)')
        if tracks.dtype != torch.int16 or tracks.dim() != 2 or int(tracks.shape[1]) != 2:
            raise ValueError(f'compute_track_occupancy: tracks is {tracks.dtype} {tuple(tracks.shape)}, expected int16 '
                             '(points, 2)')
        if not is_tensor(offsets):
            offsets = np.asarray(offsets)
        if offsets.dtype not in (torch.int64, np.int64) or len(offsets.shape) != 1 or int(offsets.shape[0]) < 1:
            raise ValueError('compute_track_occupancy: offsets must be int64 (ntracks + 1)')
        flat = tracks
    pts = to_dev(flat, torch.int16)
    off = to_dev(offsets, torch.int64)
    ntracks = int(off.numel()) - 1
    dev = device()
    if counts is None:
        counts = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
    elif not is_tensor(counts) or counts.dtype != torch.int32 or tuple(counts.shape) != (rows, cols) or \
            not counts.is_contiguous() or not counts.is_cuda:
        raise ValueError(f'compute_track_occupancy: counts must be a contiguous int32 device tensor ({rows}, {cols})')
    per_track = torch.zeros(ntracks, dtype=torch.int32, device=dev) if cells_per_track else None
    if ntracks > 0 and pts.numel() > 0:                  # (empty tensors have no address to hand over)
        if planes is None:
            planes = occupancy_planes(ntracks, gridshape)
        if workspace is None:
            workspace = occupancy_workspace(gridshape, planes)
        elif not is_tensor(workspace) or not workspace.is_cuda or not workspace.is_contiguous():
            raise ValueError('compute_track_occupancy: workspace must be a contiguous device tensor (occupancy_workspace)')
        nbytes = int(workspace.numel()) * workspace.element_size()
        try:
            nat.check(nat.lib().ssrs_track_occupancy(
                nat.ptr(pts), nat.ptr(off), ntracks, rows, cols, int(planes), nat.ptr(counts),
                nat.ptr(per_track), nat.ptr(workspace), nbytes, stream_ptr()))
        except Exception:
            workspace.zero_()
            raise
    out = like_input(counts, None if as_numpy else counts)
    if cells_per_track:
        return out, like_input(per_track, None if as_numpy else per_track)
    return out


MAX_PASSAGE_PLANES = nat.PASSAGE_MAX_PLANES
MAX_PASSAGE_RADIUS = nat.PASSAGE_MAX_RADIUS


def passage_r2(radius_m, resolution):
    """The r2 of compute_track_passage for a radius in metres: radius_cells = radius_m / resolution in f64 and
    floor(radius_cells * radius_cells), no epsilon (a turbine on a cell centre is then counted by
    turbines.turbine_encounters' f64 test for exactly the tracks the passage map counts at that cell).  ValueError for a
    negative or NaN radius and for one of more than 255 cells."""
    radius_m, resolution = float(radius_m), float(resolution)
    if not resolution > 0.:
        raise ValueError(f'passage_r2: resolution = {resolution!r}, expected metres > 0')
    cells = radius_m / resolution
    if not 0. <= cells <= float(MAX_PASSAGE_RADIUS):
        raise ValueError(f'passage_r2: a radius of {radius_m!r} m at a resolution of {resolution!r} m is {cells!r} cells, '
                         f'expected 0 to {MAX_PASSAGE_RADIUS}')
    return int(math.floor(cells * cells))


def passage_workspace(gridshape, planes):
    """A workspace of ssrs_track_passage for `planes` rasters of `gridshape`.  Plain scratch: a call clears what it uses
    itself, so one serves any number of calls, and what it holds in between means nothing."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    nbytes = nat.lib().ssrs_track_passage_workspace_bytes(rows, cols, int(planes))
    return torch.empty(nbytes, dtype=torch.uint8, device=device())


def compute_track_passage(tracks, gridshape, r2, *, offsets=None, counts=None, cells_per_track=False, planes=None,
                          workspace=None, stats=None):
    """How many DISTINCT tracks came within a radius of each cell (K17, ssrs_track_passage): +1 in cell (r, c) for every
    track with an in-raster point p such that (r, c) - p lies in D = {(dr, dc) : dr*dr + dc*dc <= r2}; points outside the
    raster are ignored and disks are clipped to it.  r2: an int in 0..255*255 (passage_r2 makes it from metres); r2 = 0
    is compute_track_occupancy.
    `tracks`, `offsets`, `counts` (ADDED to), `cells_per_track` and what is returned: exactly as
    compute_track_occupancy; cells_per_track counts each track's distinct in-raster cells within the radius, and their
    sum is the raster's sum.
    planes: 1..8 mask rasters of the workspace (None: occupancy_planes); the result does not depend on it.  workspace: of
    passage_workspace(gridshape, planes), scratch whose contents mean nothing before or after; None allocates one.
    stats: an int64 device tensor of two entries, ADDED to: [0] the mask words the set kernels tested (the work),
    [1] the bits they won (= what the call added to the raster)."""
    rows, cols = int(gridshape[0]), int(gridshape[1])
    if isinstance(r2, bool) or not isinstance(r2, (int, np.integer)) or not 0 <= int(r2) <= MAX_PASSAGE_RADIUS ** 2:
        raise ValueError(f'compute_track_passage: r2 = {r2!r}, expected an int from 0 to {MAX_PASSAGE_RADIUS} ** 2')
    if planes is not None and not 1 <= int(planes) <= MAX_PASSAGE_PLANES:
        raise ValueError(f'compute_track_passage: planes = {planes!r}, expected 1 to {MAX_PASSAGE_PLANES}')
    as_numpy = not is_tensor(tracks)
    if as_numpy:
        if offsets is not None:
            raise ValueError('compute_track_passage: offsets goes with a device tensor of points, not with a list of tracks')
        tracks = [np.asarray(t) for t in tracks]
        for k, t in enumerate(tracks):
            if t.dtype != np.int16 or t.ndim != 2 or t.shape[1] != 2:
                raise ValueError(f'compute_track_passage: track {k} is {t.dtype} {t.shape}, expected int16 (n, 2)')
        flat = np.concatenate(tracks) if tracks else np.zeros((0, 2), dtype=np.int16)
        offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    else:
        if offsets is None:
            raise ValueError('compute_track_passage: a tensor of points needs offsets= (int64, ntracks + 1)')
        if tracks.dtype != torch.int16 or tracks.dim() != 2 or int(tracks.shape[1]) != 2:
            raise ValueError(f'compute_track_passage: tracks is {tracks.dtype} {tuple(tracks.shape)}, expected int16 '
                             '(points, 2)')
        if not is_tensor(offsets):
            offsets = np.asarray(offsets)
        if offsets.dtype not in (torch.int64, np.int64) or len(offsets.shape) != 1 or int(offsets.shape[0]) < 1:
            raise ValueError('compute_track_passage: offsets must be int64 (ntracks + 1)')
        flat = tracks
    if stats is not None and (not is_tensor(stats) or stats.dtype != torch.int64 or int(stats.numel()) != 2 or
                              not stats.is_contiguous() or not stats.is_cuda):
        raise ValueError('compute_track_passage: stats must be a contiguous int64 device tensor of two entries')
    pts = to_dev(flat, torch.int16)
    off = to_dev(offsets, torch.int64)
    ntracks = int(off.numel()) - 1
    dev = device()
    if counts is None:
        counts = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
    elif not is_tensor(counts) or counts.dtype != torch.int32 or tuple(counts.shape) != (rows, cols) or \
            not counts.is_contiguous() or not counts.is_cuda:
        raise ValueError(f'compute_track_passage: counts must be a contiguous int32 device tensor ({rows}, {cols})')
    per_track = torch.zeros(ntracks, dtype=torch.int32, device=dev) if cells_per_track else None
    if ntracks > 0 and pts.numel() > 0:                  # (empty tensors have no address to hand over)
        if planes is None:
            planes = occupancy_planes(ntracks, gridshape)
        if workspace is None:
            workspace = passage_workspace(gridshape, planes)
        elif not is_tensor(workspace) or not workspace.is_cuda or not workspace.is_contiguous():
            raise ValueError('compute_track_passage: workspace must be a contiguous device tensor (passage_workspace)')
        nbytes = int(workspace.numel()) * workspace.element_size()
        nat.check(nat.lib().ssrs_track_passage(
            nat.ptr(pts), nat.ptr(off), ntracks, rows, cols, int(r2), int(planes), nat.ptr(counts),
            nat.ptr(per_track), nat.ptr(stats), nat.ptr(workspace), nbytes, stream_ptr()))
    out = like_input(counts, None if as_numpy else counts)
    if cells_per_track:
        return out, like_input(per_track, None if as_numpy else per_track)
    return out


def smooth_presence_counts(count_mat, radius):
    """Disk smoothing of a count matrix (movmodel.py:431-439) -> f32.  int64 counts (the
    widened sum of distributed.reduce_histogram) take the 64-bit kernel, everything else is
    read as uint32-in-int32."""
    cnt = to_dev(count_mat)
    wide = cnt.dtype == torch.int64
    if not wide and cnt.dtype != torch.int32:
        cnt = cnt.to(torch.int32)
    rows, cols = int(cnt.shape[0]), int(cnt.shape[1])
    krad = int(radius)
    out = torch.empty((rows, cols), dtype=torch.float32, device=cnt.device)
    nbytes = nat.lib().ssrs_presence_workspace_bytes(rows, cols, krad)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cnt.device)
    fn = nat.lib().ssrs_presence_smooth_u64 if wide else nat.lib().ssrs_presence_smooth
    nat.check(fn(
        nat.ptr(cnt), krad, nat.ptr(out), rows, cols, nat.ptr(ws), nbytes, stream_ptr()))
    return like_input(out, count_mat)


def compute_smooth_presence_counts(tracks, gridshape, radius):
    """movmodel.py:422-439: histogram + disk smoothing -> f32 (rows, cols)."""
    hist = compute_presence_counts(tracks, gridshape)
    return smooth_presence_counts(hist, radius)


def presence_kernel_radius(radius_m, resolution, gridsize):
    """simulator.py:520 (+ the int(round()) of :530)."""
    krad = min(max(radius_m / resolution, 2), min(gridsize) / 2)
    return int(round(krad))


def windplant_kernel_radius(radius_m, resolution, gridsize):
    """plot_windplant_presence_map hands the same `krad` on UNROUNDED (simulator.py:571, :580) and
    compute_smooth_presence_counts truncates it with int() (movmodel.py:431): 270 m at 100 m is 2 cells here, 3 above."""
    return int(min(max(radius_m / resolution, 2), min(gridsize) / 2))


def normalise_add(src, acc):
    """acc += src / max(src) on the device (simulator.py:531-532, :538-539)."""
    s = to_dev(src)
    if s.dtype not in (torch.float32, torch.float64):
        s = s.to(torch.float64)
    nat.check(nat.lib().ssrs_presence_normalise_add(
        nat.ptr(s), nat.SSRS_F64 if s.dtype == torch.float64 else nat.SSRS_F32,
        nat.ptr(acc), s.numel(), nat.ptr(_scratch(s.device)), stream_ptr()))
    return acc


def normalise_to_f32(src):
    """f32(src / max(src)) (simulator.py:544-546)."""
    s = to_dev(src, torch.float64)
    out = torch.empty(s.shape, dtype=torch.float32, device=s.device)
    nat.check(nat.lib().ssrs_presence_normalise_f32(
        nat.ptr(s), nat.ptr(out), s.numel(), nat.ptr(_scratch(s.device)), stream_ptr()))
    return out
