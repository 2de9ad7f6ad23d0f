"""Flight height along the tracks and rotor-zone presence (K14, include/ssrs_hip.h "altitude"): THIS BUILD'S OWN model --
the reference has no altitude model.  Heights are int32 millimetres above ground inside the library; metres come in
here."""
import ctypes as C

import numpy as np
import torch

from . import _native as nat
from ._device import device, stream_ptr, to_dev, is_tensor, like_input, ftype

TILE = nat.SSRS_ALTITUDE_TILE
_I32 = (-2 ** 31, 2 ** 31 - 1)


def to_mm(metres, name='height'):
    """int(round(1000 * metres)), refused outside int32."""
    x = float(metres)
    if x != x:
        raise ValueError(f'{name} = {metres!r}: not a number')
    mm = int(round(1000. * x))
    if not _I32[0] <= mm <= _I32[1]:
        raise ValueError(f'{name} = {metres!r} m does not fit int32 millimetres')
    return mm


def height_params(start, floor, ceil, band, who='compute_track_altitudes'):
    """SsrsAltitudeParams of heights in metres; band = (lo, hi) inclusive."""
    try:
        band_lo, band_hi = band
    except (TypeError, ValueError):
        raise ValueError(f'{who}: band = {band!r}, expected (lo, hi) in metres') from None
    p = nat.SsrsAltitudeParams(to_mm(start, 'start'), to_mm(floor, 'floor'), to_mm(ceil, 'ceil'),
                               to_mm(band_lo, 'band[0]'), to_mm(band_hi, 'band[1]'))
    if p.floor > p.ceil:
        raise ValueError(f'{who}: floor = {floor!r} m above ceil = {ceil!r} m')
    if p.band_lo > p.band_hi:
        raise ValueError(f'{who}: band = {band!r}, its lower end is above its upper end')
    return p


def _points_and_offsets(tracks, offsets, who):
    """(host input?, the points int16 (points, 2), the offsets int64 (ntracks + 1)) of the two forms the track consumers take:
    a list of int16 (n_i, 2) host arrays, or a device tensor of points with `offsets`."""
    as_numpy = not is_tensor(tracks)
    if as_numpy:
        if offsets is not None:
            raise ValueError(f'{who}: offsets goes with a device tensor of points, not with a list of tracks')
        tracks = [np.asarray(t) for t in tracks]
        for k, t in enumerate(tracks):
            if t.dtype != np.int16 or t.ndim != 2 or t.shape[1] != 2:
                raise ValueError(f'{who}: track {k} is {t.dtype} {t.shape}, expected int16 (n, 2)')
        flat = np.concatenate(tracks) if tracks else np.zeros((0, 2), dtype=np.int16)
        offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    else:
        if offsets is None:
            raise ValueError(f'{who}: a tensor of points needs offsets= (int64, ntracks + 1)')
        if tracks.dtype != torch.int16 or tracks.dim() != 2 or int(tracks.shape[1]) != 2:
            raise ValueError(f'{who}: tracks is {tracks.dtype} {tuple(tracks.shape)}, expected int16 (points, 2)')
        if not is_tensor(offsets):
            offsets = np.asarray(offsets)
        if offsets.dtype not in (torch.int64, np.int64) or len(offsets.shape) != 1 or int(offsets.shape[0]) < 1:
            raise ValueError(f'{who}: offsets must be int64 (ntracks + 1)')
        flat = tracks
    return as_numpy, flat, offsets


def altitude_cellinfo(updraft, dem, resolution, airspeed, sink):
    """The packed int32 (rows, cols, 2) raster {climb, elev} that compute_track_altitudes reads (ssrs_altitude_cellinfo):
    climb = rint((w - sink) * 1000 * resolution / airspeed) millimetres gained on one orthogonal move out of the cell, from
    the UN-thresholded updraft w (m/s; NaN read as 0), the sink rate (m/s) and the still-air airspeed (m/s); elev =
    rint(1000 * dem), INT32_MIN where the DEM is NaN.  Always a device tensor."""
    resolution, airspeed, sink = float(resolution), float(airspeed), float(sink)
    if not resolution > 0. or not airspeed > 0. or sink != sink:
        raise ValueError(f'altitude_cellinfo: resolution = {resolution!r}, airspeed = {airspeed!r}, sink = {sink!r} '
                         '(resolution, airspeed > 0)')
    w, z = to_dev(updraft), to_dev(dem)
    if w.dtype not in (torch.float32, torch.float64):
        w = w.to(torch.float64)
    if z.dtype not in (torch.float32, torch.float64):
        z = z.to(torch.float64)
    if w.dim() != 2 or tuple(w.shape) != tuple(z.shape):
        raise ValueError(f'altitude_cellinfo: updraft is {tuple(w.shape)}, dem {tuple(z.shape)}: expected the same (rows, cols)')
    rows, cols = int(w.shape[0]), int(w.shape[1])
    out = torch.empty((rows, cols, 2), dtype=torch.int32, device=w.device)
    nat.check(nat.lib().ssrs_altitude_cellinfo(nat.ptr(w), ftype(w), nat.ptr(z), ftype(z), rows, cols, sink,
                                               1000. * resolution / airspeed, nat.ptr(out), stream_ptr()))
    return out


def altitude_workspace(npoints):
    """A workspace of ssrs_track_altitude for chunks of up to `npoints` points (24 bytes per TILE points)."""
    nbytes = nat.lib().ssrs_track_altitude_workspace_bytes(int(npoints))
    return torch.empty(nbytes, dtype=torch.uint8, device=device())


def compute_track_altitudes(tracks, cellinfo, gridshape, *, offsets=None, start, floor, ceil, band, want_alt=False,
                            want_masked=False, band_hist=None, workspace=None):
    """Height above ground along every track and its presence in the rotor zone (K14, ssrs_track_altitude): h starts at
    clamp(start), every move adds the climb of the cell it leaves (times sqrt(2) on a diagonal) less the terrain's rise,
    and h is clamped to [floor, ceil] after every move; a point is in the rotor zone iff it lies inside the raster and
    band[0] <= h <= band[1].  start, floor, ceil and band are METRES (int(round(1000 x)) millimetres inside).
    `tracks`: a list of int16 (n_i, 2) host arrays, or a device int16 (points, 2) tensor with `offsets` int64
    (ntracks + 1) as movmodel.simulate_tracks / TrackBatch.iter_device_chunks() give them (their first entry need not be
    0).  cellinfo: of altitude_cellinfo (int32 (rows, cols, 2)).
    Returns a dict -- numpy for host input, tensors for device input, like presence.compute_track_occupancy:
      band_hist  int32 raster holding uint32: the in-zone points per cell.  band_hist=: an int32 device raster that is
                 ADDED to (chunks accumulate in one raster) and returned
      heights    int32 (ntracks, 3): [points in the zone, least height, greatest height] in mm, the heights over ALL
                 points of the track; an empty track has [0, INT32_MAX, INT32_MIN].  heights[:, 0].sum() is what was
                 added to band_hist
      alt        (want_alt) int32 (points): the height at every point, in mm
      masked     (want_masked) int16 (points, 2): the points, (-1, -1) where not in the zone.  turbines.turbine_encounters
                 and presence.compute_track_occupancy ignore such points, so it feeds them with the same offsets
    With device input alt / masked are as long as `tracks`, and the entries outside [offsets[0], offsets[-1]) are 0 /
    (-1, -1).  workspace: of altitude_workspace(points) or larger; None allocates one."""
    who = 'compute_track_altitudes'
    rows, cols = int(gridshape[0]), int(gridshape[1])
    params = height_params(start, floor, ceil, band, who)
    as_numpy, flat, offsets = _points_and_offsets(tracks, offsets, who)
    if not is_tensor(cellinfo) or cellinfo.dtype != torch.int32 or tuple(cellinfo.shape) != (rows, cols, 2) or \
            not cellinfo.is_contiguous():
        raise ValueError(f'{who}: cellinfo must be a contiguous int32 tensor ({rows}, {cols}, 2) (altitude_cellinfo)')
    if band_hist is not None and (not is_tensor(band_hist) or band_hist.dtype != torch.int32 or
                                  tuple(band_hist.shape) != (rows, cols) or not band_hist.is_contiguous() or
                                  not band_hist.is_cuda):
        raise ValueError(f'{who}: band_hist must be a contiguous int32 device tensor ({rows}, {cols})')
    if workspace is not None and (not is_tensor(workspace) or not workspace.is_cuda or not workspace.is_contiguous()):
        raise ValueError(f'{who}: workspace must be a contiguous device tensor (altitude_workspace)')
    pts = to_dev(flat, torch.int16)
    off = to_dev(offsets, torch.int64)
    info = to_dev(cellinfo)
    ntracks = int(off.numel()) - 1
    npoints = int(pts.shape[0])
    dev = device()
    if band_hist is None:
        band_hist = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
    heights = torch.empty((3, ntracks), dtype=torch.int32, device=dev)
    heights[0], heights[1], heights[2] = 0, _I32[1], _I32[0]          # (a call without points writes nothing)
    alt = torch.zeros(npoints, dtype=torch.int32, device=dev) if want_alt else None
    masked = torch.full((npoints, 2), -1, dtype=torch.int16, device=dev) if want_masked else None
    if ntracks > 0 and npoints > 0:                      # (empty tensors have no address to hand over)
        if workspace is None:
            workspace = altitude_workspace(npoints)
        nbytes = int(workspace.numel()) * workspace.element_size()
        nat.check(nat.lib().ssrs_track_altitude(
            nat.ptr(pts), nat.ptr(off), ntracks, nat.ptr(info), rows, cols, C.byref(params), nat.ptr(alt),
            nat.ptr(band_hist), nat.ptr(masked), nat.ptr(heights[0]), nat.ptr(heights[1]), nat.ptr(heights[2]),
            nat.ptr(workspace), nbytes, stream_ptr()))
    ref = None if as_numpy else band_hist
    out = dict(band_hist=like_input(band_hist, ref), heights=like_input(heights.t().contiguous(), ref))
    if want_alt:
        out['alt'] = like_input(alt, ref)
    if want_masked:
        out['masked'] = like_input(masked, ref)
    return out


# ------------------------------------------------------------------ flight time (K16, include/ssrs_hip.h "flight time")
WIND_CLIP = 2 ** 20             # |wr|, |wc| and the airspeed in mm/s
TIME_CAP = 2 ** 31 - 1          # microseconds: the longest a move can take


def time_params(resolution, airspeed, min_groundspeed=1., who='compute_track_times'):
    """SsrsFlightTimeParams of the cell size (m), the still-air airspeed and the least ground speed (m/s), as
    int(round(1000 x)) millimetres (per second): 1 <= va <= 2^20, 1 <= gmin <= va, 1 <= res_mm <= 10^6."""
    values = []
    for name, x in (('airspeed', airspeed), ('min_groundspeed', min_groundspeed), ('resolution', resolution)):
        try:
            x = float(x)
        except (TypeError, ValueError):
            raise ValueError(f'{who}: {name} = {x!r}: not a number') from None
        if not abs(x) < float('inf'):
            raise ValueError(f'{who}: {name} = {x!r}: not a finite number')
        values.append(int(round(1000. * x)))
    va, gmin, res_mm = values
    if not 1 <= va <= WIND_CLIP:
        raise ValueError(f'{who}: airspeed = {airspeed!r} m/s: expected 0.001 to {WIND_CLIP / 1000.} m/s')
    if not 1 <= gmin <= va:
        raise ValueError(f'{who}: min_groundspeed = {min_groundspeed!r} m/s: expected 0.001 m/s to the airspeed {airspeed!r}')
    if not 1 <= res_mm <= 10 ** 6:
        raise ValueError(f'{who}: resolution = {resolution!r} m: expected 0.001 to 1000 m')
    return nat.SsrsFlightTimeParams(va, gmin, res_mm)


def _check_ray_axes(ray_axes, who):
    if ray_axes not in nat.SSRS_RAY_AXES:
        raise ValueError(f'{who}: ray_axes = {ray_axes!r}: expected one of {tuple(nat.SSRS_RAY_AXES)}')


def wind_pair(wspeed, wdirn, ray_axes='row_east'):
    """(wr, wc) of one wind for the whole raster, on the host: the velocity of the AIR along +row and +col in mm/s,
    clip(rint((-1000 wspeed) u), +-2^20) with u the components of layers.ray_step(wdirn, ray_axes), the upwind unit step;
    a NaN speed or direction gives (0, 0), still air.  What ssrs_flight_windinfo writes per cell."""
    from .layers import ray_step
    _check_ray_axes(ray_axes, 'wind_pair')
    ur, uc = ray_step(float(wdirn), ray_axes)
    with np.errstate(invalid='ignore'):
        pair = [np.rint((-1000. * np.float64(wspeed)) * np.float64(u[0])) for u in (ur, uc)]
    return tuple(0 if v != v else int(min(max(v, -WIND_CLIP), WIND_CLIP)) for v in pair)


def wind_cellinfo(wspeed, wdirn, ray_axes='row_east'):
    """The packed int32 (rows, cols, 2) raster {wr, wc} that compute_track_times reads (ssrs_flight_windinfo), from per-cell
    wind speed (m/s) and direction (degrees clockwise from north, where the wind comes FROM): wind_pair cell by cell.
    f32 or f64 rasters of one shape (anything else is read as f64).  Always a device tensor."""
    _check_ray_axes(ray_axes, 'wind_cellinfo')
    ws, wd = to_dev(wspeed), to_dev(wdirn)
    if ws.dtype != wd.dtype or ws.dtype not in (torch.float32, torch.float64):
        ws, wd = ws.to(torch.float64), wd.to(torch.float64)
    if ws.dim() != 2 or tuple(ws.shape) != tuple(wd.shape):
        raise ValueError(f'wind_cellinfo: wspeed is {tuple(ws.shape)}, wdirn {tuple(wd.shape)}: expected the same (rows, cols)')
    ws, wd = ws.contiguous(), wd.contiguous()
    rows, cols = int(ws.shape[0]), int(ws.shape[1])
    out = torch.empty((rows, cols, 2), dtype=torch.int32, device=ws.device)
    nat.check(nat.lib().ssrs_flight_windinfo(nat.ptr(ws), nat.ptr(wd), ftype(ws), rows, cols, nat.SSRS_RAY_AXES[ray_axes],
                                             nat.ptr(out), stream_ptr()))
    return out


def compute_track_times(tracks, gridshape, *, offsets=None, resolution, airspeed, min_groundspeed=1., wind,
                        ray_axes='row_east', masked=None, want_dt=False, time_hist=None, band_time_hist=None):
    """Flight time along every track (K16, ssrs_track_time) -- THIS BUILD'S OWN model: a move takes its length
    (`resolution`, times sqrt(2) on a diagonal) over the ground speed the bird keeps along it at `airspeed` in the wind
    of the cell it LEAVES, never less than `min_groundspeed` (all m, m/s), in integer microseconds as include/ssrs_hip.h
    "flight time" defines them; a move with an end outside the raster takes 0.
    `tracks`, `offsets`: as compute_track_altitudes takes them.  wind: a pair (wspeed m/s, wdirn degrees) for the whole
    raster (`ray_axes` as wind_pair reads it), or a raster of wind_cellinfo (int32 (rows, cols, 2) device tensor).
    masked: compute_track_altitudes' `masked` of the same points (int16, shaped like the points): a point with row >= 0
    is in the rotor zone.
    Returns a dict -- numpy for host input, tensors for device input:
      time_hist       int64 raster holding uint64 microseconds: the time of every move, in the cell it leaves.
                      time_hist=: an int64 device raster that is ADDED to (chunks accumulate in one raster) and returned
      times           int64 (ntracks, 2): [total, in the zone] of each track; times[:, 0].sum() is what was added to
                      time_hist, times[:, 1].sum() to band_time_hist (modulo 2^64)
      band_time_hist  (with masked) the raster of the moves that leave a point in the zone; band_time_hist=: ADDED to
      dt              (want_dt) int32 (points): the time of the move that leaves each point, 0 at a track's last point
    With device input dt is as long as `tracks`, and the entries outside [offsets[0], offsets[-1]) are 0."""
    who = 'compute_track_times'
    rows, cols = int(gridshape[0]), int(gridshape[1])
    params = time_params(resolution, airspeed, min_groundspeed, who)
    _check_ray_axes(ray_axes, who)
    as_numpy, flat, offsets = _points_and_offsets(tracks, offsets, who)
    npoints = int(flat.shape[0])
    if masked is not None:
        if not is_tensor(masked):
            masked = np.asarray(masked)
        if masked.dtype not in (torch.int16, np.int16) or tuple(masked.shape) != (npoints, 2):
            raise ValueError(f'{who}: masked must be int16 ({npoints}, 2), the points with (-1, -1) outside the zone')
    info, pair = None, (0, 0)
    if is_tensor(wind) or isinstance(wind, np.ndarray):
        if not is_tensor(wind) or wind.dtype != torch.int32 or tuple(wind.shape) != (rows, cols, 2) or \
                not wind.is_contiguous():
            raise ValueError(f'{who}: wind must be (wspeed, wdirn) or a contiguous int32 tensor ({rows}, {cols}, 2) '
                             '(wind_cellinfo)')
        info = to_dev(wind)
    else:
        try:
            wspeed, wdirn = wind
            pair = wind_pair(float(wspeed), float(wdirn), ray_axes)
        except (TypeError, ValueError):
            raise ValueError(f'{who}: wind = {wind!r}, expected (wspeed, wdirn) or a raster of wind_cellinfo') from None
    for name, hist in (('time_hist', time_hist), ('band_time_hist', band_time_hist)):
        if hist is not None and (not is_tensor(hist) or hist.dtype != torch.int64 or tuple(hist.shape) != (rows, cols) or
                                 not hist.is_contiguous() or not hist.is_cuda):
            raise ValueError(f'{who}: {name} must be a contiguous int64 device tensor ({rows}, {cols})')
    if band_time_hist is not None and masked is None:
        raise ValueError(f'{who}: band_time_hist goes with masked=')
    pts = to_dev(flat, torch.int16)
    off = to_dev(offsets, torch.int64)
    zone = None if masked is None else to_dev(masked, torch.int16).contiguous()
    ntracks = int(off.numel()) - 1
    dev = device()
    if time_hist is None:
        time_hist = torch.zeros((rows, cols), dtype=torch.int64, device=dev)
    if zone is not None and band_time_hist is None:
        band_time_hist = torch.zeros((rows, cols), dtype=torch.int64, device=dev)
    times = torch.zeros((ntracks, 2), dtype=torch.int64, device=dev)
    dt = torch.zeros(npoints, dtype=torch.int32, device=dev) if want_dt else None
    if ntracks > 0 and npoints > 0:                      # (empty tensors have no address to hand over)
        nat.check(nat.lib().ssrs_track_time(
            nat.ptr(pts), nat.ptr(off), ntracks, nat.ptr(zone), nat.ptr(info), pair[0], pair[1], rows, cols,
            C.byref(params), nat.ptr(time_hist), nat.ptr(band_time_hist), nat.ptr(times), nat.ptr(dt), stream_ptr()))
    ref = None if as_numpy else time_hist
    out = dict(time_hist=like_input(time_hist, ref), times=like_input(times, ref))
    if zone is not None:
        out['band_time_hist'] = like_input(band_time_hist, ref)
    if want_dt:
        out['dt'] = like_input(dt, ref)
    return out
