"""Updraft raster layer functions on the MI355X (K1), behind the reference's
function names and argument meaning (/root/reference/ssrs/layers.py).

Inputs may be numpy arrays (copied to HBM, result returned as numpy) or CUDA
torch tensors (zero-copy, result is a tensor).  All arithmetic is f64 on the
device; there is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as nat
from ._device import (device, stream_ptr, to_dev, float_dev, like_input, ftype,
                      is_tensor)


def _shape2(t):
    if t.dim() != 2:
        raise ValueError(f'expected a 2-D raster, got shape {tuple(t.shape)}')
    return int(t.shape[0]), int(t.shape[1])


def compute_slope_degrees(z_mat, res):
    """layers.py:63-93.  Returns f64 (rows, cols); border cells 0."""
    return slope_aspect(z_mat, res, want_aspect=False)[0]


def compute_aspect_degrees(z_mat, res):
    """layers.py:96-128."""
    return slope_aspect(z_mat, res, want_slope=False)[1]


def slope_aspect(z_mat, res, want_slope=True, want_aspect=True, out_dtype=torch.float64):
    """Both Horn-stencil layers in one pass over an LDS-staged DEM tile."""
    dem = float_dev(z_mat)
    rows, cols = _shape2(dem)
    slope = torch.empty((rows, cols), dtype=out_dtype, device=dem.device) if want_slope else None
    aspect = torch.empty((rows, cols), dtype=out_dtype, device=dem.device) if want_aspect else None
    nat.check(nat.lib().ssrs_slope_aspect(
        nat.ptr(dem), ftype(dem), res, nat.ptr(slope), nat.ptr(aspect),
        nat.SSRS_F64 if out_dtype == torch.float64 else nat.SSRS_F32, rows, cols, stream_ptr()))
    return (None if slope is None else like_input(slope, z_mat),
            None if aspect is None else like_input(aspect, z_mat))


def orographic_updraft(wspeed, wdirn, slope, aspect, min_updraft_val=0.,
                       threshold=None, want_orograph=True):
    """Batched compute_orographic_updraft (+ fused threshold).

    wspeed/wdirn: python scalars or 1-D sequences of B scalars (uniform mode),
    or rasters (rows, cols) / (B, rows, cols) (snapshot / seasonal).
    Returns (orograph f32 | None, usable f64 | None) device tensors shaped
    (rows, cols) for a single case, else (B, rows, cols).
    """
    s = float_dev(slope)
    a = float_dev(aspect)
    if a.dtype != s.dtype:
        a = a.to(s.dtype)
    rows, cols = _shape2(s)
    if tuple(a.shape) != (rows, cols):
        raise ValueError('slope and aspect shapes differ')
    uniform = (wspeed.dim() if is_tensor(wspeed) else np.ndim(wspeed)) <= 1
    single = False
    if uniform:
        ws0 = np.atleast_1d(np.asarray(wspeed.cpu() if is_tensor(wspeed) else wspeed,
                                       dtype=np.float64))
        wd0 = np.atleast_1d(np.asarray(wdirn.cpu() if is_tensor(wdirn) else wdirn,
                                       dtype=np.float64))
        if ws0.shape != wd0.shape:
            raise ValueError('wspeed and wdirn lengths differ')
        batch = ws0.size
        single = (wspeed.dim() if is_tensor(wspeed) else np.ndim(wspeed)) == 0
        ws = wd = None
        wtype = nat.SSRS_F32
        ws0p = ws0.ctypes.data_as(C.POINTER(C.c_double))
        wd0p = wd0.ctypes.data_as(C.POINTER(C.c_double))
    else:
        ws = float_dev(wspeed)
        wd = float_dev(wdirn)
        if wd.dtype != ws.dtype:
            wd = wd.to(ws.dtype)
        if ws.shape != wd.shape:
            raise ValueError('wspeed and wdirn shapes differ')
        if ws.dim() == 2:
            single = True
            ws, wd = ws[None], wd[None]
        if tuple(ws.shape[1:]) != (rows, cols):
            raise ValueError('wind raster shape does not match the terrain')
        batch = int(ws.shape[0])
        wtype = ftype(ws)
        ws0p = wd0p = None
    oro = torch.empty((batch, rows, cols), dtype=torch.float32, device=s.device) \
        if want_orograph else None
    use = torch.empty((batch, rows, cols), dtype=torch.float64, device=s.device) \
        if threshold is not None else None
    nat.check(nat.lib().ssrs_orographic_updraft(
        nat.ptr(s), nat.ptr(a), ftype(s), nat.ptr(ws), nat.ptr(wd), wtype, ws0p, wd0p,
        min_updraft_val, nat.ptr(oro), -1.0 if threshold is None else threshold, nat.ptr(use),
        rows, cols, batch, stream_ptr()))
    if single:
        oro = None if oro is None else oro[0]
        use = None if use is None else use[0]
    return oro, use


def compute_orographic_updraft(wspeed, wdirn, slope, aspect, min_updraft_val=0.):
    """layers.py:11-22 with the reference's argument order.  wspeed/wdirn may be
    rasters like the reference passes (constant-filled in uniform mode,
    simulator.py:194-195) or plain scalars.  Returns the f32 raster the
    reference persists (simulator.py:198: `orograph.astype(np.float32)`)."""
    oro, _ = orographic_updraft(wspeed, wdirn, slope, aspect, min_updraft_val)
    return like_input(oro, slope)


def get_above_threshold_speed(in_array, threshold):
    """layers.py:171-185 (f64 output; input is rounded through f32 first when it
    is not f32 already, as the reference only ever feeds the saved f32 raster)."""
    x = to_dev(in_array, torch.float32)
    out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    nat.check(nat.lib().ssrs_threshold_updraft(
        nat.ptr(x), threshold, nat.ptr(out), x.numel(), stream_ptr()))
    return like_input(out, in_array)


def updraft_from_dem(z_mat, res, wspeed, wdirn, threshold=None, min_updraft_val=0.,
                     want_orograph=True, out=None):
    """Fused uniform-mode raster: DEM -> (orograph f32, usable f64 | None).
    One HBM pass (8-12 B/cell + outputs), no trig; see DESIGN.md K1.
    `out` = (orograph f32, usable f64) CUDA tensors to write into (either may be None)."""
    dem = float_dev(z_mat)
    rows, cols = _shape2(dem)
    oro = use = None
    if out is not None:
        oro, use = out
        for t, dt in ((oro, torch.float32), (use, torch.float64)):
            if t is not None and not (t.is_cuda and t.dtype == dt and tuple(t.shape) == (rows, cols) and t.is_contiguous()):
                raise ValueError(f'out tensors must be contiguous CUDA ({rows}, {cols}) float32 / float64')
    if oro is None and want_orograph:
        oro = torch.empty((rows, cols), dtype=torch.float32, device=dem.device)
    if use is None and threshold is not None:
        use = torch.empty((rows, cols), dtype=torch.float64, device=dem.device)
    nat.check(nat.lib().ssrs_updraft_from_dem(
        nat.ptr(dem), ftype(dem), res, wspeed, wdirn, min_updraft_val, nat.ptr(oro),
        -1.0 if threshold is None else threshold, nat.ptr(use), rows, cols, stream_ptr()))
    return (None if oro is None else like_input(oro, z_mat),
            None if use is None else like_input(use, z_mat))


def updraft_from_dem_lattice(z_mat, res, x_km, y_km, wspeed, wdirn, threshold=None,
                             min_updraft_val=0., want_orograph=True):
    """Snapshot / seasonal raster in one pass: DEM + wind samples on a regular lattice
    (x_km[nx], y_km[ny] relative to the south-west cell centre; wspeed / wdirn (ny, nx)
    or (B, ny, nx)) -> (orograph f32 | None, usable f64 | None), shaped (rows, cols) for
    one snapshot, else (B, rows, cols).  Equivalent to wind.interpolate_wind_lattice +
    slope_aspect + orographic_updraft without materialising any of their rasters."""
    import numpy as np
    dem = float_dev(z_mat)
    rows, cols = _shape2(dem)
    x = np.asarray(x_km, dtype=np.float64)
    y = np.asarray(y_km, dtype=np.float64)
    nx, ny = x.size, y.size
    dx = float(x[1] - x[0]) if nx > 1 else 1.0
    dy = float(y[1] - y[0]) if ny > 1 else 1.0
    if nx > 2 and not np.allclose(np.diff(x), dx) or ny > 2 and not np.allclose(np.diff(y), dy):
        raise ValueError('wind lattice must be uniformly spaced')
    ws = to_dev(wspeed, torch.float64)
    wd = to_dev(wdirn, torch.float64)
    single = ws.dim() == 2
    if single:
        ws, wd = ws[None], wd[None]
    if tuple(ws.shape[1:]) != (ny, nx) or ws.shape != wd.shape:
        raise ValueError(f'lattice arrays must be (ny, nx) = {(ny, nx)}')
    batch = int(ws.shape[0])
    oro = torch.empty((batch, rows, cols), dtype=torch.float32, device=dem.device) if want_orograph else None
    use = torch.empty((batch, rows, cols), dtype=torch.float64, device=dem.device) \
        if threshold is not None else None
    nbytes = nat.lib().ssrs_lattice_workspace_bytes(nx, ny, batch)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dem.device)
    nat.check(nat.lib().ssrs_updraft_from_dem_lattice(
        nat.ptr(dem), ftype(dem), res, nat.ptr(ws.contiguous()), nat.ptr(wd.contiguous()),
        nx, ny, x[0], y[0], dx, dy, min_updraft_val, nat.ptr(oro), -1. if threshold is None else threshold,
        nat.ptr(use), rows, cols, batch, nat.ptr(scratch), nbytes, stream_ptr()))
    if single:
        oro = None if oro is None else oro[0]
        use = None if use is None else use[0]
    return oro, use


def _elementwise_f64(arrays):
    """The arguments as contiguous f64 device tensors of their common (broadcast) shape, and whether any was a tensor."""
    devs = [to_dev(a, torch.float64) for a in arrays]
    shape = torch.broadcast_shapes(*[tuple(d.shape) for d in devs])
    return [d.expand(shape).contiguous() for d in devs], any(is_tensor(a) for a in arrays)


def _elementwise_out(out, tensor_in):
    return out if tensor_in else out.cpu().numpy()


def compute_potential_temperature(pressure, temperature):
    """layers.py:40-48: potential temperature in degrees Celsius from pressure (Pa) and temperature (deg C), f64."""
    (p, t), tensor_in = _elementwise_f64((pressure, temperature))
    out = torch.empty_like(p)
    if out.numel():
        nat.check(nat.lib().ssrs_potential_temperature(nat.ptr(p), nat.ptr(t), nat.ptr(out), out.numel(), stream_ptr()))
    return _elementwise_out(out, tensor_in)


def deardoff_velocity_function(pot_temperature, blayer_height, surface_heat_flux, min_updraft_val=1e-5):
    """layers.py:25-37 (the reference's spelling): the convective velocity scale w*, f64.  NaN in, NaN out, as
    np.maximum / ndarray.clip."""
    (th, zi, q), tensor_in = _elementwise_f64((pot_temperature, blayer_height, surface_heat_flux))
    out = torch.empty_like(th)
    if out.numel():
        nat.check(nat.lib().ssrs_deardorff_velocity(nat.ptr(th), nat.ptr(zi), nat.ptr(q), min_updraft_val,
                                                    nat.ptr(out), out.numel(), stream_ptr()))
    return _elementwise_out(out, tensor_in)


def compute_thermal_updraft(zmat, deardoff_vel, blayer_height, min_updraft_val=1e-5):
    """layers.py:51-60: thermal updraft at height `zmat` (a scalar or an array like the others), f64."""
    scalar_z = not is_tensor(zmat) and np.ndim(zmat) == 0
    if scalar_z:
        (w, zi), tensor_in = _elementwise_f64((deardoff_vel, blayer_height))
        z, z0 = None, float(zmat)
    else:
        (z, w, zi), tensor_in = _elementwise_f64((zmat, deardoff_vel, blayer_height))
        z0 = 0.
    out = torch.empty_like(w)
    if out.numel():
        nat.check(nat.lib().ssrs_thermal_updraft(nat.ptr(z), z0, nat.ptr(w), nat.ptr(zi), min_updraft_val, nat.ptr(out),
                                                 out.numel(), stream_ptr()))
    return _elementwise_out(out, tensor_in)


# ---------------------------------------------------------------------------- K9: shelter angle, improved model
IMPROVED_COEFFS = (4e-5, 2.8e-3, 0.8, 0.35, 0.095, -0.09, 1.0)     # (a, b, c, d, e, f, g): UNVERIFIED, see DESIGN.md K9


def ray_step(wdirn, ray_axes='row_east'):
    """Upwind unit step (ur, uc) in (row, col) of a wind from `wdirn` degrees (clockwise from north), f64 arrays:
    'row_north' (+row = north, +col = east) -> (cos A, sin A); 'row_east' (the frame of the Horn aspect computed
    from a DEM alone: +row = east, +col = north) -> (sin A, cos A)."""
    if ray_axes not in nat.SSRS_RAY_AXES:
        raise ValueError(f'ray_axes = {ray_axes!r}: expected one of {tuple(nat.SSRS_RAY_AXES)}')
    rad = np.atleast_1d(np.asarray(wdirn, dtype=np.float64)) * np.pi / 180.
    return (np.cos(rad), np.sin(rad)) if ray_axes == 'row_north' else (np.sin(rad), np.cos(rad))


def check_improved_parameters(dmax, res, height, coeffs):
    """ValueError unless K = floor(dmax / res) >= 1, height >= 0, seven finite coefficients with d > 0 and
    F_h = (a h^2 + b h + c) d^(e - cos(slope)) + f > 0 at both ends cos(slope) = 0 and 1.  Host only."""
    if not (float(dmax) > 0. and np.isfinite(dmax) and np.floor(float(dmax) / float(res)) >= 1.):
        raise ValueError(f'orographic_sx_dmax = {dmax!r} m is less than one cell of {res!r} m')
    if not (float(height) >= 0. and np.isfinite(height)):
        raise ValueError(f'orographic_height = {height!r}: expected metres >= 0')
    try:
        cf = tuple(float(x) for x in coeffs)
    except (TypeError, ValueError):
        cf = ()
    if len(cf) != 7 or not np.all(np.isfinite(cf)):
        raise ValueError(f'orographic_coeffs = {coeffs!r}: expected 7 finite numbers (a, b, c, d, e, f, g)')
    a, b, c, d, e, f, _ = cf
    if not d > 0.:
        raise ValueError(f'orographic_coeffs: d = {d!r} must be > 0')
    poly = a * float(height) ** 2 + b * float(height) + c
    ends = (poly * d ** e + f, poly * d ** (e - 1.) + f)
    if not (np.all(np.isfinite(ends)) and min(ends) > 0.):
        raise ValueError(f'orographic_coeffs = {coeffs!r} with height {height!r} allow F_h <= 0 '
                         f'(F_h = {ends[1]:g} on flat ground, {ends[0]:g} on a vertical face)')
    return cf


SECTOR_MAX_RAYS = 61


def sector_rays(sector, sector_step):
    """(H, M) of a shelter sector of half-width `sector` in steps of `sector_step` degrees: H = floor(W / S + 1e-9),
    M = 2 H + 1 azimuths A + (m - H) S.  ValueError unless W is finite and in [0, 90], S finite and > 0, M <= 61.
    Host only."""
    try:
        w, s = float(sector), float(sector_step)
    except (TypeError, ValueError):
        w = s = np.nan
    if not (np.isfinite(w) and 0. <= w <= 90.):
        raise ValueError(f'orographic_sx_sector = {sector!r}: expected a half-width in degrees in [0, 90]')
    if not (np.isfinite(s) and s > 0.):
        raise ValueError(f'orographic_sx_step = {sector_step!r}: expected degrees > 0')
    h = np.floor(w / s + 1e-9)
    if not 2. * h + 1. <= SECTOR_MAX_RAYS:
        raise ValueError(f'orographic_sx_sector = {sector!r} in steps of orographic_sx_step = {sector_step!r} takes '
                         f'M = {2. * h + 1.:.0f} rays, more than {SECTOR_MAX_RAYS}')
    return int(h), 2 * int(h) + 1


def _wind_direction_args(wdirn, ray_axes, rows, cols, sector=0., sector_step=5.):
    """(batch, single, ur, uc, wdirn device raster | None) from scalars / a 1-D sequence (uniform) or rasters.  With a
    sector, ur / uc hold the M steps of every case, case-major."""
    if (wdirn.dim() if is_tensor(wdirn) else np.ndim(wdirn)) <= 1:
        wd0 = np.asarray(wdirn.cpu() if is_tensor(wdirn) else wdirn, dtype=np.float64)
        if sector > 0.:
            half, count = sector_rays(sector, sector_step)
            wd_m = np.atleast_1d(wd0)[:, None] + np.arange(-half, half + 1).astype(np.float64) * float(sector_step)
            ur, uc = ray_step(wd_m.ravel(), ray_axes)
            return ur.size // count, wd0.ndim == 0, np.ascontiguousarray(ur), np.ascontiguousarray(uc), None
        ur, uc = ray_step(wd0, ray_axes)
        return ur.size, wd0.ndim == 0, np.ascontiguousarray(ur), np.ascontiguousarray(uc), None
    wd = to_dev(wdirn, torch.float64)
    single = wd.dim() == 2
    if single:
        wd = wd[None]
    if wd.dim() != 3 or tuple(wd.shape[1:]) != (rows, cols):
        raise ValueError('wind raster shape does not match the terrain')
    return int(wd.shape[0]), single, None, None, wd.contiguous()


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def compute_sx(z_mat, res, wdirn, dmax=500., ray_axes='row_east', want='deg', path='auto', sector=0., sector_step=5.):
    """Winstral's terrain-shelter angle: per cell the steepest angle at which it sees terrain within `dmax` metres
    upwind (K = floor(dmax / res) bilinear samples along the ray; DESIGN.md K9 states the sample exactly).
    wdirn: a scalar or B scalars (uniform wind; the ray step is numpy's cos / sin, handed to the device), or a raster
    (rows, cols) / (B, rows, cols) of degrees.  want: 'deg' -> Sx in degrees, 'tan' -> tan(Sx), 'both' -> (tan, deg);
    f64, shaped (rows, cols) for a single case, else (B, rows, cols).  path: 'auto' | 'lds' | 'global' (A/B).
    sector > 0: Winstral's sector average -- the mean of Sx over the azimuths wdirn + j sector_step within
    +- sector degrees, in one fused device call (ssrs_shelter_sx_sector); 'deg' is that mean, 'tan' its tangent.
    sector = 0 is the single ray."""
    if want not in ('deg', 'tan', 'both'):
        raise ValueError(f"want = {want!r}: expected 'deg', 'tan' or 'both'")
    sector_rays(sector, sector_step)
    if ray_axes not in nat.SSRS_RAY_AXES or path not in nat.SSRS_SHELTER_PATH:
        raise ValueError(f'ray_axes = {ray_axes!r} / path = {path!r}: expected one of {tuple(nat.SSRS_RAY_AXES)} / '
                         f'{tuple(nat.SSRS_SHELTER_PATH)}')
    dem = float_dev(z_mat)
    rows, cols = _shape2(dem)
    batch, single, ur, uc, wd = _wind_direction_args(wdirn, ray_axes, rows, cols, sector, sector_step)
    tan = torch.empty((batch, rows, cols), dtype=torch.float64, device=dem.device) if want != 'deg' else None
    deg = torch.empty((batch, rows, cols), dtype=torch.float64, device=dem.device) if want != 'tan' else None
    if sector > 0.:
        nat.check(nat.lib().ssrs_shelter_sx_sector(
            nat.ptr(dem), ftype(dem), res, _dptr(ur), _dptr(uc), nat.ptr(wd), dmax,
            nat.SSRS_RAY_AXES[ray_axes], nat.SSRS_SHELTER_PATH[path], sector, sector_step,
            nat.ptr(tan), nat.ptr(deg), rows, cols, batch, stream_ptr()))
    else:
        nat.check(nat.lib().ssrs_shelter_sx(
            nat.ptr(dem), ftype(dem), res, _dptr(ur), _dptr(uc), nat.ptr(wd), dmax,
            nat.SSRS_RAY_AXES[ray_axes], nat.SSRS_SHELTER_PATH[path], nat.ptr(tan), nat.ptr(deg), rows, cols, batch,
            stream_ptr()))
    out = [None if t is None else like_input(t[0] if single else t, z_mat) for t in (tan, deg)]
    return out[1] if want == 'deg' else out[0] if want == 'tan' else tuple(out)


def orographic_updraft_improved(z_mat, res, wspeed, wdirn, slope=None, aspect=None, dmax=500., height=80.,
                                coeffs=IMPROVED_COEFFS, ray_axes=None, min_updraft_val=0., threshold=None,
                                want_orograph=True, want_sx=False, path='auto', sector=0., sector_step=5., smooth_sigma=0.):
    """The orographic updraft sheltered by upwind terrain and scaled to a flight height:
    w = max(min_updraft_val, w0 F_sx / F_h), w0 the value of updraft_from_dem (slope / aspect None: Horn stencil of
    the DEM) or of orographic_updraft (slope / aspect rasters) before its clamp, F_sx = max(0, 1 + g tan Sx),
    F_h = (a h^2 + b h + c) d^(e - cos(slope)) + f.  wspeed / wdirn: scalars or B scalars, or rasters (rows, cols) /
    (B, rows, cols).  ray_axes: the frame of the shelter ray, by default that of the aspect it multiplies --
    'row_east' for the DEM's own Horn aspect, 'row_north' for given layers.  sector / sector_step: as compute_sx
    (tan Sx becomes the tangent of the sector's mean angle, Sx that mean).  smooth_sigma > 0 (metres; 0 = off): the
    field is computed without its clamp, rounded to f32 and blurred by a Gaussian of that width (smooth_orograph with
    sigma_cells = smooth_sigma / res: scipy's gaussian_filter, mode='reflect', a nodata cell entering as 0), and the
    clamp and the threshold act on the smoothed field; Sx is unaffected.  Returns (orograph f32 | None,
    usable f64 | None[, Sx degrees f64]) shaped (rows, cols) for a single case, else (B, rows, cols); numpy when
    z_mat is numpy."""
    if (slope is None) != (aspect is None):
        raise ValueError('give both slope and aspect or neither')
    if ray_axes is None:
        ray_axes = 'row_east' if slope is None else 'row_north'
    if ray_axes not in nat.SSRS_RAY_AXES or path not in nat.SSRS_SHELTER_PATH:
        raise ValueError(f'ray_axes = {ray_axes!r} / path = {path!r}: expected one of {tuple(nat.SSRS_RAY_AXES)} / '
                         f'{tuple(nat.SSRS_SHELTER_PATH)}')
    cf = check_improved_parameters(dmax, res, height, coeffs)
    sector_rays(sector, sector_step)
    smooth = float(smooth_sigma) != 0.
    if smooth:
        smoothing_radius(float(smooth_sigma) / float(res), 'smooth_sigma / res')
    dem = float_dev(z_mat)
    rows, cols = _shape2(dem)
    s = a = None
    if slope is not None:
        s = float_dev(slope)
        a = float_dev(aspect)
        if a.dtype != s.dtype:
            a = a.to(s.dtype)
        if tuple(s.shape) != (rows, cols) or tuple(a.shape) != (rows, cols):
            raise ValueError('slope / aspect shapes do not match the terrain')
    batch, single, ur, uc, wd = _wind_direction_args(wdirn, ray_axes, rows, cols, sector, sector_step)
    ws = ws0 = wd0 = None
    if wd is None:
        ws0 = np.atleast_1d(np.asarray(wspeed.cpu() if is_tensor(wspeed) else wspeed, dtype=np.float64))
        wd0 = np.atleast_1d(np.asarray(wdirn.cpu() if is_tensor(wdirn) else wdirn, dtype=np.float64))
        if ws0.shape != wd0.shape:
            raise ValueError('wspeed and wdirn lengths differ')
        ws0, wd0 = np.ascontiguousarray(ws0), np.ascontiguousarray(wd0)
    else:
        ws = to_dev(wspeed, torch.float64)
        ws = (ws[None] if ws.dim() == 2 else ws).contiguous()
        if ws.shape != wd.shape:
            raise ValueError('wspeed and wdirn shapes differ')
    params = nat.SsrsShelterParams(float(dmax), nat.SSRS_RAY_AXES[ray_axes], nat.SSRS_SHELTER_PATH[path], float(height),
                                   (C.c_double * 7)(*cf))
    oro = torch.empty((batch, rows, cols), dtype=torch.float32, device=dem.device) if want_orograph or smooth else None
    use = torch.empty((batch, rows, cols), dtype=torch.float64, device=dem.device) if threshold is not None else None
    sx = torch.empty((batch, rows, cols), dtype=torch.float64, device=dem.device) if want_sx else None
    head = (nat.ptr(dem), ftype(dem), res, _dptr(ur), _dptr(uc), _dptr(ws0), _dptr(wd0), nat.ptr(ws),
            nat.ptr(wd), nat.ptr(s), nat.ptr(a), nat.SSRS_F64 if s is None else ftype(s), C.byref(params))
    tail = (min_updraft_val, -1. if threshold is None else threshold, nat.ptr(oro), nat.ptr(use), nat.ptr(sx), rows, cols,
            batch, stream_ptr())
    if smooth:                                  # the unclamped field, no threshold: both act on the smoothed field below
        tail = (-np.inf, -1., nat.ptr(oro), None) + tail[4:]
    if sector > 0.:
        nat.check(nat.lib().ssrs_updraft_sheltered_sector(*head, sector, sector_step, *tail))
    else:
        nat.check(nat.lib().ssrs_updraft_sheltered(*head, *tail))
    if smooth:
        _smooth_reflect(oro, float(smooth_sigma) / float(res), min_updraft_val, threshold, None,
                        oro if want_orograph else None, use, 'auto')
        oro = oro if want_orograph else None
    out = tuple(None if t is None else like_input(t[0] if single else t, z_mat) for t in (oro, use, sx))
    return out if want_sx else out[:2]


# ---------------------------------------------------------------------------- K11: Gaussian smoothing of the updraft
SMOOTH_MAX_RADIUS = 512


def smoothing_sigma_m(height, sigma=0.):
    """Width in metres of the Gaussian that smooths the improved orographic updraft: `sigma` when > 0, else the model's
    own min(0.8 height + 16, 300) (recalled from the published model, UNVERIFIED: DESIGN.md limit 10).  ValueError for a
    negative or non-finite sigma.  Host only."""
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        s = np.nan
    if not (np.isfinite(s) and s >= 0.):
        raise ValueError(f'orographic_smooth_sigma = {sigma!r}: expected metres >= 0 (0 = the model\'s own width)')
    return s if s > 0. else min(0.8 * float(height) + 16., 300.)


def smoothing_radius(sigma_cells, name='sigma_cells'):
    """R = int(4 sigma + 0.5) of a Gaussian of `sigma_cells` cells (scipy's truncate = 4).  ValueError unless sigma is
    finite and > 0 and R <= 512.  Host only."""
    try:
        s = float(sigma_cells)
    except (TypeError, ValueError):
        s = np.nan
    if not (np.isfinite(s) and s > 0.):
        raise ValueError(f'{name} = {sigma_cells!r}: expected a width in cells > 0')
    if not 4. * s + 0.5 < SMOOTH_MAX_RADIUS + 1.:
        raise ValueError(f'{name} = {s:g} cells takes a radius R = int(4 sigma + 0.5) of more than {SMOOTH_MAX_RADIUS} cells')
    return int(4. * s + 0.5)


def _smooth_reflect(x, sigma_cells, min_updraft_val, threshold, smooth, oro, use, path):
    """ssrs_smooth_reflect on the device tensor x f32 (B, rows, cols) into the given outputs (None = not asked for; oro
    may be x itself: the first pass has read a case before the second writes it)."""
    batch, rows, cols = x.shape
    lib = nat.lib()
    nbytes = lib.ssrs_smooth_workspace_bytes(rows, cols, batch, sigma_cells)
    work = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=x.device)
    nat.check(lib.ssrs_smooth_reflect(nat.ptr(x), sigma_cells, nat.SSRS_SMOOTH_PATH[path], min_updraft_val,
                                      -1. if threshold is None else threshold, nat.ptr(smooth), nat.ptr(oro), nat.ptr(use),
                                      rows, cols, batch, nat.ptr(work), nbytes, stream_ptr()))


def smooth_orograph(orograph, sigma_cells, min_updraft_val=0., threshold=None, want_smooth=False, path='auto'):
    """Gaussian smoothing of an orographic updraft raster: scipy.ndimage.gaussian_filter(x, sigma_cells,
    mode='reflect') of the f32 raster `orograph`, (rows, cols) or (B, rows, cols), a non-finite value entering as 0; f64
    inside, axis 0 first.  Returns (orograph f32 = the smoothed field clamped at min_updraft_val, usable f64 | None = its
    threshold function when `threshold` is given[, smooth f64 = the unclamped sum]); numpy in, numpy out.
    path: 'auto' | 'lds' | 'global' (A/B, the same bits)."""
    smoothing_radius(sigma_cells)
    if path not in nat.SSRS_SMOOTH_PATH:
        raise ValueError(f'path = {path!r}: expected one of {tuple(nat.SSRS_SMOOTH_PATH)}')
    if threshold is not None and not float(threshold) > 0.:
        raise ValueError(f'threshold = {threshold!r}: expected > 0')
    if np.isnan(float(min_updraft_val)):
        raise ValueError('min_updraft_val is NaN')
    if (orograph.dim() if is_tensor(orograph) else np.ndim(orograph)) not in (2, 3):
        raise ValueError('orograph: expected a raster (rows, cols) or (B, rows, cols)')
    x = to_dev(orograph, torch.float32)
    single = x.dim() == 2
    if single:
        x = x[None]
    oro = torch.empty_like(x)
    use = torch.empty(x.shape, dtype=torch.float64, device=x.device) if threshold is not None else None
    smooth = torch.empty(x.shape, dtype=torch.float64, device=x.device) if want_smooth else None
    _smooth_reflect(x, float(sigma_cells), float(min_updraft_val), threshold, smooth, oro, use, path)
    out = tuple(None if t is None else like_input(t[0] if single else t, orograph) for t in (oro, use, smooth))
    return out if want_smooth else out[:2]
