"""Thermal updraft realisations (a5) on the device, behind the reference's
`compute_thermals(aspect, thermal_intensity_scale)` (/root/reference/ssrs/
layers.py:188-214).  Statistical parity only: see csrc/thermals.hip.
`compute_wtk_thermals` is the other thermal model (Config.thermal_model = 'wtk'): the Deardorff-velocity updraft of
ssrs/layers.py:25-60 from a snapshot's own WTK layers, deterministic; see csrc/wtk_thermals.hip."""
import ctypes as C

import torch

from . import _native as nat
from ._device import stream_ptr, to_dev, like_input


def gaussian_blur(field, sigma):
    """scipy.ndimage.gaussian_filter(field, sigma, mode='constant') in f64."""
    x = to_dev(field, torch.float64)
    rows, cols = int(x.shape[0]), int(x.shape[1])
    out = torch.empty_like(x)
    nbytes = nat.lib().ssrs_blur_workspace_bytes(rows, cols, C.c_double(sigma))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    nat.check(nat.lib().ssrs_gaussian_blur(nat.ptr(x), nat.ptr(out), C.c_double(sigma), rows, cols,
                                           nat.ptr(ws), C.c_size_t(nbytes), stream_ptr()))
    return like_input(out, field)


def thermal_seeds(aspect, thermal_intensity_scale, seed=0):
    a = to_dev(aspect, torch.float64)
    rows, cols = int(a.shape[0]), int(a.shape[1])
    out = torch.empty_like(a)
    nat.check(nat.lib().ssrs_thermal_seeds(nat.ptr(a), C.c_double(thermal_intensity_scale),
                                           C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                           nat.ptr(out), rows, cols, stream_ptr()))
    return like_input(out, aspect)


def compute_thermals_batch(aspect, thermal_intensity_scale, seeds, dtype=torch.float64, sigma=4.0):
    """One field of smoothed random thermals per entry of `seeds`, (len(seeds), rows, cols) in
    `dtype` (f64, or f32 = the f64 field rounded once), from one fused device call: field k is
    bit for bit gaussian_blur(thermal_seeds(aspect, scale, seeds[k]), sigma)."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError('compute_thermals_batch: dtype must be torch.float32 or torch.float64')
    a = to_dev(aspect, torch.float64)
    if a.dim() != 2:
        raise ValueError('compute_thermals_batch: aspect must be a (rows, cols) raster')
    rows, cols = int(a.shape[0]), int(a.shape[1])
    keys = [int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]
    out = torch.empty((len(keys), rows, cols), dtype=dtype, device=a.device)
    nat.check(nat.lib().ssrs_thermal_fields(nat.ptr(a), C.c_double(thermal_intensity_scale), C.c_double(sigma),
                                            (C.c_uint64 * len(keys))(*keys), len(keys), nat.ptr(out),
                                            int(dtype == torch.float32), rows, cols, stream_ptr()))
    return like_input(out, aspect)


def compute_thermals(aspect, thermal_intensity_scale, seed=0):
    """Field of smoothed random thermals (f64), one realisation per `seed`."""
    return compute_thermals_batch(aspect, thermal_intensity_scale, [seed])[0]


def compute_wtk_thermals(x_km, y_km, pressure, temperature, blheight, surfheatflux, gridsize, resolution, height,
                         method='linear', dtype=torch.float32, min_updraft_val=1e-5, index=None):
    """Thermal updraft at `height` from the four WIND Toolkit layers of a snapshot, sampled at x_km[npts], y_km[npts]
    (relative to the raster's south-west cell centre): the reference's `_interpolate_wtk_vardata` of each layer, then
    `compute_potential_temperature`, `deardoff_velocity_function` and `compute_thermal_updraft`
    (ssrs/layers.py:25-60), as ONE device call in which no interpolated raster is written.
    pressure / temperature / blheight / surfheatflux: (npts,) or (B, npts); height: a scalar or a (rows, cols) raster.
    Returns (rows, cols) or (B, rows, cols) in `dtype`: f64, bit for bit `wind.interpolate_scalar_scattered` followed
    by the three `layers` functions, or f32 = that result rounded once; NaN outside the samples' convex hull for
    'linear' and 'cubic'.  method, index: as `wind.interpolate_wind_scattered`."""
    import numpy as np
    from .inputs import host_f64
    from .wind import check_method, _scalar_geometry
    if dtype not in (torch.float32, torch.float64):
        raise ValueError('compute_wtk_thermals: dtype must be torch.float32 or torch.float64')
    method = check_method(method)
    given = (pressure, temperature, blheight, surfheatflux)
    fields = [host_f64(a) for a in given]
    single = fields[0].ndim == 1
    fields = [a[None] if a.ndim == 1 else a for a in fields]
    if any(a.ndim != 2 or a.shape != fields[0].shape for a in fields):
        raise ValueError('compute_wtk_thermals: the four layers must share one shape, (npts,) or (B, npts)')
    batch, npts = fields[0].shape
    rows, cols = int(gridsize[0]), int(gridsize[1])
    raster_z = isinstance(height, torch.Tensor) or np.ndim(height) != 0
    if raster_z and tuple(np.shape(height)) != (rows, cols):
        raise ValueError(f'compute_wtk_thermals: height must be a scalar or a raster of shape {(rows, cols)}')
    head, tail, keep = _scalar_geometry(x_km, y_km, np.stack(fields).reshape(4 * batch, npts), gridsize, resolution, method,
                                        index, 'compute_wtk_thermals')
    zmat = to_dev(height, torch.float64) if raster_z else None
    z0 = 0. if raster_z else float(height)
    out = torch.empty((batch, rows, cols), dtype=dtype, device=keep['values'].device)
    nat.check(nat.lib().ssrs_wtk_thermal_fields(*head, nat.ptr(zmat), C.c_double(z0), C.c_double(min_updraft_val),
                                                nat.ptr(out), int(dtype == torch.float32), rows, cols, int(batch), *tail))
    out = out[0] if single else out
    return out if any(isinstance(a, torch.Tensor) for a in given) else out.cpu().numpy()
