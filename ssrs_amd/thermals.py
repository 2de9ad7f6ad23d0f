"""Thermal updraft realisations (a5) on the device, behind the reference's
`compute_thermals(aspect, thermal_intensity_scale)` (/root/reference/ssrs/
layers.py:188-214).  Statistical parity with the reference's RNG stream only: see csrc/thermals.hip; the device's own
rule is restated cell by cell in tests/thermals_ref.py.
`compute_wtk_thermals` is the other thermal model (Config.thermal_model = 'wtk'): the Deardorff-velocity updraft of
ssrs/layers.py:25-60 from a snapshot's own WTK layers, deterministic; see csrc/wtk_thermals.hip.
`compute_allen_thermals` is the third (Config.thermal_model = 'allen'): Allen's (2006) field of discrete updrafts, the
model ssrs/layers.py:217-493 carries commented out, stochastic and scaled by zi and w*; see csrc/allen_thermals.hip."""
import ctypes as C

import torch

from . import _native as nat
from ._device import stream_ptr, to_dev, like_input


def gaussian_blur(field, sigma):
    """scipy.ndimage.gaussian_filter(field, sigma, mode='constant') in f64."""
    x = to_dev(field, torch.float64)
    rows, cols = int(x.shape[0]), int(x.shape[1])
    out = torch.empty_like(x)
    nbytes = nat.lib().ssrs_blur_workspace_bytes(rows, cols, sigma)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    nat.check(nat.lib().ssrs_gaussian_blur(nat.ptr(x), nat.ptr(out), sigma, rows, cols, nat.ptr(ws), nbytes, stream_ptr()))
    return like_input(out, field)


def thermal_seeds(aspect, thermal_intensity_scale, seed=0):
    a = to_dev(aspect, torch.float64)
    rows, cols = int(a.shape[0]), int(a.shape[1])
    out = torch.empty_like(a)
    nat.check(nat.lib().ssrs_thermal_seeds(nat.ptr(a), thermal_intensity_scale, int(seed) & 0xFFFFFFFFFFFFFFFF,
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
    nat.check(nat.lib().ssrs_thermal_fields(nat.ptr(a), thermal_intensity_scale, sigma,
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
    nat.check(nat.lib().ssrs_wtk_thermal_fields(*head, nat.ptr(zmat), z0, min_updraft_val,
                                                nat.ptr(out), int(dtype == torch.float32), rows, cols, int(batch), *tail))
    out = out[0] if single else out
    return out if any(isinstance(a, torch.Tensor) for a in given) else out.cpu().numpy()


# ---------------------------------------------------------------------------- K12: Allen's (2006) discrete updrafts
ALLEN_MAX_UPDRAFTS = nat.SSRS_ALLEN_MAX_UPDRAFTS
ALLEN_PER_BIN = 3.          # updrafts a bin holds on average


def allen_scalars(z, zi, wstar, gridsize, resolution, sink=False):
    """The host scalars of one Allen field (ssrs/layers.py:244-253, 339-344, 424-435 of the reference, commented out
    there), Python f64: dict(zzi, rbar, wtbar, N, we, z_below_zi).  z: height above ground, zi: boundary-layer height,
    wstar: convective velocity scale; all three finite and > 0."""
    import math
    z, zi, wstar = float(z), float(zi), float(wstar)
    for name, v in (('z', z), ('zi', zi), ('wstar', wstar)):
        if not (math.isfinite(v) and v > 0.):
            raise ValueError(f'allen_scalars: {name} = {v!r}: expected a finite number > 0')
    rows, cols, res = int(gridsize[0]), int(gridsize[1]), float(resolution)
    zzi = z / zi
    rbar = 0.102 * zzi ** (1 / 3) * (1 - 0.25 * zzi) * zi
    wtbar = zzi ** (1 / 3) * (1 - 1.1 * zzi) * wstar
    X, Y = cols * res, rows * res
    N = int(round(0.6 * Y * X / (zi * rbar)))
    we = 0.
    if sink:
        area = N * math.pi * rbar ** 2
        if not area < X * Y:
            raise ValueError(f'allen_scalars: the {N} updrafts of radius {rbar:g} m cover the whole raster (z / zi = {zzi:g})')
        we = min(-(wtbar * area * (-2.5 * (zzi - 0.5))) / (X * Y - area), 0.)
    return dict(zzi=zzi, rbar=rbar, wtbar=wtbar, N=N, we=we, z_below_zi=z < zi)


def _allen_gain_curve(start, end, top, floor_, last):
    import numpy as np
    t = np.linspace(start, end, 100)
    period = start - end
    phase = period / 2 + start
    amp, offset = (top - floor_) / 2, (top + floor_) / 2
    w = amp * np.cos(2 * np.pi * (t - phase) / period) + offset
    return np.concatenate(([0], t, [last])), np.concatenate(([floor_], w, [floor_]))


def allen_datetime_gains(dtime):
    """(diurnal gain, seasonal gain) of a datetime (computeDatetimeGain, ssrs/layers.py:444-493 of the reference);
    (1, 1) for None."""
    import numpy as np
    if dtime is None:
        return 1., 1.
    dg = np.interp(dtime.hour, *_allen_gain_curve(6, 18, 1.2, 0., 24))
    sg = np.interp(dtime.month, *_allen_gain_curve(4, 9, 1.1, 0.5, 12))
    return float(dg), float(sg)


def allen_updrafts(n, gridsize, resolution, seed, gains=(1., 1.)):
    """xt, yt, wgain, rgain of `n` updrafts, f64: positions uniform over [0, cols res) x [0, rows res) metres from the
    centre of cell (0, 0), wgain ~ U(0.7 dg, 1.3 dg), rgain ~ U(0.8 sg, 1.2 sg) with gains = (dg, sg), drawn in that
    order from np.random.default_rng(seed)."""
    import numpy as np
    rows, cols, res = int(gridsize[0]), int(gridsize[1]), float(resolution)
    dg, sg = float(gains[0]), float(gains[1])
    rng = np.random.default_rng(seed)
    n = int(n)
    xt = rng.uniform(0., cols * res, n)
    yt = rng.uniform(0., rows * res, n)
    wgain = rng.uniform(0.7 * dg, 1.3 * dg, n)
    rgain = rng.uniform(0.8 * sg, 1.2 * sg, n)
    return xt, yt, wgain, rgain


def allen_bins(xt, yt, gridsize, resolution):
    """The CSR of ssrs_allen_thermal_field: (bin_start int32 (nbx nby + 1), bin_items int32, bin_size_m, nbx, nby).
    Square bins of bin_size_m metres -- chosen so that a bin holds ALLEN_PER_BIN updrafts on average, never smaller
    than a cell -- bin = by nbx + bx; an updraft lies in (min(floor(xt / bin_size_m), nbx - 1), likewise for yt), and
    the items ascend inside a bin."""
    import numpy as np
    rows, cols, res = int(gridsize[0]), int(gridsize[1]), float(resolution)
    xt, yt = np.asarray(xt, dtype=np.float64).reshape(-1), np.asarray(yt, dtype=np.float64).reshape(-1)
    X, Y = cols * res, rows * res
    bin_size_m = max(res, float(np.sqrt(ALLEN_PER_BIN * X * Y / max(1, xt.size))))
    bin_size_m = max(bin_size_m, max(X, Y) / 32768.)           # (the library takes at most 32 768 bins along an axis)
    nbx, nby = max(1, int(np.ceil(X / bin_size_m))), max(1, int(np.ceil(Y / bin_size_m)))
    bx = np.minimum(np.floor(xt / bin_size_m), nbx - 1).astype(np.int64)
    by = np.minimum(np.floor(yt / bin_size_m), nby - 1).astype(np.int64)
    b = by * nbx + bx
    order = np.argsort(b, kind='stable')                    # (stable: the items of a bin stay in ascending order)
    bin_start = np.zeros(nbx * nby + 1, dtype=np.int64)
    np.cumsum(np.bincount(b, minlength=nbx * nby), out=bin_start[1:])
    return bin_start.astype(np.int32), order.astype(np.int32), bin_size_m, nbx, nby


def _allen_check_updrafts(xt, yt, wgain, rgain, gridsize, resolution):
    import numpy as np
    rows, cols, res = int(gridsize[0]), int(gridsize[1]), float(resolution)
    arrays = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (xt, yt, wgain, rgain)]
    n = arrays[0].size
    for name, a in zip(('xt', 'yt', 'wgain', 'rgain'), arrays):
        if a.size != n:
            raise ValueError(f'compute_allen_thermals: {name} has {a.size} values, xt {n}')
        if not np.isfinite(a).all():
            raise ValueError(f'compute_allen_thermals: {name} holds a non-finite value')
    for name, a, top in (('xt', arrays[0], cols * res), ('yt', arrays[1], rows * res)):
        if n and (a.min() < 0. or a.max() > top):
            raise ValueError(f'compute_allen_thermals: {name} leaves the domain [0, {top:g}] m '
                             f'(it spans {a.min():g} to {a.max():g})')
    return arrays


def compute_allen_thermals(xt, yt, wgain, rgain, gridsize, resolution, z, zi, wstar, sink=False, dtype=torch.float32,
                           path='auto', want_nearest=False, want_table=False, return_stats=False):
    """The vertical velocity of Allen's (2006) field of discrete updrafts at height z, one device call:
    every cell of the (rows, cols) raster takes the updraft nearest to it -- the lowest index among equally near ones --
    and evaluates its profile.  xt, yt (metres from the centre of cell (0, 0), inside [0, cols res] x [0, rows res]),
    wgain, rgain: host arrays as allen_updrafts gives them; their number is the field's N.  Returns a device tensor
    (rows, cols) in `dtype` (f64, or f32 = the f64 value rounded once), then the int32 raster of the nearest updraft
    (want_nearest), the (N, 6) f64 table r2, r1r2, r1, wbar, wpeak, row (want_table) and the number of cells that left
    the LDS path (return_stats) when asked, as a tuple."""
    import numpy as np
    if dtype not in (torch.float32, torch.float64):
        raise ValueError('compute_allen_thermals: dtype must be torch.float32 or torch.float64')
    if path not in nat.SSRS_ALLEN_PATH:
        raise ValueError(f'compute_allen_thermals: path = {path!r}: expected one of {tuple(nat.SSRS_ALLEN_PATH)}')
    rows, cols, res = int(gridsize[0]), int(gridsize[1]), float(resolution)
    xt, yt, wgain, rgain = _allen_check_updrafts(xt, yt, wgain, rgain, gridsize, resolution)
    n = xt.size
    if n > ALLEN_MAX_UPDRAFTS:
        raise ValueError(f'compute_allen_thermals: N = {n} updrafts, at most {ALLEN_MAX_UPDRAFTS} (SSRS_ALLEN_MAX_UPDRAFTS)')
    sc = allen_scalars(z, zi, wstar, gridsize, resolution, sink=False)
    we = 0.
    if sink:                                                 # (the sink of THIS field: its own N)
        area = n * np.pi * sc['rbar'] ** 2
        if not area < cols * res * rows * res:
            raise ValueError(f'compute_allen_thermals: the {n} updrafts of radius {sc["rbar"]:g} m cover the whole raster')
        we = min(-(sc['wtbar'] * area * (-2.5 * (sc['zzi'] - 0.5))) / (cols * res * rows * res - area), 0.)
    from ._device import device
    if n == 0:
        out = [torch.full((rows, cols), we, dtype=dtype, device=device())]
        if want_nearest:
            out.append(torch.full((rows, cols), -1, dtype=torch.int32, device=device()))
        if want_table:
            out.append(torch.empty((0, nat.SSRS_ALLEN_TABLE_COLS), dtype=torch.float64, device=device()))
        if return_stats:
            out.append(0)
        return out[0] if len(out) == 1 else tuple(out)
    bin_start, bin_items, bin_size_m, nbx, nby = allen_bins(xt, yt, gridsize, resolution)
    d = [to_dev(a, torch.float64) for a in (xt, yt, wgain, rgain)]
    d_start, d_items = to_dev(bin_start, torch.int32), to_dev(bin_items, torch.int32)
    out = torch.empty((rows, cols), dtype=dtype, device=d[0].device)
    nearest = torch.empty((rows, cols), dtype=torch.int32, device=out.device) if want_nearest else None
    table = torch.empty((n, nat.SSRS_ALLEN_TABLE_COLS), dtype=torch.float64, device=out.device) if want_table else None
    nbytes = nat.lib().ssrs_allen_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=out.device)
    nat.check(nat.lib().ssrs_allen_thermal_field(
        *(nat.ptr(a) for a in d), n, nat.ptr(d_start), nat.ptr(d_items), bin_size_m, nbx, nby,
        sc['rbar'], sc['wtbar'], sc['zzi'], int(sc['z_below_zi']), we, res, rows, cols, nat.SSRS_ALLEN_PATH[path],
        nat.ptr(out), nat.SSRS_F32 if dtype == torch.float32 else nat.SSRS_F64, nat.ptr(nearest), nat.ptr(table),
        nat.ptr(ws), nbytes, stream_ptr()))
    res_ = [out] + [t for t in (nearest, table) if t is not None]
    if return_stats:
        res_.append(int(ws[:8].view(torch.int64).item()))
    return res_[0] if len(res_) == 1 else tuple(res_)
