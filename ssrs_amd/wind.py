"""Wind-field preparation (K6) for snapshot / seasonal modes: WTK-shaped
lattice samples -> per-cell speed and direction rasters, following the u/v
recipe of /root/reference/ssrs/simulator.py:778-792."""

import numpy as np
import torch

from . import _native as nat
from ._device import stream_ptr, to_dev
from .inputs import METHODS, host_f64


def interpolate_wind_lattice(x_km, y_km, wspeed, wdirn, gridsize, resolution):
    """x_km[nx], y_km[ny]: lattice coordinates (uniform spacing) relative to
    the raster's south-west cell centre; wspeed/wdirn: (ny, nx) or (B, ny, nx).
    Returns (wspeed, wdirn) f64 CUDA tensors (rows, cols) or (B, rows, cols)."""
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
    rows, cols = int(gridsize[0]), int(gridsize[1])
    out_s = torch.empty((batch, rows, cols), dtype=torch.float64, device=ws.device)
    out_d = torch.empty_like(out_s)
    nat.check(nat.lib().ssrs_wind_from_lattice(
        nat.ptr(ws.contiguous()), nat.ptr(wd.contiguous()), nx, ny, x[0], y[0], dx, dy, resolution / 1000.,
        nat.ptr(out_s), nat.ptr(out_d), rows, cols, batch, stream_ptr()))
    return (out_s[0], out_d[0]) if single else (out_s, out_d)


def check_method(method):
    """Lower-cased interpolation method; ValueError for anything griddata does not know (as griddata)."""
    name = str(method).lower()
    if name not in METHODS:
        raise ValueError(f"unknown interpolation method {method!r}: expected one of {METHODS}")
    return name


def _points(x_km, y_km, least, what='scattered wind samples'):
    """The sample points as a contiguous (npts, 2) f64 array."""
    x, y = host_f64(x_km).ravel(), host_f64(y_km).ravel()
    if x.size != y.size or x.size < least:
        raise ValueError(f'{what} need x_km, y_km of equal length >= {least}')
    return np.ascontiguousarray(np.stack([x, y], 1))


def _geometry(pts, method, grad_values, index, gridsize, resolution):
    """What scipy builds from the points (npts, 2) for griddata's `method`, as device tensors: 'pts', 'tri' and 'tr' (the
    Delaunay triangulation LinearNDInterpolator and CloughTocher2DInterpolator both start from); for 'cubic' also 'nbr'
    and 'grad' (F, npts, 2), the vertex gradients of the fields grad_values (npts, F) from scipy's estimator with
    griddata's parameters -- every field in one call, column by column the same bits as the single-field calls griddata
    makes; for 'nearest' only 'index', the given or freshly built `nearest_sample_index` raster."""
    if method == 'nearest':
        rows, cols = int(gridsize[0]), int(gridsize[1])
        if index is None:
            index = nearest_sample_index(pts[:, 0], pts[:, 1], gridsize, resolution)
        if not (isinstance(index, torch.Tensor) and index.is_cuda and index.dtype == torch.int32 and
                tuple(index.shape) == (rows, cols)):
            raise ValueError(f'index must be an int32 CUDA tensor of shape {(rows, cols)} (nearest_sample_index)')
        return {'index': index.contiguous()}
    from scipy.spatial import Delaunay
    tri = Delaunay(pts)
    geo = {'pts': to_dev(pts), 'tri': to_dev(tri.simplices.astype(np.int32)), 'tr': to_dev(tri.transform.astype(np.float64))}
    if method == 'cubic':
        from scipy.interpolate import CloughTocher2DInterpolator
        grad = CloughTocher2DInterpolator(tri, np.ascontiguousarray(grad_values), tol=1e-6, maxiter=400).grad   # (npts, F, 2)
        geo['grad'] = to_dev(np.transpose(grad, (1, 0, 2)))
        geo['nbr'] = to_dev(tri.neighbors.astype(np.int32))
    return geo


def interpolate_wind_scattered(x_km, y_km, wspeed, wdirn, gridsize, resolution, method='linear', index=None):
    """The reference's general case (/root/reference/ssrs/simulator.py:765-792): wind samples at SCATTERED points
    x_km[npts], y_km[npts] (relative to the raster's south-west cell centre), wspeed / wdirn (npts,) or (B, npts).
    `scipy.interpolate.griddata(..., method='linear')` is a Delaunay triangulation + barycentric interpolation: the
    triangulation is built here on the host by the same scipy class griddata uses (a few thousand points), the
    30 M cells are interpolated by the HIP kernels behind `ssrs_wind_from_triangles`.  Returns (wspeed, wdirn) f64
    CUDA tensors (rows, cols) or (B, rows, cols); NaN outside the convex hull of the points, as griddata.
    method: griddata's 'nearest' | 'linear' | 'cubic' (any case).  'nearest' has no hull and no NaN; `index` is its
    optional prebuilt `nearest_sample_index` raster (it depends on the points only).  'cubic' takes the vertex
    gradients from scipy's own estimator and evaluates the Clough-Tocher patches on the device."""
    method = check_method(method)
    pts = _points(x_km, y_km, 1 if method == 'nearest' else 3)
    npts = int(pts.shape[0])
    ws, wd = host_f64(wspeed), host_f64(wdirn)
    single = ws.ndim == 1
    if single:
        ws, wd = ws[None], wd[None]
    if ws.ndim != 2 or ws.shape[1] != npts or ws.shape != wd.shape:
        raise ValueError(f'scattered wind arrays must be (npts,) or (B, npts) with npts = {npts}')
    batch = int(ws.shape[0])
    if method == 'cubic':
        ws, wd = ws * np.sin(wd * np.pi / 180.), ws * np.cos(wd * np.pi / 180.)      # east, north: simulator.py:784-785
    geo = _geometry(pts, method, np.concatenate([ws, wd], 0).T, index, gridsize, resolution)
    d_a, d_b = to_dev(ws, torch.float64), to_dev(wd, torch.float64)
    rows, cols = int(gridsize[0]), int(gridsize[1])
    out_s = torch.empty((batch, rows, cols), dtype=torch.float64, device=d_a.device)
    out_d = torch.empty_like(out_s)
    L = nat.lib()
    cell, out = resolution / 1000., (nat.ptr(out_s), nat.ptr(out_d), rows, cols, batch)
    if method == 'nearest':
        nat.check(L.ssrs_wind_from_nearest(nat.ptr(geo['index']), nat.ptr(d_a), nat.ptr(d_b), npts, *out, stream_ptr()))
        return (out_s[0], out_d[0]) if single else (out_s, out_d)
    ntri = int(geo['tri'].shape[0])
    if method == 'linear':
        nbytes = int(L.ssrs_wind_triangles_workspace_bytes(npts, rows, cols, batch))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=d_a.device)
        nat.check(L.ssrs_wind_from_triangles(
            nat.ptr(geo['pts']), nat.ptr(geo['tri']), nat.ptr(geo['tr']), nat.ptr(d_a), nat.ptr(d_b), npts, ntri, cell, *out,
            nat.ptr(scratch), nbytes, stream_ptr()))
    else:
        nbytes = int(L.ssrs_wind_cubic_workspace_bytes(npts, ntri, rows, cols, batch))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=d_a.device)
        nat.check(L.ssrs_wind_from_triangles_cubic(
            nat.ptr(geo['pts']), nat.ptr(geo['tri']), nat.ptr(geo['nbr']), nat.ptr(geo['tr']), nat.ptr(d_a), nat.ptr(d_b),
            nat.ptr(geo['grad'][:batch]), nat.ptr(geo['grad'][batch:]), npts, ntri, cell, *out,
            nat.ptr(scratch), nbytes, stream_ptr()))
    return (out_s[0], out_d[0]) if single else (out_s, out_d)


def nearest_sample_index(x_km, y_km, gridsize, resolution):
    """(rows, cols) int32 CUDA raster: per cell the index of the sample nearest to its centre (Euclidean, the lowest
    index among equally near ones) -- what griddata's 'nearest' looks up through cKDTree.  It depends on the points
    only: build it once and hand it to `interpolate_wind_scattered(..., method='nearest', index=...)`."""
    pts = _points(x_km, y_km, 1)
    rows, cols = int(gridsize[0]), int(gridsize[1])
    d_pts = to_dev(pts, torch.float64)
    index = torch.empty((rows, cols), dtype=torch.int32, device=d_pts.device)
    L = nat.lib()
    nbytes = int(L.ssrs_wind_nearest_workspace_bytes(int(pts.shape[0]), rows, cols))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=d_pts.device)
    nat.check(L.ssrs_wind_nearest_index(nat.ptr(d_pts), int(pts.shape[0]), resolution / 1000., nat.ptr(index),
                                        rows, cols, nat.ptr(scratch), nbytes, stream_ptr()))
    return index


def _scalar_geometry(x_km, y_km, values, gridsize, resolution, method, index, what):
    """Host side of a scalar interpolation: `_geometry` of the points and of the fields values (numpy (F, npts) f64).
    Returns the leading arguments of ssrs_scalar_from_samples / ssrs_wtk_thermal_fields up to cell_size, the tensors
    that back them, and the workspace."""
    pts = _points(x_km, y_km, 1 if method == 'nearest' else 3, f'{what}: samples')
    npts = int(pts.shape[0])
    if values.ndim != 2 or values.shape[1] != npts:
        raise ValueError(f'{what}: sample arrays must be (npts,) or (F, npts) with npts = {npts}')
    rows, cols = int(gridsize[0]), int(gridsize[1])
    keep = _geometry(pts, method, values.T, index, gridsize, resolution)
    keep['values'] = to_dev(np.ascontiguousarray(values), torch.float64)
    ntri = int(keep['tri'].shape[0]) if 'tri' in keep else 0
    code = nat.SSRS_INTERP[method]
    nbytes = int(nat.lib().ssrs_scalar_interp_workspace_bytes(code, ntri, rows, cols, int(values.shape[0])))
    keep['scratch'] = torch.empty(nbytes, dtype=torch.uint8, device=keep['values'].device)
    head = [code, nat.ptr(keep.get('pts')), nat.ptr(keep.get('tri')), nat.ptr(keep.get('nbr')), nat.ptr(keep.get('tr')),
            nat.ptr(keep.get('index')), nat.ptr(keep['values']), nat.ptr(keep.get('grad')), npts, ntri, resolution / 1000.]
    tail = [nat.ptr(keep['scratch']), nbytes, stream_ptr()]
    return head, tail, keep


def interpolate_scalar_scattered(x_km, y_km, values, gridsize, resolution, method='linear', index=None):
    """The reference's `_interpolate_wtk_vardata` (ssrs/simulator.py:765-776): scipy griddata of
    scalar samples at SCATTERED points x_km[npts], y_km[npts] (relative to the raster's south-west cell centre) onto
    the raster's cell centres.  values: (npts,) or (F, npts) for F fields on the same points.  Returns an f64 CUDA
    tensor (rows, cols) or (F, rows, cols); NaN outside the convex hull for 'linear' and 'cubic', as griddata.
    method, index: as `interpolate_wind_scattered`.  The cells are evaluated by the expressions of the wind kernels."""
    method = check_method(method)
    vals = host_f64(values)
    single = vals.ndim == 1
    if single:
        vals = vals[None]
    head, tail, keep = _scalar_geometry(x_km, y_km, vals, gridsize, resolution, method, index, 'interpolate_scalar_scattered')
    rows, cols = int(gridsize[0]), int(gridsize[1])
    out = torch.empty((vals.shape[0], rows, cols), dtype=torch.float64, device=keep['values'].device)
    nat.check(nat.lib().ssrs_scalar_from_samples(*head, nat.ptr(out), rows, cols, int(vals.shape[0]), *tail))
    return out[0] if single else out
