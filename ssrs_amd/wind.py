"""Wind-field preparation (K6) for snapshot / seasonal modes: WTK-shaped
lattice samples -> per-cell speed and direction rasters, following the u/v
recipe of /root/reference/ssrs/simulator.py:778-792."""
import ctypes as C

import numpy as np
import torch

from . import _native as nat
from ._device import stream_ptr, to_dev


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
        nat.ptr(ws.contiguous()), nat.ptr(wd.contiguous()), nx, ny, C.c_double(x[0]),
        C.c_double(y[0]), C.c_double(dx), C.c_double(dy), C.c_double(resolution / 1000.),
        nat.ptr(out_s), nat.ptr(out_d), rows, cols, batch, stream_ptr()))
    return (out_s[0], out_d[0]) if single else (out_s, out_d)


METHODS = ('nearest', 'linear', 'cubic')                       # scipy griddata's (reference: ssrs/config.py:44)


def check_method(method):
    """Lower-cased interpolation method; ValueError for anything griddata does not know (as griddata)."""
    name = str(method).lower()
    if name not in METHODS:
        raise ValueError(f"unknown interpolation method {method!r}: expected one of {METHODS}")
    return name


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
    if method == 'nearest':
        return _scattered_nearest(x_km, y_km, wspeed, wdirn, gridsize, resolution, index)
    if method == 'cubic':
        return _scattered_cubic(x_km, y_km, wspeed, wdirn, gridsize, resolution)
    from scipy.spatial import Delaunay
    x = np.asarray(x_km, dtype=np.float64).ravel()
    y = np.asarray(y_km, dtype=np.float64).ravel()
    if x.size != y.size or x.size < 3:
        raise ValueError('scattered wind samples need x_km, y_km of equal length >= 3')
    pts = np.ascontiguousarray(np.stack([x, y], 1))
    tri = Delaunay(pts)                                        # what griddata -> LinearNDInterpolator builds
    ws = to_dev(wspeed, torch.float64)
    wd = to_dev(wdirn, torch.float64)
    single = ws.dim() == 1
    if single:
        ws, wd = ws[None], wd[None]
    if ws.dim() != 2 or int(ws.shape[1]) != x.size or ws.shape != wd.shape:
        raise ValueError(f'scattered wind arrays must be (npts,) or (B, npts) with npts = {x.size}')
    batch = int(ws.shape[0])
    rows, cols = int(gridsize[0]), int(gridsize[1])
    dev = ws.device
    d_pts = torch.from_numpy(pts).to(dev)
    d_tri = torch.from_numpy(np.ascontiguousarray(tri.simplices.astype(np.int32))).to(dev)
    d_tr = torch.from_numpy(np.ascontiguousarray(tri.transform.astype(np.float64))).to(dev)
    out_s = torch.empty((batch, rows, cols), dtype=torch.float64, device=dev)
    out_d = torch.empty_like(out_s)
    L = nat.lib()
    nbytes = int(L.ssrs_wind_triangles_workspace_bytes(int(x.size), rows, cols, batch))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat.check(L.ssrs_wind_from_triangles(
        nat.ptr(d_pts), nat.ptr(d_tri), nat.ptr(d_tr), nat.ptr(ws.contiguous()), nat.ptr(wd.contiguous()),
        int(x.size), int(d_tri.shape[0]), C.c_double(resolution / 1000.), nat.ptr(out_s), nat.ptr(out_d), rows, cols, batch,
        nat.ptr(scratch), C.c_size_t(nbytes), stream_ptr()))
    return (out_s[0], out_d[0]) if single else (out_s, out_d)


def _samples(x_km, y_km, wspeed, wdirn, least):
    """points (npts, 2), wspeed / wdirn as (B, npts) numpy f64, and whether the caller gave one snapshot."""
    x = np.asarray(x_km, dtype=np.float64).ravel()
    y = np.asarray(y_km, dtype=np.float64).ravel()
    if x.size != y.size or x.size < least:
        raise ValueError(f'scattered wind samples need x_km, y_km of equal length >= {least}')
    ws = np.asarray(wspeed.cpu() if isinstance(wspeed, torch.Tensor) else wspeed, dtype=np.float64)
    wd = np.asarray(wdirn.cpu() if isinstance(wdirn, torch.Tensor) else wdirn, dtype=np.float64)
    single = ws.ndim == 1
    if single:
        ws, wd = ws[None], wd[None]
    if ws.ndim != 2 or ws.shape[1] != x.size or ws.shape != wd.shape:
        raise ValueError(f'scattered wind arrays must be (npts,) or (B, npts) with npts = {x.size}')
    return np.ascontiguousarray(np.stack([x, y], 1)), np.ascontiguousarray(ws), np.ascontiguousarray(wd), single


def nearest_sample_index(x_km, y_km, gridsize, resolution):
    """(rows, cols) int32 CUDA raster: per cell the index of the sample nearest to its centre (Euclidean, the lowest
    index among equally near ones) -- what griddata's 'nearest' looks up through cKDTree.  It depends on the points
    only: build it once and hand it to `interpolate_wind_scattered(..., method='nearest', index=...)`."""
    x = np.asarray(x_km, dtype=np.float64).ravel()
    y = np.asarray(y_km, dtype=np.float64).ravel()
    if x.size != y.size or x.size < 1:
        raise ValueError('scattered wind samples need x_km, y_km of equal length >= 1')
    rows, cols = int(gridsize[0]), int(gridsize[1])
    d_pts = to_dev(np.ascontiguousarray(np.stack([x, y], 1)), torch.float64)
    index = torch.empty((rows, cols), dtype=torch.int32, device=d_pts.device)
    L = nat.lib()
    nbytes = int(L.ssrs_wind_nearest_workspace_bytes(int(x.size), rows, cols))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=d_pts.device)
    nat.check(L.ssrs_wind_nearest_index(nat.ptr(d_pts), int(x.size), C.c_double(resolution / 1000.), nat.ptr(index),
                                        rows, cols, nat.ptr(scratch), C.c_size_t(nbytes), stream_ptr()))
    return index


def _scattered_nearest(x_km, y_km, wspeed, wdirn, gridsize, resolution, index):
    pts, ws, wd, single = _samples(x_km, y_km, wspeed, wdirn, 1)
    rows, cols = int(gridsize[0]), int(gridsize[1])
    if index is None:
        index = nearest_sample_index(pts[:, 0], pts[:, 1], gridsize, resolution)
    if not (isinstance(index, torch.Tensor) and index.is_cuda and index.dtype == torch.int32 and
            tuple(index.shape) == (rows, cols)):
        raise ValueError(f'index must be an int32 CUDA tensor of shape {(rows, cols)} (nearest_sample_index)')
    d_ws, d_wd = to_dev(ws, torch.float64), to_dev(wd, torch.float64)
    batch = int(ws.shape[0])
    out_s = torch.empty((batch, rows, cols), dtype=torch.float64, device=index.device)
    out_d = torch.empty_like(out_s)
    nat.check(nat.lib().ssrs_wind_from_nearest(nat.ptr(index.contiguous()), nat.ptr(d_ws), nat.ptr(d_wd), int(pts.shape[0]),
                                               nat.ptr(out_s), nat.ptr(out_d), rows, cols, batch, stream_ptr()))
    return (out_s[0], out_d[0]) if single else (out_s, out_d)


def _scattered_cubic(x_km, y_km, wspeed, wdirn, gridsize, resolution):
    from scipy.interpolate import CloughTocher2DInterpolator
    from scipy.spatial import Delaunay
    pts, ws, wd, single = _samples(x_km, y_km, wspeed, wdirn, 3)
    batch, npts = ws.shape
    tri = Delaunay(pts)                                        # what griddata -> CloughTocher2DInterpolator builds
    east = ws * np.sin(wd * np.pi / 180.)                      # simulator.py:784-785
    north = ws * np.cos(wd * np.pi / 180.)
    # the vertex gradients: scipy's estimator with griddata's parameters, every field in one call (column by column
    # the same bits as the single-field calls griddata makes)
    values = np.ascontiguousarray(np.concatenate([east, north], 0).T)             # (npts, 2 B)
    grad = CloughTocher2DInterpolator(tri, values, tol=1e-6, maxiter=400).grad     # (npts, 2 B, 2)
    grad = np.ascontiguousarray(np.transpose(grad, (1, 0, 2)))                     # (2 B, npts, 2)
    rows, cols = int(gridsize[0]), int(gridsize[1])
    d_pts = to_dev(pts, torch.float64)
    dev = d_pts.device
    d_tri = torch.from_numpy(np.ascontiguousarray(tri.simplices.astype(np.int32))).to(dev)
    d_nbr = torch.from_numpy(np.ascontiguousarray(tri.neighbors.astype(np.int32))).to(dev)
    d_tr = torch.from_numpy(np.ascontiguousarray(tri.transform.astype(np.float64))).to(dev)
    d_east, d_north = torch.from_numpy(np.ascontiguousarray(east)).to(dev), torch.from_numpy(np.ascontiguousarray(north)).to(dev)
    d_ge, d_gn = torch.from_numpy(grad[:batch].copy()).to(dev), torch.from_numpy(grad[batch:].copy()).to(dev)
    out_s = torch.empty((batch, rows, cols), dtype=torch.float64, device=dev)
    out_d = torch.empty_like(out_s)
    L = nat.lib()
    ntri = int(d_tri.shape[0])
    nbytes = int(L.ssrs_wind_cubic_workspace_bytes(int(npts), ntri, rows, cols, int(batch)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat.check(L.ssrs_wind_from_triangles_cubic(
        nat.ptr(d_pts), nat.ptr(d_tri), nat.ptr(d_nbr), nat.ptr(d_tr), nat.ptr(d_east), nat.ptr(d_north), nat.ptr(d_ge),
        nat.ptr(d_gn), int(npts), ntri, C.c_double(resolution / 1000.), nat.ptr(out_s), nat.ptr(out_d), rows, cols, int(batch),
        nat.ptr(scratch), C.c_size_t(nbytes), stream_ptr()))
    return (out_s[0], out_d[0]) if single else (out_s, out_d)


def _scalar_geometry(x_km, y_km, values, gridsize, resolution, method, index, what):
    """Host side of a scalar interpolation: what scipy builds from the points (the triangulation, for 'cubic' the
    vertex gradients of every field) or the nearest-index raster, as device tensors.  values: numpy (F, npts) f64.
    Returns the leading arguments of ssrs_scalar_from_samples / ssrs_wtk_thermal_fields up to cell_size, the tensors
    that back them, and the workspace."""
    x = np.asarray(x_km, dtype=np.float64).ravel()
    y = np.asarray(y_km, dtype=np.float64).ravel()
    least = 1 if method == 'nearest' else 3
    if x.size != y.size or x.size < least:
        raise ValueError(f'{what}: samples need x_km, y_km of equal length >= {least}')
    if values.ndim != 2 or values.shape[1] != x.size:
        raise ValueError(f'{what}: sample arrays must be (npts,) or (F, npts) with npts = {x.size}')
    rows, cols = int(gridsize[0]), int(gridsize[1])
    npts, nfield = int(x.size), int(values.shape[0])
    pts = np.ascontiguousarray(np.stack([x, y], 1))
    keep = {'values': to_dev(np.ascontiguousarray(values), torch.float64)}
    dev = keep['values'].device
    ntri = 0
    if method == 'nearest':
        if index is None:
            index = nearest_sample_index(x, y, gridsize, resolution)
        if not (isinstance(index, torch.Tensor) and index.is_cuda and index.dtype == torch.int32 and
                tuple(index.shape) == (rows, cols)):
            raise ValueError(f'index must be an int32 CUDA tensor of shape {(rows, cols)} (nearest_sample_index)')
        keep['index'] = index.contiguous()
    else:
        from scipy.spatial import Delaunay
        tri = Delaunay(pts)                                    # what griddata builds for 'linear' and 'cubic'
        keep['pts'] = torch.from_numpy(pts).to(dev)
        keep['tri'] = torch.from_numpy(np.ascontiguousarray(tri.simplices.astype(np.int32))).to(dev)
        keep['tr'] = torch.from_numpy(np.ascontiguousarray(tri.transform.astype(np.float64))).to(dev)
        ntri = int(keep['tri'].shape[0])
        if method == 'cubic':
            from scipy.interpolate import CloughTocher2DInterpolator
            # scipy's gradient estimator with griddata's parameters, every field in one call (column by column the
            # same bits as the single-field calls griddata makes)
            grad = CloughTocher2DInterpolator(tri, np.ascontiguousarray(values.T), tol=1e-6, maxiter=400).grad
            keep['grad'] = torch.from_numpy(np.ascontiguousarray(np.transpose(grad, (1, 0, 2)))).to(dev)   # (F, npts, 2)
            keep['nbr'] = torch.from_numpy(np.ascontiguousarray(tri.neighbors.astype(np.int32))).to(dev)
    code = nat.SSRS_INTERP[method]
    nbytes = int(nat.lib().ssrs_scalar_interp_workspace_bytes(code, ntri, rows, cols, nfield))
    keep['scratch'] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    head = [code, nat.ptr(keep.get('pts')), nat.ptr(keep.get('tri')), nat.ptr(keep.get('nbr')), nat.ptr(keep.get('tr')),
            nat.ptr(keep.get('index')), nat.ptr(keep['values']), nat.ptr(keep.get('grad')), npts, ntri,
            C.c_double(resolution / 1000.)]
    tail = [nat.ptr(keep['scratch']), C.c_size_t(nbytes), stream_ptr()]
    return head, tail, keep


def _host_f64(a):
    return np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def interpolate_scalar_scattered(x_km, y_km, values, gridsize, resolution, method='linear', index=None):
    """The reference's `_interpolate_wtk_vardata` (ssrs/simulator.py:765-776): scipy griddata of
    scalar samples at SCATTERED points x_km[npts], y_km[npts] (relative to the raster's south-west cell centre) onto
    the raster's cell centres.  values: (npts,) or (F, npts) for F fields on the same points.  Returns an f64 CUDA
    tensor (rows, cols) or (F, rows, cols); NaN outside the convex hull for 'linear' and 'cubic', as griddata.
    method, index: as `interpolate_wind_scattered`.  The cells are evaluated by the expressions of the wind kernels."""
    method = check_method(method)
    vals = _host_f64(values)
    single = vals.ndim == 1
    if single:
        vals = vals[None]
    head, tail, keep = _scalar_geometry(x_km, y_km, vals, gridsize, resolution, method, index, 'interpolate_scalar_scattered')
    rows, cols = int(gridsize[0]), int(gridsize[1])
    out = torch.empty((vals.shape[0], rows, cols), dtype=torch.float64, device=keep['values'].device)
    nat.check(nat.lib().ssrs_scalar_from_samples(*head, nat.ptr(out), rows, cols, int(vals.shape[0]), *tail))
    return out[0] if single else out
