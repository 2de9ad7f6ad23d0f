"""Georeferencing (K10): the Albers Equal Area Conic projection and the warp of a longitude / latitude raster onto
the projected grid -- the stand-in for what the reference does through GDAL / PROJ in ssrs/raster.py
(get_raster_in_projected_crs, transform_coordinates, transform_bounds).

`Projection.forward` / `.inverse` are NumPy f64 transcriptions of ssrs_amd/csrc/georef.h, expression by expression
and in the same order: the CPU restatement the device is tested against, and what the simulator uses for the few
points it projects itself (corners, turbines, wind samples).  `warp_to_grid` is the device call."""
import ctypes as C
import re

import numpy as np
import torch

from . import _native as nat
from ._device import device, ftype, stream_ptr, to_dev, is_tensor

ITERATIONS = 4                       # kAlbersIterations of georef.h
_DEG = np.pi / 180.0                 # kDegToRad
_RAD = 180.0 / np.pi                 # kRadToDeg

# (a, 1 / f) or (a, b): e2 = 2 f - f^2
ELLIPSOIDS = {'GRS80': dict(a=6378137.0, rf=298.257222101), 'WGS84': dict(a=6378137.0, rf=298.257223563),
              'clrk66': dict(a=6378206.4, b=6356583.8)}
DATUMS = {'NAD83': 'GRS80', 'WGS84': 'WGS84'}
# (lat_1, lat_2, lat_0, lon_0, ellipsoid), recalled from the ESRI / EPSG registries (not verified
# against them here; the PROJ.4 form is the one a user can check)
NAMED = {'ESRI:102008': (20.0, 60.0, 40.0, -96.0, 'GRS80'), 'ESRI:102003': (29.5, 45.5, 37.5, -96.0, 'GRS80'),
         'EPSG:5070': (29.5, 45.5, 23.0, -96.0, 'GRS80')}
SUPPORTED = ('a PROJ.4 string "+proj=aea +lat_1= +lat_2= +lat_0= +lon_0= [+x_0= +y_0=] '
             f'(+ellps={"|".join(ELLIPSOIDS)} | +datum={"|".join(DATUMS)} | +a= +rf=)" or one of {", ".join(NAMED)}')


def _e2_of(a, rf=None, b=None):
    f = (a - b) / a if rf is None else 1.0 / rf
    return 2.0 * f - f * f


def _q(e2, e, sinphi):
    es = e * sinphi
    return (1.0 - e2) * (sinphi / (1.0 - e2 * (sinphi * sinphi)) - (1.0 / (2.0 * e)) * np.log((1.0 - es) / (1.0 + es)))


def _m(e2, sinphi, cosphi):
    return cosphi / np.sqrt(1.0 - e2 * (sinphi * sinphi))


class Projection:
    """Albers Equal Area Conic on an ellipsoid (Snyder, USGS PP 1395): the fields of SsrsProjection."""

    FIELDS = tuple(name for name, _ in nat.SsrsProjection._fields_)

    def __init__(self, a, e2, lat_1, lat_2, lat_0, lon_0, x_0=0.0, y_0=0.0, iterations=ITERATIONS):
        vals = [float(v) for v in (a, e2, lat_1, lat_2, lat_0, lon_0, x_0, y_0)]
        self.a, self.e2, self.lat_1, self.lat_2, self.lat_0, self.lon_0, self.x_0, self.y_0 = vals
        self.iterations = int(iterations)
        if not all(np.isfinite(vals)):
            raise ValueError(f'Projection: a non-finite parameter in {vals}')
        if not self.a > 0.0:
            raise ValueError(f'Projection: a = {self.a!r} must be > 0')
        if not 0.0 < self.e2 < 1.0:
            raise ValueError(f'Projection: e2 = {self.e2!r} must lie in (0, 1)')
        e = np.sqrt(self.e2)
        phi1, phi2, phi0 = self.lat_1 * _DEG, self.lat_2 * _DEG, self.lat_0 * _DEG
        s1, s2, s0 = np.sin(phi1), np.sin(phi2), np.sin(phi0)
        m1, m2 = _m(self.e2, s1, np.cos(phi1)), _m(self.e2, s2, np.cos(phi2))
        q1, q2, q0 = _q(self.e2, e, s1), _q(self.e2, e, s2), _q(self.e2, e, s0)
        n = (m1 * m1 - m2 * m2) / (q2 - q1) if q2 != q1 else s1
        if not np.isfinite(n) or abs(n) < 1e-12:
            raise ValueError(f'Projection: lat_1 = {self.lat_1!r}, lat_2 = {self.lat_2!r} give no cone (|n| < 1e-12: '
                             'lat_1 = -lat_2 is the cylindrical limit)')
        self.e, self.n = float(e), float(n)
        self.C = float(m1 * m1 + n * q1)
        self.rho0 = float(self.a * np.sqrt(self.C - n * q0) / n)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_crs(cls, crs):
        """A PROJ.4 string of an Albers projection or one of the named codes (`SUPPORTED`); ValueError otherwise."""
        if isinstance(crs, Projection):
            return crs
        text = str(crs).strip()
        if text.upper() in NAMED:
            lat_1, lat_2, lat_0, lon_0, ellps = NAMED[text.upper()]
            return cls(ELLIPSOIDS[ellps]['a'], _e2_of(**ELLIPSOIDS[ellps]), lat_1, lat_2, lat_0, lon_0)
        if not text.startswith('+'):
            raise ValueError(f'projected_crs = {crs!r} is not supported: expected {SUPPORTED}')
        args = {}
        for token in text.split():
            m = re.fullmatch(r'\+([A-Za-z_0-9]+)(?:=(\S+))?', token)
            if not m or m.group(1) in args:
                raise ValueError(f'projected_crs = {crs!r}: cannot read {token!r}; expected {SUPPORTED}')
            args[m.group(1)] = m.group(2)
        try:
            if args.pop('proj', None) != 'aea':
                raise KeyError('+proj=aea')
            if args.pop('units', 'm') != 'm' or args.pop('type', 'crs') != 'crs':
                raise KeyError('+units=m')
            args.pop('no_defs', None)
            num = {key: float(args.pop(key)) for key in ('lat_1', 'lat_2', 'lat_0', 'lon_0')}
            num.update({key: float(args.pop(key, 0.0)) for key in ('x_0', 'y_0')})
            given = [key for key in ('ellps', 'datum', 'a') if key in args]
            if len(given) != 1:
                raise KeyError('exactly one of +ellps=, +datum=, +a= +rf=')
            if given[0] == 'a':
                ell = dict(a=float(args.pop('a')), rf=float(args.pop('rf')))
            elif given[0] == 'datum':
                ell = ELLIPSOIDS[DATUMS[args.pop('datum')]]
            else:
                ell = ELLIPSOIDS[args.pop('ellps')]
            if args:
                raise KeyError(' '.join(f'+{key}' for key in args))
        except (KeyError, TypeError, ValueError) as exc:
            raise ValueError(f'projected_crs = {crs!r} is not supported ({exc}): expected {SUPPORTED}') from None
        return cls(ell['a'], _e2_of(**ell), **num)

    def as_struct(self):
        """The SsrsProjection the library takes, its derived fields filled by ssrs_projection_init_albers."""
        s = nat.SsrsProjection(self.a, self.e2, self.lat_1, self.lat_2, self.lat_0, self.lon_0, self.x_0, self.y_0)
        nat.check(nat.lib().ssrs_projection_init_albers(C.byref(s)))
        return s

    def __eq__(self, other):
        return isinstance(other, Projection) and all(getattr(self, f) == getattr(other, f) for f in self.FIELDS)

    def __repr__(self):
        return 'Projection(' + ', '.join(f'{f}={getattr(self, f)!r}' for f in self.FIELDS[:8]) + ')'

    # ------------------------------------------------------------------- arithmetic
    def forward(self, lon, lat):
        """(lon, lat) in degrees -> (x, y) in metres, f64 arrays of the broadcast shape (albers_forward)."""
        lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
        phi = lat * _DEG
        rho = self.a * np.sqrt(self.C - self.n * _q(self.e2, self.e, np.sin(phi))) / self.n
        theta = self.n * ((lon - self.lon_0) * _DEG)
        return self.x_0 + rho * np.sin(theta), self.y_0 + self.rho0 - rho * np.cos(theta)

    def inverse(self, x, y):
        """(x, y) in metres -> (lon, lat) in degrees (albers_inverse)."""
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        X = x - self.x_0
        Y = self.rho0 - (y - self.y_0)
        rho = np.sqrt(X * X + Y * Y)
        if self.n < 0.0:
            X, Y = -X, -Y
        theta = np.arctan2(X, Y)
        rn = rho * self.n / self.a
        qv = (self.C - rn * rn) / self.n
        lon = self.lon_0 + (theta / self.n) * _RAD
        with np.errstate(invalid='ignore', divide='ignore'):
            phi = np.arcsin(np.clip(qv / 2.0, -1.0, 1.0))
            qe, inv2e = qv / (1.0 - self.e2), 1.0 / (2.0 * self.e)
            for _ in range(self.iterations):
                s, c = np.sin(phi), np.cos(phi)
                es = self.e * s
                w = 1.0 - self.e2 * (s * s)
                phi = phi + (w * w) / (2.0 * c) * (qe - s / w + inv2e * np.log((1.0 - es) / (1.0 + es)))
        return lon, phi * _RAD


class LonLatRaster:
    """A raster on a regular longitude / latitude grid: `data` (rows, cols), a NumPy array or a tensor of f32 or f64,
    whose pixel (i, j) has its centre at (lon0 + j * dlon, lat0 + i * dlat) degrees.  The steps are signed: dlat < 0
    is a north-up array, the order a GeoTIFF comes in.  Pixels that are NaN or equal `nodata` are missing."""

    def __init__(self, data, lon0, lat0, dlon, dlat, nodata=None):
        dtype = data.dtype if is_tensor(data) else np.asarray(data).dtype
        if str(dtype).replace('torch.', '') not in ('float32', 'float64'):
            raise TypeError(f'LonLatRaster: data must be float32 or float64, not {dtype}')
        if len(data.shape) != 2 or min(data.shape) < 2:
            raise ValueError(f'LonLatRaster: data has shape {tuple(data.shape)}, expected (rows >= 2, cols >= 2)')
        self.data = data if is_tensor(data) else np.asarray(data)
        self.lon0, self.lat0, self.dlon, self.dlat = float(lon0), float(lat0), float(dlon), float(dlat)
        self.nodata = None if nodata is None else float(nodata)
        if not all(np.isfinite([self.lon0, self.lat0, self.dlon, self.dlat])) or self.dlon == 0. or self.dlat == 0.:
            raise ValueError(f'LonLatRaster: lon0, lat0 = {self.lon0!r}, {self.lat0!r} and the steps dlon, dlat = '
                             f'{self.dlon!r}, {self.dlat!r} must be finite and the steps not 0')

    @property
    def shape(self):
        return tuple(int(n) for n in self.data.shape)

    @property
    def lonlat_bounds(self):
        """(min_lon, min_lat, max_lon, max_lat) of the pixel centres: what a destination must stay inside."""
        lon1 = self.lon0 + (self.shape[1] - 1) * self.dlon
        lat1 = self.lat0 + (self.shape[0] - 1) * self.dlat
        return (min(self.lon0, lon1), min(self.lat0, lat1), max(self.lon0, lon1), max(self.lat0, lat1))


def warp_to_grid(raster, projection, west, south, gridsize, resolution, out_dtype=torch.float64, want_lonlat=False,
                 uncovered=None):
    """`raster` (a LonLatRaster) resampled bilinearly onto the projected grid whose cell (0, 0) has its centre at
    (west, south) metres, row 0 = south: ssrs_warp_lonlat_raster (include/ssrs_hip.h states the rule).
    Returns (dst, count), or (dst, lon, lat, count) with want_lonlat: device tensors (rows, cols) -- dst of
    `out_dtype`, lon / lat the f64 inverse projection of the cell centres in degrees -- and the number of cells of
    dst that are NaN because the source does not cover them or a pixel they need is missing.  `uncovered`: a device
    int64 tensor of one value to ACCUMULATE that number into (count is then its value after the call)."""
    if not isinstance(raster, LonLatRaster):
        raise TypeError(f'warp_to_grid: expected a LonLatRaster, not {type(raster).__name__}')
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f'warp_to_grid: out_dtype must be torch.float32 or torch.float64, not {out_dtype}')
    proj = Projection.from_crs(projection).as_struct()
    rows, cols = int(gridsize[0]), int(gridsize[1])
    if not (1 <= rows <= 32767 and 1 <= cols <= 32767):
        raise ValueError(f'warp_to_grid: gridsize = {(rows, cols)} must lie in [1, 32767]')
    dev = device()
    src = to_dev(raster.data)
    dst = torch.empty((rows, cols), dtype=out_dtype, device=dev)
    lon = torch.empty_like(dst, dtype=torch.float64) if want_lonlat else None
    lat = torch.empty_like(dst, dtype=torch.float64) if want_lonlat else None
    if uncovered is None:
        uncovered = torch.zeros(1, dtype=torch.int64, device=dev)
    elif not (is_tensor(uncovered) and uncovered.is_cuda and uncovered.dtype == torch.int64 and uncovered.numel() == 1):
        raise TypeError('warp_to_grid: uncovered must be a device int64 tensor of one value')
    nat.check(nat.lib().ssrs_warp_lonlat_raster(
        nat.ptr(src), ftype(src), src.shape[0], src.shape[1], raster.lon0, raster.lat0, raster.dlon, raster.dlat,
        float('nan') if raster.nodata is None else raster.nodata, C.byref(proj), float(west), float(south),
        float(resolution), nat.ptr(dst), ftype(dst), nat.ptr(lon), nat.ptr(lat), nat.ptr(uncovered), rows, cols,
        stream_ptr()))
    count = int(uncovered.item())
    return (dst, lon, lat, count) if want_lonlat else (dst, count)
