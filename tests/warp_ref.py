"""NumPy restatement of the warp rule of ssrs_warp_lonlat_raster (include/ssrs_hip.h) and the small geometries the
K10 tests share: an analytic longitude / latitude DEM placed under a destination grid on ESRI:102008."""
import numpy as np

from ssrs_amd.georef import LonLatRaster, Projection

EDGE_PX = 1e-6            # cells this close to the source's edge are left out: rounding may decide their coverage


def bilinear_ref(src, fr, fc, nodata=None):
    """The rule at the fractional pixel (fr, fc), in f64 and in the kernel's order; NaN where the cell is not covered
    or a neighbour of non-zero weight is NaN or equals nodata.  Also returns max - min of the neighbours read."""
    src = np.asarray(src)
    rows, cols = src.shape
    fr, fc = np.asarray(fr, dtype=np.float64), np.asarray(fc, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        covered = (fr >= 0.) & (fr <= rows - 1) & (fc >= 0.) & (fc <= cols - 1)
    i = np.minimum(np.floor(np.where(covered, fr, 0.)).astype(np.int64), rows - 2)
    j = np.minimum(np.floor(np.where(covered, fc, 0.)).astype(np.int64), cols - 2)
    tr, tc = np.where(covered, fr, 0.) - i, np.where(covered, fc, 0.) - j
    ur, uc = 1. - tr, 1. - tc

    def pixel(di, dj, used):
        v = src[i + di, j + dj].astype(np.float64)
        if nodata is not None:
            v = np.where(v == nodata, np.nan, v)
        return np.where(used, v, 0.), np.where(used, v, np.nan)

    (z00, s00), (z01, s01) = pixel(0, 0, (ur != 0.) & (uc != 0.)), pixel(0, 1, (ur != 0.) & (tc != 0.))
    (z10, s10), (z11, s11) = pixel(1, 0, (tr != 0.) & (uc != 0.)), pixel(1, 1, (tr != 0.) & (tc != 0.))
    val = (z00 * uc + z01 * tc) * ur + (z10 * uc + z11 * tc) * tr
    seen = np.stack([s00, s01, s10, s11])
    spread = np.nan_to_num(np.fmax.reduce(seen, 0) - np.fmin.reduce(seen, 0))     # (fmax / fmin skip NaN)
    return np.where(covered, val, np.nan), spread


def pixel_coordinates(raster, lon, lat):
    """(fr, fc) of the points in the raster: the two IEEE operations the kernel makes."""
    return (np.asarray(lat) - raster.lat0) / raster.dlat, (np.asarray(lon) - raster.lon0) / raster.dlon


def near_edge(raster, fr, fc):
    rows, cols = raster.shape
    return (np.abs(fr) <= EDGE_PX) | (np.abs(fr - (rows - 1)) <= EDGE_PX) | \
        (np.abs(fc) <= EDGE_PX) | (np.abs(fc - (cols - 1)) <= EDGE_PX)


def analytic_dem(lon, lat):
    """Smooth terrain in metres as a function of degrees."""
    return 1500. + 300. * np.sin(lon * 9.) * np.cos(lat * 7.) + 120. * np.sin(lon * 31. + lat * 17.) + 40. * (lon + 106.)


class Geometry:
    """A destination grid (rows, cols) at `res` metres whose cell (0, 0) is the image of (-106.21, 42.78), and a source
    of `src_shape` pixels with dyadic steps (1 / 64 degree in longitude, `dlat` in latitude) centred under it and
    shifted by `shift_px` source pixels east.  Dyadic steps and origins make (phi - lat0) / dlat exact, so that the
    flipped source gives the same fr mirrored and the bits of dst do not depend on the row order."""

    def __init__(self, shape, src_shape, res=400., dlat=1. / 64., shift_px=0, crs='ESRI:102008'):
        self.proj = Projection.from_crs(crs)
        self.shape, self.res = shape, res
        self.west, self.south = (float(v) for v in self.proj.forward(-106.21, 42.78))
        x = self.west + np.arange(shape[1], dtype=np.float64) * res
        y = self.south + np.arange(shape[0], dtype=np.float64) * res
        self.lon, self.lat = self.proj.inverse(*np.meshgrid(x, y))
        dlon = 1. / 64.
        mid_lon, mid_lat = 0.5 * (self.lon.min() + self.lon.max()), 0.5 * (self.lat.min() + self.lat.max())
        lon0 = np.round((mid_lon - 0.5 * (src_shape[1] - 1) * dlon) * 128.) / 128. + shift_px * dlon
        lat0 = np.round((mid_lat - 0.5 * (src_shape[0] - 1) * dlat) * 128.) / 128.
        self.src_lon = lon0 + np.arange(src_shape[1]) * dlon
        self.src_lat = lat0 + np.arange(src_shape[0]) * dlat
        self.values = analytic_dem(*np.meshgrid(self.src_lon, self.src_lat))
        self.grid = (lon0, lat0, dlon, dlat)

    def raster(self, dtype=np.float64, north_up=False, values=None, nodata=None):
        lon0, lat0, dlon, dlat = self.grid
        data = np.ascontiguousarray((self.values if values is None else values).astype(dtype))
        if north_up:
            return LonLatRaster(np.ascontiguousarray(data[::-1]), lon0, lat0 + (data.shape[0] - 1) * dlat, dlon, -dlat, nodata)
        return LonLatRaster(data, lon0, lat0, dlon, dlat, nodata)

    def cpu(self, raster):
        """(values, spread, near_edge) of the full CPU restatement on this destination."""
        fr, fc = pixel_coordinates(raster, self.lon, self.lat)
        val, spread = bilinear_ref(raster.data, fr, fc, raster.nodata)
        return val, spread, near_edge(raster, fr, fc)


DESTINATIONS = ((37, 53), (40, 64))                       # scalar tail / vector stores
SOURCES = (((41, 29), 1. / 64.), ((64, 48), 1. / 128.))   # (shape, dlat)


def geometries(overhang=False):
    """Every destination over every source; overhang: the source moved east by half its width, so that the western
    half of the destination has nothing under it."""
    return [Geometry(dst, src, dlat=dlat, shift_px=src[1] // 2 if overhang else 0) for dst in DESTINATIONS for src, dlat in SOURCES]
