"""The contract of the K6 interpolation family (include/ssrs_hip.h: ssrs_wind_from_lattice, ssrs_wind_from_triangles,
ssrs_wind_nearest_index, ssrs_wind_from_nearest, ssrs_wind_from_triangles_cubic, ssrs_scalar_from_samples) in plain
numpy f64, and the tiny geometries on which the device is held to it.  test_interp_ref_host.py pins these functions to
scipy before test_gpu_interp_edges.py judges the kernels by them.

Points are in km relative to the centre of cell (0, 0), x along columns and y along rows; the centre of cell (r, c) is
(c * cell, r * cell)."""
import numpy as np

EPS = 100. * np.finfo(np.float64).eps          # scipy's containment tolerance, the header's eps


def mesh(rows, cols, cell):
    """(xm, ym): the cell centres, each (rows, cols)."""
    return np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)


def owner_linear(points, rows, cols, cell, values):
    """'linear' by the header's rule: scipy.spatial.Delaunay(points); a triangle contains a cell centre when all three
    barycentric coordinates lie within [-eps, 1 + eps]; the LOWEST triangle index wins a cell, a cell without an owner is
    NaN; value = b0 * v0 + b1 * v1 + b2 * v2 summed left to right.  values: (npts,) or (F, npts).
    Returns (values (rows, cols) or (F, rows, cols), owner (rows, cols) int64 with -1 for none, mask of the cells that
    more than one triangle contains)."""
    from scipy.spatial import Delaunay
    points = np.asarray(points, dtype=np.float64)
    tri = Delaunay(points)
    vals = np.asarray(values, dtype=np.float64)
    single = vals.ndim == 1
    if single:
        vals = vals[None]
    xm, ym = mesh(rows, cols, cell)
    owner = np.full((rows, cols), -1, dtype=np.int64)
    count = np.zeros((rows, cols), dtype=np.int64)
    out = np.full((vals.shape[0], rows, cols), np.nan)
    for t in range(tri.simplices.shape[0] - 1, -1, -1):           # downwards: the lowest index writes last
        T = tri.transform[t]
        dx, dy = xm - T[2, 0], ym - T[2, 1]
        b0 = T[0, 0] * dx + T[0, 1] * dy
        b1 = T[1, 0] * dx + T[1, 1] * dy
        b2 = 1. - b0 - b1
        with np.errstate(invalid='ignore'):
            inside = np.ones((rows, cols), dtype=bool)
            for b in (b0, b1, b2):
                inside &= (b >= -EPS) & (b <= 1. + EPS)
        count += inside
        owner[inside] = t
        v0, v1, v2 = tri.simplices[t]
        with np.errstate(invalid='ignore'):
            for f in range(vals.shape[0]):
                v = b0 * vals[f, v0] + b1 * vals[f, v1] + b2 * vals[f, v2]
                out[f][inside] = v[inside]
    return (out[0] if single else out), owner, count > 1


def nearest_index(points, rows, cols, cell):
    """'nearest' by the header's rule: argmin of dx * dx + dy * dy over all samples, the first (lowest) index among
    equal minima.  (rows, cols) int64."""
    points = np.asarray(points, dtype=np.float64)
    xm, ym = mesh(rows, cols, cell)
    dx, dy = xm[..., None] - points[:, 0], ym[..., None] - points[:, 1]
    return np.argmin(dx * dx + dy * dy, axis=2)


def components(speed, dirn):
    """east, north of speed / direction samples (simulator.py:784-785 of the reference)."""
    a = np.asarray(dirn, dtype=np.float64) * np.pi / 180.
    return speed * np.sin(a), speed * np.cos(a)


def uv_recipe(east, north):
    """speed = sqrt(e^2 + n^2), direction = mod(atan2(e, n) + 2 pi, 2 pi) in degrees."""
    east, north = np.asarray(east, dtype=np.float64), np.asarray(north, dtype=np.float64)
    spd = np.sqrt(np.square(east) + np.square(north))
    ang = np.mod(np.arctan2(east, north) + 2. * np.pi, 2. * np.pi) * 180. / np.pi
    return spd, ang


def direction_gap(a, b):
    """The gap between two directions on the circle, degrees."""
    dd = np.abs(np.asarray(a) - np.asarray(b)) % 360.
    return np.minimum(dd, 360. - dd)


def _axis(coord, lattice):
    """Per cell coordinate: lower lattice index, upper lattice index and weight of the upper one, after the clamp to
    [lattice[0], lattice[-1]].  One lattice point collapses the axis."""
    n = lattice.size
    if n == 1:
        zero = np.zeros(coord.size, dtype=np.int64)
        return zero, zero, np.zeros(coord.size)
    x = np.clip(coord, lattice[0], lattice[-1])
    lo = np.clip(np.searchsorted(lattice, x, side='right') - 1, 0, n - 2)
    return lo, lo + 1, (x - lattice[lo]) / (lattice[lo + 1] - lattice[lo])


def lattice_uv(x, y, ws, wd, rows, cols, cell):
    """ssrs_wind_from_lattice up to the recipe: cell centres clamped to the hull of the lattice x[nx] x y[ny], then
    bilinear interpolation of the east / north components of ws, wd (ny, nx).  Returns (east, north), each (rows, cols)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    e, n = components(np.asarray(ws, dtype=np.float64), wd)
    ix0, ix1, tx = _axis(np.arange(cols) * cell, x)
    iy0, iy1, ty = _axis(np.arange(rows) * cell, y)
    tx, ty = tx[None, :], ty[:, None]

    def bilinear(v):
        v00, v01 = v[np.ix_(iy0, ix0)], v[np.ix_(iy0, ix1)]
        v10, v11 = v[np.ix_(iy1, ix0)], v[np.ix_(iy1, ix1)]
        return (1. - ty) * ((1. - tx) * v00 + tx * v01) + ty * ((1. - tx) * v10 + tx * v11)
    return bilinear(e), bilinear(n)


def ct_exact(points, values, grads):
    """scipy's CloughTocher2DInterpolator on Delaunay(points) with the EXACT vertex gradients grads (npts, 2) written
    over scipy's estimate: the Clough-Tocher patch itself, free of the estimator's 1e-7 noise."""
    from scipy.interpolate import CloughTocher2DInterpolator
    from scipy.spatial import Delaunay
    ct = CloughTocher2DInterpolator(Delaunay(np.asarray(points, dtype=np.float64)), np.asarray(values, dtype=np.float64),
                                    tol=1e-6, maxiter=400)
    ct.grad[...] = np.asarray(grads, dtype=np.float64).reshape(ct.grad.shape)
    return ct


def griddata(points, values, rows, cols, cell, method):
    """scipy.interpolate.griddata on the cell centres, as the reference calls it (simulator.py:774-775)."""
    from scipy.interpolate import griddata as scipy_griddata
    return scipy_griddata(np.asarray(points, dtype=np.float64), values, mesh(rows, cols, cell), method=method)


# --------------------------------------------------------------------------------------------------- the fields
AFFINE = (2., 0.5, -0.25)


def affine(x, y):
    a, b, c = AFFINE
    return a + b * x + c * y


def affine_grad(x, y):
    return np.stack([np.full_like(x, AFFINE[1]), np.full_like(y, AFFINE[2])], -1)


def quadratic(x, y):
    return 1. + 0.3 * x * x - 0.2 * x * y + 0.1 * y * y


def quadratic_grad(x, y):
    return np.stack([0.6 * x - 0.2 * y, -0.2 * x + 0.2 * y], -1)


def sample_values(points, k=0):
    """A smooth, non-polynomial scalar on the points (field k of a batch)."""
    x, y = points[:, 0], points[:, 1]
    return 3. + 0.37 * x - 0.21 * y + 0.05 * x * y + np.sin(1.3 * np.arange(x.size) + k) + 0.5 * k


def sample_wind(points, k=0):
    """Speed (2..14) and direction samples on the points (snapshot k of a batch)."""
    i = np.arange(points.shape[0])
    ws = 8. + 6. * np.sin(0.9 * i + 0.7 * k + 0.3 * points[:, 0])
    wd = np.mod(250. + 70. * np.cos(1.7 * i + k) + 5. * points[:, 1], 360.)
    return ws, wd


# ------------------------------------------------------------------------------------------------ the geometries
def _grid(xs, ys):
    gx, gy = np.meshgrid(np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64))
    return np.stack([gx.ravel(), gy.ravel()], 1)


def _beyond_corners(rows, cols):
    """Four points one cell beyond the corners of a raster with cell 1."""
    return np.array([(-1., -1.), (cols, -1.), (cols, rows), (-1., rows)], dtype=np.float64)


# name -> (points (npts, 2), rows, cols, cell)
CASES = {
    'one_triangle': (np.array([(1., 1.), (10., 2.), (4., 7.)]), 9, 13, 1.0),
    # row 2 lies on a hull edge; the hull is strictly inside the raster
    'hull_inside': (np.array([(3., 2.), (9., 2.), (10., 6.), (6., 8.), (2., 6.), (6., 4.)]), 11, 14, 1.0),
    # triangles overhang the raster on every side
    'overhang': (np.array([(-3., -2.), (20., -4.), (22., 9.), (5., 14.), (-4., 8.), (6., 3.), (12., 5.)]), 9, 13, 1.0),
    # every border cell lies on the hull
    'corners': (np.array([(0., 0.), (3., 0.), (3., 1.75), (0., 1.75)]), 8, 13, 0.25),
    # vertices and edges on cell centres
    'lattice': (_grid(np.arange(0., 11., 2.), np.arange(0., 9., 2.)), 17, 21, 0.5),
    # coordinates that are no binary fractions: the rounding on the edges
    'lattice_tenths': (_grid(0.9 * np.arange(4), 0.9 * np.arange(3)), 19, 28, 0.1),
    # every cell NaN for 'linear' and 'cubic', defined for 'nearest'
    'outside': (np.array([(-9., 0.), (-5., 0.), (-7., 3.)]), 5, 5, 1.0),
    'duplicates': (np.array([(0., 0.), (4., 0.), (4., 4.), (0., 4.), (2., 2.), (2., 2.)]), 5, 5, 1.0),
    'line_1x7': (_beyond_corners(1, 7), 1, 7, 1.0),
    'line_7x1': (_beyond_corners(7, 1), 7, 1, 1.0),
    'line_1x1': (_beyond_corners(1, 1), 1, 1, 1.0),
}
DUPLICATE_VALUES = np.array([1., 2., 3., 4., 5., 50.])
POLYNOMIAL_CASES = ('hull_inside', 'overhang', 'lattice_tenths')

# what a numpy model of the owner rule gave against scipy 1.15.3 when the geometries were chosen:
# name -> (triangles, NaN cells, cells that more than one triangle contains)
EXPECTED_COUNTS = {
    'one_triangle': (1, 88, 0),
    'hull_inside': (5, 111, 11),
    'overhang': (7, 0, 9),
    'corners': (2, 0, 2),
    'lattice': (40, 0, 181),
    'lattice_tenths': (12, 0, 112),
}


def case_values(name, k=0):
    """The scalar samples a test interpolates on geometry `name` (the issue's values on `duplicates`)."""
    pts = CASES[name][0]
    if name == 'duplicates':
        return DUPLICATE_VALUES + k
    return sample_values(pts, k)
