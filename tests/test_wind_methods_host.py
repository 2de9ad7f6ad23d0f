"""`wtk_interp_type` 'nearest' and 'cubic' (the reference hands the field to scipy griddata, ssrs/simulator.py:774-775),
the parts that need no GPU: the five entry points exist and validate their arguments before any device work, unknown
methods are a ValueError at both public levels, and the Clough-Tocher patch the cubic kernels evaluate -- restated
here in numpy from the vertex gradients scipy estimates -- is griddata(method='cubic') to rounding."""
import ctypes as C

import numpy as np
import pytest

CLOUDS = [(180, 230, 0.1, 60, 1), (400, 300, 0.01, 400, 2), (97, 1031, 0.05, 12, 3)]


def geometries():
    """(name, rows, cols, cell, x, y, wspeed (B, npts), wdirn (B, npts)): three random clouds, a jittered 2 km lattice
    with three snapshots, and the same lattice without the jitter."""
    out = []
    for rows, cols, cell, npts, seed in CLOUDS:
        rng = np.random.default_rng(seed)
        w, h = (cols - 1) * cell, (rows - 1) * cell
        x = rng.uniform(-0.1 * w, 1.1 * w, npts)
        y = rng.uniform(-0.1 * h, 1.1 * h, npts)
        ws = rng.uniform(0., 15., npts)
        wd = rng.uniform(0., 360., npts)
        out.append((f'cloud{seed}', rows, cols, cell, x, y, ws[None], wd[None]))
    for name, jitter in (('jittered', 1.), ('lattice', 0.)):
        rng = np.random.default_rng(9)
        gx, gy = np.meshgrid(np.arange(-2., 33., 2.), np.arange(-2., 23., 2.))
        x = (gx + jitter * rng.uniform(-0.3, 0.3, gx.shape)).ravel()
        y = (gy + jitter * rng.uniform(-0.3, 0.3, gy.shape)).ravel()
        ws = rng.uniform(2., 14., (3, x.size))
        wd = (270. + rng.normal(0., 40., (3, x.size))) % 360.
        out.append((name, 200, 300, 0.1, x, y, ws, wd))
    return out


def clough_tocher_coefficients(tri, f, grad):
    """The 19 Bezier ordinates of every macro-triangle, (ntri, 19) in the order of the evaluation below.
    tri: scipy.spatial.Delaunay; f (npts,); grad (npts, 2)."""
    pts, simp = tri.points, tri.simplices
    p0, p1, p2 = pts[simp[:, 0]], pts[simp[:, 1]], pts[simp[:, 2]]
    f1, f2, f3 = f[simp[:, 0]], f[simp[:, 1]], f[simp[:, 2]]
    g0, g1, g2 = grad[simp[:, 0]], grad[simp[:, 1]], grad[simp[:, 2]]
    e12, e23, e31 = p1 - p0, p2 - p1, p0 - p2
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
    df12, df21, df23 = dot(g0, e12), -dot(g1, e12), dot(g1, e23)
    df32, df31, df13 = -dot(g2, e23), dot(g2, e31), -dot(g0, e31)
    c3000, c2100, c2010 = f1, (df12 + 3 * f1) / 3, (df13 + 3 * f1) / 3
    c0300, c1200, c0210 = f2, (df21 + 3 * f2) / 3, (df23 + 3 * f2) / 3
    c0030, c1020, c0120 = f3, (df31 + 3 * f3) / 3, (df32 + 3 * f3) / 3
    c2001 = (c2100 + c2010 + c3000) / 3
    c0201 = (c1200 + c0300 + c0210) / 3
    c0021 = (c1020 + c0120 + c0030) / 3
    g = np.empty((simp.shape[0], 3))
    T = tri.transform
    for k in range(3):
        n = tri.neighbors[:, k]
        nn = np.where(n < 0, 0, n)
        yc = (pts[simp[nn, 0]] + pts[simp[nn, 1]] + pts[simp[nn, 2]]) / 3
        d = yc - T[:, 2, :]
        ca = T[:, 0, 0] * d[:, 0] + T[:, 0, 1] * d[:, 1]
        cb = T[:, 1, 0] * d[:, 0] + T[:, 1, 1] * d[:, 1]
        c = (ca, cb, 1 - ca - cb)
        a, b = c[(2, 0, 1)[k]], c[(1, 2, 0)[k]]
        with np.errstate(divide='ignore', invalid='ignore'):
            g[:, k] = np.where(n < 0, -0.5, (2 * a + b - 1) / (2 - 3 * a - 3 * b))
    c0111 = (g[:, 0] * (-c0300 + 3 * c0210 - 3 * c0120 + c0030) + (-c0300 + 2 * c0210 - c0120 + c0021 + c0201)) / 2
    c1011 = (g[:, 1] * (-c0030 + 3 * c1020 - 3 * c2010 + c3000) + (-c0030 + 2 * c1020 - c2010 + c2001 + c0021)) / 2
    c1101 = (g[:, 2] * (-c3000 + 3 * c2100 - 3 * c1200 + c0300) + (-c3000 + 2 * c2100 - c1200 + c2001 + c0201)) / 2
    c1002 = (c1101 + c1011 + c2001) / 3
    c0102 = (c1101 + c0111 + c0201) / 3
    c0012 = (c1011 + c0111 + c0021) / 3
    c0003 = (c1002 + c0102 + c0012) / 3
    return np.stack([c3000, c2100, c2010, c2001, c1200, c1101, c1020, c1011, c1002, c0300,
                     c0210, c0201, c0120, c0111, c0102, c0030, c0021, c0012, c0003], 1)


def clough_tocher_evaluate(tri, coef, xy):
    """The cubic at the points xy (n, 2); NaN outside the hull."""
    t = tri.find_simplex(xy)
    tt = np.where(t < 0, 0, t)
    T = tri.transform[tt]
    d = xy - T[:, 2, :]
    b0 = T[:, 0, 0] * d[:, 0] + T[:, 0, 1] * d[:, 1]
    b1 = T[:, 1, 0] * d[:, 0] + T[:, 1, 1] * d[:, 1]
    b2 = 1 - b0 - b1
    m = np.minimum(b0, np.minimum(b1, b2))
    a1, a2, a3, a4 = b0 - m, b1 - m, b2 - m, 3 * m
    mono = [a1**3, 3 * a1**2 * a2, 3 * a1**2 * a3, 3 * a1**2 * a4, 3 * a1 * a2**2, 6 * a1 * a2 * a4, 3 * a1 * a3**2,
            6 * a1 * a3 * a4, 3 * a1 * a4**2, a2**3, 3 * a2**2 * a3, 3 * a2**2 * a4, 3 * a2 * a3**2, 6 * a2 * a3 * a4,
            3 * a2 * a4**2, a3**3, 3 * a3**2 * a4, 3 * a3 * a4**2, a4**3]
    w = np.zeros(xy.shape[0])
    for k in range(19):
        w = w + mono[k] * coef[tt, k]
    return np.where(t < 0, np.nan, w)


def test_new_entry_points_validate_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    INV = _native.SSRS_ERR_INVALID
    for name in ('ssrs_wind_nearest_workspace_bytes', 'ssrs_wind_nearest_index', 'ssrs_wind_from_nearest',
                 'ssrs_wind_cubic_workspace_bytes', 'ssrs_wind_from_triangles_cubic'):
        assert hasattr(lib, name) and name in _native.EXPORTS
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)
    d = lambda v: C.c_double(v)
    # nearest: sizes
    nb = lib.ssrs_wind_nearest_workspace_bytes(10, 8, 8)
    assert 0 < nb <= 4096
    assert lib.ssrs_wind_nearest_workspace_bytes(0, 8, 8) == 0
    assert lib.ssrs_wind_nearest_workspace_bytes(10, 0, 8) == 0
    assert lib.ssrs_wind_nearest_workspace_bytes(10, 8, -1) == 0
    good = dict(points=p, npts=10, cell=d(0.1), index=p, rows=8, cols=8, ws=p, nb=C.c_size_t(nb))

    def nearest_index(**kw):
        a = dict(good, **kw)
        return lib.ssrs_wind_nearest_index(a['points'], a['npts'], a['cell'], a['index'], a['rows'], a['cols'],
                                           a['ws'], a['nb'], None)
    for bad in (dict(points=None), dict(index=None), dict(ws=None), dict(npts=0), dict(rows=0), dict(cols=-3),
                dict(cell=d(0.)), dict(cell=d(-1.)), dict(nb=C.c_size_t(nb - 1))):
        assert nearest_index(**bad) == INV, bad
        assert b'ssrs_wind_nearest_index' in lib.ssrs_last_error()

    def from_nearest(index=p, speed=p, dirn=p, npts=10, wspeed=p, wdirn=p, rows=8, cols=8, batch=1):
        return lib.ssrs_wind_from_nearest(index, speed, dirn, npts, wspeed, wdirn, rows, cols, batch, None)
    for bad in (dict(index=None), dict(speed=None), dict(dirn=None), dict(wspeed=None), dict(wdirn=None),
                dict(npts=0), dict(rows=0), dict(cols=0), dict(batch=0)):
        assert from_nearest(**bad) == INV, bad
        assert b'ssrs_wind_from_nearest' in lib.ssrs_last_error()
    # cubic
    cb = lib.ssrs_wind_cubic_workspace_bytes(10, 12, 8, 8, 2)
    assert cb >= 8 * 8 * 4 + 12 * 2 * 2 * 19 * 8
    for args in ((2, 12, 8, 8, 2), (10, 0, 8, 8, 2), (10, 12, 0, 8, 2), (10, 12, 8, 0, 2), (10, 12, 8, 8, 0)):
        assert lib.ssrs_wind_cubic_workspace_bytes(*args) == 0, args
    big = (C.c_char * int(cb))()
    q = C.cast(big, C.c_void_p)
    cgood = dict(points=q, tri=q, nbr=q, tr=q, east=q, north=q, ge=q, gn=q, npts=10, ntri=12, cell=d(0.1), ws=q, wd=q,
                 rows=8, cols=8, batch=2, work=q, nb=C.c_size_t(cb))

    def cubic(**kw):
        a = dict(cgood, **kw)
        return lib.ssrs_wind_from_triangles_cubic(a['points'], a['tri'], a['nbr'], a['tr'], a['east'], a['north'], a['ge'],
                                                  a['gn'], a['npts'], a['ntri'], a['cell'], a['ws'], a['wd'], a['rows'],
                                                  a['cols'], a['batch'], a['work'], a['nb'], None)
    for bad in [{k: None} for k in ('points', 'tri', 'nbr', 'tr', 'east', 'north', 'ge', 'gn', 'ws', 'wd', 'work')] + \
               [dict(npts=2), dict(ntri=0), dict(rows=0), dict(cols=0), dict(batch=0), dict(cell=d(0.)),
                dict(nb=C.c_size_t(cb - 1)), dict(nb=C.c_size_t(0))]:
        assert cubic(**bad) == INV, bad
        assert b'ssrs_wind_from_triangles_cubic' in lib.ssrs_last_error()
    assert lib.ssrs_version() == 109


def test_unknown_method_is_a_value_error(tmp_path):
    from ssrs_amd import Config, Simulator
    from ssrs_amd.wind import interpolate_wind_scattered
    x, y = np.array([0., 1., 0., 1.]), np.array([0., 0., 1., 1.])
    ws, wd = np.full(4, 5.), np.full(4, 270.)
    with pytest.raises(ValueError):
        interpolate_wind_scattered(x, y, ws, wd, (10, 10), 100., method='spline')
    cfg = Config(run_name='bad', out_dir=str(tmp_path), region_width_km=(1., 1.), resolution=100., sim_mode='snapshot',
                 snapshot_datetime=(2010, 6, 17, 13), track_count=1, sim_seed=1, wtk_interp_type='spline')
    with pytest.raises(ValueError, match='wtk_interp_type'):
        Simulator(cfg, terrain=np.zeros((10, 10)),
                  wind=[dict(datetime=(2010, 6, 17, 13), wspeed=ws, wdirn=wd, x_km=x, y_km=y)])


@pytest.mark.parametrize('geometry', geometries(), ids=lambda g: g[0])
def test_numpy_restatement_of_the_cubic_patch_vs_griddata(geometry):
    """The yardstick the kernels are held to: the patch, fed with scipy's own gradient estimate (all fields in one
    call), against griddata(method='cubic'), <= 1e-12 x max(1, max |reference|)."""
    from scipy.interpolate import CloughTocher2DInterpolator, griddata
    from scipy.spatial import Delaunay
    _, rows, cols, cell, x, y, ws, wd = geometry
    pts = np.ascontiguousarray(np.stack([x, y], 1))
    tri = Delaunay(pts)
    east, north = ws * np.sin(wd * np.pi / 180.), ws * np.cos(wd * np.pi / 180.)
    values = np.concatenate([east, north], 0).T                                   # (npts, 2 B)
    grad = CloughTocher2DInterpolator(tri, values, tol=1e-6, maxiter=400).grad      # (npts, 2 B, 2)
    xm, ym = np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)
    xy = np.stack([xm.ravel(), ym.ravel()], 1)
    for f in range(values.shape[1]):
        ref = griddata(pts, values[:, f], (xm, ym), method='cubic').ravel()
        got = clough_tocher_evaluate(tri, clough_tocher_coefficients(tri, values[:, f], grad[:, f, :]), xy)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        err = float(np.max(np.abs(got[ok] - ref[ok])))
        bound = 1e-12 * max(1., float(np.max(np.abs(ref[ok]))))
        print(f'{geometry[0]} field {f}: max |restatement - griddata| = {err:.3g} (bound {bound:.3g})')
        assert err <= bound


CASE = 'y2010m06d17h13'
_XY5 = dict(x_km=np.array([0., 1., 0., 1., .5]), y_km=np.array([0., 0., 1., 1., .4]))
_AXES = dict(x_km=np.array([0., .5, 1.]), y_km=np.array([0., 1.]))
MALFORMED = {                                       # name -> (entry, the field the message must name)
    'rasters of the wrong shape': (dict(wspeed=np.full((10, 9), 5.), wdirn=np.full((10, 9), 270.)), 'wspeed'),
    'samples shorter than their points': (dict(wspeed=np.full(4, 5.), wdirn=np.full(4, 270.), **_XY5), 'wspeed'),
    'lattice arrays of the wrong shape': (dict(wspeed=np.full((3, 2), 5.), wdirn=np.full((3, 2), 270.), **_AXES), 'wspeed'),
    'wdirn shorter than wspeed': (dict(wspeed=np.full(5, 5.), wdirn=np.full(4, 270.), **_XY5), 'wdirn'),
    'rasters beside x_km': (dict(wspeed=np.full((10, 10), 5.), wdirn=np.full((10, 10), 270.), **_XY5), 'wspeed'),
}


@pytest.mark.parametrize('method', ['linear', 'cubic'])
@pytest.mark.parametrize('fault', list(MALFORMED))
def test_malformed_wind_pair_is_a_value_error_before_device_work(tmp_path, fault, method):
    """Raised by the constructor from the resolver: this test runs without a GPU, where the first device call would be
    a RuntimeError instead.  The message names the case and the field."""
    from ssrs_amd import Config, Simulator
    entry, field = MALFORMED[fault]
    cfg = Config(run_name='bad', out_dir=str(tmp_path), region_width_km=(1., 1.), resolution=100., sim_mode='snapshot',
                 snapshot_datetime=(2010, 6, 17, 13), track_count=1, sim_seed=1, wtk_interp_type=method)
    with pytest.raises(ValueError) as err:
        Simulator(cfg, terrain=np.zeros((10, 10)), wind=[dict(datetime=(2010, 6, 17, 13), **entry)])
    assert CASE in str(err.value) and field in str(err.value)


@pytest.mark.parametrize('tensor', [False, True], ids=['numpy', 'torch'])
def test_classifier_on_the_wind_pair(tensor):
    import torch
    from ssrs_amd.inputs import classify
    give = (lambda a: torch.from_numpy(a)) if tensor else (lambda a: a)
    pair = lambda shape, dtype=np.float32: [('wspeed', give(np.full(shape, 5., dtype=dtype))),
                                            ('wdirn', give(np.full(shape, 270., dtype=dtype)))]
    fields = pair((10, 10))
    got = classify(fields, None, None, (10, 10), CASE)
    assert got.form == 'raster' and got.x_km is None and got.y_km is None
    assert got.values[0] is fields[0][1] and got.values[1] is fields[1][1]            # neither copied nor moved
    assert got.as_points() is got
    got = classify(pair((2, 3)), _AXES['x_km'], _AXES['y_km'], (10, 10), CASE)
    assert got.form == 'lattice' and isinstance(got.values, np.ndarray)
    assert got.values.dtype == np.float64 and got.values.shape == (2, 2, 3)
    assert got.x_km.shape == (3,) and got.y_km.shape == (2,)
    pts = got.as_points()
    gx, gy = np.meshgrid(_AXES['x_km'], _AXES['y_km'])
    assert pts.form == 'scattered' and pts.values.shape == (2, 6)
    assert np.array_equal(pts.x_km, gx.ravel()) and np.array_equal(pts.y_km, gy.ravel())
    got = classify(pair((5,)), _XY5['x_km'], _XY5['y_km'], (10, 10), CASE)
    assert got.form == 'scattered' and isinstance(got.values, np.ndarray)
    assert got.values.dtype == np.float64 and got.values.shape == (2, 5)
    assert got.x_km.dtype == np.float64 and got.as_points() is got
    other = classify(pair((5,)), _XY5['x_km'][::-1].copy(), _XY5['y_km'], (10, 10), CASE)
    assert got.same_points(got) and not got.same_points(other)                        # equal length, other points
    with pytest.raises(ValueError, match='wdirn.*one form'):
        classify([fields[0], pair((5,))[1]], _XY5['x_km'], _XY5['y_km'], (10, 10), CASE)


def test_resolve_wind_projects_samples_in_degrees():
    """Scattered points at lon / lat, and lattice axes with (lat, lon) arrays, both come back as scattered samples in
    kilometres from the centre of cell (0, 0); a linear stand-in for the projection, so no device and no library."""
    from ssrs_amd.inputs import resolve_wind
    west, south = 2000., -3000.
    forward = lambda lon, lat: (1000. * lon + 50. * lat, 700. * lat - 20. * lon)
    project = lambda lon, lat: ((forward(lon, lat)[0] - west) / 1000., (forward(lon, lat)[1] - south) / 1000.)
    names = dict(wspeed='windspeed_100m', wdirn='winddirection_100m')
    lon, lat = np.array([1., 2., 4.]), np.array([10., 12.])
    glon, glat = (a.ravel() for a in np.meshgrid(lon, lat))
    ws, wd = np.arange(6.).reshape(2, 3) + 3., np.arange(6.).reshape(2, 3) + 250.
    entries = [dict(datetime=(2010, 6, 17, 13), wspeed=ws.ravel(), wdirn=wd.ravel(), lon=glon, lat=glat),
               dict(datetime=(2010, 6, 18, 13), wspeed=ws, wdirn=wd, lon=lon, lat=lat)]
    cases = resolve_wind(entries, 'seasonal', 'y%Ym%md%dh%H', (10, 10), 'linear', False, names, project)
    assert [c.case_id for c in cases] == [CASE, 'y2010m06d18h13'] and all(c.thermal is None for c in cases)
    x, y = forward(glon, glat)
    for case in cases:
        assert case.wind.form == 'scattered' and case.wind.values.shape == (2, 6)
        assert np.array_equal(case.wind.x_km, (x - west) / 1000.) and np.array_equal(case.wind.y_km, (y - south) / 1000.)
        assert np.array_equal(case.wind.values, np.stack([ws.ravel(), wd.ravel()]))
    assert cases[0].wind.same_points(cases[1].wind)
    with pytest.raises(ValueError, match="both 'lon' / 'lat' and 'x_km' / 'y_km'"):
        resolve_wind([dict(entries[0], x_km=glon, y_km=glat)], 'seasonal', 'y%Ym%md%dh%H', (10, 10), 'linear', False, names,
                     project)


@pytest.mark.parametrize('dtype', [np.int64, np.float64, np.int32])
def test_collectives_without_a_process_group_return_their_input(dtype):
    from ssrs_amd import distributed
    assert not distributed.is_on() and distributed.rank() == 0 and distributed.world_size() == 1
    distributed.barrier()
    arr = np.arange(6, dtype=dtype).reshape(2, 3)
    for got in (distributed.broadcast(arr), distributed.broadcast(arr, src=0), distributed.all_reduce_sum(arr)):
        assert got.dtype == dtype and np.array_equal(got, arr)
