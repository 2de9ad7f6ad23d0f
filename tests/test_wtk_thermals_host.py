"""The physical thermal model (thermal_model = 'wtk'; the reference's ssrs/layers.py:25-60 behind scipy's griddata), the
parts that need no GPU: fixture G15 is consistent with itself and with scipy, the six new entry points exist and
validate their arguments before any device work, `Config.thermal_model` defaults to today's behaviour, and `Simulator`
refuses a 'wtk' run it cannot serve before it touches the device."""
import ctypes as C

import numpy as np
import pytest

import g15_cases as g15c


@pytest.fixture(scope='module')
def g15():
    return g15c.load()


@pytest.mark.parametrize('name', g15c.GEOMETRIES)
def test_g15_masks_nan_pattern_and_floor(g15, name):
    """Mask share <= 1e-4; NaN exactly where 'linear' / 'cubic' griddata has it and none for 'nearest'; cells the
    model floors (no positive heat flux) hold exactly 1e-5."""
    rows, cols, cell, x, y, layers = g15c.geometry(g15, name)
    assert layers.shape == (4, x.size) and x.shape == y.shape
    for method in g15c.METHODS:
        want, mask = g15[f'{name}_{method}_updraft'], g15[f'{name}_{method}_mask']
        assert want.dtype == np.float32 and want.shape == (rows, cols) == mask.shape and mask.dtype == np.bool_
        assert mask.mean() <= g15c.MASK_SHARE
        p, t, zi, q = g15c.griddata_layers(x, y, layers, rows, cols, cell, method)
        assert np.array_equal(np.isnan(want), np.isnan(p))
        if method == 'nearest':
            assert not np.isnan(want).any()
        else:
            assert np.isnan(want).any()                      # the samples' hull does not cover the raster
        assert np.nanmin(p) > 0.
        with np.errstate(invalid='ignore'):
            floor = (q <= 0.) & ~mask
            assert np.array_equal(mask, ((q > 0.) & (q < 1e-3)) | (np.abs(zi) < 1e-3) | (np.abs(p) < 1.))
        assert floor.sum() > 0
        assert np.all(want[floor] == np.float32(1e-5))
        ok = ~np.isnan(want)
        assert np.all(want[ok] >= np.float32(1e-5)) and float(want[ok].max()) > 0.5


def test_g15_sweep_covers_the_special_cases(g15):
    p, t, zi, q, z = (g15[f'sweep_{k}'] for k in ('pressure', 'temperature', 'blheight', 'flux', 'z'))
    theta, wstar, up, up100 = (g15[f'sweep_{k}'] for k in ('theta', 'wstar', 'updraft', 'updraft_z100'))
    assert all(a.shape == (4096,) and a.dtype == np.float64 for a in (p, t, zi, q, z, theta, wstar, up, up100))
    with np.errstate(invalid='ignore', divide='ignore'):
        for cond in (q <= 0., zi < 100., zi <= 0., z == 0., z > zi, p == 0., p < 0.,
                     np.isnan(p), np.isnan(t), np.isnan(zi), np.isnan(q), np.isnan(z)):
            assert cond.sum() >= 1
        # numpy's maximum / clip propagate NaN: a NaN in any argument is a NaN out
        for arg in (p, t, zi, q, z):
            assert np.all(np.isnan(up[np.isnan(arg)]))
        assert np.all(np.isnan(wstar[(p < 0.) & ~np.isnan(t)]))                 # a negative base of pow(., 0.2857)
        assert np.all(theta[(p == 0.) & ~np.isnan(t)] == np.inf)
        assert np.all(wstar[(p == 0.) & ~np.isnan(t + zi + q)] == 1e-5)         # theta = inf: the floor
        plain = ~np.isnan(p + t + zi + q + z) & (p > 0.) & (t > -273.15) & np.isfinite(p + t + zi + q + z)
        assert np.all(up[plain & (zi < 0.) & (z > 0.)] == 1e-5)                 # zi < 0: x = 0, the floor
        assert np.all(wstar[plain & (q <= 0.)] == 1e-5)
        assert np.all(np.isnan(up[plain & (zi == 0.) & (z == 0.)]))                 # 0 / 0
        plain &= ~((zi == 0.) & (z == 0.))
        assert np.all(up[plain] >= 1e-5) and np.all(up100[plain] >= 1e-5)
    assert not np.array_equal(z, np.full_like(z, 100.))                         # a per-element height


def test_new_entry_points_validate_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    INV = _native.SSRS_ERR_INVALID
    for name in ('ssrs_potential_temperature', 'ssrs_deardorff_velocity', 'ssrs_thermal_updraft',
                 'ssrs_scalar_interp_workspace_bytes', 'ssrs_scalar_from_samples', 'ssrs_wtk_thermal_fields'):
        assert hasattr(lib, name) and name in _native.EXPORTS
    assert lib.ssrs_version() == 109
    buf = (C.c_char * (1 << 16))()
    p = C.cast(buf, C.c_void_p)
    d = lambda v: C.c_double(v)
    n = C.c_size_t

    def pot(pressure=p, temperature=p, out=p, count=n(8)):
        return lib.ssrs_potential_temperature(pressure, temperature, out, count, None)
    for bad in (dict(pressure=None), dict(temperature=None), dict(out=None), dict(count=n(0))):
        assert pot(**bad) == INV, bad
        assert b'ssrs_potential_temperature' in lib.ssrs_last_error()

    def dear(theta=p, zi=p, q=p, out=p, count=n(8)):
        return lib.ssrs_deardorff_velocity(theta, zi, q, d(1e-5), out, count, None)
    for bad in (dict(theta=None), dict(zi=None), dict(q=None), dict(out=None), dict(count=n(0))):
        assert dear(**bad) == INV, bad
        assert b'ssrs_deardorff_velocity' in lib.ssrs_last_error()

    def therm(w=p, zi=p, out=p, count=n(8)):
        return lib.ssrs_thermal_updraft(None, d(100.), w, zi, d(1e-5), out, count, None)      # (zmat may be NULL)
    for bad in (dict(w=None), dict(zi=None), dict(out=None), dict(count=n(0))):
        assert therm(**bad) == INV, bad
        assert b'ssrs_thermal_updraft' in lib.ssrs_last_error()

    NEAREST, LINEAR, CUBIC = (_native.SSRS_INTERP[m] for m in ('nearest', 'linear', 'cubic'))
    size = lib.ssrs_scalar_interp_workspace_bytes
    assert 0 < size(NEAREST, 0, 8, 8, 4) <= 4096
    assert size(LINEAR, 12, 8, 8, 4) >= 8 * 8 * 4
    assert size(CUBIC, 12, 8, 8, 4) >= 8 * 8 * 4 + 12 * 4 * 19 * 8
    for args in ((3, 12, 8, 8, 4), (-1, 12, 8, 8, 4), (LINEAR, 0, 8, 8, 4), (CUBIC, 12, 0, 8, 4), (CUBIC, 12, 8, 0, 4),
                 (NEAREST, 0, 8, 8, 0)):
        assert size(*args) == 0, args
    good = dict(method=CUBIC, points=p, tri=p, nbr=p, tr=p, index=p, values=p, grad=p, npts=10, ntri=12, cell=d(0.1), out=p,
                rows=8, cols=8, count=4, work=p)

    def scalar(**kw):
        a = dict(good, **kw)
        nb = a.get('nb', n(size(a['method'], a['ntri'], 8, 8, 4) if a['method'] in (NEAREST, LINEAR, CUBIC) else 4096))
        return lib.ssrs_scalar_from_samples(a['method'], a['points'], a['tri'], a['nbr'], a['tr'], a['index'], a['values'],
                                            a['grad'], a['npts'], a['ntri'], a['cell'], a['out'], a['rows'], a['cols'],
                                            a['count'], a['work'], nb, None)

    def fused(**kw):
        a = dict(good, **kw)
        nb = a.get('nb', n(size(a['method'], a['ntri'], 8, 8, 16) if a['method'] in (NEAREST, LINEAR, CUBIC) else 4096))
        return lib.ssrs_wtk_thermal_fields(a['method'], a['points'], a['tri'], a['nbr'], a['tr'], a['index'], a['values'],
                                           a['grad'], a['npts'], a['ntri'], a['cell'], None, d(100.), d(1e-5), a['out'], 1,
                                           a['rows'], a['cols'], a['count'], a['work'], nb, None)
    cases = [dict(method=3), dict(method=-1), dict(values=None), dict(out=None), dict(work=None), dict(count=0),
             dict(rows=0), dict(cols=-2), dict(cell=d(0.)), dict(cell=d(-1.)), dict(nb=n(0)), dict(nb=n(255)),
             dict(points=None), dict(tri=None), dict(tr=None), dict(nbr=None), dict(grad=None), dict(npts=2), dict(ntri=0),
             dict(method=LINEAR, points=None), dict(method=LINEAR, tri=None), dict(method=LINEAR, tr=None),
             dict(method=LINEAR, npts=2), dict(method=LINEAR, ntri=0), dict(method=LINEAR, nb=n(255)),
             dict(method=NEAREST, index=None), dict(method=NEAREST, npts=0), dict(method=NEAREST, nb=n(8))]
    for call, name in ((scalar, b'ssrs_scalar_from_samples'), (fused, b'ssrs_wtk_thermal_fields')):
        for bad in cases:
            assert call(**bad) == INV, (name, bad)
            assert name in lib.ssrs_last_error(), (name, bad)


def test_config_default_is_todays_behaviour():
    from dataclasses import fields
    from ssrs_amd import Config
    cfg = Config()
    assert cfg.thermal_model == 'random'
    assert [f.name for f in fields(Config)][-1] == 'thermal_model'               # appended after hist_safe_tracks
    assert [f.name for f in fields(Config)][-2] == 'hist_safe_tracks'
    assert 'thermal_model = random' in str(cfg).split(':::: MI355X build')[1]


def _wtk_config(tmp_path, **kw):
    from ssrs_amd import Config
    args = dict(run_name='wtk', out_dir=str(tmp_path), region_width_km=(1., 1.), resolution=100., sim_mode='snapshot',
                snapshot_datetime=(2010, 6, 17, 13), track_count=1, sim_seed=1, thermal_model='wtk',
                thermals_realization_count=1)
    args.update(kw)
    return Config(**args)


def _entry(**kw):
    x, y = np.array([0., 1., 0., 1., .5]), np.array([0., 0., 1., 1., .4])
    item = dict(datetime=(2010, 6, 17, 13), x_km=x, y_km=y, wspeed=np.full(5, 5.), wdirn=np.full(5, 270.),
                pressure=np.full(5, 9e4), temperature=np.full(5, 15.), blheight=np.full(5, 800.),
                surfheatflux=np.full(5, 200.))
    item.update(kw)
    return {k: v for k, v in item.items() if v is not ...}


def test_wtk_thermal_model_value_errors_need_no_gpu(tmp_path):
    """Raised in the constructor before any device work: this test runs on a box without a GPU, where the first device
    call would be a RuntimeError instead."""
    from ssrs_amd import Simulator
    dem = np.zeros((10, 10))
    with pytest.raises(ValueError, match='thermal_model'):
        Simulator(_wtk_config(tmp_path, thermal_model='blobs'), terrain=dem, wind=[_entry()])
    with pytest.raises(ValueError, match='snapshot.*seasonal'):
        Simulator(_wtk_config(tmp_path, sim_mode='uniform'), terrain=dem)
    for count in (0, 2):
        with pytest.raises(ValueError, match='thermals_realization_count'):
            Simulator(_wtk_config(tmp_path, thermals_realization_count=count), terrain=dem, wind=[_entry()])
    for name in ('pressure', 'temperature', 'blheight', 'surfheatflux'):
        with pytest.raises(ValueError, match=name):
            Simulator(_wtk_config(tmp_path), terrain=dem, wind=[_entry(**{name: ...})])
        with pytest.raises(ValueError, match=name):                              # neither samples, lattice nor raster
            Simulator(_wtk_config(tmp_path), terrain=dem, wind=[_entry(**{name: np.full(4, 1.)})])
        with pytest.raises(ValueError, match=name):
            Simulator(_wtk_config(tmp_path), terrain=dem, wind=[_entry(**{name: np.full((3, 3), 1.)})])
        with pytest.raises(ValueError, match=name):
            Simulator(_wtk_config(tmp_path), terrain=dem, wind=[_entry(**{name: np.full((2, 5, 1), 1.)})])
    with pytest.raises(ValueError, match='temperature'):                         # a raster beside samples: one form only
        Simulator(_wtk_config(tmp_path), terrain=dem, wind=[_entry(temperature=np.full((10, 10), 15.))])
    with pytest.raises(ValueError, match='pressure'):                            # samples without their coordinates
        Simulator(_wtk_config(tmp_path), terrain=dem,
                  wind=[_entry(x_km=..., y_km=..., wspeed=np.full((10, 10), 5.), wdirn=np.full((10, 10), 270.))])
    with pytest.raises(ValueError, match='pressure'):                            # the second entry of a seasonal run
        Simulator(_wtk_config(tmp_path, sim_mode='seasonal'), terrain=dem,
                  wind=[_entry(), _entry(datetime=(2010, 6, 18, 13), pressure=...)])


def test_wtk_layer_forms_are_resolved_on_the_host():
    """Rasters, scattered samples and a lattice (-> its meshgrid points) are all accepted; checked through the
    classifier itself, which needs no device."""
    from ssrs_amd import Simulator
    from ssrs_amd.inputs import classify
    entry = _entry()
    layers = lambda item: [(k, item[k]) for k in Simulator.THERMAL_LAYERS]
    got = classify(layers(entry), entry['x_km'], entry['y_km'], (10, 10), 'c')
    assert got.form == 'scattered' and got.values.shape == (4, 5) and got.x_km.shape == (5,) and got.as_points() is got
    xk, yk = np.array([0., .5, 1.]), np.array([0., 1.])
    lat = {k: np.arange(6.).reshape(2, 3) + i for i, k in enumerate(Simulator.THERMAL_LAYERS)}
    got = classify(layers(lat), xk, yk, (10, 10), 'c')
    assert got.form == 'lattice' and got.values.shape == (4, 2, 3)
    pts = got.as_points()
    assert pts.form == 'scattered' and pts.values.shape == (4, 6)
    gx, gy = np.meshgrid(xk, yk)
    assert np.array_equal(pts.x_km, gx.ravel()) and np.array_equal(pts.y_km, gy.ravel())
    assert np.array_equal(pts.values[2], lat['blheight'].ravel())
    ras = {k: np.full((10, 10), 1. + i) for i, k in enumerate(Simulator.THERMAL_LAYERS)}
    got = classify(layers(ras), None, None, (10, 10), 'c')
    assert got.form == 'raster' and got.x_km is None and np.shape(got.values) == (4, 10, 10)
