"""K9 on the host: the Config fields of the improved orographic model, the ValueErrors and SSRS_ERR_INVALID returns
that need no GPU, and analytic checks of the numpy reference (tests/shelter_ref.py) that the GPU tests judge the
kernels by."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import shelter_ref as ref
from oracle import ssrs_oracle as orc

DEFAULTS = (4e-5, 2.8e-3, 0.8, 0.35, 0.095, -0.09, 1.0)


# ------------------------------------------------------------------------------------------------ Config
def test_config_defaults_and_placement():
    from ssrs_amd.config import Config, _SECTIONS
    cfg = Config()
    assert cfg.orographic_model == 'original'
    assert cfg.orographic_sx_dmax == 500. and cfg.orographic_height == 80.
    assert tuple(cfg.orographic_coeffs) == DEFAULTS
    names = [f.name for f in dataclasses.fields(cfg)]
    new = ['orographic_model', 'orographic_sx_dmax', 'orographic_height', 'orographic_coeffs']
    at = names.index('turbine_encounter_radius')
    assert names[at + 1:at + 5] == new
    assert names[-2:] == ['hist_safe_tracks', 'thermal_model']
    sections = dict(_SECTIONS)
    assert list(sections['Updraft computation'][-4:]) == new
    assert sections['MI355X build'][-1] == 'turbine_encounter_radius'
    text = str(dataclasses.replace(cfg, orographic_model='improved', orographic_height=120.))
    block = text.split(':::: Updraft computation')[1].split('::::')[0]
    assert 'orographic_model = improved' in block and 'orographic_height = 120.0' in block
    assert 'orographic_sx_dmax = 500.0' in block and 'orographic_coeffs = (4e-05' in block


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda unavailable, and any attempt to reach the device fails the test."""
    import torch
    from ssrs_amd import _device
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_device, 'device', boom)
    monkeypatch.setattr(_device, 'to_dev', boom)


@pytest.mark.parametrize('bad, match', [
    (dict(orographic_model='bogus'), 'orographic_model'),
    (dict(orographic_sx_dmax=50.), 'orographic_sx_dmax'),                  # < resolution (100 m): K < 1
    (dict(orographic_height=-1.), 'orographic_height'),
    (dict(orographic_coeffs=(4e-5, 2.8e-3, 0.8, 0.35, 0.095, -2., 1.0)), 'F_h'),     # f = -2: F_h < 0 on flat ground
    (dict(orographic_coeffs=(0., 0., 1., 0.35, 0.095, -1.05, 1.0)), 'F_h'),          # > 0 at one end only
    (dict(orographic_coeffs=(1., 2., 3.)), 'orographic_coeffs'),
    (dict(orographic_coeffs=(0., 0., 1., -1., 0., 0., 0.)), 'd ='),
])
def test_simulator_refuses_bad_fields_before_device_work(tmp_path, no_gpu, bad, match):
    from ssrs_amd import Config, Simulator
    fields = dict(run_name='bad', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100.,
                  orographic_model='improved')
    fields.update(bad)
    with pytest.raises(ValueError, match=match):
        Simulator(Config(**fields), terrain=np.zeros((50, 60)))
    assert not (tmp_path / 'bad').exists()


def test_original_model_ignores_the_improved_fields(tmp_path, no_gpu):
    """'original' changes nothing: a dmax below the resolution is not looked at (the constructor gets as far as the
    device, which the fixture turns into an AssertionError)."""
    from ssrs_amd import Config, Simulator
    cfg = Config(run_name='orig', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100., orographic_sx_dmax=50.)
    with pytest.raises((AssertionError, RuntimeError)):
        Simulator(cfg, terrain=np.zeros((50, 60)))


# ------------------------------------------------------------------------------------------------ C ABI
def _sx(lib, dem, res=10., ur=None, uc=None, wdirn=None, dmax=50., axes=1, path=0, tan=None, rows=8, cols=8, batch=1,
        dem_type=1):
    return lib.ssrs_shelter_sx(dem, dem_type, C.c_double(res), ur, uc, wdirn, C.c_double(dmax), axes, path, tan, None,
                               rows, cols, batch, None)


def test_shelter_sx_validates_without_a_gpu():
    from ssrs_amd import _native as nat
    lib = nat.lib()
    buf = (C.c_double * 64)()
    one = (C.c_double * 1)(1.)
    dem, out, u = C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(one, C.c_void_p)
    cases = [
        (dict(dem=None, ur=u, uc=u), b'dem is NULL'),
        (dict(dem=dem, ur=u, uc=u, rows=1), b'rows, cols'),
        (dict(dem=dem, ur=u, uc=u, batch=0), b'batch'),
        (dict(dem=dem, ur=u, uc=u, dem_type=7), b'element type'),
        (dict(dem=dem, ur=u, uc=u, res=0.), b'res'),
        (dict(dem=dem, ur=u, uc=u, dmax=9.99), b'K = floor(dmax / res) < 1'),
        (dict(dem=dem, ur=u, uc=u, axes=2), b'ray_axes'),
        (dict(dem=dem, ur=u, uc=u, path=3), b'path'),
        (dict(dem=dem, ur=u, uc=None), b'ray_ur'),
        (dict(dem=dem), b'wind direction'),
        (dict(dem=dem, ur=u, uc=u, wdirn=dem), b'wind direction'),
    ]
    for kwargs, text in cases:
        rc = _sx(lib, tan=out, **kwargs)
        assert rc == nat.SSRS_ERR_INVALID, kwargs
        assert text in lib.ssrs_last_error(), (kwargs, lib.ssrs_last_error())
    with pytest.raises(ValueError):
        nat.check(rc)
    # nothing asked for: fine, and still no GPU needed
    assert _sx(lib, dem=dem, ur=u, uc=u) == nat.SSRS_OK


def test_updraft_sheltered_validates_without_a_gpu():
    from ssrs_amd import _native as nat
    lib = nat.lib()
    buf = (C.c_double * 64)()
    one = (C.c_double * 1)(1.)
    dem, u = C.cast(buf, C.c_void_p), C.cast(one, C.c_void_p)

    def call(dem=dem, ur=u, uc=u, ws0=u, wd0=u, ws=None, wd=None, slope=None, aspect=None, sa_type=1, dmax=50., axes=1,
             height=80., coef=DEFAULTS, params=True, thr=-1., usable=None, rows=8, cols=8, batch=1, res=10.):
        p = nat.SsrsShelterParams(dmax, axes, 0, height, (C.c_double * 7)(*coef))
        return lib.ssrs_updraft_sheltered(dem, 1, C.c_double(res), ur, uc, ws0, wd0, ws, wd, slope, aspect, sa_type,
                                          C.byref(p) if params else None, C.c_double(0.), C.c_double(thr), dem, usable,
                                          None, rows, cols, batch, None)
    cases = [
        (dict(dem=None), b'dem is NULL'),
        (dict(params=False), b'params is NULL'),
        (dict(rows=2), b'rows, cols'),
        (dict(dmax=5.), b'K = floor(dmax / res) < 1'),
        (dict(axes=5), b'ray_axes'),
        (dict(ws0=None), b'uniform wind takes'),
        (dict(ws=dem), b'uniform wind takes'),
        (dict(ur=None, uc=None, ws0=None, wd0=None, wd=dem), b'per-cell wind takes'),
        (dict(slope=dem), b'both slope and aspect'),
        (dict(slope=dem, aspect=dem, sa_type=9), b'slope / aspect element type'),
        (dict(usable=dem), b'positive threshold'),
        (dict(height=-1.), b'height'),
        (dict(coef=(0., 0., 1., 0., 0., 0., 0.)), b'd must be > 0'),
        (dict(coef=(4e-5, 2.8e-3, 0.8, 0.35, 0.095, -2., 1.0)), b'F_h <= 0'),
        (dict(coef=(0., 0., 1., 0.35, 0.095, -1.05, 1.0)), b'F_h <= 0'),
        (dict(coef=(0., 0., 1., 1., 0., float('nan'), 0.)), b'not finite'),
    ]
    for kwargs, text in cases:
        rc = call(**kwargs)
        assert rc == nat.SSRS_ERR_INVALID, kwargs
        assert text in lib.ssrs_last_error(), (kwargs, lib.ssrs_last_error())


def test_layers_parameter_check_matches_the_library():
    from ssrs_amd import layers
    assert layers.check_improved_parameters(500., 100., 80., DEFAULTS) == DEFAULTS
    assert tuple(layers.IMPROVED_COEFFS) == DEFAULTS == ref.DEFAULT_COEFFS
    for args in ((50., 100., 80., DEFAULTS), (500., 100., -1., DEFAULTS), (500., 100., 80., DEFAULTS[:6]),
                 (500., 100., 80., (0., 0., 1., 0.35, 0.095, -1.05, 1.0))):
        with pytest.raises(ValueError):
            layers.check_improved_parameters(*args)
    ur, uc = layers.ray_step(237.3, 'row_north')
    assert (ur[0], uc[0]) == tuple(float(x) for x in ref.ray_step(237.3, 'row_north'))
    ur, uc = layers.ray_step([0., 90.], 'row_east')
    assert np.array_equal(ur, ref.ray_step(np.array([0., 90.]), 'row_east')[0])
    with pytest.raises(ValueError):
        layers.ray_step(0., 'row_south')


# ------------------------------------------------------------------------------------------------ the reference
def scalar_tan_sx(z, res, ur, uc, K):
    """The model's text once more, one cell and one sample at a time in python floats."""
    rows, cols = z.shape
    out = np.zeros(z.shape)
    for r0 in range(rows):
        for c0 in range(cols):
            best = None
            for k in range(1, K + 1):
                cell, frac = [], []
                for u in (ur, uc):
                    o = float(k) * u
                    io = math.floor(o)
                    fo = o - io
                    if fo < 1e-9:
                        fo = 0.
                    elif fo > 1. - 1e-9:
                        io, fo = io + 1, 0.
                    cell.append(io)
                    frac.append(fo)
                i, j = r0 + cell[0], c0 + cell[1]
                fr, fc = frac
                if not (0 <= i and (i + 1 <= rows - 1 or (fr == 0. and i <= rows - 1))):
                    continue
                if not (0 <= j and (j + 1 <= cols - 1 or (fc == 0. and j <= cols - 1))):
                    continue
                z00 = float(z[i, j])
                z01 = float(z[i, j + 1]) if fc != 0. else 0.
                z10 = float(z[i + 1, j]) if fr != 0. else 0.
                z11 = float(z[i + 1, j + 1]) if fr != 0. and fc != 0. else 0.
                zs = (z00 * (1. - fc) + z01 * fc) * (1. - fr) + (z10 * (1. - fc) + z11 * fc) * fr
                tk = (zs - float(z[r0, c0])) * (1.0 / (float(k) * res))
                if tk != tk:
                    continue
                if best is None or tk > best:
                    best = tk
            out[r0, c0] = 0. if best is None or np.isnan(z[r0, c0]) else best
    return out


@pytest.mark.parametrize('axes', ['row_north', 'row_east'])
@pytest.mark.parametrize('wdirn', [90., 270., 237.3, 45., 0., 133.7])
def test_reference_on_a_plane_rising_eastwards(axes, wdirn):
    """z = s * (distance east): the tangent towards azimuth A is s sin A at every distance (bilinear interpolation is
    exact on a plane), so T = s sin A wherever a sample is valid: +s for an east wind, -s for a west wind."""
    s, res, rows, cols = 0.3, 10., 23, 29
    east = np.arange(cols)[None, :] if axes == 'row_north' else np.arange(rows)[:, None]
    z = np.broadcast_to(s * res * east, (rows, cols)).astype(np.float64)
    T, count = ref.tan_sx(z, res, wdirn, dmax=55., ray_axes=axes, return_count=True)       # K = 5
    assert count.max() == 5 and (count > 0).sum() > rows * cols // 2
    expect = s * math.sin(math.radians(wdirn))
    np.testing.assert_allclose(T[count > 0], expect, rtol=1e-12, atol=1e-13)
    assert (T[count == 0] == 0.).all()
    if wdirn == 90.:
        np.testing.assert_allclose(T[count > 0], s, rtol=1e-13)
    if wdirn == 270.:
        np.testing.assert_allclose(T[count > 0], -s, rtol=1e-13)


def test_reference_on_a_ridge_in_the_fallback_frame():
    """A symmetric triangular ridge whose crest runs along the columns, slope / aspect from the oracle's Horn functions
    (the transposed fallback: a ramp rising with the row index is windward for a wind from 270), ray in 'row_east':
    every cell that carries an updraft looks upwind at lower ground (T <= 0), the lee cells within dmax of the crest look
    up at it (T > 0)."""
    rows, cols, res, crest, K = 41, 17, 100., 20, 5
    z = np.broadcast_to((2000. - 40. * np.abs(np.arange(rows) - crest))[:, None], (rows, cols)).astype(np.float64)
    slope, aspect = orc.compute_slope_degrees(z, res), orc.compute_aspect_degrees(z, res)
    w0 = orc.compute_orographic_updraft(10., 270., slope, aspect)
    assert (w0[1:crest, 1:-1] > 1.).all() and (w0[crest + 1:] < 1e-9).all()         # windward = rising with the row index
    T = ref.tan_sx(z, res, 270., dmax=K * res, ray_axes='row_east')
    assert (T[w0 > 0.] <= 0.).all() and (T[1:crest + 1] < 0.).all()
    assert (T[crest + 1:crest + 1 + K] > 0.).all()
    np.testing.assert_allclose(T[crest + 1:], 0.4, rtol=1e-12)
    # in the geographic frame the same ray would run along the crest and see nothing
    assert (ref.tan_sx(z, res, 270., dmax=K * res, ray_axes='row_north') == 0.).all()
    # the adjustment: sheltered lee stays 0, the windward face is reduced by its negative Sx (g = +1) and by F_h
    w = ref.adjust(w0, T, slope)
    f_h = ref.height_factor(slope, 80., ref.DEFAULT_COEFFS)
    assert (f_h > 0.).all()
    np.testing.assert_allclose(w[2:crest - 1, 1:-1], w0[2:crest - 1, 1:-1] * 0.6 / f_h[2:crest - 1, 1:-1], rtol=1e-12)
    assert np.array_equal(ref.adjust(w0, T, slope, coeffs=ref.NEUTRAL_COEFFS), w0)


@pytest.mark.parametrize('axes', ['row_north', 'row_east'])
@pytest.mark.parametrize('wdirn', [0., 90., 180., 270.])
def test_axis_winds_lose_no_sample(axes, wdirn):
    """cos(270 deg) = -1.8e-16: without the snap the sample cell would be one row off and every weight on its
    neighbour.  With it an axis wind steps along the lattice: min(K, cells to the edge) valid samples, and T is the
    plain maximum over the cells it passes."""
    rng = np.random.default_rng(5)
    rows, cols, res, K = 9, 11, 10., 4
    z = rng.uniform(0., 100., (rows, cols))
    ur, uc = (float(x) for x in ref.ray_step(wdirn, axes))
    dr, dc = int(round(ur)), int(round(uc))
    assert abs(dr) + abs(dc) == 1 and (ur != dr or uc != dc or wdirn == 0.)
    T, count = ref.tan_sx(z, res, wdirn, dmax=K * res, ray_axes=axes, return_count=True)
    for r in range(rows):
        for c in range(cols):
            room = (rows - 1 - r if dr > 0 else r if dr < 0 else cols - 1 - c if dc > 0 else c)
            assert count[r, c] == min(K, room), (r, c)
            vals = [(z[r + k * dr, c + k * dc] - z[r, c]) * (1.0 / (float(k) * res)) for k in range(1, min(K, room) + 1)]
            assert T[r, c] == (max(vals) if vals else 0.), (r, c)


@pytest.mark.parametrize('wdirn', [0., 45., 237.3, 270., 359.9])
def test_reference_equals_the_scalar_statement_with_a_nan_cell(wdirn):
    """Against the text restated cell by cell, on a DEM with a nodata cell: equal bits.  And the NaN removes only the
    samples that touch it with non-zero weight: every cell whose value changes against the filled DEM has the NaN cell
    on its ray, the others keep their bits."""
    rng = np.random.default_rng(11)
    rows, cols, res, K = 12, 13, 10., 4
    filled = rng.uniform(0., 50., (rows, cols))
    z = filled.copy()
    z[6, 7] = np.nan
    for axes in ('row_north', 'row_east'):
        ur, uc = (float(x) for x in ref.ray_step(wdirn, axes))
        T = ref.tan_sx(z, res, wdirn, dmax=K * res + 3., ray_axes=axes)
        assert not np.isnan(T).any() and T[6, 7] == 0.
        assert np.array_equal(T, scalar_tan_sx(z, res, ur, uc, K))
        T_filled = ref.tan_sx(filled, res, wdirn, dmax=K * res + 3., ray_axes=axes)
        assert np.array_equal(T_filled, scalar_tan_sx(filled, res, ur, uc, K))
        changed = np.argwhere(T != T_filled)
        assert len(changed) >= 1
        for r, c in changed:
            # the NaN cell lies within the 2 x 2 footprint of one of this cell's samples
            near = [(abs(r + k * ur - 6) < 1. + 1e-9) and (abs(c + k * uc - 7) < 1. + 1e-9) for k in range(0, K + 1)]
            assert any(near), (r, c)
        # an axis wind touches one cell per sample: only the cells exactly downwind of the NaN can change
        if wdirn in (0., 270.):
            dr, dc = int(round(ur)), int(round(uc))
            allowed = {(6 - k * dr, 7 - k * dc) for k in range(0, K + 1)}
            assert {tuple(x) for x in changed} <= allowed
