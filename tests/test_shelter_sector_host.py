"""The sector-averaged Sx (K9) on the host: the Config fields, the ValueErrors and SSRS_ERR_INVALID returns that need no
GPU, the ray counts, and an analytic pin of the numpy reference (tests/shelter_sector_ref.py) that the emulation and GPU
tests judge the kernel by."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import shelter_ref as ref
import shelter_sector_ref as sref

DEFAULTS = (4e-5, 2.8e-3, 0.8, 0.35, 0.095, -0.09, 1.0)
BAD_SECTORS = [(-1., 5., 'orographic_sx_sector'), (91., 5., 'orographic_sx_sector'),
               (float('nan'), 5., 'orographic_sx_sector'), (15., 0., 'orographic_sx_step'),
               (90., 2.9, 'more than 61')]                                 # H = 31: M = 63


# ------------------------------------------------------------------------------------------------ Config
def test_config_defaults_and_placement():
    from ssrs_amd.config import Config, _SECTIONS
    cfg = Config()
    assert cfg.orographic_sx_sector == 0. and cfg.orographic_sx_step == 5.
    names = [f.name for f in dataclasses.fields(cfg)]
    at = names.index('orographic_coeffs')
    assert names[at + 1:at + 3] == ['orographic_sx_sector', 'orographic_sx_step']
    section = list(dict(_SECTIONS)['Updraft computation'])
    at = section.index('movement_model')
    assert section[at + 1:at + 4] == ['orographic_sx_sector', 'orographic_sx_step', 'orographic_model']
    block = str(dataclasses.replace(cfg, orographic_sx_sector=15.)).split(':::: Updraft computation')[1].split('::::')[0]
    assert 'orographic_sx_sector = 15.0' in block and 'orographic_sx_step = 5.0' in block


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


@pytest.mark.parametrize('sector, step, match', BAD_SECTORS)
def test_bad_sectors_are_refused_before_device_work(tmp_path, no_gpu, sector, step, match):
    from ssrs_amd import Config, Simulator, layers
    cfg = Config(run_name='bad', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100.,
                 orographic_model='improved', orographic_sx_sector=sector, orographic_sx_step=step)
    with pytest.raises(ValueError, match=match):
        Simulator(cfg, terrain=np.zeros((50, 60)))
    assert not (tmp_path / 'bad').exists()
    z = np.zeros((8, 9))
    with pytest.raises(ValueError, match=match):
        layers.compute_sx(z, 10., 270., dmax=50., sector=sector, sector_step=step)
    with pytest.raises(ValueError, match=match):
        layers.orographic_updraft_improved(z, 10., 10., 270., dmax=50., sector=sector, sector_step=step)


def test_original_model_ignores_the_sector_fields(tmp_path, no_gpu):
    """'original' does not look at them: the constructor gets as far as the device (the fixture's AssertionError)."""
    from ssrs_amd import Config, Simulator
    cfg = Config(run_name='orig', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100.,
                 orographic_sx_sector=-1., orographic_sx_step=0.)
    with pytest.raises(AssertionError, match='device work before'):
        Simulator(cfg, terrain=np.zeros((50, 60)))


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.mark.parametrize('sector, step', [(s, t) for s, t, _ in BAD_SECTORS] + [(15., float('inf')), (15., -5.)])
def test_library_refuses_bad_sectors_without_a_gpu(sector, step):
    """NULL pointers and a NULL stream throughout: the sector is checked before anything else is looked at."""
    from ssrs_amd import _native as nat
    lib = nat.lib()
    rc = lib.ssrs_shelter_sx_sector(None, 1, C.c_double(10.), None, None, None, C.c_double(50.), 1, 0, C.c_double(sector),
                                    C.c_double(step), None, None, 8, 8, 1, None)
    assert rc == nat.SSRS_ERR_INVALID
    text = lib.ssrs_last_error()
    assert b'ssrs_shelter_sx_sector' in text and (b'sector_half_width' in text or b'sector_step' in text or b'rays' in text)
    rc = lib.ssrs_updraft_sheltered_sector(None, 1, C.c_double(10.), None, None, None, None, None, None, None, None, 1, None,
                                           C.c_double(sector), C.c_double(step), C.c_double(0.), C.c_double(0.75), None,
                                           None, None, 8, 8, 1, None)
    assert rc == nat.SSRS_ERR_INVALID
    text = lib.ssrs_last_error()
    assert b'ssrs_updraft_sheltered_sector' in text and b'NULL' not in text
    with pytest.raises(ValueError):
        nat.check(rc)


def test_library_checks_the_rest_as_the_single_ray_calls_do():
    from ssrs_amd import _native as nat
    lib = nat.lib()
    buf = (C.c_double * 64)()
    rays = (C.c_double * 14)(*([1.] * 14))
    dem, u = C.cast(buf, C.c_void_p), C.cast(rays, C.c_void_p)

    def sx(dem=dem, ur=u, uc=u, wdirn=None, dmax=50., out=None, rows=8, cols=8, batch=2, path=0):
        return lib.ssrs_shelter_sx_sector(dem, 1, C.c_double(10.), ur, uc, wdirn, C.c_double(dmax), 1, path, C.c_double(15.),
                                          C.c_double(5.), out, None, rows, cols, batch, None)
    for kwargs, text in [(dict(dem=None), b'dem is NULL'), (dict(rows=1), b'rows, cols'), (dict(dmax=9.), b'K = floor'),
                         (dict(uc=None), b'ray_ur'), (dict(wdirn=dem), b'wind direction'), (dict(path=3), b'path')]:
        assert sx(out=dem, **kwargs) == nat.SSRS_ERR_INVALID, kwargs
        assert text in lib.ssrs_last_error(), (kwargs, lib.ssrs_last_error())
    # all batch x M = 14 steps are looked at, not the first `batch`
    rays[13] = 1.5
    assert sx(out=dem) == nat.SSRS_ERR_INVALID and b'ray step 6 of case 1' in lib.ssrs_last_error()
    rays[13] = 1.
    # a forced LDS path whose sector halo cannot fit: K = 400 along both axes
    assert sx(out=dem, dmax=4005., path=1) == nat.SSRS_ERR_INVALID and b'does not fit' in lib.ssrs_last_error()
    # nothing asked for: fine, and still no GPU needed
    assert sx() == nat.SSRS_OK
    prm = nat.SsrsShelterParams(50., 1, 0, 80., (C.c_double * 7)(*DEFAULTS))
    rc = lib.ssrs_updraft_sheltered_sector(dem, 1, C.c_double(10.), u, u, u, u, None, None, None, None, 1, C.byref(prm),
                                           C.c_double(15.), C.c_double(5.), C.c_double(0.), C.c_double(-1.), None, dem,
                                           None, 8, 8, 2, None)
    assert rc == nat.SSRS_ERR_INVALID and b'positive threshold' in lib.ssrs_last_error()


# ------------------------------------------------------------------------------------------------ the ray counts
@pytest.mark.parametrize('sector, step, count', [(15., 5., 7), (10., 2.5, 9), (14.999, 5., 5), (0., 5., 1)])
def test_ray_counts(sector, step, count):
    from ssrs_amd import layers
    assert layers.sector_rays(sector, step) == ((count - 1) // 2, count)
    assert sref.ray_count(sector, step) == ((count - 1) // 2, count)
    az = sref.azimuths(237.3, sector, step)
    assert len(az) == count and az[count // 2] == 237.3
    assert [float(a) for a in az] == [237.3 + float(m - count // 2) * step for m in range(count)]


def test_layers_hands_over_the_steps_case_major():
    from ssrs_amd import layers
    batch, single, ur, uc, wd = layers._wind_direction_args([10., 237.3], 'row_north', 4, 4, 15., 5.)
    assert (batch, single, wd) == (2, False, None) and ur.shape == uc.shape == (14,)
    for j, a in enumerate((10., 237.3)):
        for m, a_m in enumerate(sref.azimuths(a, 15., 5.)):
            want = ref.ray_step(a_m, 'row_north')
            assert (ur[j * 7 + m], uc[j * 7 + m]) == (float(want[0]), float(want[1]))
    assert layers._wind_direction_args(10., 'row_east', 4, 4, 15., 5.)[:2] == (1, True)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize('axes', ['row_north', 'row_east'])
@pytest.mark.parametrize('wdirn', [0., 237.3, 270.])
def test_reference_on_a_plane(axes, wdirn):
    """z = 1200 + p r res + q c res: bilinear interpolation is exact on a plane, so every valid sample of the ray
    (ur, uc) gives the tangent p ur + q uc, and Sx-bar is the mean of the M angles.  Cells at least 8 from every edge
    have a valid sample on every ray (K = 6).  Measured: at most 2.0e-12 degrees off; the bound is 50 times that."""
    p, q, res, dmax, shape, (W, S) = 0.31, -0.17, 10., 60., (70, 45), (15., 5.)
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    z = 1200. + p * r * res + q * c * res
    tbar, sx = sref.sector_sx(z, res, wdirn, W, S, dmax=dmax, ray_axes=axes)
    steps = [ref.ray_step(a, axes) for a in sref.azimuths(wdirn, W, S)]
    assert len(steps) == 7
    expect = np.mean([np.degrees(np.arctan(p * float(ur) + q * float(uc))) for ur, uc in steps])
    inner = (slice(8, -8), slice(8, -8))
    worst = float(np.abs(sx[inner] - expect).max())
    print(f'{axes} {wdirn:g}: largest |Sx-bar - analytic| = {worst:.3e} degrees')
    assert worst <= 1e-10
    np.testing.assert_allclose(tbar[inner], np.tan(np.radians(expect)), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize('axes', ['row_north', 'row_east'])
def test_reference_without_a_sector_is_the_single_ray(axes):
    rng = np.random.default_rng(3)
    z = rng.uniform(0., 80., (17, 19))
    z[8, 9] = np.nan
    _, wd = np.mgrid[0:17, 0:19].astype(np.float64)
    wd = 200. + 9. * wd
    wd[2, 3] = np.nan
    for wdirn in (0., 237.3, wd):
        for W, S in ((0., 5.), (4.9, 5.)):
            tbar, sx = sref.sector_sx(z, 10., wdirn, W, S, dmax=45., ray_axes=axes)
            want = ref.tan_sx(z, 10., wdirn, dmax=45., ray_axes=axes)
            assert np.array_equal(tbar.view(np.int64), want.view(np.int64))
            assert np.array_equal(sx.view(np.int64), ref.sx_degrees(want).view(np.int64))
