"""K12 on the host (no GPU): the scalars and the updraft count of an Allen field, the datetime gains, the draws, the bins,
the Config fields and every refusal that must come before device work."""
import ctypes as C
import datetime
from dataclasses import fields

import numpy as np
import pytest

import allen_ref as ref


def test_scalars_and_updraft_count():
    from ssrs_amd.thermals import allen_scalars
    grid = ((5000, 6000), 10.)                                                   # 60 x 50 km at 10 m
    for (z, zi), n in (((100., 1000.), 38994), ((100., 150.), 1077378), ((700., 1000.), 24091)):
        sc = allen_scalars(z, zi, 2., *grid)
        zzi = z / zi
        rbar = 0.102 * zzi ** (1 / 3) * (1 - 0.25 * zzi) * zi
        assert sc['N'] == n == int(round(0.6 * 50000. * 60000. / (zi * rbar)))
        assert sc['zzi'] == zzi and sc['rbar'] == rbar and sc['wtbar'] == zzi ** (1 / 3) * (1 - 1.1 * zzi) * 2.
        assert sc['we'] == 0. and sc['z_below_zi']
    assert allen_scalars(100., 1000., 2., (512, 640), 10.)['N'] == 426
    sunk = allen_scalars(100., 1000., 2., *grid, sink=True)
    area = 38994 * np.pi * sunk['rbar'] ** 2
    assert sunk['we'] == -(sunk['wtbar'] * area * (-2.5 * (0.1 - 0.5))) / (3e9 - area) < 0.
    assert allen_scalars(700., 1000., 2., *grid, sink=True)['we'] == 0.          # a positive sink is not allowed
    assert not allen_scalars(1200., 1000., 2., *grid)['z_below_zi']
    for bad in (dict(z=0.), dict(zi=-1.), dict(wstar=0.), dict(zi=np.nan), dict(wstar=np.inf)):
        args = dict(z=100., zi=1000., wstar=2.)
        args.update(bad)
        with pytest.raises(ValueError, match=next(iter(bad))):
            allen_scalars(args['z'], args['zi'], args['wstar'], *grid)


def test_datetime_gains():
    from ssrs_amd.thermals import allen_datetime_gains
    assert allen_datetime_gains(None) == (1., 1.)
    at = lambda month, hour: allen_datetime_gains(datetime.datetime(2010, month, 15, hour))
    assert at(6, 3)[0] == 0. and at(6, 6)[0] == 0. and at(6, 21)[0] == 0.
    assert abs(at(6, 12)[0] - 1.2) < 1e-3
    assert at(1, 12)[1] == 0.5 and at(11, 12)[1] == 0.5
    assert abs(at(6, 12)[1] - (0.8 + 0.3 * np.cos(1.8 * np.pi))) < 1e-3


def test_updraft_draws():
    from ssrs_amd.thermals import allen_updrafts, allen_datetime_gains
    grid = ((97, 131), 30.)
    a, b = allen_updrafts(149, *grid, 5), allen_updrafts(149, *grid, 5)
    assert all(np.array_equal(x, y) and x.dtype == np.float64 and x.shape == (149,) for x, y in zip(a, b))
    assert not np.array_equal(a[0], allen_updrafts(149, *grid, 6)[0])
    rng = np.random.default_rng(5)                                               # the stated order of the draws
    assert np.array_equal(a[0], rng.uniform(0., 131 * 30., 149)) and np.array_equal(a[1], rng.uniform(0., 97 * 30., 149))
    xt, yt, wgain, rgain = allen_updrafts(5000, *grid, 7, gains=(1.2, 0.5))
    assert 0. <= xt.min() and xt.max() < 131 * 30. and 0. <= yt.min() and yt.max() < 97 * 30.
    assert yt.max() > 0.9 * 97 * 30.                                             # yt is drawn over the raster's HEIGHT
    assert 0.7 * 1.2 <= wgain.min() and wgain.max() <= 1.3 * 1.2 and 0.8 * 0.5 <= rgain.min() and rgain.max() <= 1.2 * 0.5
    night = allen_updrafts(50, *grid, 7, gains=allen_datetime_gains(datetime.datetime(2010, 6, 17, 2)))
    assert (night[2] == 0.).all() and (night[3] > 0.).all()


def test_bins():
    from ssrs_amd.thermals import allen_bins
    shape, res = (97, 131), 30.
    xt, yt = ref.CASES[0]['xt'].copy(), ref.CASES[0]['yt'].copy()
    xt[3], yt[3] = 131 * res, 97 * res                                           # the far corner of the domain
    xt[4], yt[4] = 0., 97 * res
    start, items, bin_m, nbx, nby = allen_bins(xt, yt, shape, res)
    assert start.dtype == items.dtype == np.int32 and start.shape == (nbx * nby + 1,)
    assert bin_m >= res and nbx == int(np.ceil(131 * res / bin_m)) and nby == int(np.ceil(97 * res / bin_m))
    assert 1. <= xt.size / (nbx * nby) <= 4.                                     # a few updrafts per bin
    assert start[0] == 0 and start[-1] == xt.size and (np.diff(start) >= 0).all()
    assert np.array_equal(np.sort(items), np.arange(xt.size))                    # each updraft in exactly one bin
    for b in range(nbx * nby):
        mine = items[start[b]:start[b + 1]]
        assert (np.diff(mine) > 0).all()                                         # ascending inside a bin
        bx = np.minimum(np.floor(xt[mine] / bin_m), nbx - 1)
        by = np.minimum(np.floor(yt[mine] / bin_m), nby - 1)
        assert (by * nbx + bx == b).all()
    assert 3 in items[start[nbx * nby - 1]:] and 4 in items[start[(nby - 1) * nbx]:start[(nby - 1) * nbx + 1]]
    rng = np.random.default_rng(0)
    crowd = allen_bins(rng.uniform(0., 300., 10000), rng.uniform(0., 300., 10000), (10, 10), 30.)
    assert crowd[2] == 30. and crowd[3] == crowd[4] == 10                        # never smaller than a cell
    one = allen_bins(np.array([5.]), np.array([7.]), shape, res)
    assert one[3] == one[4] == 1 and list(one[0]) == [0, 1]


def test_tie_case_has_the_ties_it_is_there_for():
    e, c = ref.expected('ties'), ref.CASES[ref.CASE_IDS.index('ties')]
    xc, yc = np.meshgrid(np.arange(131) * 30., np.arange(97) * 30.)
    d2 = (xc[..., None] - c['xt']) ** 2 + (yc[..., None] - c['yt']) ** 2
    equal = (d2 == e['d2'][..., None]).sum(-1)
    assert (equal == 2).mean() > 0.2 and (equal >= 4).mean() > 0.01


def test_config_fields():
    from ssrs_amd import Config
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    assert (cfg.thermal_allen_zi, cfg.thermal_allen_wstar, cfg.thermal_allen_sink) == (0., 0., False)
    assert cfg.thermal_model == 'random'
    names = [f.name for f in fields(Config)]
    at = names.index('turbine_encounter_radius')
    assert names[at - 3:at] == ['thermal_allen_zi', 'thermal_allen_wstar', 'thermal_allen_sink']
    assert names[-2:] == ['hist_safe_tracks', 'thermal_model']
    build = dict(_SECTIONS)['MI355X build']
    assert build[-5:] == ('thermal_model', 'thermal_allen_zi', 'thermal_allen_wstar', 'thermal_allen_sink',
                          'turbine_encounter_radius')
    text = str(Config(thermal_model='allen', thermal_allen_zi=900., thermal_allen_sink=True)).split(':::: MI355X build')[1]
    assert 'thermal_model = allen' in text and 'thermal_allen_zi = 900.0' in text and 'thermal_allen_sink = True' in text
    assert text.index('thermal_allen_sink') < text.index('turbine_encounter_radius')


def _config(tmp_path, **kw):
    from ssrs_amd import Config
    args = dict(run_name='allen', out_dir=str(tmp_path), region_width_km=(1., 1.), resolution=100., track_count=1, sim_seed=1,
                thermal_model='allen', thermals_realization_count=1, thermal_allen_zi=1000., thermal_allen_wstar=2.)
    args.update(kw)
    return Config(**args)


def _entry(**kw):
    x, y = np.array([0., 1., 0., 1., .5]), np.array([0., 0., 1., 1., .4])
    item = dict(datetime=(2010, 6, 17, 13), x_km=x, y_km=y, wspeed=np.full(5, 5.), wdirn=np.full(5, 270.),
                pressure=np.full(5, 9e4), temperature=np.full(5, 15.), blheight=np.full(5, 800.),
                surfheatflux=np.full(5, 200.))
    item.update(kw)
    return {k: v for k, v in item.items() if v is not ...}


def test_constructor_errors_need_no_gpu(tmp_path):
    """Raised before any device work: on a box without a GPU the first device call would be a RuntimeError instead."""
    from ssrs_amd import Simulator
    dem = np.zeros((10, 10))
    with pytest.raises(ValueError, match="thermal_model = 'blobs'"):
        Simulator(_config(tmp_path, thermal_model='blobs'), terrain=dem)
    for missing in (dict(thermal_allen_zi=0.), dict(thermal_allen_wstar=0.), dict(thermal_allen_zi=0., thermal_allen_wstar=0.)):
        with pytest.raises(ValueError, match='thermal_allen_zi and thermal_allen_wstar'):
            Simulator(_config(tmp_path, **missing), terrain=dem)
    with pytest.raises(ValueError, match='thermal_allen_zi'):
        Simulator(_config(tmp_path, thermal_allen_zi=-5.), terrain=dem)
    with pytest.raises(ValueError, match='thermals_realization_count'):
        Simulator(_config(tmp_path, thermals_realization_count=0), terrain=dem)
    with pytest.raises(ValueError, match=r'N = \d+ updrafts for zi = 100 m'):       # too many updrafts: N and zi are named
        Simulator(_config(tmp_path, region_width_km=(600., 500.), resolution=10., wtk_thermal_height=20,
                          thermal_allen_zi=100.), terrain=dem)
    snap = dict(sim_mode='snapshot', thermal_allen_zi=0., thermal_allen_wstar=0.)
    for name in ('pressure', 'temperature', 'blheight', 'surfheatflux'):
        with pytest.raises(ValueError, match=f"'allen' needs the layer '{name}'"):
            Simulator(_config(tmp_path, **snap), terrain=dem, wind=[_entry(**{name: ...})])
    with pytest.raises(ValueError, match='blheight'):                             # one of the two left at 0 is enough
        Simulator(_config(tmp_path, sim_mode='snapshot', thermal_allen_wstar=0.), terrain=dem, wind=[_entry(blheight=...)])


def test_wrapper_refuses_bad_updrafts_without_a_gpu():
    from ssrs_amd.thermals import compute_allen_thermals
    shape, res = (20, 30), 30.
    good = dict(xt=np.array([10., 50.]), yt=np.array([10., 50.]), wgain=np.ones(2), rgain=np.ones(2))

    def call(**kw):
        a = dict(good, **kw)
        return compute_allen_thermals(a['xt'], a['yt'], a['wgain'], a['rgain'], shape, res, 100., 1000., 2.)
    for bad, match in ((dict(xt=np.array([10., np.nan])), 'xt holds a non-finite'), (dict(yt=np.array([np.inf, 1.])), 'yt holds'),
                       (dict(xt=np.array([-1e-9, 5.])), 'xt leaves the domain'), (dict(xt=np.array([5., 900.01])), 'xt leaves'),
                       (dict(yt=np.array([5., 600.5])), 'yt leaves the domain'), (dict(wgain=np.array([1., np.nan])), 'wgain'),
                       (dict(rgain=np.ones(3)), 'rgain has 3 values')):
        with pytest.raises(ValueError, match=match):
            call(**bad)
    with pytest.raises(ValueError, match='path'):
        compute_allen_thermals(*good.values(), shape, res, 100., 1000., 2., path='fast')
    with pytest.raises(ValueError, match='zi'):
        compute_allen_thermals(*good.values(), shape, res, 100., 0., 2.)


def test_c_abi_argument_errors():
    from ssrs_amd import _native
    lib = _native.lib()
    INV = _native.SSRS_ERR_INVALID
    for name in ('ssrs_allen_workspace_bytes', 'ssrs_allen_thermal_field'):
        assert hasattr(lib, name) and name in _native.EXPORTS
    assert lib.ssrs_version() == 109
    size = lib.ssrs_allen_workspace_bytes
    assert size(1) == 512 and size(149) == 256 + (149 * 48 + 255) // 256 * 256 and size(1 << 22) == 256 + (48 << 22)
    assert size(0) == 0 and size(-3) == 0 and size((1 << 22) + 1) == 0
    buf = (C.c_char * (1 << 16))()
    p = C.cast(buf, C.c_void_p)
    good = dict(xt=p, yt=p, wgain=p, rgain=p, n=10, bin_start=p, bin_items=p, bin=60., nbx=4, nby=4, rbar=46., wtbar=0.8,
                zzi=0.1, below=1, we=0., res=30., rows=8, cols=8, path=0, out=p, out_type=1, nearest=None, table=None,
                work=p, nb=1 << 16)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ssrs_allen_thermal_field(*(a[k] for k in good), None)
    nan, inf = float('nan'), float('inf')
    cases = [(dict(xt=None), b'xt'), (dict(yt=None), b'yt'), (dict(wgain=None), b'wgain'), (dict(rgain=None), b'rgain'),
             (dict(n=0), b'n_updrafts'), (dict(n=-4), b'n_updrafts'), (dict(n=(1 << 22) + 1), b'n_updrafts'),
             (dict(bin_start=None), b'bin_start'), (dict(bin_items=None), b'bin_items'), (dict(bin=0.), b'bin_size_m'),
             (dict(bin=29.), b'bin_size_m'), (dict(bin=nan), b'bin_size_m'), (dict(nbx=0), b'nbx'), (dict(nby=-1), b'nby'),
             (dict(nbx=1 << 16), b'nbx'), (dict(rbar=nan), b'rbar'), (dict(wtbar=inf), b'wtbar'), (dict(zzi=0.), b'zzi'),
             (dict(zzi=nan), b'zzi'), (dict(we=0.5), b'we'), (dict(we=nan), b'we'), (dict(res=0.), b'res'),
             (dict(res=-30.), b'res'), (dict(rows=0), b'rows'), (dict(cols=-2), b'cols'), (dict(path=3), b'path'),
             (dict(path=-1), b'path'), (dict(out=None), b'out'), (dict(out_type=2), b'out_type'), (dict(work=None), b'workspace'),
             (dict(nb=0), b'workspace'), (dict(nb=size(10) - 1), b'workspace')]
    for bad, word in cases:
        assert call(**bad) == INV, bad
        msg = lib.ssrs_last_error()
        assert b'ssrs_allen_thermal_field' in msg and word in msg, (bad, msg)
