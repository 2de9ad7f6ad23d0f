"""Rotor exposure time (K15's timed form), the parts that need no GPU: the restatement of tests/rotor_time_ref.py against a
second, independent form, the Config field and the constructor's refusals, and the library's
argument validation."""
import ctypes as C

import numpy as np
import pytest

import rotor_ref
import rotor_time_ref as ref
from ssrs_amd import Config
from ssrs_amd.simulator import Simulator


@pytest.mark.parametrize('name', ['planted', 'lead_5_shift_1', 'loiter_shift_3'])
def test_restatement_against_a_second_form(name):
    c = rotor_ref.case(name)
    inside = ref.inside_of(c)[c['lead']:]
    # dt = 1 everywhere: the time is rotor_ref's own points
    ones = np.ones(inside.shape[0], dtype=np.int32)
    assert np.array_equal(ref.time_per_turbine(inside, ones), rotor_ref.expected(name)['points'])
    for pattern in ref.PATTERNS:
        dt, time = ref.expected(name, pattern)
        assert dt.dtype == np.int32 and dt.shape == (c['lead'] + inside.shape[0],) and time.dtype == np.int64
        assert (dt[:c['lead']] == ref.LEAD_DT).all()
        exact = ref.time_per_turbine_python(inside, dt[c['lead']:])
        assert [int(v) % 2 ** 64 for v in time] == [v % 2 ** 64 for v in exact]
        # nothing hits turbines 5 .. 8, and the planted ones carry time
        assert not time[5:9].any() and (time[[0, 1, 31, 32, 63, 64]] > 0).all()
    random, zeros, negative = (ref.expected(name, p) for p in ref.PATTERNS)
    assert (zeros[1] <= random[1]).all() and zeros[1][0] < random[1][0] and (zeros[0] == 0).sum() > 10
    assert (negative[0] < 0).sum() == 1 and negative[1][0] < random[1][0] and negative[1][1] < random[1][1]
    assert np.array_equal(np.delete(negative[1], [0, 1]), np.delete(random[1], [0, 1]))
    if 'loiter' in name:
        # 4097 points of 2^31 - 1 inside turbine 0: past 2^32 many times over, for one lane's 4 points x spans and for a block
        assert int(random[1][0]) > 4097 * ref.CAP > 2 ** 43


def test_a_negative_dt_is_added_as_it_stands():
    inside = np.ones((5, 2), dtype=bool)
    inside[4, 1] = False
    dt = np.array([ref.CAP, -1, -2 ** 31, 7, 100], dtype=np.int32)
    got = ref.time_per_turbine(inside, dt)
    assert got.tolist() == [ref.CAP - 1 - 2 ** 31 + 107, ref.CAP - 1 - 2 ** 31 + 7] == [105, 5]
    assert ref.time_per_turbine_python(inside, dt) == [105, 5]


def test_config_field(tmp_path):
    from dataclasses import fields
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    assert cfg.rotor_exposure_time is False
    names = [f.name for f in fields(Config)]
    at = names.index('flight_min_groundspeed')
    assert names[at + 1] == 'rotor_exposure_time'
    build = list(dict(_SECTIONS)['MI355X build'])
    assert build[build.index('flight_min_groundspeed') + 1] == 'rotor_exposure_time'
    assert build[-1] == 'turbine_encounter_radius'
    assert 'rotor_exposure_time = False' in str(cfg).split(':::: MI355X build')[1]
    assert 'rotor_exposure_time = True' in str(Config(rotor_exposure_time=True)).split(':::: MI355X build')[1]


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


def _table(**extra):
    cols = dict(x=[1500., 2550., 3000.], y=[700., 900., 1500.], t_hh=[80., 90., 100.], t_rd=[100., 110., 120.])
    cols.update(extra)
    return cols


def test_constructor_refuses_each_missing_prerequisite(tmp_path, no_gpu):
    base = dict(run_name='t', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100., track_count=10, sim_seed=1,
                rotor_exposure_time=True)
    full = dict(flight_height=True, rotor_geometry='turbine', flight_time=True)
    dem = np.zeros((50, 60))
    for drop, match in (('flight_height', 'flight_height=True'), ('rotor_geometry', "rotor_geometry='turbine'"),
                        ('flight_time', 'flight_time=True')):
        kw = {k: v for k, v in full.items() if k != drop}
        with pytest.raises(ValueError, match=f'rotor_exposure_time = True needs {match}'):
            Simulator(Config(**base, **kw), terrain=dem, turbines=_table())
    with pytest.raises(ValueError, match='needs turbines: none were given'):
        Simulator(Config(**base, **full), terrain=dem)
    for column in ('t_hh', 't_rd'):
        table = _table()
        del table[column]
        with pytest.raises(ValueError, match=column):
            Simulator(Config(**base, **full), terrain=dem, turbines=table)
    # the prerequisites without the option are what they were: nothing is asked of them
    cfg = Config(**{**base, 'rotor_exposure_time': False})
    assert cfg.rotor_exposure_time is False and Simulator._check_rotor_exposure_time(cfg) is None


def test_summary_needs_a_timed_run():
    sim = object.__new__(Simulator)
    sim.turbine_rotor_encounters = {}
    with pytest.raises(ValueError, match='no rotor exposure time'):
        sim.compute_turbine_rotor_time()
    # an untimed rotor run leaves no time either
    sim.turbine_rotor_encounters = {('c', 0): dict(tracks_per_turbine=np.zeros(3, dtype=np.int64),
                                                   points_per_turbine=np.zeros(3, dtype=np.int64))}
    with pytest.raises(ValueError, match='no rotor exposure time'):
        sim.compute_turbine_rotor_time()


INV = -1


def _call(lib, **kw):
    buf = (C.c_char * 64)()
    a = dict(traj=buf, off=buf, ntracks=1, alt=buf, dt=buf, info=buf, rows=70, cols=90, turb=buf, reach=buf, zband=buf, nturb=1,
             bin_start=buf, bin_items=buf, hits=buf, first=None, points=None, time=buf)
    a.update(kw)
    return lib.ssrs_rotor_encounters_timed(a['traj'], a['off'], C.c_int64(a['ntracks']), a['alt'], a['dt'], a['info'], a['rows'],
                                           a['cols'], a['turb'], a['reach'], a['zband'], a['nturb'], a['bin_start'],
                                           a['bin_items'], a['hits'], a['first'], a['points'], a['time'], None)


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    assert 'ssrs_rotor_encounters_timed' in _native.EXPORTS and lib.ssrs_version() == 109
    assert len(_native.ROTOR_ENCOUNTERS_TIMED_ARGTYPES) == len(_native.ROTOR_ENCOUNTERS_ARGTYPES) + 2 == 19
    header = open(_native.os.path.join(_native.os.path.dirname(_native._HERE), 'include', 'ssrs_hip.h')).read()
    assert f'#define SSRS_ROTOR_TIMED_LDS_TURBINES {_native.SSRS_ROTOR_TIMED_LDS_TURBINES}' in header
    buf = (C.c_char * 64)()
    odd = C.c_void_p(C.addressof(buf) + 2)
    four = C.c_void_p(C.addressof(buf) + 4)
    for bad in (dict(dt=None), dict(time=None), dict(dt=odd), dict(time=four), dict(time=odd),
                # ... and everything ssrs_rotor_encounters refuses
                dict(traj=None), dict(off=None), dict(alt=None), dict(info=None), dict(turb=None), dict(reach=None),
                dict(zband=None), dict(bin_start=None), dict(bin_items=None), dict(hits=None),
                dict(ntracks=-1), dict(ntracks=2 ** 31), dict(nturb=0), dict(nturb=_native.SSRS_TURBINE_MAX + 1),
                dict(rows=0), dict(cols=0), dict(rows=32768), dict(cols=40000),
                dict(traj=odd), dict(alt=odd), dict(info=four), dict(zband=four), dict(points=four)):
        assert _call(lib, **bad) == INV, bad
        assert b'ssrs_rotor_encounters_timed' in lib.ssrs_last_error(), bad
    # nothing to do is not an error, and is decided before the device is touched
    assert _call(lib, ntracks=0) == _native.SSRS_OK
    assert _call(lib, ntracks=0, points=buf, first=buf) == _native.SSRS_OK
