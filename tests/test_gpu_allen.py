"""K12 on the device: the cases of tests/allen_ref.py through ssrs_amd.thermals.compute_allen_thermals with the assertions
of tests/test_allen_emulation.py, then thermal_model = 'allen' through Simulator."""
import datetime
import os
from dataclasses import replace

import numpy as np
import pytest

import allen_ref as ref

pytestmark = pytest.mark.gpu


def gpu_field(case, path='auto', dtype=None):
    import torch
    from ssrs_amd.thermals import compute_allen_thermals
    out = compute_allen_thermals(case['xt'], case['yt'], case['wgain'], case['rgain'], case['shape'], case['res'], case['z'],
                                 case['zi'], case['wstar'], sink=case['sink'], dtype=dtype or torch.float64, path=path,
                                 want_nearest=True, want_table=True, return_stats=True)
    return tuple(t.cpu().numpy() for t in out[:3]) + (out[3],)


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('case', ref.CASES, ids=ref.CASE_IDS)
def test_field(gpu, case):
    """Every case: the nearest updraft of every cell, the table's bits, the field within the bound, and the same bits on
    the LDS and the global path."""
    import torch
    name = case['name']
    fld, near, tab, left = gpu_field(case)
    ref.check_case(name, near, tab, fld)
    glob = gpu_field(case, 'global')
    assert glob[3] == 0
    assert all(same_bits(a, b) for a, b in zip((fld, near, tab), glob)), name
    if case['overflow']:
        assert left > 0                                                     # auto fell back ...
        with pytest.raises(ValueError, match='does not fit'):               # ... and the forced path is refused
            gpu_field(case, 'lds')
    else:
        lds = gpu_field(case, 'lds')
        assert all(same_bits(a, b) for a, b in zip((fld, near, tab), lds[:3])) and lds[3] == left, name
    if name in ('ragged', 'tiles'):
        assert left < fld.size // 2
        f32 = gpu_field(case, dtype=torch.float32)[0]
        assert same_bits(f32, fld.astype(np.float32))                       # the f64 value rounded once
    if name == 'clustered':
        assert left > fld.size // 2


def test_no_updrafts_is_the_constant_sink(gpu):
    import torch
    from ssrs_amd.thermals import compute_allen_thermals
    none = np.zeros(0)
    out, near = compute_allen_thermals(none, none, none, none, (7, 9), 30., 100., 1000., 2., sink=True, dtype=torch.float64,
                                       want_nearest=True)
    assert out.shape == (7, 9) and bool((out == 0.).all()) and bool((near == -1).all())


def make_config(tmp_path, **kw):
    from ssrs_amd import Config
    base = Config(run_name='t', out_dir=str(tmp_path), sim_seed=11, region_width_km=(8., 6.), resolution=100., track_count=1,
                  track_start_region=(1, 7, 0.2, 0.6), track_direction=0., thermals_realization_count=2,
                  thermal_model='allen', thermal_allen_zi=1000., thermal_allen_wstar=2.)
    return replace(base, **kw)


def _thermal_files(sim, case_id, count=2):
    return [np.load(os.path.join(sim.mode_data_dir, f'{case_id}_r{k}_thermals.npy')) for k in range(count)]


def test_simulator_uniform_mode(gpu, tmp_path):
    import torch
    from ssrs_amd import Simulator
    from ssrs_amd.thermals import allen_scalars, allen_updrafts, compute_allen_thermals
    sim = Simulator(make_config(tmp_path), terrain='synthetic')
    assert sim.gridsize == (60, 80)
    fields = _thermal_files(sim, 's10d270')
    assert all(f.dtype == np.float32 and f.shape == (60, 80) for f in fields) and not np.array_equal(*fields)
    n = allen_scalars(100., 1000., 2., (60, 80), 100.)['N']
    assert n == 624
    for k, got in enumerate(fields):
        ups = allen_updrafts(n, (60, 80), 100., 11 + 7919 * (k + 1), (1., 1.))
        want = compute_allen_thermals(*ups, (60, 80), 100., 100., 1000., 2., dtype=torch.float32)
        assert same_bits(got, want.cpu().numpy()), k
    again = Simulator(make_config(tmp_path, run_name='again'), terrain='synthetic')
    assert all(same_bits(a, b) for a, b in zip(fields, _thermal_files(again, 's10d270')))
    assert sim._get_id_string('s10d270', 1) == 's10d270_d0_t75_fluidflow-allen_r1'
    sim.simulate_tracks()
    for k in range(3):
        assert os.path.exists(os.path.join(sim.mode_data_dir, f's10d270_d0_t75_fluidflow-allen_r{k}_potential.npy'))
        assert os.path.exists(os.path.join(sim.mode_data_dir, f's10d270_d0_t75_fluidflow-allen_r{k}_tracks.pkl'))


def test_simulator_snapshot_mode_takes_zi_and_wstar_from_the_layers(gpu, tmp_path):
    import torch
    from ssrs_amd import Simulator, layers
    from ssrs_amd.thermals import allen_datetime_gains, allen_scalars, allen_updrafts, compute_allen_thermals
    x, y = np.array([0., 1., 0., 1., .5]), np.array([0., 0., 1., 1., .4])
    bl, q = np.array([60., 700., 800., 900., 1000.]), np.array([200., 150., -20., 300., 250.])
    entry = dict(datetime=(2010, 6, 17, 13), x_km=x, y_km=y, wspeed=np.full(5, 5.), wdirn=np.full(5, 270.),
                 pressure=np.full(5, 9e4), temperature=np.full(5, 15.), blheight=bl, surfheatflux=q)
    cfg = make_config(tmp_path, region_width_km=(1., 1.), sim_mode='snapshot', thermal_allen_zi=0., thermal_allen_wstar=0.,
                      thermals_realization_count=1, track_start_region=(0.1, 0.9, 0.1, 0.3))
    sim = Simulator(cfg, terrain=np.zeros((10, 10)), wind=[entry])
    case_id = sim.case_ids[0]
    zi, wstar = sim.allen_case_scalars(case_id)
    assert zi == bl.clip(min=100.).mean() == 700.
    theta = layers.compute_potential_temperature(entry['pressure'], entry['temperature'])
    assert wstar == float(np.mean(layers.deardoff_velocity_function(theta, bl, q))) > 0.
    n = allen_scalars(100., zi, wstar, (10, 10), 100.)['N']
    ups = allen_updrafts(n, (10, 10), 100., 11 + 7919, allen_datetime_gains(datetime.datetime(2010, 6, 17, 13)))
    want = compute_allen_thermals(*ups, (10, 10), 100., 100., zi, wstar, dtype=torch.float32)
    assert same_bits(_thermal_files(sim, case_id, 1)[0], want.cpu().numpy())
    fixed = Simulator(replace(cfg, run_name='fixed', thermal_allen_zi=900.), terrain=np.zeros((10, 10)), wind=[entry])
    assert fixed.allen_case_scalars(case_id) == (900., wstar)                # a positive field overrides


def test_default_thermal_model_is_unchanged(gpu, tmp_path):
    import torch
    from ssrs_amd import Simulator
    from ssrs_amd.thermals import compute_thermals_batch
    cfg = make_config(tmp_path, thermal_model='random', thermal_allen_zi=0., thermal_allen_wstar=0.)
    sim = Simulator(cfg, terrain='synthetic')
    want = compute_thermals_batch(sim.get_terrain_aspect(), 2.0, [11 + 7919 * (k + 1) for k in range(2)], dtype=torch.float32)
    for got, w in zip(_thermal_files(sim, 's10d270'), want):
        assert same_bits(got, np.asarray(w))
    assert sim._get_id_string('s10d270', 0) == 's10d270_d0_t75_fluidflow_r0'
