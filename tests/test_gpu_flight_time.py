"""K16 on the device: ssrs_track_time / ssrs_flight_windinfo through ssrs_amd/flight.py on every case of
tests/flight_time_ref.py (the cases tests/test_flight_time_emulation.py runs on the CPU), accumulation, the optional
outputs, the wind's components against numpy, one physical check, and Simulator(flight_time=True) end to end.  Every
comparison of times is integer equality; the one f32 map is checked for its range and its sum."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import altitude_ref
import flight_time_ref as ref

pytestmark = pytest.mark.gpu


def scalars(params):
    """The keyword arguments of flight.compute_track_times for a case's integers (int(round(1000 x)) gives them back)."""
    from ssrs_amd import flight
    va, gmin, res_mm = params
    kw = dict(resolution=res_mm / 1000., airspeed=va / 1000., min_groundspeed=gmin / 1000.)
    p = flight.time_params(**kw)
    assert (p.va, p.gmin, p.res_mm) == tuple(params)
    return kw


def shifted(values, shift, gpu):
    """`values` on the device, `shift` elements of 4 bytes past torch's alignment, in-raster points around it."""
    raw = torch.full((values.shape[0] + 8, 2), 3, dtype=torch.int16, device=gpu)
    assert raw.data_ptr() % 16 == 0
    view = raw[shift:shift + values.shape[0]]
    view.copy_(torch.from_numpy(values))
    assert view.shape[0] == 0 or view.data_ptr() % 16 == 4 * (shift % 4)
    return view


def device_case(c, gpu):
    """(traj, offsets, masked, windinfo) of a case on the device; offsets the slice [1:] of the longer vector."""
    traj, off, masked = ref.points(c)
    return shifted(traj, c['shift'], gpu), torch.from_numpy(off).to(gpu)[1:], shifted(masked, c['shift'], gpu), \
        torch.from_numpy(ref.packed(c)).to(gpu)


def outputs(out, lead):
    """flight's dict as flight_time_ref.check takes it (dt without the lead points)."""
    got = {k: v for k, v in out.items()}
    if 'dt' in got:
        got['dt'] = got['dt'][lead:]
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_cases_on_the_device(gpu, c):
    from ssrs_amd import flight
    traj, off, masked, info = device_case(c, gpu)
    assert int(off[0]) == c['lead']
    kw = scalars(c['params'])
    out = flight.compute_track_times(traj, c['shape'], offsets=off, wind=info, masked=masked, want_dt=True, **kw)
    assert set(out) == set(ref.KEYS) and all(v.is_cuda for v in out.values())
    assert out['time_hist'].dtype == out['band_time_hist'].dtype == out['times'].dtype == torch.int64
    assert tuple(out['times'].shape) == (len(c['tracks']), 2) and out['dt'].dtype == torch.int32
    assert tuple(out['dt'].shape) == (traj.shape[0],)
    ref.check(c['name'], outputs(out, c['lead']))
    assert not bool(out['dt'][:c['lead']].any())           # what lies in front of the chunk's points is not written
    # once more into the same rasters, without dt: everything twice
    again = flight.compute_track_times(traj, c['shape'], offsets=off, wind=info, masked=masked, time_hist=out['time_hist'],
                                       band_time_hist=out['band_time_hist'], **kw)
    assert again['time_hist'] is out['time_hist'] and again['band_time_hist'] is out['band_time_hist'] and 'dt' not in again
    ref.check(c['name'], outputs(dict(time_hist=again['time_hist'], band_time_hist=again['band_time_hist']), 0), times=2)
    assert torch.equal(again['times'], out['times'])
    want = ref.expected(c['name'])
    # each optional output alone equals the same output of the full call
    plain = flight.compute_track_times(traj, c['shape'], offsets=off, wind=info, **kw)
    assert set(plain) == {'time_hist', 'times'}
    assert np.array_equal(plain['time_hist'].cpu().numpy().view(np.uint64), want['time_hist'])
    assert torch.equal(plain['times'][:, 0], out['times'][:, 0]) and not bool(plain['times'][:, 1].any())
    only_dt = flight.compute_track_times(traj, c['shape'], offsets=off, wind=info, want_dt=True, **kw)
    assert torch.equal(only_dt['dt'], out['dt'])
    only_band = flight.compute_track_times(traj, c['shape'], offsets=off, wind=info, masked=masked, **kw)
    assert np.array_equal(only_band['band_time_hist'].cpu().numpy().view(np.uint64), want['band_time_hist'])
    assert torch.equal(only_band['times'], out['times'])
    if c['uniform'] is not None:
        # one wind everywhere: no raster.  The pair goes in through a (speed, direction) that gives it back
        flat = flight.compute_track_times(traj, c['shape'], offsets=off, wind=_wind_of_pair(c['uniform']), masked=masked,
                                          want_dt=True, **kw)
        ref.check(c['name'], outputs(flat, c['lead']))
    if c['lead'] == 0:
        # a list of host tracks gives numpy
        host = flight.compute_track_times(c['tracks'], c['shape'], wind=info, masked=ref.points(c)[2], want_dt=True, **kw)
        assert all(isinstance(v, np.ndarray) for v in host.values())
        ref.check(c['name'], outputs(host, 0))


def _wind_of_pair(pair):
    """(wspeed, wdirn) whose flight.wind_pair(.., 'row_east') is `pair`, checked."""
    from ssrs_amd import flight
    wr, wc = pair
    speed = float(np.hypot(wr, wc)) / 1000.
    dirn = float(np.degrees(np.arctan2(-wr, -wc))) if speed > 0. else 0.
    assert flight.wind_pair(speed, dirn, 'row_east') == tuple(pair), (pair, flight.wind_pair(speed, dirn, 'row_east'))
    return speed, dirn


def test_accumulation_over_disjoint_track_ranges(gpu):
    """Two calls into one pair of rasters on disjoint track ranges equal one call on the union, and what the rasters held
    before is kept."""
    from ssrs_amd import flight
    c = ref.case('short_300')
    traj, off, masked, info = device_case(c, gpu)
    kw = scalars(c['params'])
    pattern = ((np.arange(ref.SHAPE[0] * ref.SHAPE[1], dtype=np.uint64).reshape(ref.SHAPE) * np.uint64(0x9E3779B97F4A7C15)) |
               np.uint64(1)).view(np.int64)
    before = dict(time_hist=pattern, band_time_hist=pattern + 5)
    acc = {k: torch.from_numpy(v.copy()).to(gpu) for k, v in before.items()}
    first = flight.compute_track_times(traj, c['shape'], offsets=off[:121], wind=info, masked=masked, **acc, **kw)
    second = flight.compute_track_times(traj, c['shape'], offsets=off[120:], wind=info, masked=masked, **acc, **kw)
    rows = torch.cat([first['times'], second['times']])
    ref.check(c['name'], outputs(dict(acc, times=rows), 0), before=before)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=lambda d: d.__name__)
@pytest.mark.parametrize('ray_axes', ['row_east', 'row_north'])
def test_windinfo_on_the_device(gpu, dtype, ray_axes):
    """ssrs_flight_windinfo against numpy: equal wherever numpy's unrounded component is farther than 1e-6 from a
    half-integer, within 1 elsewhere (the device's sin and cos may differ from numpy's in the last bit), and fewer than 1 %
    of the cells are exempted; numpy and tensor inputs."""
    from ssrs_amd import flight
    ws, wd = ref.windinfo_inputs(dtype)
    want = np.stack(ref.windinfo(ws, wd, ray_axes), -1)
    exempt = ref.windinfo_exempt(ws, wd, ray_axes)
    assert exempt.mean() < 0.01
    out = flight.wind_cellinfo(ws, wd, ray_axes)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == ref.SHAPE + (2,)
    got = out.cpu().numpy()
    assert np.array_equal(got[~exempt], want[~exempt])
    assert (np.abs(got.astype(np.int64) - want) <= 1).all()
    assert (got[0, :3] == 0).all() and (got[0, 3:5] == -2 ** 20).all()
    again = flight.wind_cellinfo(torch.from_numpy(ws).to(gpu), torch.from_numpy(wd).to(gpu), ray_axes)
    assert torch.equal(again, out)


def test_tailwind_is_faster_and_cross_winds_are_alike(gpu):
    """The same straight northward track ('row_north': +row = north) takes strictly less time under a wind from the south
    than under one from the north, and the same time under east and west winds."""
    from ssrs_amd import flight
    track = [np.stack([np.arange(2, 30), np.full(28, 100)], 1).astype(np.int16)]
    kw = dict(resolution=100., airspeed=15., ray_axes='row_north')
    total = {d: int(flight.compute_track_times(track, ref.SHAPE, wind=(8., d), **kw)['times'][0, 0]) for d in (0., 90., 180., 270.)}
    calm = int(flight.compute_track_times(track, ref.SHAPE, wind=(0., 0.), **kw)['times'][0, 0])
    assert total[180.] < calm < total[0.] and total[90.] == total[270.] > calm
    assert calm == 27 * 6_666_667 and total[180.] == 27 * ((10 ** 11 + 11_500) // 23_000)


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Config, Simulator, flight
    cfg = Config(run_name='timed', out_dir=str(tmp_path), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=64,
                 track_start_region=(1, 5, 0.2, 0.6), track_direction=0., thermals_realization_count=1,
                 flight_time=True, flight_height=True, save_tracks=True)
    sim = Simulator(cfg, terrain='synthetic')
    with pytest.raises(ValueError, match='flight_time=True'):
        sim.compute_residence_time_map()
    sim.simulate_tracks()
    plain = Simulator(replace(cfg, run_name='untimed', flight_time=False), terrain='synthetic')
    plain.simulate_tracks()
    assert plain.residence_time_counts == {} and plain.rotor_residence_time_counts == {} and plain.flight_times == {}
    assert not [f for f in os.listdir(plain.mode_data_dir) if 'residence' in f or 'flight_times' in f]
    with pytest.raises(ValueError, match='flight_time=True'):
        plain.compute_rotor_residence_time_map()

    orograph = np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy'))
    fields = [orograph, orograph + np.load(os.path.join(sim.mode_data_dir, 's10d270_r0_thermals.npy'))]
    pair = flight.wind_pair(10., 270., 'row_east')         # DEM-only terrain
    assert pair == (10_000, 0)
    wr, wc = (np.full((50, 60), v, dtype=np.int32) for v in pair)
    for real_id, field in enumerate(fields):
        key = ('s10d270', real_id)
        stem = f's10d270_d0_t75_fluidflow_r{real_id}'
        path = lambda name, d=sim.mode_data_dir: os.path.join(d, f'{stem}_{name}')
        with open(path('tracks.pkl'), 'rb') as f:
            tracks = pickle.load(f)
        assert len(tracks) == 64
        climb, elev = altitude_ref.cellinfo(field, sim.get_terrain_elevation(), 100., 15., 0.75)
        zone = altitude_ref.altitude(tracks, climb, elev, (50, 60), altitude_ref.DEFAULT)['traj_band']
        want = ref.flight_times(tracks, wr, wc, (50, 60), (15_000, 1_000, 100_000), zone)
        raster = np.load(path('residence_time.npy'))
        assert raster.dtype == np.int64 and np.array_equal(raster.view(np.uint64), want['time_hist'])
        band = np.load(path('rotor_residence_time.npy'))
        assert band.dtype == np.int64 and np.array_equal(band.view(np.uint64), want['band_time_hist'])
        rows = np.load(path('flight_times.npy'))
        assert rows.dtype == np.int64 and rows.shape == (64, 2) and np.array_equal(rows, want['times'])
        assert np.array_equal(sim.residence_time_counts[key], raster) and np.array_equal(sim.flight_times[key], rows)
        assert np.array_equal(sim.rotor_residence_time_counts[key], band)
        # both checksums
        assert int(raster.view(np.uint64).sum(dtype=np.uint64)) == int(rows[:, 0].sum()) > 0
        assert int(band.view(np.uint64).sum(dtype=np.uint64)) == int(rows[:, 1].sum()) > 0
        assert (rows[:, 1] <= rows[:, 0]).all() and int(rows[:, 1].sum()) < int(rows[:, 0].sum())
        # what there was before is that of the run without flight_time, byte for byte
        assert torch.equal(sim._presence_counts[key], plain._presence_counts[key])
        same = [f for f in os.listdir(plain.mode_data_dir)
                if f.startswith(stem) and f.endswith(('presence.npy', 'tracks.pkl', 'flight_heights.npy'))]
        assert f'{stem}_rotor_presence.npy' in same and f'{stem}_tracks.pkl' in same and f'{stem}_flight_heights.npy' in same
        for name in same:
            with open(os.path.join(sim.mode_data_dir, name), 'rb') as a, open(os.path.join(plain.mode_data_dir, name), 'rb') as b:
                assert a.read() == b.read(), name

    share = sim.compute_residence_time_map(radius=0.)
    assert share.dtype == np.float32 and share.shape == (50, 60) and np.isfinite(share).all() and share.min() >= 0.
    assert abs(float(share.sum(dtype=np.float64)) - 1.) < 1e-6
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_residence_time.npy')), share)
    smooth = sim.compute_residence_time_map()
    assert np.isfinite(smooth).all() and smooth.min() >= 0. and abs(float(smooth.sum(dtype=np.float64)) - 1.) < 1e-5
    rotor = sim.compute_rotor_residence_time_map(radius=0.)
    assert np.isfinite(rotor).all() and rotor.min() >= 0. and abs(float(rotor.sum(dtype=np.float64)) - 1.) < 1e-6
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_rotor_residence_time.npy')), rotor)
    assert np.array_equal(sim.compute_presence_map(), plain.compute_presence_map())

    # without flight_height and without the pickle: the trajectories are still produced on the device, no zone outputs
    bare = Simulator(replace(cfg, run_name='bare', flight_height=False, save_tracks=False), terrain='synthetic')
    bare.simulate_tracks()
    names = os.listdir(bare.mode_data_dir)
    assert not [f for f in names if f.endswith('.pkl') or 'rotor' in f] and bare.rotor_residence_time_counts == {}
    for real_id in (0, 1):
        stem = f's10d270_d0_t75_fluidflow_r{real_id}'
        assert np.array_equal(np.load(os.path.join(bare.mode_data_dir, f'{stem}_residence_time.npy')),
                              np.load(os.path.join(sim.mode_data_dir, f'{stem}_residence_time.npy')))
        rows = np.load(os.path.join(bare.mode_data_dir, f'{stem}_flight_times.npy'))
        assert np.array_equal(rows[:, 0], sim.flight_times[('s10d270', real_id)][:, 0]) and not rows[:, 1].any()


def test_simulator_snapshot_mode_reads_the_case_wind(gpu, tmp_path):
    """Snapshot mode: the windinfo raster comes from the case's own per-cell wind (DEM-only terrain: 'row_east')."""
    from ssrs_amd import Config, Simulator, flight
    rng = np.random.default_rng(4)
    ws = rng.uniform(2., 14., (50, 60))
    wd = rng.uniform(200., 340., (50, 60))
    cfg = Config(run_name='snap', out_dir=str(tmp_path), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=32,
                 track_start_region=(1, 5, 0.2, 0.6), track_direction=0., sim_mode='snapshot',
                 snapshot_datetime=(2010, 6, 17, 13), flight_time=True, flight_airspeed=12., flight_min_groundspeed=2.)
    sim = Simulator(cfg, terrain='synthetic', wind=[dict(datetime=(2010, 6, 17, 13), wspeed=ws, wdirn=wd)])
    sim.simulate_tracks()
    case = sim.case_ids[0]
    stem = os.path.join(sim.mode_data_dir, sim._get_id_string(case, 0))
    with open(f'{stem}_tracks.pkl', 'rb') as f:
        tracks = pickle.load(f)
    info = flight.wind_cellinfo(ws, wd, 'row_east').cpu().numpy()
    assert len(np.unique(info[..., 0])) > 100
    want = ref.flight_times(tracks, info[..., 0], info[..., 1], (50, 60), (12_000, 2_000, 100_000))
    assert np.array_equal(np.load(f'{stem}_residence_time.npy').view(np.uint64), want['time_hist'])
    assert np.array_equal(np.load(f'{stem}_flight_times.npy'), want['times']) and want['times'][:, 0].sum() > 0
    assert not os.path.exists(f'{stem}_rotor_residence_time.npy')
