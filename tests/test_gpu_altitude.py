"""K14 on the device: ssrs_track_altitude / ssrs_altitude_cellinfo through ssrs_amd/flight.py on every case of
tests/altitude_ref.py (the cases tests/test_altitude_emulation.py runs on the CPU), the rotor-zone trajectories through
the encounter kernel, the chunked replay path, and Simulator(flight_height=True) end to end.  Every comparison is integer
equality; the one f32 summary map is checked for its range."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import altitude_ref as ref

pytestmark = pytest.mark.gpu


def metres(params):
    """The keyword arguments of flight.compute_track_altitudes for a case's millimetres (int(round(1000 x)) gives them
    back: |mm| < 2^31 is exact in f64 and 1000 * (mm / 1000) rounds to mm)."""
    start, floor, ceil, lo, hi = (v / 1000. for v in params)
    from ssrs_amd import flight
    p = flight.height_params(start, floor, ceil, (lo, hi))
    assert (p.start, p.floor, p.ceil, p.band_lo, p.band_hi) == tuple(params)
    return dict(start=start, floor=floor, ceil=ceil, band=(lo, hi))


def device_case(c, gpu):
    """(traj, offsets, cellinfo) of a case on the device: traj `shift` points (4 bytes each) past torch's alignment,
    in-raster points around it; offsets the slice [1:] of the longer vector."""
    traj, off = ref.flat(c)
    raw = torch.full((traj.shape[0] + 8, 2), 3, dtype=torch.int16, device=gpu)
    assert raw.data_ptr() % 16 == 0
    view = raw[c['shift']:c['shift'] + traj.shape[0]]
    view.copy_(torch.from_numpy(traj))
    assert view.shape[0] == 0 or view.data_ptr() % 16 == 4 * (c['shift'] % 4)
    return view, torch.from_numpy(off).to(gpu)[1:], torch.from_numpy(ref.packed(c)).to(gpu)


def outputs(out, lead):
    """flight's dict as altitude_ref.check takes it (the per-point outputs without the lead points)."""
    got = dict(band_hist=out['band_hist'], in_band=out['heights'][:, 0], h_min=out['heights'][:, 1], h_max=out['heights'][:, 2])
    if 'alt' in out:
        got['alt'] = out['alt'][lead:]
    if 'masked' in out:
        got['traj_band'] = out['masked'][lead:]
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_cases_on_the_device(gpu, c):
    from ssrs_amd import flight
    traj, off, info = device_case(c, gpu)
    assert int(off[0]) == c['lead']
    kw = metres(c['params'])
    out = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, want_alt=True, want_masked=True, **kw)
    assert all(v.is_cuda for v in out.values()) and out['band_hist'].dtype == torch.int32
    assert out['heights'].dtype == torch.int32 and tuple(out['heights'].shape) == (len(c['tracks']), 3)
    assert out['alt'].dtype == torch.int32 and out['masked'].dtype == torch.int16
    ref.check(c['name'], outputs(out, c['lead']))
    # what lies in front of the chunk's points is not written
    assert not bool(out['alt'][:c['lead']].any()) and bool((out['masked'][:c['lead']] == -1).all())
    # once more into the same raster, on a workspace of the caller's, without the per-point outputs: everything twice
    ws = flight.altitude_workspace(int(traj.shape[0]))
    again = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, band_hist=out['band_hist'], workspace=ws, **kw)
    assert again['band_hist'] is out['band_hist'] and set(again) == {'band_hist', 'heights'}
    assert np.array_equal(again['band_hist'].cpu().numpy().view(np.uint32), 2 * ref.expected(c['name'])['band_hist'])
    assert torch.equal(again['heights'], out['heights'])
    # each per-point output alone
    only_alt = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, want_alt=True, **kw)
    only_masked = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, want_masked=True, **kw)
    assert torch.equal(only_alt['alt'], out['alt']) and torch.equal(only_masked['masked'], out['masked'])
    assert 'masked' not in only_alt and 'alt' not in only_masked
    if c['lead'] == 0:
        # a list of host tracks gives numpy
        host = flight.compute_track_altitudes(c['tracks'], info, c['shape'], want_alt=True, want_masked=True, **kw)
        assert all(isinstance(v, np.ndarray) for v in host.values())
        ref.check(c['name'], outputs(host, 0))


def test_accumulation_over_disjoint_track_ranges(gpu):
    """Two calls into one band_hist on disjoint track ranges equal one call on the union, and what the raster held
    before is kept; a workspace that is too small is refused."""
    from ssrs_amd import flight
    c = ref.case('short_300')
    traj, off, info = device_case(c, gpu)
    kw = metres(c['params'])
    pattern = ((np.arange(ref.SHAPE[0] * ref.SHAPE[1], dtype=np.uint32).reshape(ref.SHAPE) * 2654435761) | 1).view(np.int32)
    acc = torch.from_numpy(pattern.copy()).to(gpu)
    first = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off[:121], band_hist=acc, **kw)
    second = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off[120:], band_hist=acc, **kw)
    rows = torch.cat([first['heights'], second['heights']]).cpu().numpy()
    ref.check(c['name'], dict(band_hist=acc.cpu().numpy(), in_band=rows[:, 0], h_min=rows[:, 1], h_max=rows[:, 2]),
              before=pattern)
    long = ref.case('lengths')
    traj, off, info = device_case(long, gpu)
    with pytest.raises(ValueError, match='workspace'):
        flight.compute_track_altitudes(traj, info, long['shape'], offsets=off, **metres(long['params']),
                                       workspace=flight.altitude_workspace(0)[:255])     # (256 bytes serve 8 tiles)


@pytest.mark.parametrize('dtypes', [(np.float32, np.float64), (np.float64, np.float32)], ids=['f32-f64', 'f64-f32'])
def test_cellinfo_on_the_device(gpu, dtypes):
    """ssrs_altitude_cellinfo against numpy: NaN updraft, NaN elevation, exact .5 ties, values that clip, infinities; numpy
    and tensor inputs."""
    from ssrs_amd import flight
    rows, cols = 37, 301                                  # more than one block, no multiple of it
    rng = np.random.default_rng(3)
    w = rng.normal(0.5, 2., (rows, cols))
    z = rng.uniform(-50., 3000., (rows, cols))
    resolution, airspeed, sink = 100., 16., 0.75           # scale = 6250
    w[0, :6] = sink + np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5]) / 6250.
    w[1, :5] = (np.nan, 1e9, -1e9, np.inf, -np.inf)
    w[2, :3] = (sink + 2. ** 26 / 6250., sink - 2. ** 26 / 6250., sink + (2. ** 26 - 1) / 6250.)
    z[3, :6] = (0.0005, 0.0015, 0.0025, -0.0005, -0.0015, 1234.5675)
    z[4, :5] = (np.nan, 2e6, -2e6, np.inf, -np.inf)
    z[-1, -1], w[-1, -1] = np.nan, np.nan
    w, z = w.astype(dtypes[0]), z.astype(dtypes[1])
    climb, elev = ref.cellinfo(w, z, resolution, airspeed, sink)
    out = flight.altitude_cellinfo(w, z, resolution, airspeed, sink)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (rows, cols, 2)
    got = out.cpu().numpy()
    assert np.array_equal(got[..., 0], climb) and np.array_equal(got[..., 1], elev)
    again = flight.altitude_cellinfo(torch.from_numpy(w).to(gpu), torch.from_numpy(z).to(gpu), resolution, airspeed, sink)
    assert torch.equal(again, out)


def test_all_holding_band_is_the_visit_histogram(gpu):
    from ssrs_amd import flight, presence
    c = ref.case('band_all')
    traj, off, info = device_case(c, gpu)
    out = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, want_masked=True, **metres(c['params']))
    assert torch.equal(out['band_hist'], presence.compute_presence_counts(traj, c['shape']))
    assert torch.equal(out['masked'], traj) and int(out['heights'][:, 0].sum()) == int(traj.shape[0])


def test_rotor_height_encounters(gpu):
    """turbines.turbine_encounters on traj_band equals the brute-force encounters of the oracle's rotor-zone points, and
    they are a subset of the 2-D ones."""
    from ssrs_amd import flight
    from ssrs_amd import turbines as tb
    from test_gpu_turbines import brute_force
    c = ref.case('nodata')
    traj, off, info = device_case(c, gpu)
    out = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, want_masked=True, **metres(c['params']))
    rng = np.random.default_rng(5)
    xy = np.stack([rng.uniform(0., ref.SHAPE[1] - 1., 40), rng.uniform(0., ref.SHAPE[0] - 1., 40)], 1)
    radius = 1.5
    flat_hits, flat_first = tb.turbine_encounters(traj, off, xy, radius, c['shape'])
    band_hits, band_first = tb.turbine_encounters(out['masked'], off, xy, radius, c['shape'])
    host_off = off.cpu().numpy()
    want_hits, per_turbine, _, want_first = brute_force(ref.expected(c['name'])['traj_band'], host_off - host_off[0], xy, radius)
    assert np.array_equal(band_hits.cpu().numpy().view(np.uint32), want_hits)
    assert np.array_equal(band_first.cpu().numpy(), want_first)
    assert not bool((band_hits & ~flat_hits).any())
    assert 0 < per_turbine.sum() < int(tb.encounter_counts(flat_hits, 40)[0].sum())      # the zone does thin them out


def test_replay_chunks_accumulate(gpu):
    """The smoke inputs with a budget too small for one trajectory tensor: iter_device_chunks() hands over the replay
    ranges, and the rotor raster and the per-track rows gathered chunk by chunk equal those of the run that holds its
    tensor, and the oracle's."""
    from ssrs_amd import flight, layers, movmodel
    from ssrs_amd.synthetic import synthetic_dem
    from oracle import ssrs_oracle as orc
    rows, cols, res = 96, 128, 100.
    dem = synthetic_dem((rows, cols), res)
    oro, _ = layers.updraft_from_dem(dem, res, 10., 270., threshold=0.75)
    upd = orc.get_above_threshold_speed(oro, 0.75)
    pot = orc.solve_potential(upd, 0.)
    rng = np.random.default_rng(0)
    starts = np.stack([rng.integers(1, 12, 256), rng.integers(0, cols, 256)], 1)
    whole = movmodel.simulate_tracks(0., starts, (rows, cols), 1, 1., upd, pot, seed=30, want_tracks=True,
                                     traj_budget_bytes=1 << 30)
    assert whole.traj is not None
    ranged = movmodel.simulate_tracks(0., starts, (rows, cols), 1, 1., upd, pot, seed=30, want_tracks=True,
                                      record_pool_bytes=4096, traj_budget_bytes=8 * 1024)
    assert ranged.traj is None
    info = flight.altitude_cellinfo(oro, dem, res, 15., 0.75)
    kw = dict(start=100., floor=10., ceil=1000., band=(30., 150.))
    acc = torch.zeros((rows, cols), dtype=torch.int32, device=gpu)
    parts, nchunks = [], 0
    for t0, t1, traj, off in ranged.iter_device_chunks():
        parts.append(flight.compute_track_altitudes(traj, info, (rows, cols), offsets=off, band_hist=acc, **kw)['heights'])
        nchunks += 1
    assert nchunks >= 3
    one = flight.compute_track_altitudes(whole.traj, info, (rows, cols), offsets=whole.offsets, **kw)
    assert torch.equal(acc, one['band_hist']) and torch.equal(torch.cat(parts), one['heights'])
    climb, elev = ref.cellinfo(np.asarray(oro), dem, res, 15., 0.75)
    want = ref.altitude(whole.tracks(), climb, elev, (rows, cols), ref.DEFAULT)
    assert np.array_equal(one['band_hist'].cpu().numpy().view(np.uint32), want['band_hist'])
    assert np.array_equal(one['heights'].cpu().numpy(), np.stack([want['in_band'], want['h_min'], want['h_max']], 1))


def _turbines():
    # 50 x 60 cells at 100 m from (0, 0); the tracks start in rows 2 .. 6 and head north
    return dict(x=[1500., 2550., 3000., 4000., 4500.], y=[700., 900., 1500., 800., 1250.], p_name=['A'] * 5,
                t_hh=[80.] * 5, t_rd=[100.] * 5)


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Config, Simulator
    from test_gpu_turbines import brute_force, _pack
    cfg = Config(run_name='fly', out_dir=str(tmp_path), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=64,
                 track_start_region=(1, 5, 0.2, 0.6), track_direction=0., thermals_realization_count=1,
                 turbine_encounter_radius=150., flight_height=True)
    sim = Simulator(cfg, terrain='synthetic', turbines=_turbines())
    with pytest.raises(ValueError, match='flight_height=True'):
        sim.compute_rotor_presence_map()
    sim.simulate_tracks()
    plain = Simulator(replace(cfg, run_name='plain', flight_height=False), terrain='synthetic', turbines=_turbines())
    plain.simulate_tracks()
    assert plain.rotor_presence_counts == {} and plain.flight_heights == {} and plain.rotor_turbine_encounters == {}
    assert not [f for f in os.listdir(plain.mode_data_dir) if 'rotor' in f or 'flight' in f]

    orograph = np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy'))
    fields = [orograph, orograph + np.load(os.path.join(sim.mode_data_dir, 's10d270_r0_thermals.npy'))]
    assert fields[1].dtype == np.float32
    xy = sim.turbines.cell_coordinates(sim.bounds, 100.)
    for real_id, field in enumerate(fields):
        key = ('s10d270', real_id)
        stem = f's10d270_d0_t75_fluidflow_r{real_id}'
        path = lambda name, d=sim.mode_data_dir: os.path.join(d, f'{stem}_{name}')
        with open(path('tracks.pkl'), 'rb') as f:
            tracks = pickle.load(f)
        assert len(tracks) == 64
        climb, elev = ref.cellinfo(field, sim.get_terrain_elevation(), 100., 15., 0.75)      # sink: updraft_threshold
        want = ref.altitude(tracks, climb, elev, (50, 60), ref.DEFAULT)
        raster = np.load(path('rotor_presence.npy'))
        assert raster.dtype == np.int32 and np.array_equal(raster.view(np.uint32), want['band_hist'])
        assert np.array_equal(sim.rotor_presence_counts[key], raster)
        rows = np.load(path('flight_heights.npy'))
        assert rows.dtype == np.int32 and rows.shape == (64, 3)
        assert np.array_equal(rows, np.stack([want['in_band'], want['h_min'], want['h_max']], 1))
        assert np.array_equal(sim.flight_heights[key], rows)
        assert int(raster.view(np.uint32).sum(dtype=np.int64)) == int(rows[:, 0].sum(dtype=np.int64)) > 0
        # the encounters at rotor height: the oracle's, and a subset of the 2-D ones
        traj, off = _pack(tracks)
        _, per_turbine, per_track, first = brute_force(want['traj_band'], off, xy, 1.5)
        enc = sim.rotor_turbine_encounters[key]
        assert np.array_equal(enc['tracks_per_turbine'], per_turbine) and enc['tracks_per_turbine'].dtype == np.int64
        assert np.array_equal(enc['turbines_per_track'], per_track) and np.array_equal(enc['first_step'], first)
        assert np.array_equal(np.load(path('rotor_turbine_encounters.npy')), per_turbine)
        flat = sim.turbine_encounters[key]
        assert (enc['tracks_per_turbine'] <= flat['tracks_per_turbine']).all()
        assert (enc['turbines_per_track'] <= flat['turbines_per_track']).all()
        # the 2-D outputs are those of the run without flight_height, byte for byte
        assert torch.equal(sim._presence_counts[key], plain._presence_counts[key])
        other = lambda name: path(name, plain.mode_data_dir)
        for name in ('tracks.pkl', 'turbine_encounters.npy'):
            with open(path(name), 'rb') as a, open(other(name), 'rb') as b:
                assert a.read() == b.read(), name
        for name in ('tracks_per_turbine', 'turbines_per_track', 'first_step'):
            assert np.array_equal(flat[name], plain.turbine_encounters[key][name]), name
    summary = sim.compute_rotor_presence_map()
    assert summary.dtype == np.float32 and summary.shape == (50, 60) and np.isfinite(summary).all()
    assert summary.min() >= 0. and summary.max() <= 1. and summary.max() > 0.
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_rotor_presence.npy')), summary)
    assert np.array_equal(sim.compute_presence_map(), plain.compute_presence_map())

    # an item without a point in the zone contributes zeros, and a run of such items is a map of zeros
    sim.rotor_presence_counts[('s10d270', 1)] = np.zeros((50, 60), dtype=np.int32)
    one = sim.compute_rotor_presence_map()
    assert np.isfinite(one).all() and one.max() == 1. and one.min() >= 0.
    sim.rotor_presence_counts[('s10d270', 0)] = np.zeros((50, 60), dtype=np.int32)
    none = sim.compute_rotor_presence_map()
    assert none.dtype == np.float32 and not none.any()

    # without the pickle: the trajectories are still produced on the device, the results are the same
    quiet = Simulator(replace(cfg, run_name='quiet', save_tracks=False, turbine_encounter_radius=0.), terrain='synthetic')
    quiet.simulate_tracks()
    assert not [f for f in os.listdir(quiet.mode_data_dir) if f.endswith('.pkl') or 'turbine' in f]
    assert quiet.rotor_turbine_encounters == {}
    for real_id in (0, 1):
        stem = f's10d270_d0_t75_fluidflow_r{real_id}'
        for name in ('rotor_presence.npy', 'flight_heights.npy'):
            assert np.array_equal(np.load(os.path.join(quiet.mode_data_dir, f'{stem}_{name}')),
                                  np.load(os.path.join(sim.mode_data_dir, f'{stem}_{name}'))), name
