"""K15's timed form on the device: ssrs_rotor_encounters_timed through ssrs_amd/turbines.py on every case of
tests/rotor_ref.py against the restatement of tests/rotor_time_ref.py, accumulation over calls, the trapped track, either side
of the LDS rule's boundary, the dt of K16 fed straight in, the chunked replay path, and
Simulator(rotor_exposure_time=True) end to end.  Every comparison is integer equality."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import altitude_ref as alt_ref
import flight_time_ref as ft_ref
import rotor_ref
import rotor_time_ref as ref
from test_gpu_rotor_encounters import check, shifted

pytestmark = pytest.mark.gpu

POISON_DT = 1_777_777_777       # around the shifted dt: a load outside the buffer's points would show


def device_case(c, gpu, pattern='random'):
    """(traj, alt, dt, offsets, cellinfo) of a case on the device: traj, alt and dt `shift` points past a 16-byte boundary
    with in-cylinder points, their height and a large dt around them; offsets the slice [1:] of the longer vector."""
    traj, alt, off = rotor_ref.flat(c)
    dt = np.array(ref.expected(c['name'], pattern)[0])          # (a writable copy for torch.from_numpy)
    return (shifted(traj, c['shift'], gpu, 20), shifted(alt, c['shift'], gpu, 50_000), shifted(dt, c['shift'], gpu, POISON_DT),
            torch.from_numpy(off).to(gpu)[1:], torch.from_numpy(rotor_ref.packed(c['elev'])).to(gpu))


def same(timed, untimed):
    """hits, first_step and points of a timed call are the untimed call's, bit for bit."""
    for a, b in zip(timed[:3], untimed):
        assert (a is None and b is None) or torch.equal(a, b)


def time_is(got, want):
    assert got.dtype == torch.int64 and got.is_cuda
    g = got.cpu().numpy()
    assert np.array_equal(g, want), (np.flatnonzero(g != want)[:8], g[g != want][:8], want[g != want][:8])


@pytest.mark.parametrize('c', rotor_ref.CASES, ids=rotor_ref.CASE_IDS)
def test_cases_on_the_device(gpu, c):
    from ssrs_amd import turbines as tb
    traj, alt, dt, off, info = device_case(c, gpu)
    assert int(off[0]) == c['lead'] and dt.data_ptr() % 16 == 4 * (c['shift'] % 4)
    args = (info, c['xy'], c['reach'], c['zband'], c['shape'])
    want = rotor_ref.expected(c['name'])
    want_time = ref.expected(c['name'])[1]
    untimed = tb.rotor_encounters(traj, alt, off, *args)
    got = tb.rotor_encounters(traj, alt, off, *args, dt=dt)
    assert len(got) == 4
    time_is(got[3], want_time)
    same(got, untimed)
    check(got[:3], want, rotor_ref.NTURB)
    assert (want_time[[0, 1, 2, 3, 4, 9, 10, 11, 12, 31, 32, 63, 64]] > 0).all() and not want_time[5:9].any()
    if 'loiter' in c['name']:
        assert int(want_time[0]) > 4097 * ref.CAP and int(want_time[1]) >= 4097 * ref.CAP
    # each combination of the optional outputs: the time does not depend on them, nor they on the time
    for kw in (dict(points=False), dict(first_step=False), dict(first_step=False, points=False)):
        other = tb.rotor_encounters(traj, alt, off, *args, dt=dt, **kw)
        time_is(other[3], want_time)
        same(other, tb.rotor_encounters(traj, alt, off, *args, **kw))
        check(other[:3], want, rotor_ref.NTURB)
    # cull lists of the caller's, numpy or device tensors
    bins = tb.build_bins(c['xy'], c['reach'], c['shape'])
    for given in (bins, tuple(torch.from_numpy(b).to(gpu) for b in bins)):
        other = tb.rotor_encounters(traj, alt, off, *args, bins=given, dt=dt)
        time_is(other[3], want_time)
        same(other, untimed)
    # points counted without time, and one negative dt added as it stands
    for pattern in ('zeros', 'negative'):
        dt_p = device_case(c, gpu, pattern)[2]
        other = tb.rotor_encounters(traj, alt, off, *args, dt=dt_p)
        time_is(other[3], ref.expected(c['name'], pattern)[1])
        same(other, untimed)
    assert not np.array_equal(ref.expected(c['name'], 'zeros')[1], want_time)
    assert int(ref.expected(c['name'], 'negative')[1][0]) == int(want_time[0]) - int(ref.expected(c['name'])[0][c['lead'] + sum(
        rotor_ref.LENGTHS[:10]) + 100]) - 123_456_789


def test_accumulation_over_disjoint_track_ranges(gpu):
    """Two calls on disjoint track ranges into one time vector seeded with 2^32 - 3 equal one call on the union; a second call
    over the same tracks doubles the time and the points and nothing else."""
    from ssrs_amd import turbines as tb
    c = rotor_ref.case('lead_5_shift_1')
    traj, alt, dt, off, info = device_case(c, gpu)
    want = rotor_ref.expected(c['name'])
    want_time = ref.expected(c['name'])[1]
    n = len(rotor_ref.LENGTHS)
    seed = 2 ** 32 - 3
    args = (info, c['xy'], c['reach'], c['zband'], c['shape'])
    for k in (9, 11, 150):                         # inside the long tracks; inside the run of short ones
        hits = torch.zeros((n, 3), dtype=torch.int32, device=gpu)
        first = torch.full((n,), -1, dtype=torch.int32, device=gpu)
        points = torch.full((rotor_ref.NTURB,), seed, dtype=torch.int64, device=gpu)
        time = torch.full((rotor_ref.NTURB,), seed, dtype=torch.int64, device=gpu)
        tb.rotor_encounters(traj, alt, off[:k + 1], *args, hits=hits[:k], first_step=first[:k], points=points, dt=dt, time=time)
        out = tb.rotor_encounters(traj, alt, off[k:], *args, hits=hits[k:], first_step=first[k:], points=points, dt=dt, time=time)
        assert out[2] is points and out[3] is time
        time_is(time, want_time + seed)
        check((hits, first, points - seed), want, rotor_ref.NTURB)
    again = tb.rotor_encounters(traj, alt, off, *args, hits=hits, first_step=first, points=points - seed, dt=dt, time=time - seed)
    check((again[0], again[1], None), want, rotor_ref.NTURB)
    assert np.array_equal(again[2].cpu().numpy(), 2 * want['points'])
    time_is(again[3], 2 * want_time)


def test_a_track_trapped_inside_a_cylinder(gpu):
    """The 200 000 points of the untimed test that alternate between two cells inside two cylinders and at the edge of a
    third, every dt 2^31 - 1: a sum of 4.3e14 microseconds counted in full."""
    from ssrs_amd import turbines as tb
    rng = np.random.default_rng(4)
    trap = np.empty((200_000, 2), dtype=np.int16)
    trap[0::2], trap[1::2] = (20, 30), (20, 31)
    tracks = [rotor_ref.walk(rng, 3) for _ in range(5)] + [trap] + [rotor_ref.walk(rng, 3, start=(21, 31))] + \
        [rotor_ref.walk(rng, 3) for _ in range(5)]
    traj = np.concatenate(tracks)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    alt = np.tile(np.array([80_000, 80_001, 80_002], dtype=np.int32), traj.shape[0] // 3 + 1)[:traj.shape[0]]
    dt = np.full(traj.shape[0], ref.CAP, dtype=np.int32)
    elev = np.full(rotor_ref.SHAPE, 1000, dtype=np.int32)
    xy = np.array([[30., 20.], [31.5, 20.5], [29., 20.], [60., 60.]])
    reach = np.array([2.5, 2.5, 1., 3.])
    zband = np.array([rotor_ref.WIDE, (81_000, 81_001), rotor_ref.WIDE, rotor_ref.WIDE], dtype=np.int32)
    want = rotor_ref.brute_force(traj, alt, off, elev, xy, reach, zband, rotor_ref.SHAPE)
    want_time = ref.time_per_turbine(rotor_ref.inside_matrix(traj, alt, elev, xy, reach, zband, rotor_ref.SHAPE), dt)
    assert np.array_equal(want_time, want['points'] * ref.CAP) and int(want_time[0]) >= 200_000 * ref.CAP > 4.29e14
    dev = [torch.from_numpy(a).to(gpu) for a in (traj, alt, off, rotor_ref.packed(elev))]
    got = tb.rotor_encounters(dev[0], dev[1], dev[2], dev[3], xy, reach, zband, rotor_ref.SHAPE, dt=torch.from_numpy(dt).to(gpu))
    time_is(got[3], want_time)
    check(got[:3], want, 4)


def test_either_side_of_the_lds_boundary(gpu):
    """Up to SSRS_ROTOR_TIMED_LDS_TURBINES turbines every counter of a block is in LDS (half as many again without the point
    counters); beyond, the highest turbines' time goes to global adds.  The largest count inside, one more, and
    SSRS_TURBINE_MAX, on 2 000 points that hit hundreds of cylinders -- the last three of every count among them."""
    from ssrs_amd import _native
    from ssrs_amd import turbines as tb
    edge, most = _native.SSRS_ROTOR_TIMED_LDS_TURBINES, _native.SSRS_TURBINE_MAX
    assert edge + 1 < edge * 3 // 2 + 1 < most
    rng = np.random.default_rng(17)
    shape = rotor_ref.SHAPE
    tracks = [rotor_ref.walk(rng, n) for n in (700, 1, 0, 300, 64, 257, 5, 5, 5, 600)]
    traj = np.concatenate(tracks)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    assert traj.shape[0] <= 2000
    alt = rng.integers(10_000, 300_000, traj.shape[0]).astype(np.int32)
    dt = rng.integers(0, ref.CAP + 1, traj.shape[0]).astype(np.int32)
    elev = np.full(shape, 5000, dtype=np.int32)
    xy, reach, zband = rotor_ref.random_turbines(rng, shape, most, 0, 600_000)
    # the last three stand on points of the first, fourth and last track, at every height
    for k, at in enumerate((350, int(off[3]) + 150, int(off[9]) + 300)):
        xy[most - 3 + k], reach[most - 3 + k], zband[most - 3 + k] = traj[at][::-1].astype(np.float64), 2., rotor_ref.WIDE
    inside = rotor_ref.inside_matrix(traj, alt, elev, xy, reach, zband, shape)
    dev = [torch.from_numpy(a).to(gpu) for a in (traj, alt, off, rotor_ref.packed(elev))]
    dt_dev = torch.from_numpy(dt).to(gpu)
    for nturb, kw in ((edge, {}), (edge + 1, {}), (most, {}), (edge * 3 // 2, dict(points=False)),
                      (edge * 3 // 2 + 1, dict(points=False))):
        sel = np.concatenate([np.arange(nturb - 3), np.arange(most - 3, most)])
        want_time = ref.time_per_turbine(inside[:, sel], dt)
        want_points = inside[:, sel].sum(0).astype(np.int64)
        assert (want_time > 0).sum() >= 300 and (want_time[-3:] > 0).all(), nturb
        args = (dev[0], dev[1], dev[2], dev[3], xy[sel], reach[sel], zband[sel], shape)
        got = tb.rotor_encounters(*args, dt=dt_dev, **kw)
        time_is(got[3], want_time)
        same(got, tb.rotor_encounters(*args, **kw))
        if not kw:
            assert np.array_equal(got[2].cpu().numpy(), want_points)


def _wind(shape, seed):
    """(wr, wc) int32 rasters of a random wind, NaN cells and stalls included, and the packed raster the library reads."""
    rng = np.random.default_rng(seed)
    ws, wd = rng.uniform(0., 26., shape), rng.uniform(0., 360., shape)
    ws[rng.random(shape) < 0.05] = np.nan
    wr, wc = ft_ref.windinfo(ws, wd)
    return wr, wc, np.ascontiguousarray(np.stack([wr, wc], -1), dtype=np.int32)


@pytest.mark.parametrize('c', alt_ref.CASES, ids=alt_ref.CASE_IDS)
def test_alt_of_k14_and_dt_of_k16_fed_straight_in(gpu, c):
    """alt of flight.compute_track_altitudes and dt of flight.compute_track_times, as they leave the device, into the timed
    rotor kernel: the restatement over the two oracles' own heights and times."""
    from ssrs_amd import flight
    from ssrs_amd import turbines as tb
    from test_gpu_altitude import device_case as altitude_case, metres
    from test_gpu_flight_time import scalars
    traj, off, info = altitude_case(c, gpu)
    wr, wc, wind = _wind(c['shape'], 5)
    out = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, want_alt=True, want_masked=True,
                                         **metres(c['params']))
    spent = flight.compute_track_times(traj, c['shape'], offsets=off, wind=torch.from_numpy(wind).to(gpu), masked=out['masked'],
                                       want_dt=True, **scalars(ft_ref.DEFAULT))
    rng = np.random.default_rng(7)
    xy, reach, zband = rotor_ref.random_turbines(rng, c['shape'], 40, 0, 900_000)
    zband[:2] = rotor_ref.WIDE
    got = tb.rotor_encounters(traj, out['alt'], off, info, xy, reach, zband, c['shape'], dt=spent['dt'])
    same(got, tb.rotor_encounters(traj, out['alt'], off, info, xy, reach, zband, c['shape']))
    host_traj, host_off = alt_ref.flat(c)
    lead = c['lead']
    heights = alt_ref.expected(c['name'])['alt']
    times = ft_ref.flight_times(c['tracks'], wr, wc, c['shape'], ft_ref.DEFAULT)['dt']
    assert np.array_equal(spent['dt'][lead:].cpu().numpy(), times)
    inside = rotor_ref.inside_matrix(host_traj[lead:], heights, c['elev'], xy, reach, zband, c['shape'])
    want_time = ref.time_per_turbine(inside, times)
    time_is(got[3], want_time)
    assert np.array_equal(got[2].cpu().numpy(), inside.sum(0))
    assert bool(want_time.sum() > 0) == (c['name'] not in ('all_empty', 'beyond_int32'))


def test_replay_chunks_accumulate(gpu):
    """The smoke inputs with a budget too small for one trajectory tensor: every replay range through K14, K16 and the timed
    K15 into one time vector gives the integers of the run that holds its tensor, and the restatement's."""
    from ssrs_amd import flight, layers, movmodel
    from ssrs_amd import turbines as tb
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
    tkw = dict(resolution=res, airspeed=15., min_groundspeed=1., wind=(10., 270.))
    climb, elev = alt_ref.cellinfo(np.asarray(oro), dem, res, 15., 0.75)
    xy, reach, _ = rotor_ref.random_turbines(rng, (rows, cols), 40, 0, 1)
    zband = np.stack([elev[rng.integers(0, rows, 40), rng.integers(0, cols, 40)] + 20_000] * 2, 1).astype(np.int32)
    zband[:, 1] += rng.integers(50_000, 300_000, 40).astype(np.int32)
    bins = tuple(torch.from_numpy(b).to(gpu) for b in tb.build_bins(xy, reach, (rows, cols)))
    hits = torch.zeros((256, 2), dtype=torch.int32, device=gpu)
    first = torch.full((256,), -1, dtype=torch.int32, device=gpu)
    points = torch.zeros(40, dtype=torch.int64, device=gpu)
    time = torch.zeros(40, dtype=torch.int64, device=gpu)
    nchunks = 0
    for t0, t1, traj, off in ranged.iter_device_chunks():
        out = flight.compute_track_altitudes(traj, info, (rows, cols), offsets=off, want_alt=True, want_masked=True, **kw)
        spent = flight.compute_track_times(traj, (rows, cols), offsets=off, masked=out['masked'], want_dt=True, **tkw)
        tb.rotor_encounters(traj, out['alt'], off, info, xy, reach, zband, (rows, cols), bins=bins, hits=hits[t0:t1],
                            first_step=first[t0:t1], points=points, dt=spent['dt'], time=time)
        nchunks += 1
    assert nchunks >= 3
    one = flight.compute_track_altitudes(whole.traj, info, (rows, cols), offsets=whole.offsets, want_alt=True, **kw)
    one_dt = flight.compute_track_times(whole.traj, (rows, cols), offsets=whole.offsets, want_dt=True, **tkw)['dt']
    got = tb.rotor_encounters(whole.traj, one['alt'], whole.offsets, info, xy, reach, zband, (rows, cols), dt=one_dt)
    assert torch.equal(hits, got[0]) and torch.equal(first, got[1]) and torch.equal(points, got[2]) and torch.equal(time, got[3])
    same(got, tb.rotor_encounters(whole.traj, one['alt'], whole.offsets, info, xy, reach, zband, (rows, cols)))
    tracks = whole.tracks()
    heights = alt_ref.altitude(tracks, climb, elev, (rows, cols), alt_ref.DEFAULT)['alt']
    pair = flight.wind_pair(10., 270., 'row_east')
    wr, wc = (np.full((rows, cols), v, dtype=np.int32) for v in pair)
    times = ft_ref.flight_times(tracks, wr, wc, (rows, cols), (15_000, 1_000, 100_000))['dt']
    inside = rotor_ref.inside_matrix(whole.traj.cpu().numpy(), heights, elev, xy, reach, zband, (rows, cols))
    want_time = ref.time_per_turbine(inside, times)
    time_is(got[3], want_time)
    assert (want_time > 0).sum() >= 2 and np.array_equal(got[2].cpu().numpy(), inside.sum(0))


def test_argument_errors(gpu):
    from ssrs_amd import turbines as tb
    c = rotor_ref.case('planted')
    traj, alt, dt, off, info = device_case(c, gpu)
    args = dict(traj=traj, alt=alt, offsets=off, cellinfo=info, xy_cells=c['xy'], reach=c['reach'], zband=c['zband'],
                gridshape=c['shape'], dt=dt)
    n = rotor_ref.NTURB
    for bad, match in ((dict(dt=dt[:-1]), 'indexed like traj'), (dict(dt=dt.to(torch.int64)), 'indexed like traj'),
                       (dict(time=torch.zeros(n, dtype=torch.int32, device=gpu)), 'time'),
                       (dict(time=torch.zeros(n + 1, dtype=torch.int64, device=gpu)), 'time'),
                       (dict(time=torch.zeros(n, dtype=torch.int64)), 'time'),
                       (dict(dt=None, time=torch.zeros(n, dtype=torch.int64, device=gpu)), 'time'),
                       (dict(alt=alt[:-1]), 'indexed like traj'), (dict(points=torch.zeros(n, dtype=torch.int32, device=gpu)), 'points')):
        with pytest.raises(ValueError, match=match):
            tb.rotor_encounters(**{**args, **bad})
    # no tracks, and no cylinder that reaches the raster: the 4-tuple, untouched
    seeded = torch.full((n,), 5, dtype=torch.int64, device=gpu)
    none = tb.rotor_encounters(**{**args, 'offsets': off[:1], 'time': seeded})
    assert len(none) == 4 and tuple(none[0].shape) == (0, 3) and none[3] is seeded and bool((seeded == 5).all())
    far = tb.rotor_encounters(**{**args, 'xy_cells': c['xy'] + 1e6})
    assert len(far) == 4 and not far[0].any() and not far[2].any() and not far[3].any() and far[3].dtype == torch.int64
    # without dt the call and its 3-tuple are what they were
    assert len(tb.rotor_encounters(**{**args, 'dt': None})) == 3


def _turbines():
    # the five turbines of the K15 test: 50 x 60 cells at 100 m from (0, 0); the tracks start in rows 2 .. 6 and head north
    return dict(x=[1500., 2550., 3000., 4000., 4500.], y=[700., 900., 1500., 800., 1250.], p_name=['A'] * 5,
                t_hh=[80., 90., 100., 110., 80.], t_rd=[100., 110., 120., 90., 130.])


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Config, Simulator, flight
    from ssrs_amd import turbines as tb
    from test_gpu_turbines import _pack
    cfg = Config(run_name='off', out_dir=str(tmp_path), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=64,
                 track_start_region=(1, 5, 0.2, 0.6), track_direction=0., thermals_realization_count=1,
                 flight_height=True, rotor_geometry='turbine', rotor_clearance=100., flight_time=True)
    off = Simulator(cfg, terrain='synthetic', turbines=_turbines())
    off.simulate_tracks()
    with pytest.raises(ValueError, match='no rotor exposure time'):
        off.compute_turbine_rotor_time()
    sim = Simulator(replace(cfg, run_name='on', rotor_exposure_time=True), terrain='synthetic', turbines=_turbines())
    with pytest.raises(ValueError, match='no rotor exposure time'):
        sim.compute_turbine_rotor_time()
    sim.simulate_tracks()

    # the option off writes what it wrote before the option existed; on, the same files byte for byte plus its own
    stems = [f's10d270_d0_t75_fluidflow_r{k}' for k in (0, 1)]
    names = set(os.listdir(off.mode_data_dir))
    assert {f'{s}_turbine_rotor_encounters.npy' for s in stems} | {f'{s}_flight_times.npy' for s in stems} <= names
    assert not [f for f in names if 'rotor_time' in f]
    assert set(os.listdir(sim.mode_data_dir)) == names | {f'{s}_turbine_rotor_time.npy' for s in stems}
    for name in names:
        with open(os.path.join(sim.mode_data_dir, name), 'rb') as a, open(os.path.join(off.mode_data_dir, name), 'rb') as b:
            assert a.read() == b.read(), name

    dem = sim.get_terrain_elevation()
    xy = sim.turbines.cell_coordinates(sim.bounds, 100.)
    reach, zband = tb.rotor_geometry(sim.turbines, dem, sim.bounds, 100., clearance=100.)
    orograph = np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy'))
    fields = [orograph, orograph + np.load(os.path.join(sim.mode_data_dir, 's10d270_r0_thermals.npy'))]
    pair = flight.wind_pair(10., 270., 'row_east')         # DEM-only terrain
    wr, wc = (np.full((50, 60), v, dtype=np.int32) for v in pair)
    seconds = []
    for real_id, field in enumerate(fields):
        key = ('s10d270', real_id)
        path = lambda name: os.path.join(sim.mode_data_dir, f'{stems[real_id]}_{name}')
        with open(path('tracks.pkl'), 'rb') as f:
            tracks = pickle.load(f)
        assert len(tracks) == 64
        climb, elev = alt_ref.cellinfo(field, dem, 100., 15., 0.75)
        heights = alt_ref.altitude(tracks, climb, elev, (50, 60), alt_ref.DEFAULT)['alt']
        times = ft_ref.flight_times(tracks, wr, wc, (50, 60), (15_000, 1_000, 100_000))['dt']
        traj, _ = _pack(tracks)
        inside = rotor_ref.inside_matrix(traj, heights, elev, xy, reach, zband, (50, 60))
        want_time = ref.time_per_turbine(inside, times)
        assert (want_time > 0).sum() >= 2
        saved = np.load(path('turbine_rotor_time.npy'))
        assert saved.dtype == np.int64 and saved.shape == (5,) and np.array_equal(saved, want_time)
        both = np.load(path('turbine_rotor_encounters.npy'))
        assert both.shape == (5, 2) and np.array_equal(both[:, 1], inside.sum(0))
        enc = sim.turbine_rotor_encounters[key]
        assert enc['time_per_turbine'].dtype == np.int64 and np.array_equal(enc['time_per_turbine'], saved)
        assert 'time_per_turbine' not in off.turbine_rotor_encounters[key]
        for name in ('tracks_per_turbine', 'points_per_turbine', 'turbines_per_track', 'first_step'):
            assert np.array_equal(enc[name], off.turbine_rotor_encounters[key][name]), name
        # the invariant Simulator raises on
        assert (saved <= both[:, 1] * ref.CAP).all() and not saved[both[:, 1] == 0].any()
        seconds.append(saved / 1e6 / 64.)
    summary = sim.compute_turbine_rotor_time()
    assert summary.dtype == np.float64 and summary.shape == (5,) and (summary > 0.).sum() >= 2
    assert np.array_equal(summary, (seconds[0] + seconds[1]) / 2.)
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_turbine_rotor_time.npy')), summary)
    assert np.array_equal(sim.compute_turbine_rotor_encounters(), off.compute_turbine_rotor_encounters())

    # without the pickle: the same integers
    bare = Simulator(replace(cfg, run_name='bare', rotor_exposure_time=True, save_tracks=False), terrain='synthetic',
                     turbines=_turbines())
    bare.simulate_tracks()
    assert not [f for f in os.listdir(bare.mode_data_dir) if f.endswith('.pkl')]
    for real_id in (0, 1):
        key = ('s10d270', real_id)
        for name in ('tracks_per_turbine', 'points_per_turbine', 'time_per_turbine', 'turbines_per_track', 'first_step'):
            assert np.array_equal(bare.turbine_rotor_encounters[key][name], sim.turbine_rotor_encounters[key][name]), name
        for name in ('turbine_rotor_time.npy', 'turbine_rotor_encounters.npy', 'flight_times.npy', 'rotor_residence_time.npy'):
            assert np.array_equal(np.load(os.path.join(bare.mode_data_dir, f'{stems[real_id]}_{name}')),
                                  np.load(os.path.join(sim.mode_data_dir, f'{stems[real_id]}_{name}'))), name

    # the invariant the heights' store raises on through its cylinders (last: it overwrites this run's files): time without
    # points, and more time than the points' dt can hold
    from types import SimpleNamespace
    from ssrs_amd.products import Heights
    heights = Heights(bare)

    def fly(points, time):
        rotor = SimpleNamespace(hits=torch.zeros((64, 1), dtype=torch.int32, device=gpu),
                                first_step=torch.full((64,), -1, dtype=torch.int32, device=gpu),
                                points=torch.tensor(points, dtype=torch.int64, device=gpu),
                                time=torch.tensor(time, dtype=torch.int64, device=gpu))
        return SimpleNamespace(band_hist=torch.zeros((50, 60), dtype=torch.int32, device=gpu),
                               rows=torch.zeros((64, 3), dtype=torch.int32, device=gpu), subs={heights.deferred: rotor})
    for points, time in (([0, 3, 0, 0, 0], [1, 0, 0, 0, 0]), ([0, 3, 0, 0, 0], [0, 3 * ref.CAP + 1, 0, 0, 0])):
        with pytest.raises(RuntimeError, match='rotor exposure time'):
            heights.store(fly(points, time), ('s10d270', 0), False)
    heights.store(fly([0, 3, 0, 0, 0], [0, 3 * ref.CAP, 0, 0, 0]), ('s10d270', 0), False)
    assert bare.turbine_rotor_encounters[('s10d270', 0)]['time_per_turbine'].tolist() == [0, 3 * ref.CAP, 0, 0, 0]

