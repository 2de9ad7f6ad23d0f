"""K18 on the device (ssrs_rotor_transits through turbines.rotor_transits) against the brute force of tests/transit_ref.py:
every case on dirty, guarded memory, accumulation over calls and replay chunks, K14's heights fed straight in, a raster too
large for the LDS mask, either side of the LDS rule, the cull contract, the point-by-point path, and Simulator end to end.
Every comparison is integer equality."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import altitude_ref as alt_ref
import transit_ref as ref
from dirty_memory import dirty
from test_gpu_rotor_encounters import shifted

pytestmark = pytest.mark.gpu


def device_case(c, gpu, shift=None, alt_shift=None):
    """(traj, alt, offsets, cellinfo) of a case on the device: traj and alt `shift` points past a 16-byte boundary with
    other values around them; offsets the slice [1:] of the longer vector."""
    traj, alt, off = ref.flat(c)
    shift = c['shift'] if shift is None else shift
    return (shifted(traj, shift, gpu, 20), shifted(alt, shift if alt_shift is None else alt_shift, gpu, ref.LEVEL),
            torch.from_numpy(off).to(gpu)[1:], torch.from_numpy(ref.packed(c['elev'])).to(gpu))


def run(c, gpu, dev=None, **kw):
    from ssrs_amd import turbines as tb
    traj, alt, off, info = device_case(c, gpu) if dev is None else dev
    return tb.rotor_transits(traj, alt, off, info, c['xy'], c['reach'], c['hub'], c['axis'], c['shape'], ref.RESOLUTION, **kw)


def check(got, want):
    assert got['hits'].dtype == torch.int32 and got['transits'].dtype == torch.int64 and got['transits'].is_cuda
    bitmap = got['hits'].cpu().numpy().view(np.uint32)
    assert np.array_equal(bitmap, want['bitmap']), np.argwhere(bitmap != want['bitmap'])[:8]
    transits = got['transits'].cpu().numpy()
    assert np.array_equal(transits, want['transits']), np.argwhere(transits != want['transits'])[:8]
    assert np.array_equal(got['tracks_per_turbine'].cpu().numpy(), want['tracks_per_turbine'])
    assert np.array_equal(got['turbines_per_track'].cpu().numpy(), want['turbines_per_track'])


@pytest.mark.parametrize('c', ref.DEVICE_CASES, ids=ref.DEVICE_IDS)
def test_cases_on_dirty_guarded_memory(gpu, c):
    want = ref.expected(c['name'])
    for fill in (0x00, 0xFF):
        with dirty(fill) as arena:
            got = run(c, gpu)
            check(got, want)
            arena.assert_clean()
            assert arena.buffers
    # the planted cases are really in the data
    t = want['transits']
    assert (t[[ref.A, ref.B, ref.C2, ref.DIAG, ref.OUTSIDE, ref.BIG_HI]].sum(1) > 0).all()
    assert not t[[ref.NAN_REACH, ref.NEG_REACH, ref.NAN_XY, ref.NAN_AXIS, ref.BIG_LO]].any()
    if c['name'] != 'short':
        assert (want['tracks_per_turbine'][[31, 32, 63, 64]] > 0).all()
    if 'pingpong' in c['name']:
        assert (t[[ref.A, ref.C2]] >= 2048).all()
    # cull lists of the caller's, numpy or device tensors
    for given in (ref.bins(c), tuple(torch.from_numpy(b).to(gpu) for b in ref.bins(c))):
        check(run(c, gpu, bins=given), want)


def test_accumulation_over_disjoint_track_ranges(gpu):
    """Two calls on disjoint track ranges into slices of one bitmap and one `transits` equal one call on the union;
    `transits` seeded with 2^32 - 3 comes back with the carry."""
    c = ref.case('lead_5_shift_1')
    dev = device_case(c, gpu)
    traj, alt, off, info = dev
    want = ref.expected(c['name'])
    n, nturb = len(c['tracks']), ref.NTURB
    seed = 2 ** 32 - 3
    for k in (9, 11, 150):                         # inside the long tracks; inside the run of short ones
        hits = torch.zeros((n, 3), dtype=torch.int32, device=gpu)
        transits = torch.full((nturb, 2), seed, dtype=torch.int64, device=gpu)
        run(c, gpu, (traj, alt, off[:k + 1], info), hits=hits[:k], transits=transits)
        assert not hits[k:].any()
        out = run(c, gpu, (traj, alt, off[k:], info), hits=hits[k:], transits=transits)
        assert out['transits'] is transits and int(transits.max()) >= 2 ** 32
        got = dict(out, hits=hits, transits=transits - seed)
        from ssrs_amd import turbines as tb
        got['tracks_per_turbine'], got['turbines_per_track'] = tb.encounter_counts(hits, nturb)
        check(got, want)


def test_a_trapped_track_costs_no_wrong_count(gpu):
    """200 001 points that ping-pong across a plane inside two disks, short tracks before and after."""
    rng = np.random.default_rng(4)
    trap = np.empty((200_001, 2), dtype=np.int16)
    trap[0::2], trap[1::2] = (20, 30), (21, 30)
    walk = ref.rotor_ref.walk
    tracks = [walk(rng, 3) for _ in range(5)] + [trap] + [walk(rng, 3, start=(21, 31))] + [walk(rng, 3) for _ in range(5)]
    c = dict(ref.case('planted'), tracks=tracks, alts=[np.full(len(t), ref.LEVEL, dtype=np.int32) for t in tracks],
             lead=0, tail=0, shift=0)
    want = ref.compute(c)
    assert (want['transits'][[ref.A, ref.C2]] >= 100_000).all()
    check(run(c, gpu), want)


@pytest.mark.parametrize('c', alt_ref.CASES, ids=alt_ref.CASE_IDS)
def test_heights_of_the_altitude_scan_fed_straight_in(gpu, c):
    from ssrs_amd import flight
    from ssrs_amd import turbines as tb
    from test_gpu_altitude import device_case as altitude_case, metres
    traj, off, info = altitude_case(c, gpu)
    out = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, want_alt=True, **metres(c['params']))
    rng = np.random.default_rng(7)
    xy, reach, _ = ref.rotor_ref.random_turbines(rng, c['shape'], 40, 0, 900_000)
    hub = rng.integers(0, 900_000, 40).astype(np.int32)
    angle = rng.uniform(0., 2. * np.pi, 40)
    axis = np.stack([np.sin(angle), np.cos(angle)], 1)
    got = tb.rotor_transits(traj, out['alt'], off, info, xy, reach, hub, axis, c['shape'], ref.RESOLUTION)
    host_traj, host_off = alt_ref.flat(c)
    heights = np.concatenate([np.zeros(c['lead'], dtype=np.int32), alt_ref.expected(c['name'])['alt']])
    want = ref.brute_force(host_traj, heights, host_off[1:], c['elev'], xy, reach, hub, axis, c['shape'])
    check(got, want)


def test_raster_too_large_for_the_lds_mask(gpu):
    """16 416 x 16 416 cells are 513 x 513 = 263 169 bins, more than the mask in LDS holds: bin_start is read per point
    (test_gpu_rotor_encounters' shape).  An aligned and an unaligned buffer; one elevation everywhere."""
    from ssrs_amd import turbines as tb
    rows = cols = 16416
    rng = np.random.default_rng(21)
    xy = np.array([[14000., 15000.5], [14003.5, 15002.5], [16415., 16414.5], [0.5, 0.], [31.5, 9000.2], [-3., 8000.]])
    reach = np.array([3., 2.5, 4., 1., 3.5, 5.])
    hub = np.array([60_000, 70_000, 80_000, 65_000, 90_000, 75_000], dtype=np.int32)
    angle = np.array([0., 0.3, 0., np.pi / 2., 2., 4.])
    axis = np.stack([np.sin(angle), np.cos(angle)], 1)
    tracks = []
    for n in (1, 0, 300, 64, 257, 5, 5, 5, 700):
        which = xy[rng.integers(0, len(xy))]
        start = (int(np.clip(np.round(which[1]), 2, rows - 3)), int(np.clip(np.round(which[0]), 2, cols - 3)))
        near = np.clip(start + np.cumsum(rng.integers(-1, 2, (n, 2)), 0), 0, rows - 1)       # a walk around a turbine
        tracks.append(near.astype(np.int16).reshape(-1, 2))
    traj = np.concatenate(tracks)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    alt = rng.integers(10_000, 120_000, traj.shape[0]).astype(np.int32)
    info = torch.empty((rows, cols, 2), dtype=torch.int32, device=gpu)
    info[..., 0], info[..., 1] = 123_456_789, 5000
    elev = np.broadcast_to(np.int32(5000), (rows, cols))
    want = ref.brute_force(traj, alt, off, elev, xy, reach, hub, axis, (rows, cols))
    assert (want['transits'].sum(1) > 0).sum() >= 3
    for shift in (0, 1):
        got = tb.rotor_transits(shifted(traj, shift, gpu, 3), shifted(alt, shift, gpu, 0), torch.from_numpy(off).to(gpu),
                                info, xy, reach, hub, axis, (rows, cols), ref.RESOLUTION)
        check(got, want)


@pytest.mark.parametrize('nturb', [7679, 7680, 7681, 8192])
def test_either_side_of_the_lds_rule(gpu, nturb):
    """7679 turbines keep the mask beside their counters, 7680 fill the 60 KB with counters, from 7681 on the hand-overs of
    the last ones go to global memory.  The short tracks only: the brute force stays small."""
    c = ref.many_turbines(nturb)
    want = ref.compute(c)
    assert want['transits'][nturb - 1].sum() > 0 and (nturb < 7681 or want['transits'][7680].sum() > 0)
    check(run(c, gpu), want)


def test_cull_contract(gpu):
    """A list that omits a turbine loses its transits; one that names it twice doubles them."""
    c = ref.case('planted')
    want = ref.expected('planted')
    assert want['transits'][ref.A].sum() > 0
    got = run(c, gpu, bins=ref.edit_bins(ref.bins(c), ref.A, 0))
    less = want['transits'].copy()
    less[ref.A] = 0
    assert np.array_equal(got['transits'].cpu().numpy(), less) and int(got['tracks_per_turbine'][ref.A]) == 0
    got = run(c, gpu, bins=ref.edit_bins(ref.bins(c), ref.A, 2))
    more = want['transits'].copy()
    more[ref.A] *= 2
    assert np.array_equal(got['transits'].cpu().numpy(), more)
    assert np.array_equal(got['hits'].cpu().numpy().view(np.uint32), want['bitmap'])


@pytest.mark.parametrize('name', ['planted', 'pingpong', 'cuts'])
def test_point_by_point_path_equals_the_vector_path(gpu, name):
    """`alt` alone off the 16-byte boundary sends every span point by point."""
    c = ref.case(name)
    vector = run(c, gpu, device_case(c, gpu, 0, 0))
    single = run(c, gpu, device_case(c, gpu, 0, 1))
    assert torch.equal(vector['hits'], single['hits']) and torch.equal(vector['transits'], single['transits'])
    check(single, ref.expected(name))


def test_replay_chunks_accumulate(gpu):
    """The smoke inputs with a budget too small for one trajectory tensor: every replay range through K14 and K18 into slices
    of one bitmap and one `transits` gives the integers of the run that holds its tensor, and the brute force's."""
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
    elev = info[..., 1].cpu().numpy()
    xy, reach, _ = ref.rotor_ref.random_turbines(rng, (rows, cols), 40, 0, 1)
    hub = (elev[rng.integers(0, rows, 40), rng.integers(0, cols, 40)] + rng.integers(50_000, 150_000, 40)).astype(np.int32)
    axis = tb.rotor_axes(rng.uniform(0., 360., 40), 'row_east')
    bins = tuple(torch.from_numpy(b).to(gpu) for b in tb.build_bins(xy, reach + 1.5, (rows, cols)))
    hits = torch.zeros((256, 2), dtype=torch.int32, device=gpu)
    transits = torch.zeros((40, 2), dtype=torch.int64, device=gpu)
    nchunks = 0
    for t0, t1, traj, off in ranged.iter_device_chunks():
        out = flight.compute_track_altitudes(traj, info, (rows, cols), offsets=off, want_alt=True, **kw)
        tb.rotor_transits(traj, out['alt'], off, info, xy, reach, hub, axis, (rows, cols), res, bins=bins, hits=hits[t0:t1],
                          transits=transits)
        nchunks += 1
    assert nchunks >= 3
    one = flight.compute_track_altitudes(whole.traj, info, (rows, cols), offsets=whole.offsets, want_alt=True, **kw)
    got = tb.rotor_transits(whole.traj, one['alt'], whole.offsets, info, xy, reach, hub, axis, (rows, cols), res)
    assert torch.equal(hits, got['hits']) and torch.equal(transits, got['transits'])
    want = ref.brute_force(whole.traj.cpu().numpy(), one['alt'].cpu().numpy(), whole.offsets.cpu().numpy(), elev, xy, reach,
                           hub, axis, (rows, cols), 1000. * res)
    check(got, want)
    assert want['transits'].sum() > 0


def test_argument_errors(gpu):
    from ssrs_amd import turbines as tb
    c = ref.case('planted')
    traj, alt, off, info = device_case(c, gpu)
    args = dict(traj=traj, alt=alt, offsets=off, cellinfo=info, xy_cells=c['xy'], reach=c['reach'], hub=c['hub'],
                axis=c['axis'], gridshape=c['shape'], resolution=ref.RESOLUTION)
    n = len(c['tracks'])
    for bad, match in ((dict(alt=alt[:-1]), 'indexed like traj'), (dict(cellinfo=info.cpu()), 'cellinfo'),
                       (dict(reach=c['reach'][:-1]), 'reach'), (dict(hub=c['hub'][:-1]), 'hub'),
                       (dict(axis=c['axis'][:-1]), 'axis'), (dict(resolution=0.), 'resolution'),
                       (dict(resolution=float('nan')), 'resolution'),
                       (dict(hits=torch.zeros((n, 2), dtype=torch.int32, device=gpu)), 'hits'),
                       (dict(transits=torch.zeros(ref.NTURB, dtype=torch.int64, device=gpu)), 'transits'),
                       (dict(bins=(np.zeros(3, dtype=np.int32), np.zeros(0, dtype=np.int32))), 'bin_start')):
        with pytest.raises(ValueError, match=match):
            tb.rotor_transits(**{**args, **bad})
    # one axis serves all turbines; no tracks, and no disk that reaches the raster: nothing is touched
    one = tb.rotor_transits(**{**args, 'axis': np.array([[0., 1.]])})
    same = tb.rotor_transits(**{**args, 'axis': np.tile(np.array([[0., 1.]]), (ref.NTURB, 1))})
    assert torch.equal(one['transits'], same['transits']) and int(one['transits'].sum()) > 0
    none = tb.rotor_transits(**{**args, 'offsets': off[:1]})
    assert tuple(none['hits'].shape) == (0, 3) and not none['transits'].any()
    far = tb.rotor_transits(**{**args, 'xy_cells': c['xy'] + 1e6})
    assert not far['hits'].any() and not far['transits'].any()


def _turbines():
    # 50 x 60 cells at 100 m from (0, 0); the tracks start in rows 2 .. 6 and head north.  30 turbines in three rows
    x = np.tile(np.linspace(450., 5450., 10), 3)
    y = np.repeat([750., 1250., 1850.], 10)
    k = np.arange(30)
    return dict(x=x, y=y, p_name=['A'] * 30, t_hh=60. + 5. * (k % 12), t_rd=80. + 4. * (k % 13))


def _transits_of_the_pickle(sim, stem, field, axes):
    """The brute force over the pickled tracks and the device's own K14 heights."""
    from ssrs_amd import flight
    from ssrs_amd import turbines as tb
    from test_gpu_turbines import _pack
    with open(os.path.join(sim.mode_data_dir, f'{stem}_tracks.pkl'), 'rb') as f:
        tracks = pickle.load(f)
    dem = sim.get_terrain_elevation()
    info = flight.altitude_cellinfo(field, dem, 100., 15., 0.75)
    traj, off = _pack(tracks)
    out = flight.compute_track_altitudes(torch.from_numpy(traj).cuda(), info, (50, 60), offsets=torch.from_numpy(off).cuda(),
                                         want_alt=True, start=100., floor=10., ceil=1000., band=(30., 150.))
    xy, reach, hub, n_empty = tb.rotor_disks(sim.turbines, dem, sim.bounds, 100., clearance=100.)
    assert n_empty == 0 and len(tracks) == 64
    want = ref.brute_force(traj, out['alt'].cpu().numpy(), off, info[..., 1].cpu().numpy(), xy, reach, hub, axes, (50, 60),
                           100_000.)
    return np.concatenate([want['tracks_per_turbine'][:, None], want['transits']], 1)


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Config, Simulator
    from ssrs_amd import turbines as tb
    cfg = Config(run_name='disk', out_dir=str(tmp_path), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=64,
                 track_start_region=(1, 5, 0.2, 0.6), track_direction=0., flight_height=True, rotor_geometry='turbine',
                 rotor_clearance=100., rotor_transits=True)
    sim = Simulator(cfg, terrain='synthetic', turbines=_turbines())
    with pytest.raises(ValueError, match='rotor_transits=True'):
        sim.compute_turbine_rotor_transits()
    sim.simulate_tracks()
    stem = 's10d270_d0_t75_fluidflow_r0'
    field = np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy'))
    saved = np.load(os.path.join(sim.mode_data_dir, f'{stem}_turbine_rotor_transits.npy'))
    assert saved.dtype == np.int64 and saved.shape == (30, 3)
    want = _transits_of_the_pickle(sim, stem, field, tb.rotor_axes(270., sim._time_ray_axes(), 30))
    assert np.array_equal(saved, want), np.argwhere(saved != want)[:8]
    assert (want[:, 0] > 0).sum() >= 3 and want[:, 1:].sum() >= want[:, 0].sum() > 0
    assert np.array_equal(sim.turbine_rotor_transits[('s10d270', 0)], saved)
    summary = sim.compute_turbine_rotor_transits()
    assert summary.dtype == np.float64 and summary.shape == (30, 3) and np.array_equal(summary, saved / 64.)
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_turbine_rotor_transits.npy')), summary)

    # beside the timed K15: its files are those of a run without rotor_transits, byte for byte, and the transits the same
    timed = replace(cfg, run_name='timed', flight_time=True, rotor_exposure_time=True)
    both = Simulator(timed, terrain='synthetic', turbines=_turbines())
    both.simulate_tracks()
    plain = Simulator(replace(timed, run_name='plain', rotor_transits=False), terrain='synthetic', turbines=_turbines())
    plain.simulate_tracks()
    assert plain.turbine_rotor_transits == {}
    names = set(os.listdir(plain.mode_data_dir))
    assert {f'{stem}_turbine_rotor_encounters.npy', f'{stem}_turbine_rotor_time.npy'} <= names
    assert set(os.listdir(both.mode_data_dir)) == names | {f'{stem}_turbine_rotor_transits.npy'}
    for name in names:
        with open(os.path.join(both.mode_data_dir, name), 'rb') as a, open(os.path.join(plain.mode_data_dir, name), 'rb') as b:
            assert a.read() == b.read(), name
    assert np.array_equal(np.load(os.path.join(both.mode_data_dir, f'{stem}_turbine_rotor_transits.npy')), saved)

    # rotor_yaw = 90 is a wind from 90 degrees for the rotors alone: the tracks are those of the 270-degree wind
    yawed = Simulator(replace(cfg, run_name='yaw', rotor_yaw=90.), terrain='synthetic', turbines=_turbines())
    yawed.simulate_tracks()
    got = np.load(os.path.join(yawed.mode_data_dir, f'{stem}_turbine_rotor_transits.npy'))
    want = _transits_of_the_pickle(yawed, stem, field, tb.rotor_axes(90., yawed._time_ray_axes(), 30))
    assert np.array_equal(got, want) and want[:, 1:].sum() > 0
    assert not np.array_equal(got[:, 1:], saved[:, 1:])                      # (the directions change sides)
