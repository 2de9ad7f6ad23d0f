"""K15 on the device: ssrs_rotor_encounters through ssrs_amd/turbines.py on every case of tests/rotor_ref.py against the
brute force over all (point, turbine) pairs, accumulation over calls, the heights of K14 fed straight in, the chunked
replay path, and Simulator(flight_height=True, rotor_geometry='turbine') end to end.  Every comparison is integer equality."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import altitude_ref as alt_ref
import rotor_ref as ref

pytestmark = pytest.mark.gpu


def shifted(host, shift, gpu, fill):
    """`host` on the device, `shift` elements of 4 bytes past torch's alignment, other values around it."""
    host = np.ascontiguousarray(host)
    raw = torch.full((host.shape[0] + 8,) + host.shape[1:], fill, dtype=torch.from_numpy(host).dtype, device=gpu)
    assert raw.data_ptr() % 16 == 0
    view = raw[shift:shift + host.shape[0]]
    view.copy_(torch.from_numpy(host))
    assert view.shape[0] == 0 or view.data_ptr() % 16 == 4 * (shift % 4)
    return view


def device_case(c, gpu):
    """(traj, alt, offsets, cellinfo) of a case on the device: traj and alt `shift` points past a 16-byte boundary with
    in-cylinder points around them; offsets the slice [1:] of the longer vector."""
    traj, alt, off = ref.flat(c)
    return (shifted(traj, c['shift'], gpu, 20), shifted(alt, c['shift'], gpu, 50_000), torch.from_numpy(off).to(gpu)[1:],
            torch.from_numpy(ref.packed(c['elev'])).to(gpu))


def check(got, want, nturb):
    """(hits, first_step, points) of a call against a brute_force dict, and both popcounts of the bitmap."""
    from ssrs_amd import turbines as tb
    hits, first, points = got
    assert hits.dtype == torch.int32 and hits.is_cuda
    bitmap = hits.cpu().numpy().view(np.uint32)
    assert np.array_equal(bitmap, want['bitmap']), np.argwhere(bitmap != want['bitmap'])[:8]
    if first is not None:
        f = first.cpu().numpy()
        assert first.dtype == torch.int32 and np.array_equal(f, want['first_step']), np.argwhere(f != want['first_step'])[:8]
    if points is not None:
        p = points.cpu().numpy()
        assert points.dtype == torch.int64 and np.array_equal(p, want['points']), np.argwhere(p != want['points'])[:8]
    per_turbine, per_track = tb.encounter_counts(hits, nturb)
    assert np.array_equal(per_turbine.cpu().numpy(), want['tracks_per_turbine'])
    assert np.array_equal(per_track.cpu().numpy(), want['turbines_per_track'])


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_cases_on_the_device(gpu, c):
    from ssrs_amd import turbines as tb
    traj, alt, off, info = device_case(c, gpu)
    assert int(off[0]) == c['lead']
    want = ref.expected(c['name'])
    got = tb.rotor_encounters(traj, alt, off, info, c['xy'], c['reach'], c['zband'], c['shape'])
    assert tuple(got[0].shape) == (len(ref.LENGTHS), 3)
    check(got, want, ref.NTURB)
    # the planted cases are really in the data: both words' border bits, the ones nothing hits, the exposure beyond the bitmap
    assert (want['tracks_per_turbine'][[0, 1, 2, 3, 4, 9, 10, 11, 12, 31, 32, 63, 64]] > 0).all()
    assert not want['tracks_per_turbine'][5:9].any() and not want['points'][5:9].any()
    assert want['points'].sum() > want['tracks_per_turbine'].sum() and want['first_step'][2] == -1
    if 'loiter' in c['name']:
        assert want['points'][0] > 4097 and want['points'][1] >= 4097
    # each optional output alone, and neither
    only_first = tb.rotor_encounters(traj, alt, off, info, c['xy'], c['reach'], c['zband'], c['shape'], points=False)
    only_points = tb.rotor_encounters(traj, alt, off, info, c['xy'], c['reach'], c['zband'], c['shape'], first_step=False)
    neither = tb.rotor_encounters(traj, alt, off, info, c['xy'], c['reach'], c['zband'], c['shape'], first_step=False, points=False)
    assert only_first[2] is None and only_points[1] is None and neither[1:] == (None, None)
    for other in (only_first, only_points, neither):
        check(other, want, ref.NTURB)
    # cull lists of the caller's, numpy or device tensors
    bins = tb.build_bins(c['xy'], c['reach'], c['shape'])
    for given in (bins, tuple(torch.from_numpy(b).to(gpu) for b in bins)):
        check(tb.rotor_encounters(traj, alt, off, info, c['xy'], c['reach'], c['zband'], c['shape'], bins=given), want, ref.NTURB)


def test_accumulation_over_disjoint_track_ranges(gpu):
    """Two calls on disjoint track ranges into slices of one bitmap and one points vector equal one call on the union; points
    seeded with 2^32 - 3 comes back with the carry; a second call over the same tracks doubles the exposure alone."""
    from ssrs_amd import turbines as tb
    c = ref.case('lead_5_shift_1')
    traj, alt, off, info = device_case(c, gpu)
    want = ref.expected(c['name'])
    n = len(ref.LENGTHS)
    args = (info, c['xy'], c['reach'], c['zband'], c['shape'])
    for k in (9, 11, 150):                         # inside the long tracks; inside the run of short ones
        hits = torch.zeros((n, 3), dtype=torch.int32, device=gpu)
        first = torch.full((n,), -1, dtype=torch.int32, device=gpu)
        points = torch.full((ref.NTURB,), 2 ** 32 - 3, dtype=torch.int64, device=gpu)
        tb.rotor_encounters(traj, alt, off[:k + 1], *args, hits=hits[:k], first_step=first[:k], points=points)
        assert not hits[k:].any() and (first[k:] == -1).all()
        out = tb.rotor_encounters(traj, alt, off[k:], *args, hits=hits[k:], first_step=first[k:], points=points)
        assert out[2] is points
        assert np.array_equal(points.cpu().numpy(), want['points'] + (2 ** 32 - 3)) and int(points.max()) >= 2 ** 32
        check((hits, first, points - (2 ** 32 - 3)), want, ref.NTURB)
    again = tb.rotor_encounters(traj, alt, off, *args, hits=hits, first_step=first, points=points - (2 ** 32 - 3))
    check((again[0], again[1], None), want, ref.NTURB)
    assert np.array_equal(again[2].cpu().numpy(), 2 * want['points'])


def test_a_track_trapped_inside_a_cylinder(gpu):
    """200 000 points that alternate between two cells inside two cylinders and at the edge of a third, short tracks before
    and after: the exposure is counted in full."""
    from ssrs_amd import turbines as tb
    rng = np.random.default_rng(4)
    trap = np.empty((200_000, 2), dtype=np.int16)
    trap[0::2], trap[1::2] = (20, 30), (20, 31)
    tracks = [ref.walk(rng, 3) for _ in range(5)] + [trap] + [ref.walk(rng, 3, start=(21, 31))] + [ref.walk(rng, 3) for _ in range(5)]
    traj = np.concatenate(tracks)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    alt = np.tile(np.array([80_000, 80_001, 80_002], dtype=np.int32), traj.shape[0] // 3 + 1)[:traj.shape[0]]
    elev = np.full(ref.SHAPE, 1000, dtype=np.int32)
    xy = np.array([[30., 20.], [31.5, 20.5], [29., 20.], [60., 60.]])
    reach = np.array([2.5, 2.5, 1., 3.])
    zband = np.array([ref.WIDE, (81_000, 81_001), ref.WIDE, ref.WIDE], dtype=np.int32)       # the second: two heights of three
    want = ref.brute_force(traj, alt, off, elev, xy, reach, zband, ref.SHAPE)
    assert want['points'][0] >= 200_000 and 100_000 < want['points'][1] < 200_000 and want['points'][2] >= 100_000
    got = tb.rotor_encounters(torch.from_numpy(traj).to(gpu), torch.from_numpy(alt).to(gpu), torch.from_numpy(off).to(gpu),
                              torch.from_numpy(ref.packed(elev)).to(gpu), xy, reach, zband, ref.SHAPE)
    check(got, want, 4)


@pytest.mark.parametrize('c', alt_ref.CASES, ids=alt_ref.CASE_IDS)
def test_heights_of_the_altitude_scan_fed_straight_in(gpu, c):
    """alt of flight.compute_track_altitudes, as it leaves the device, into the rotor kernel: the brute force over the oracle's
    heights."""
    from ssrs_amd import flight
    from ssrs_amd import turbines as tb
    from test_gpu_altitude import device_case as altitude_case, metres
    traj, off, info = altitude_case(c, gpu)
    out = flight.compute_track_altitudes(traj, info, c['shape'], offsets=off, want_alt=True, **metres(c['params']))
    rng = np.random.default_rng(7)
    xy, reach, zband = ref.random_turbines(rng, c['shape'], 40, 0, 900_000)
    zband[:2] = ref.WIDE
    got = tb.rotor_encounters(traj, out['alt'], off, info, xy, reach, zband, c['shape'])
    host_traj, host_off = alt_ref.flat(c)
    heights = np.concatenate([np.zeros(c['lead'], dtype=np.int32), alt_ref.expected(c['name'])['alt']])
    want = ref.brute_force(host_traj, heights, host_off[1:], c['elev'], xy, reach, zband, c['shape'])
    check(got, want, 40)
    # (all of them meet turbines but the one without points and the one whose heights lie beyond every band)
    assert bool(want['points'].sum() > 0) == (c['name'] not in ('all_empty', 'beyond_int32'))


def test_raster_too_large_for_the_lds_mask(gpu):
    """16 416 x 16 416 cells are 513 x 513 = 263 169 bins, more than the mask in LDS holds: bin_start is read per point.  An
    aligned and an unaligned buffer; the elevation is one value everywhere (the raster is built on the device)."""
    from ssrs_amd import turbines as tb
    rows = cols = 16416
    rng = np.random.default_rng(21)
    xy = np.array([[14000., 15000.], [14003.5, 15002.5], [16415., 16415.], [0., 0.], [31.5, 9000.2], [-3., 8000.]])
    reach = np.array([3., 2.5, 4., 1., 3.5, 5.])
    zband = np.array([ref.WIDE, (60_000, 90_000), ref.WIDE, (0, 70_000), ref.WIDE, ref.WIDE], dtype=np.int32)
    tracks = []
    for n in (1, 0, 300, 64, 257, 5, 5, 5, 700):
        t = np.stack([rng.integers(0, rows, n), rng.integers(0, cols, n)], 1)
        near = rng.random(n) < 0.5                      # half of the points within a few cells of some turbine
        which = xy[rng.integers(0, len(xy), n)]
        t[near, 0] = np.clip(np.round(which[near, 1]) + rng.integers(-4, 5, near.sum()), 0, rows - 1)
        t[near, 1] = np.clip(np.round(which[near, 0]) + rng.integers(-4, 5, near.sum()), 0, cols - 1)
        tracks.append(t.astype(np.int16))
    traj = np.concatenate(tracks)
    off = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    alt = rng.integers(10_000, 120_000, traj.shape[0]).astype(np.int32)
    info = torch.empty((rows, cols, 2), dtype=torch.int32, device=gpu)
    info[..., 0], info[..., 1] = 123_456_789, 5000
    elev = np.broadcast_to(np.int32(5000), (rows, cols))
    want = ref.brute_force(traj, alt, off, elev, xy, reach, zband, (rows, cols))
    assert (want['tracks_per_turbine'] > 0).sum() >= 5
    for shift in (0, 1):
        got = tb.rotor_encounters(shifted(traj, shift, gpu, 3), shifted(alt, shift, gpu, 0), torch.from_numpy(off).to(gpu),
                                  info, xy, reach, zband, (rows, cols))
        check(got, want, 6)


def test_replay_chunks_accumulate(gpu):
    """The smoke inputs with a budget too small for one trajectory tensor: every replay range through K14 and K15 into slices
    of one bitmap and one points vector gives the integers of the run that holds its tensor, and the brute force's."""
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
    climb, elev = alt_ref.cellinfo(np.asarray(oro), dem, res, 15., 0.75)
    xy, reach, _ = ref.random_turbines(rng, (rows, cols), 40, 0, 1)
    zband = np.stack([elev[rng.integers(0, rows, 40), rng.integers(0, cols, 40)] + 20_000] * 2, 1).astype(np.int32)
    zband[:, 1] += rng.integers(50_000, 300_000, 40).astype(np.int32)
    bins = tuple(torch.from_numpy(b).to(gpu) for b in tb.build_bins(xy, reach, (rows, cols)))
    hits = torch.zeros((256, 2), dtype=torch.int32, device=gpu)
    first = torch.full((256,), -1, dtype=torch.int32, device=gpu)
    points = torch.zeros(40, dtype=torch.int64, device=gpu)
    nchunks = 0
    for t0, t1, traj, off in ranged.iter_device_chunks():
        out = flight.compute_track_altitudes(traj, info, (rows, cols), offsets=off, want_alt=True, **kw)
        tb.rotor_encounters(traj, out['alt'], off, info, xy, reach, zband, (rows, cols), bins=bins, hits=hits[t0:t1],
                            first_step=first[t0:t1], points=points)
        nchunks += 1
    assert nchunks >= 3
    one = flight.compute_track_altitudes(whole.traj, info, (rows, cols), offsets=whole.offsets, want_alt=True, **kw)
    got = tb.rotor_encounters(whole.traj, one['alt'], whole.offsets, info, xy, reach, zband, (rows, cols))
    assert torch.equal(hits, got[0]) and torch.equal(first, got[1]) and torch.equal(points, got[2])
    tracks = whole.tracks()
    heights = alt_ref.altitude(tracks, climb, elev, (rows, cols), alt_ref.DEFAULT)['alt']
    want = ref.brute_force(whole.traj.cpu().numpy(), heights, whole.offsets.cpu().numpy(), elev, xy, reach, zband, (rows, cols))
    check(got, want, 40)
    assert want['points'].sum() > want['tracks_per_turbine'].sum() > 0


def test_argument_errors(gpu):
    from ssrs_amd import _native
    from ssrs_amd import turbines as tb
    c = ref.case('planted')
    traj, alt, off, info = device_case(c, gpu)
    args = dict(traj=traj, alt=alt, offsets=off, cellinfo=info, xy_cells=c['xy'], reach=c['reach'], zband=c['zband'],
                gridshape=c['shape'])
    n = len(ref.LENGTHS)
    for bad, match in ((dict(alt=alt[:-1]), 'indexed like traj'), (dict(cellinfo=info[:, :-1]), 'cellinfo'),
                       (dict(cellinfo=info.cpu()), 'cellinfo'), (dict(reach=c['reach'][:-1]), 'reach'),
                       (dict(zband=c['zband'][:, :1]), 'zband'), (dict(xy_cells=np.zeros((0, 2)), reach=[], zband=np.zeros((0, 2))), 'turbines'),
                       (dict(hits=torch.zeros((n, 2), dtype=torch.int32, device=gpu)), 'hits'),
                       (dict(first_step=torch.zeros(n - 1, dtype=torch.int32, device=gpu)), 'first_step'),
                       (dict(points=torch.zeros(ref.NTURB, dtype=torch.int32, device=gpu)), 'points'),
                       (dict(bins=(np.zeros(3, dtype=np.int32), np.zeros(0, dtype=np.int32))), 'bin_start'),
                       (dict(gridshape=(70, 40000), cellinfo=torch.zeros((70, 40000, 2), dtype=torch.int32, device=gpu)), 'raster')):
        with pytest.raises(ValueError, match=match):
            tb.rotor_encounters(**{**args, **bad})
    # the library itself: a misaligned alt is refused before any launch
    import ctypes as C
    lib = _native.lib()
    xy, reach, zband = (torch.from_numpy(np.ascontiguousarray(c[k])).to(gpu) for k in ('xy', 'reach', 'zband'))
    bins = tuple(torch.from_numpy(b).to(gpu) for b in tb.build_bins(c['xy'], c['reach'], c['shape']))
    hits = torch.zeros((n, 3), dtype=torch.int32, device=gpu)
    rc = lib.ssrs_rotor_encounters(traj.data_ptr(), off.data_ptr(), C.c_int64(n), alt.data_ptr() + 2, info.data_ptr(), 70, 90,
                                   xy.data_ptr(), reach.data_ptr(), zband.data_ptr(), ref.NTURB, bins[0].data_ptr(),
                                   bins[1].data_ptr(), hits.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    assert rc == _native.SSRS_ERR_INVALID and not hits.any()
    # no tracks, and no cylinder that reaches the raster: nothing is touched
    none = tb.rotor_encounters(traj, alt, off[:1], info, c['xy'], c['reach'], c['zband'], c['shape'])
    assert tuple(none[0].shape) == (0, 3) and not none[2].any()
    far = tb.rotor_encounters(traj, alt, off, info, c['xy'] + 1e6, c['reach'], c['zband'], c['shape'])
    assert not far[0].any() and (far[1] == -1).all() and not far[2].any()


def _turbines():
    # 50 x 60 cells at 100 m from (0, 0); the tracks start in rows 2 .. 6 and head north
    return dict(x=[1500., 2550., 3000., 4000., 4500.], y=[700., 900., 1500., 800., 1250.], p_name=['A'] * 5,
                t_hh=[80., 90., 100., 110., 80.], t_rd=[100., 110., 120., 90., 130.])


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Config, Simulator
    from ssrs_amd import turbines as tb
    from test_gpu_turbines import _pack
    cfg = Config(run_name='cyl', out_dir=str(tmp_path), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=64,
                 track_start_region=(1, 5, 0.2, 0.6), track_direction=0., thermals_realization_count=1,
                 flight_height=True, rotor_geometry='turbine', rotor_clearance=100.)
    sim = Simulator(cfg, terrain='synthetic', turbines=_turbines())
    with pytest.raises(ValueError, match="rotor_geometry='turbine'"):
        sim.compute_turbine_rotor_encounters()
    sim.simulate_tracks()
    band = Simulator(replace(cfg, run_name='band', rotor_geometry='band'), terrain='synthetic', turbines=_turbines())
    band.simulate_tracks()
    assert band.turbine_rotor_encounters == {}

    # 'band' writes what it wrote before this option existed, and 'turbine' the same files, byte for byte, plus its own
    stems = [f's10d270_d0_t75_fluidflow_r{k}' for k in (0, 1)]
    before = {'s10d270_orograph.npy', 's10d270_r0_thermals.npy'} | \
        {f'{s}_{name}' for s in stems for name in ('potential.npy', 'tracks.pkl', 'rotor_presence.npy', 'flight_heights.npy')}
    names = set(os.listdir(band.mode_data_dir))
    assert names == before
    new = {f'{s}_turbine_rotor_encounters.npy' for s in stems}
    assert set(os.listdir(sim.mode_data_dir)) == names | new
    for name in names:
        with open(os.path.join(sim.mode_data_dir, name), 'rb') as a, open(os.path.join(band.mode_data_dir, name), 'rb') as b:
            assert a.read() == b.read(), name

    dem = sim.get_terrain_elevation()
    xy = sim.turbines.cell_coordinates(sim.bounds, 100.)
    reach, zband = tb.rotor_geometry(sim.turbines, dem, sim.bounds, 100., clearance=100.)
    assert np.array_equal(reach, (np.array([100., 110., 120., 90., 130.]) / 2. + 100.) / 100.)
    orograph = np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy'))
    fields = [orograph, orograph + np.load(os.path.join(sim.mode_data_dir, 's10d270_r0_thermals.npy'))]
    shares = []
    for real_id, field in enumerate(fields):
        key = ('s10d270', real_id)
        path = lambda name: os.path.join(sim.mode_data_dir, f'{stems[real_id]}_{name}')
        with open(path('tracks.pkl'), 'rb') as f:
            tracks = pickle.load(f)
        assert len(tracks) == 64
        climb, elev = alt_ref.cellinfo(field, dem, 100., 15., 0.75)
        heights = alt_ref.altitude(tracks, climb, elev, (50, 60), alt_ref.DEFAULT)['alt']
        traj, off = _pack(tracks)
        want = ref.brute_force(traj, heights, off, elev, xy, reach, zband, (50, 60))
        assert want['points'].sum() > want['tracks_per_turbine'].sum() > 0 and (want['tracks_per_turbine'] > 0).sum() >= 2
        saved = np.load(path('turbine_rotor_encounters.npy'))
        assert saved.dtype == np.int64 and saved.shape == (5, 2)
        assert np.array_equal(saved[:, 0], want['tracks_per_turbine']) and np.array_equal(saved[:, 1], want['points'])
        enc = sim.turbine_rotor_encounters[key]
        assert enc['tracks_per_turbine'].dtype == np.int64 and np.array_equal(enc['tracks_per_turbine'], saved[:, 0])
        assert enc['points_per_turbine'].dtype == np.int64 and np.array_equal(enc['points_per_turbine'], saved[:, 1])
        assert enc['turbines_per_track'].dtype == np.int32 and np.array_equal(enc['turbines_per_track'], want['turbines_per_track'])
        assert enc['first_step'].dtype == np.int32 and np.array_equal(enc['first_step'], want['first_step'])
        shares.append(saved / 64.)
    summary = sim.compute_turbine_rotor_encounters()
    assert summary.dtype == np.float64 and summary.shape == (5, 2)
    assert np.array_equal(summary, (shares[0] + shares[1]) / 2.)
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_turbine_rotor_encounters.npy')), summary)
    with pytest.raises(ValueError, match='no rotor encounters'):
        band.compute_turbine_rotor_encounters()

    # beside the 2-D encounters and the band-masked ones, and without the pickle: the same integers
    both = Simulator(replace(cfg, run_name='both', turbine_encounter_radius=150., save_tracks=False), terrain='synthetic',
                     turbines=_turbines())
    both.simulate_tracks()
    assert not [f for f in os.listdir(both.mode_data_dir) if f.endswith('.pkl')]
    for real_id in (0, 1):
        key = ('s10d270', real_id)
        for name in ('tracks_per_turbine', 'points_per_turbine', 'turbines_per_track', 'first_step'):
            assert np.array_equal(both.turbine_rotor_encounters[key][name], sim.turbine_rotor_encounters[key][name]), name
        assert key in both.turbine_encounters and key in both.rotor_turbine_encounters
        for name in ('rotor_presence.npy', 'flight_heights.npy', 'turbine_rotor_encounters.npy'):
            assert np.array_equal(np.load(os.path.join(both.mode_data_dir, f'{stems[real_id]}_{name}')),
                                  np.load(os.path.join(sim.mode_data_dir, f'{stems[real_id]}_{name}'))), name
