"""K19 on the device (ssrs_rotor_collision_risk through turbines.rotor_collision_risk) against the brute force of
tests/collision_ref.py: every case on dirty, guarded memory, outputs that start non-zero, a batch cut into chunks, buffers
off the 16-byte boundary, per-track sums left out, either side of the LDS rule, and Simulator end to end.  Every comparison
of kernel outputs is integer equality."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import collision_ref as ref
import transit_ref as tref
from dirty_memory import dirty
from test_gpu_rotor_transits import _turbines, device_case

pytestmark = pytest.mark.gpu


def run(c, gpu, dev=None, **kw):
    from ssrs_amd import turbines as tb
    traj, alt, off, info = device_case(c, gpu) if dev is None else dev
    return tb.rotor_collision_risk(traj, alt, off, info, c['xy'], c['reach'], c['hub'], c['axis'], c['cls'], c['table'],
                                   c['shape'], tref.RESOLUTION, **kw)


def check(got, want):
    assert got['hits'].dtype == torch.int32 and got['transits'].dtype == got['risk'].dtype == got['track_risk'].dtype == torch.int64
    assert got['risk'].is_cuda and got['track_risk'].is_cuda
    bitmap = got['hits'].cpu().numpy().view(np.uint32)
    assert np.array_equal(bitmap, want['bitmap']), np.argwhere(bitmap != want['bitmap'])[:8]
    for key in ('transits', 'risk', 'track_risk', 'tracks_per_turbine', 'turbines_per_track'):
        mine = got[key].cpu().numpy()
        assert mine.shape == want[key].shape and np.array_equal(mine, want[key]), (key, np.argwhere(mine != want[key])[:8])


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_cases_on_dirty_guarded_memory(gpu, c):
    from ssrs_amd import turbines as tb
    want = ref.expected(c['name'])
    for fill in (0x00, 0xFF):
        with dirty(fill) as arena:
            got = run(c, gpu)
            check(got, want)
            arena.assert_clean()
            assert arena.buffers
    assert want['risk'].sum() == want['track_risk'].sum() > 0
    # hits and transits are ssrs_rotor_transits' of the same build
    traj, alt, off, info = device_case(c, gpu)
    plain = tb.rotor_transits(traj, alt, off, info, c['xy'], c['reach'], c['hub'], c['axis'], c['shape'], tref.RESOLUTION)
    assert torch.equal(plain['hits'], got['hits']) and torch.equal(plain['transits'], got['transits'])
    # cull lists of the caller's, and a table that is on the device already
    on_device = dict(c, table=torch.from_numpy(c['table'].view(np.int32)).to(gpu), cls=torch.from_numpy(c['cls']).to(gpu))
    check(run(on_device, gpu, bins=tuple(torch.from_numpy(b).to(gpu) for b in tref.bins(c))), want)


@pytest.mark.parametrize('name', ['lead_5_shift_1', 'rings'])
def test_outputs_that_start_nonzero_and_a_batch_cut_into_chunks(gpu, name):
    """Calls on disjoint track ranges into slices of one bitmap and one `track_risk`, and into one `transits` and one `risk`,
    equal one call on the whole; what the four held before is added to (`risk` seeded just below 2^63's half comes back with
    every carry)."""
    from ssrs_amd import turbines as tb
    c = ref.case(name)
    traj, alt, off, info = device_case(c, gpu)
    want = ref.expected(name)
    n, nturb = len(c['tracks']), len(c['reach'])
    seed = 2 ** 62 - 3
    cuts = [0, 3, 9, 11, 12, n - 1, n] if name != 'rings' else [0, 1, n - 2, n - 1, n]       # (inside the long tracks' run too)
    hits = torch.zeros((n, (nturb + 31) // 32), dtype=torch.int32, device=gpu)
    transits = torch.full((nturb, 2), 5, dtype=torch.int64, device=gpu)
    risk = torch.full((nturb, 2), seed, dtype=torch.int64, device=gpu)
    track_risk = torch.full((n,), 2 ** 33, dtype=torch.int64, device=gpu)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out = run(c, gpu, (traj, alt, off[lo:hi + 1], info), hits=hits[lo:hi], transits=transits, risk=risk,
                  track_risk=track_risk[lo:hi])
        assert out['risk'] is risk and out['transits'] is transits
    got = dict(hits=hits, transits=transits - 5, risk=risk - seed, track_risk=track_risk - 2 ** 33)
    got['tracks_per_turbine'], got['turbines_per_track'] = tb.encounter_counts(hits, nturb)
    check(got, want)


@pytest.mark.parametrize('name', ['pingpong', 'cuts', 'rings'])
def test_buffers_off_the_16_byte_boundary(gpu, name):
    """Both buffers at every placement, and `alt` alone off the boundary: the point-by-point path gives the vector path's
    integers."""
    c = ref.case(name)
    for shift, alt_shift in ((0, 0), (1, 1), (2, 2), (3, 3), (0, 1)):
        check(run(c, gpu, device_case(c, gpu, shift, alt_shift)), ref.expected(name))


def test_without_per_track_sums(gpu):
    """track_risk = NULL through the library's own entry: the other three outputs are the same."""
    from ssrs_amd import _native as nat
    from ssrs_amd import turbines as tb
    from ssrs_amd._device import stream_ptr
    c = ref.case('rings')
    want = ref.expected('rings')
    traj, alt, off, info = device_case(c, gpu)
    nturb, n = len(c['reach']), len(c['tracks'])
    dev = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)
    xy, reach, hub, axis = dev(c['xy'], np.float64), dev(c['reach'], np.float64), dev(c['hub'], np.int32), dev(c['axis'], np.float64)
    cls, table = dev(c['cls'], np.int32), dev(c['table'].view(np.int32), np.int32)
    bins = tuple(dev(b, np.int32) for b in tref.bins(c))
    hits = torch.zeros((n, 1), dtype=torch.int32, device=gpu)
    transits, risk = (torch.zeros((nturb, 2), dtype=torch.int64, device=gpu) for _ in range(2))
    nat.check(nat.lib().ssrs_rotor_collision_risk(
        nat.ptr(traj), nat.ptr(off), n, nat.ptr(alt), nat.ptr(info), c['shape'][0], c['shape'][1], nat.ptr(xy), nat.ptr(reach),
        nat.ptr(hub), nat.ptr(axis), tref.MM, nturb, nat.ptr(bins[0]), nat.ptr(bins[1]), nat.ptr(hits), nat.ptr(transits),
        nat.ptr(cls), nat.ptr(table), int(table.shape[0]), nat.ptr(risk), None, stream_ptr()))
    assert np.array_equal(risk.cpu().numpy(), want['risk']) and np.array_equal(transits.cpu().numpy(), want['transits'])
    assert np.array_equal(hits.cpu().numpy().view(np.uint32), want['bitmap'])
    with pytest.raises(ValueError, match='table'):
        run(dict(c, table=c['table'][:, :1]), gpu)
    with pytest.raises(ValueError, match='cls'):
        run(dict(c, cls=c['cls'][:-1]), gpu)
    with pytest.raises(ValueError, match='track_risk'):
        run(c, gpu, track_risk=torch.zeros(n + 1, dtype=torch.int64, device=gpu))
    with pytest.raises(ValueError, match='risk'):
        run(c, gpu, risk=torch.zeros((nturb, 2), dtype=torch.int32, device=gpu))
    assert tb.COLLISION_RINGS == 256


@pytest.mark.parametrize('nturb', [2559, 2560, 2561])
def test_either_side_of_the_lds_rule(gpu, nturb):
    """2559 turbines keep the mask beside their counters and sums, 2560 fill the 60 KB, from 2561 on the hand-overs of the
    last ones go to global memory.  The short tracks only: the brute force stays small."""
    c = ref.many_turbines(nturb)
    want = ref.compute(c)
    assert all(want['risk'][t].sum() > 0 for t in (2559, 2560, nturb - 1) if t < nturb)
    check(run(c, gpu), want)


def _risk_of_the_pickle(sim, stem, field, axes):
    """turbines.rotor_collision_risk over the pickled tracks and the device's own K14 heights, with the run's own table."""
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
    xy, reach, hub, n_empty = tb.rotor_disks(sim.turbines, dem, sim.bounds, 100., clearance=20.)
    assert n_empty == 0 and len(tracks) == 64
    cls, table, classes = tb.band_collision_table(
        np.asarray(sim.turbines.columns['t_rd']) / 2., 20., tb.band_parameters(sim.turbines, 3, 12., 4., 15.), 15., 0.85, 2.1,
        False, True, ref.PROFILE)
    assert len(classes) >= 14 and cls.min() == 0                              # (13 diameters, two blade counts)
    got = tb.rotor_collision_risk(traj, out['alt'], off, info, xy, reach, hub, axes, cls, table, (50, 60), 100.)
    # ... which the brute force confirms
    want = ref.brute_force(traj, out['alt'].cpu().numpy(), off, info[..., 1].cpu().numpy(), xy, reach, hub, axes, (50, 60), cls,
                           table, 100_000.)
    assert np.array_equal(got['risk'].cpu().numpy(), want['risk'])
    assert np.array_equal(got['track_risk'].cpu().numpy(), want['track_risk'])
    return want


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Config, Simulator
    from ssrs_amd import turbines as tb
    fleet = dict(_turbines(), t_blades=[3] * 15 + [2] * 15)
    cfg = Config(run_name='risk', out_dir=str(tmp_path), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=64,
                 track_start_region=(1, 5, 0.2, 0.6), track_direction=0., flight_height=True, rotor_geometry='turbine',
                 rotor_clearance=20., collision_risk=True, collision_avoidance=0.25)
    sim = Simulator(cfg, terrain='synthetic', turbines=fleet)
    with pytest.raises(ValueError, match='collision_risk=True'):
        sim.compute_turbine_collision_risk()
    sim.simulate_tracks()
    stem = 's10d270_d0_t75_fluidflow_r0'
    field = np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy'))
    saved = np.load(os.path.join(sim.mode_data_dir, f'{stem}_turbine_collision_risk.npy'))
    per_track = np.load(os.path.join(sim.mode_data_dir, f'{stem}_track_collision_risk.npy'))
    assert saved.dtype == per_track.dtype == np.int64 and saved.shape == (30, 2) and per_track.shape == (64,)
    want = _risk_of_the_pickle(sim, stem, field, tb.rotor_axes(270., sim._time_ray_axes(), 30))
    assert np.array_equal(saved, want['risk']), np.argwhere(saved != want['risk'])[:8]
    assert np.array_equal(per_track, want['track_risk'])
    assert (saved.sum(1) > 0).sum() >= 3 and saved.sum() == per_track.sum()
    assert np.array_equal(sim.turbine_collision_risk[('s10d270', 0)], saved)
    assert np.array_equal(sim.track_collision_risk[('s10d270', 0)], per_track)
    summary = sim.compute_turbine_collision_risk()
    two = saved.astype(np.float64) * 2. ** -32 * (0.75 / 64.)
    assert summary.dtype == np.float64 and summary.shape == (30, 3)
    assert np.array_equal(summary[:, :2], two) and np.array_equal(summary[:, 2], two.sum(1))
    assert 0. < summary[:, 2].max() < want['transits'].sum(1).max() / 64.   # (a probability a transit: fewer than the transits)
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_turbine_collision_risk.npy')), summary)
    names = set(os.listdir(sim.mode_data_dir))
    assert f'{stem}_turbine_rotor_transits.npy' not in names                 # (rotor_transits is off: its file is not written)

    # beside rotor_transits: one pass serves both.  The transit file is that of a run without collision_risk, byte for
    # byte, like every other file; with collision_risk off the directory is what it was
    both = Simulator(replace(cfg, run_name='both', rotor_transits=True), terrain='synthetic', turbines=fleet)
    both.simulate_tracks()
    plain = Simulator(replace(cfg, run_name='plain', rotor_transits=True, collision_risk=False), terrain='synthetic',
                      turbines=fleet)
    plain.simulate_tracks()
    assert plain.turbine_collision_risk == {} and plain.track_collision_risk == {}
    ours = {f'{stem}_turbine_collision_risk.npy', f'{stem}_track_collision_risk.npy'}
    listing = set(os.listdir(plain.mode_data_dir))
    assert f'{stem}_turbine_rotor_transits.npy' in listing and not [n for n in listing if 'collision' in n]
    assert set(os.listdir(both.mode_data_dir)) == listing | ours
    assert names - {'summary_turbine_collision_risk.npy'} == (listing | ours) - {f'{stem}_turbine_rotor_transits.npy'}
    for name in listing:
        with open(os.path.join(both.mode_data_dir, name), 'rb') as a, open(os.path.join(plain.mode_data_dir, name), 'rb') as b:
            assert a.read() == b.read(), name
    for name in ours:
        assert np.array_equal(np.load(os.path.join(both.mode_data_dir, name)), np.load(os.path.join(sim.mode_data_dir, name)))
    transits = np.load(os.path.join(both.mode_data_dir, f'{stem}_turbine_rotor_transits.npy'))
    assert np.array_equal(transits[:, 1:], want['transits']) and np.array_equal(transits[:, 0], want['tracks_per_turbine'])
