"""K20 on the device (ssrs_site_collision_risk through turbines.site_collision_risk) against tests/site_ref.py -- K19's
pinned brute force called with the sites as turbines: every case on dirty, guarded memory, K19 itself on the device with a
turbine on every cell as a second oracle, outputs that start non-zero, a batch cut into chunks, buffers off the 16-byte
boundary, and Simulator end to end.  Every comparison of kernel outputs is integer equality."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import site_ref as ref
import transit_ref as tref
from dirty_memory import dirty
from test_gpu_rotor_transits import device_case

pytestmark = pytest.mark.gpu


def run(c, k, gpu, dev=None, axis=None, **kw):
    from ssrs_amd import turbines as tb
    traj, alt, off, info = device_case(c, gpu) if dev is None else dev
    k = ref.klass(k)
    return tb.site_collision_risk(traj, alt, off, info, k['reach'], k['hub_mm'], k['axis'] if axis is None else axis, ref.TABLE,
                                  c['shape'], tref.RESOLUTION, **kw)


def check(got, want):
    assert got['risk'].dtype == torch.int64 and got['risk'].is_cuda
    for key in ('transits', 'risk'):
        if got[key] is None:
            continue
        mine = got[key].cpu().numpy()
        assert mine.shape == want[key].shape and np.array_equal(mine, want[key]), (key, np.argwhere(mine != want[key])[:8])


@pytest.mark.parametrize('c,k', ref.COMBOS, ids=ref.COMBO_IDS)
def test_cases_on_dirty_guarded_memory(gpu, c, k):
    want = ref.expected(c, k)
    for fill in (0x00, 0xFF):
        with dirty(fill) as arena:
            check(run(c, k, gpu), want)
            arena.assert_clean()
            assert arena.buffers
    # the uniform axis equals a per-cell raster filled with that axis; the counts left out
    filled = np.array(np.broadcast_to(np.array(ref.klass(k)['axis']), c['shape'] + (2,)))
    got = run(c, k, gpu, axis=torch.from_numpy(filled).to(gpu), want_transits=False)
    assert got['transits'] is None
    check(got, want)


@pytest.mark.parametrize('c,k', ref.CELL_COMBOS, ids=ref.CELL_IDS)
def test_cell_axes_on_dirty_guarded_memory(gpu, c, k):
    want = ref.expected(c, k, per_cell=True)
    for fill in (0x00, 0xFF):
        with dirty(fill) as arena:
            check(run(c, k, gpu, axis=ref.cell_axes(c['shape'])), want)
            arena.assert_clean()


@pytest.mark.parametrize('name,k,per_cell', [('planted', 'r4', False), ('pingpong', 'r65', False), ('planted', 'r65', True),
                                             ('rings', 'r0', False)])
def test_against_k19_on_the_device(gpu, name, k, per_cell):
    """turbines.rotor_collision_risk with 6300 turbines on the cell centres of the 70 x 90 raster, every one of the candidate
    class and with the site's axis, equals the site map reshaped -- the device's own arithmetic on both sides."""
    from ssrs_amd import turbines as tb
    c = ref.case(name)
    assert c['shape'] == (70, 90) and 70 * 90 <= tb.MAX_TURBINES
    kl = ref.klass(k)
    axis = ref.cell_axes(c['shape']) if per_cell else np.array(kl['axis'])
    xy, reach, hub, axes = ref.site_turbines(c['elev'], kl['reach'], kl['hub_mm'], axis)
    dev = device_case(c, gpu)
    fleet = tb.rotor_collision_risk(*dev, xy, reach, hub, axes, np.zeros(6300, dtype=np.int32), ref.TABLE[None], c['shape'],
                                    tref.RESOLUTION)
    sites = run(c, k, gpu, dev, axis=axis)
    assert torch.equal(fleet['transits'].reshape(70, 90, 2), sites['transits'])
    assert torch.equal(fleet['risk'].reshape(70, 90, 2), sites['risk'])
    assert int(sites['transits'].sum()) > 0
    check(sites, ref.expected(c, k, per_cell=per_cell))


@pytest.mark.parametrize('name', ['lead_5_shift_1', 'pingpong'])
def test_outputs_that_start_nonzero_and_a_batch_cut_into_chunks(gpu, name):
    """Calls on disjoint track ranges -- and on the pieces of the 4097-point track, each starting at the last point of the
    one before -- into one `transits` and one `risk` equal one call on the whole; what the two held before is added to
    (`risk` seeded at 2^62 - 3 comes back with every carry)."""
    c = ref.case(name)
    traj, alt, off, info = device_case(c, gpu)
    want = ref.expected(c, 'r4')
    n = len(c['tracks'])
    seed = 2 ** 62 - 3
    transits = torch.full(c['shape'] + (2,), 5, dtype=torch.int64, device=gpu)
    risk = torch.full(c['shape'] + (2,), seed, dtype=torch.int64, device=gpu)
    a, b = int(off[11]), int(off[12])
    assert b - a == 4097
    pieces = [off[lo:hi + 1] for lo, hi in ((0, 3), (3, 9), (9, 11), (12, n - 1), (n - 1, n))] + \
        [torch.tensor([lo, hi], dtype=torch.int64, device=gpu) for lo, hi in ((a, a + 1001), (a + 1000, a + 3002), (a + 3001, b))]
    for piece in pieces:
        out = run(c, 'r4', gpu, (traj, alt, piece, info), transits=transits, risk=risk)
        assert out['risk'] is risk and out['transits'] is transits
    check(dict(transits=transits - 5, risk=risk - seed), want)


@pytest.mark.parametrize('name', ['pingpong', 'cuts', 'rings'])
def test_buffers_off_the_16_byte_boundary(gpu, name):
    """Both buffers at every placement, and `alt` alone off the boundary: the point-by-point path gives the vector path's
    integers."""
    c = ref.case(name)
    for shift, alt_shift in ((0, 0), (1, 1), (2, 2), (3, 3), (0, 1)):
        check(run(c, 'r65', gpu, device_case(c, gpu, shift, alt_shift)), ref.expected(c, 'r65'))


def test_wrapper_refusals_and_nothing_to_do(gpu):
    from ssrs_amd import turbines as tb
    c = ref.case('rings')
    dev = device_case(c, gpu)
    assert tb.SITE_MAX_REACH == 62.
    with pytest.raises(ValueError, match='reach'):
        tb.site_collision_risk(*dev, 62.5, 0, ref.PLANE, ref.TABLE, c['shape'], 100.)
    with pytest.raises(ValueError, match='axis'):
        tb.site_collision_risk(*dev, 4., 0, np.zeros((70, 90)), ref.TABLE, c['shape'], 100.)
    with pytest.raises(ValueError, match='table'):
        tb.site_collision_risk(*dev, 4., 0, ref.PLANE, ref.TABLE[None], c['shape'], 100.)
    with pytest.raises(ValueError, match='risk'):
        tb.site_collision_risk(*dev, 4., 0, ref.PLANE, ref.TABLE, c['shape'], 100., risk=torch.zeros((70, 90, 2), device=gpu))
    with pytest.raises(ValueError, match='resolution'):
        tb.site_collision_risk(*dev, 4., 0, ref.PLANE, ref.TABLE, c['shape'], 0.)
    for reach in (float('nan'), -1.):
        out = tb.site_collision_risk(*dev, reach, 0, ref.PLANE, ref.TABLE, c['shape'], 100.)
        assert int(out['risk'].abs().sum()) == 0 and int(out['transits'].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ Simulator
def _fleet():
    # 50 x 60 cells at 100 m from (0, 0); the tracks start in rows 2 .. 6 and head north.  30 turbines in three rows, every one
    # on a cell centre and of the candidate class
    x = np.tile(np.linspace(500., 5000., 10), 3)
    y = np.repeat([700., 1200., 1800.], 10)
    return dict(x=x, y=y, p_name=['A'] * 30, t_hh=[95.] * 30, t_rd=[160.] * 30)


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Config, Simulator
    from ssrs_amd import flight
    from ssrs_amd import turbines as tb
    from test_gpu_turbines import _pack
    cfg = Config(run_name='sites', out_dir=str(tmp_path), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=64,
                 track_start_region=(1, 5, 0.2, 0.6), track_direction=0., flight_height=True, rotor_geometry='turbine',
                 rotor_clearance=120., collision_risk=True, collision_avoidance=0.25, site_collision_risk=True,
                 site_hub_height=95., site_rotor_diameter=160.)
    sim = Simulator(cfg, terrain='synthetic', turbines=_fleet())
    with pytest.raises(ValueError, match='site_collision_risk=True'):
        sim.compute_site_collision_risk_map()
    sim.simulate_tracks()
    stem = 's10d270_d0_t75_fluidflow_r0'
    saved = np.load(os.path.join(sim.mode_data_dir, f'{stem}_site_collision_risk.npy'))
    passes = np.load(os.path.join(sim.mode_data_dir, f'{stem}_site_transits.npy'))
    assert saved.dtype == passes.dtype == np.int64 and saved.shape == passes.shape == (50, 60, 2)
    assert np.array_equal(sim.site_collision_risk_sums[('s10d270', 0)], saved)
    assert np.array_equal(sim.site_transit_counts[('s10d270', 0)], passes)
    assert passes.sum() > 0 and saved.sum() > 0 and ((saved > 0) <= (passes > 0)).all()

    # the turbines stand on cell centres and are of the candidate class: K19's file is the site map at their cells
    per_turbine = np.load(os.path.join(sim.mode_data_dir, f'{stem}_turbine_collision_risk.npy'))
    cells = sim.turbines.cell_coordinates(sim.bounds, 100.)
    cols, rows = cells[:, 0].astype(np.int64), cells[:, 1].astype(np.int64)
    assert np.array_equal(cells[:, 0], cols) and np.array_equal(cells[:, 1], rows) and per_turbine.shape == (30, 2)
    assert np.array_equal(per_turbine, saved[rows, cols]), np.argwhere(per_turbine != saved[rows, cols])[:8]
    assert per_turbine.sum() > 0

    # the map equals turbines.site_collision_risk over the pickled tracks and the device's own K14 heights
    with open(os.path.join(sim.mode_data_dir, f'{stem}_tracks.pkl'), 'rb') as f:
        tracks = pickle.load(f)
    field = np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy'))
    info = flight.altitude_cellinfo(field, sim.get_terrain_elevation(), 100., 15., 0.75)
    traj, off = _pack(tracks)
    out = flight.compute_track_altitudes(torch.from_numpy(traj).cuda(), info, (50, 60), offsets=torch.from_numpy(off).cuda(),
                                         want_alt=True, start=100., floor=10., ceil=1000., band=(30., 150.))
    table = tb.band_collision_table(np.array([80.]), 120., np.array([[12., 4., 15., 3.]]), 15., 0.85, 2.1, False, True,
                                    cfg.rotor_chord_profile)[1][0]
    axis = tb.rotor_axes(270., sim._time_ray_axes())[0]
    again = tb.site_collision_risk(traj, out['alt'], off, info, 2.0, 95_000, axis, table, (50, 60), 100.)
    assert np.array_equal(again['risk'].cpu().numpy(), saved) and np.array_equal(again['transits'].cpu().numpy(), passes)
    # ... which the brute force confirms
    want = ref.brute_force(traj, out['alt'].cpu().numpy(), off, info[..., 1].cpu().numpy(), 2.0, 95_000, axis, table, (50, 60),
                           100_000.)
    assert np.array_equal(saved, want['risk']) and np.array_equal(passes, want['transits'])

    # the summary is its formula
    summary = sim.compute_site_collision_risk_map()
    assert summary.dtype == np.float64 and summary.shape == (50, 60)
    assert np.array_equal(summary, saved.astype(np.float64).sum(2) * 2. ** -32 * (0.75 / 64.))
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_site_collision_risk.npy')), summary)

    # with the feature off the directory is what it was, byte for byte; and it needs no turbines and no rotor_geometry
    plain = Simulator(replace(cfg, run_name='plain', site_collision_risk=False), terrain='synthetic', turbines=_fleet())
    plain.simulate_tracks()
    assert plain.site_collision_risk_sums == {} and plain.site_transit_counts == {}
    listing = set(os.listdir(plain.mode_data_dir))
    ours = {f'{stem}_site_collision_risk.npy', f'{stem}_site_transits.npy'}
    assert not [n for n in listing if 'site' in n]
    assert set(os.listdir(sim.mode_data_dir)) == listing | ours | {'summary_site_collision_risk.npy'}
    for name in listing:
        with open(os.path.join(sim.mode_data_dir, name), 'rb') as a, open(os.path.join(plain.mode_data_dir, name), 'rb') as b:
            assert a.read() == b.read(), name
    alone = Simulator(replace(cfg, run_name='alone', collision_risk=False, rotor_geometry='band'), terrain='synthetic')
    alone.simulate_tracks()
    for name in ours:
        assert np.array_equal(np.load(os.path.join(alone.mode_data_dir, name)), np.load(os.path.join(sim.mode_data_dir, name)))
