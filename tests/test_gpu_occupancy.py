"""K13 on the device: ssrs_track_occupancy through presence.compute_track_occupancy on every case of
tests/occupancy_ref.py (the cases tests/test_occupancy_emulation.py runs on the CPU), the chunked replay path, and
Simulator(track_occupancy=True) end to end.  Every comparison is integer equality but the one f32 summary map."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import occupancy_ref as ref

pytestmark = pytest.mark.gpu


def device_case(c, gpu):
    """(traj, offsets) of a case on the device: traj `shift` points (4 bytes each) past torch's 256-byte alignment,
    in-raster points around it; offsets the slice [1:] of the longer vector."""
    traj, off = ref.flat(c)
    raw = torch.full((traj.shape[0] + 8, 2), 3, dtype=torch.int16, device=gpu)
    assert raw.data_ptr() % 16 == 0
    view = raw[c['shift']:c['shift'] + traj.shape[0]]
    view.copy_(torch.from_numpy(traj))
    assert view.shape[0] == 0 or view.data_ptr() % 16 == 4 * (c['shift'] % 4)
    return view, torch.from_numpy(off).to(gpu)[1:]


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_cases_on_the_device(gpu, c):
    from ssrs_amd import presence
    traj, off = device_case(c, gpu)
    assert int(off[0]) == c['lead']
    rasters = []
    for planes in ref.PLANES:
        ws = presence.occupancy_workspace(c['shape'], planes)
        counts, per_track = presence.compute_track_occupancy(traj, c['shape'], offsets=off, cells_per_track=True,
                                                             planes=planes, workspace=ws)
        assert counts.dtype == torch.int32 and per_track.dtype == torch.int32 and counts.is_cuda
        assert not bool(ws.any()), 'the workspace is not zero after the call'
        ref.check(c['name'], counts.cpu().numpy(), per_track.cpu().numpy())
        # once more on the same workspace, into the same raster: everything twice
        again = presence.compute_track_occupancy(traj, c['shape'], offsets=off, counts=counts, planes=planes, workspace=ws)
        assert again is counts and not bool(ws.any())
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), 2 * ref.expected(c['name'])[0])
        rasters.append(counts)
    assert all(torch.equal(rasters[0], r) for r in rasters[1:])
    # the defaults: planes and workspace chosen by the function
    plain = presence.compute_track_occupancy(traj, c['shape'], offsets=off)
    assert np.array_equal(plain.cpu().numpy().view(np.uint32), ref.expected(c['name'])[0])


def test_host_input_and_accumulation(gpu):
    """A list of host tracks gives numpy; two calls on disjoint track sets into one `counts` equal one call on the union,
    and what `counts` held before is kept."""
    from ssrs_amd import presence
    c = ref.case('borders_97')
    counts, per_track = presence.compute_track_occupancy(c['tracks'], c['shape'], cells_per_track=True)
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int32 and per_track.dtype == np.int32
    ref.check(c['name'], counts, per_track)
    traj, off = device_case(c, gpu)
    pattern = ((np.arange(counts.size, dtype=np.uint32).reshape(c['shape']) * 2654435761) | 1).view(np.int32)
    acc = torch.from_numpy(pattern.copy()).to(gpu)
    ws = presence.occupancy_workspace(c['shape'], 2)
    _, first = presence.compute_track_occupancy(traj, c['shape'], offsets=off[:41], counts=acc, cells_per_track=True, planes=2,
                                                workspace=ws)
    _, second = presence.compute_track_occupancy(traj, c['shape'], offsets=off[40:], counts=acc, cells_per_track=True,
                                                 planes=2, workspace=ws)                  # (its first offset is not 0)
    ref.check(c['name'], acc.cpu().numpy(), torch.cat([first, second]).cpu().numpy(), before=pattern)
    assert not bool(ws.any())
    with pytest.raises(ValueError, match='workspace'):                                   # too small for 8 planes
        presence.compute_track_occupancy(traj, c['shape'], offsets=off, planes=8, workspace=ws)
    assert not bool(ws.any())


def test_replay_chunks_accumulate(gpu):
    """The smoke inputs with a budget too small for one trajectory tensor: iter_device_chunks() hands over the replay
    ranges, and the occupancy accumulated chunk by chunk equals that of the run that holds its tensor."""
    from ssrs_amd import layers, movmodel, presence
    from ssrs_amd.synthetic import synthetic_dem
    from oracle import ssrs_oracle as orc
    rows, cols, res = 96, 128, 100.
    oro, _ = layers.updraft_from_dem(synthetic_dem((rows, cols), res), res, 10., 270., threshold=0.75)
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
    acc = torch.zeros((rows, cols), dtype=torch.int32, device=gpu)
    ws = presence.occupancy_workspace((rows, cols), 4)
    nchunks, cells = 0, []
    for t0, t1, traj, off in ranged.iter_device_chunks():
        _, per_track = presence.compute_track_occupancy(traj, (rows, cols), offsets=off, counts=acc, cells_per_track=True,
                                                        planes=4, workspace=ws)
        cells.append(per_track)
        nchunks += 1
    assert nchunks >= 3 and not bool(ws.any())
    one, one_cells = presence.compute_track_occupancy(whole.traj, (rows, cols), offsets=whole.offsets, cells_per_track=True)
    assert torch.equal(acc, one) and torch.equal(torch.cat(cells), one_cells)
    want, want_cells = ref.occupancy(whole.tracks(), (rows, cols))
    assert np.array_equal(one.cpu().numpy().view(np.uint32), want) and int(want.max()) > 1
    assert np.array_equal(one_cells.cpu().numpy().view(np.uint32), want_cells)


def _config(tmp_path, **kw):
    from ssrs_amd import Config
    # (tracks start in rows 2 .. 6 and head north, as in test_gpu_simulator.make_config: the default start region does
    # not fit an 8 x 6 km raster)
    base = Config(run_name='occ', out_dir=str(tmp_path), sim_seed=1, region_width_km=(8., 6.), resolution=100.,
                  track_count=200, track_start_region=(1, 7, 0.2, 0.6), track_direction=0., track_occupancy=True,
                  save_tracks=True)
    return replace(base, **kw)


KEY = ('s10d270', 0)
STEM = 's10d270_d0_t75_fluidflow_r0'


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Simulator
    cfg = _config(tmp_path)
    sim = Simulator(cfg, terrain='synthetic')
    with pytest.raises(ValueError, match='no track occupancy'):
        sim.compute_occupancy_map()
    sim.simulate_tracks()
    with open(os.path.join(sim.mode_data_dir, f'{STEM}_tracks.pkl'), 'rb') as f:
        tracks = pickle.load(f)
    assert len(tracks) == 200
    want, want_cells = ref.occupancy(tracks, (60, 80))
    assert int(want.max()) > 1 and int(want.sum()) == int(want_cells.sum(dtype=np.int64))
    saved = np.load(os.path.join(sim.mode_data_dir, f'{STEM}_occupancy.npy'))
    assert saved.dtype == np.int32 and np.array_equal(saved.view(np.uint32), want)
    kept = sim.track_occupancy_counts[KEY]
    assert isinstance(kept, np.ndarray) and kept.dtype == np.int32 and np.array_equal(kept, saved)
    share = sim.compute_occupancy_map()
    assert share.dtype == np.float32 and np.array_equal(share, (want / 200).astype(np.float32))
    assert share.max() <= 1. and share.min() >= 0.
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_occupancy.npy')), share)
    # radius > 0: the disk mean of the per-cell shares (the presence map's disk), item by item
    from ssrs_amd import presence
    krad = presence.presence_kernel_radius(300., 100., (60, 80))
    disk = sim.compute_occupancy_map(radius=300.)
    smooth = presence.smooth_presence_counts(saved, krad).astype(np.float64)
    assert disk.dtype == np.float32 and np.array_equal(disk, (smooth / 200.).astype(np.float32))
    assert not np.array_equal(disk, share)

    # without the pickle: the trajectories are still produced on the device, the raster is the same
    quiet = Simulator(replace(cfg, run_name='q', save_tracks=False), terrain='synthetic')
    quiet.simulate_tracks()
    assert not [f for f in os.listdir(quiet.mode_data_dir) if f.endswith('.pkl')]
    assert np.array_equal(quiet.track_occupancy_counts[KEY], kept)
    assert np.array_equal(np.load(os.path.join(quiet.mode_data_dir, f'{STEM}_occupancy.npy')), saved)

    # switched off: nothing of it, and the histogram and the tracks of the run with it on are the plain run's
    plain = Simulator(replace(cfg, run_name='p', track_occupancy=False), terrain='synthetic')
    plain.simulate_tracks()
    assert plain.track_occupancy_counts == {}
    assert not [f for f in os.listdir(plain.mode_data_dir) if 'occupancy' in f]
    assert torch.equal(plain._presence_counts[KEY], sim._presence_counts[KEY])
    assert torch.equal(plain._presence_counts[KEY], quiet._presence_counts[KEY])
    with open(os.path.join(plain.mode_data_dir, f'{STEM}_tracks.pkl'), 'rb') as f:
        plain_tracks = pickle.load(f)
    assert len(plain_tracks) == 200 and all(np.array_equal(a, b) for a, b in zip(plain_tracks, tracks))
    with pytest.raises(ValueError, match='no track occupancy'):
        plain.compute_occupancy_map()


def test_simulator_with_turbine_encounters(gpu, tmp_path):
    """turbine_encounter_radius > 0 and track_occupancy in one run: both results, each equal to the result of the run
    with the other switched off."""
    from ssrs_amd import Simulator
    from test_gpu_turbines import _turbine_table
    cfg = _config(tmp_path, save_tracks=False, turbine_encounter_radius=150.)
    both = Simulator(cfg, terrain='synthetic', turbines=_turbine_table())
    both.simulate_tracks()
    only_occ = Simulator(replace(cfg, run_name='o', turbine_encounter_radius=0.), terrain='synthetic')
    only_occ.simulate_tracks()
    only_enc = Simulator(replace(cfg, run_name='e', track_occupancy=False), terrain='synthetic', turbines=_turbine_table())
    only_enc.simulate_tracks()
    assert only_occ.turbine_encounters == {} and only_enc.track_occupancy_counts == {}
    assert np.array_equal(both.track_occupancy_counts[KEY], only_occ.track_occupancy_counts[KEY])
    assert int(both.track_occupancy_counts[KEY].max()) > 1
    for name in ('tracks_per_turbine', 'turbines_per_track', 'first_step'):
        assert np.array_equal(both.turbine_encounters[KEY][name], only_enc.turbine_encounters[KEY][name]), name
    assert both.turbine_encounters[KEY]['tracks_per_turbine'].sum() > 0
    for name in ('occupancy', 'turbine_encounters'):
        assert os.path.exists(os.path.join(both.mode_data_dir, f'{STEM}_{name}.npy'))
    assert torch.equal(both._presence_counts[KEY], only_occ._presence_counts[KEY])
