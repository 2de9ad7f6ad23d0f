"""K17 on the device: ssrs_track_passage through presence.compute_track_passage on every case of tests/passage_ref.py
(the cases tests/test_passage_emulation.py runs on the CPU), against K13 at r2 = 0 and K8 at turbines on cell centres, on
dirty, guarded memory, and Simulator(track_passage_radius > 0) end to end.  Every comparison is integer equality but the
one f32 summary map."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

import occupancy_ref
import passage_ref as ref
from dirty_memory import FILLS, dirty

pytestmark = pytest.mark.gpu


def device_case(c, gpu, shift=0):
    """(traj, offsets) of a case on the device: traj `shift` points (4 bytes each) past torch's 256-byte alignment,
    in-raster points around it; offsets the slice [1:] of the longer vector."""
    traj, off = ref.flat(c)
    raw = torch.full((traj.shape[0] + 8, 2), 0, dtype=torch.int16, device=gpu)
    assert raw.data_ptr() % 16 == 0
    view = raw[shift:shift + traj.shape[0]]
    view.copy_(torch.from_numpy(traj))
    assert view.shape[0] == 0 or view.data_ptr() % 16 == 4 * (shift % 4)
    return view, torch.from_numpy(off).to(gpu)[1:]


def run_case(c, gpu, planes, shift, ws=None):
    from ssrs_amd import presence
    traj, off = device_case(c, gpu, shift)
    assert int(off[0]) == c['lead']
    stats = torch.zeros(2, dtype=torch.int64, device=gpu)
    counts, per_track = presence.compute_track_passage(traj, c['shape'], c['r2'], offsets=off, cells_per_track=True,
                                                       planes=planes, workspace=ws, stats=stats)
    assert counts.dtype == torch.int32 and per_track.dtype == torch.int32 and counts.is_cuda
    ref.check(c['name'], counts.cpu().numpy(), per_track.cpu().numpy())
    assert int(stats[1]) == int(ref.expected(c['name'])[0].sum(dtype=np.int64)) and int(stats[0]) >= int(stats[1])
    return counts, stats


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_cases_on_the_device(gpu, c):
    """planes 1, 3 and 8, aligned and at the three misaligned placements, on one workspace per planes that is never cleaned: the
    restatement's integers every time."""
    from ssrs_amd import presence
    rasters = []
    for planes in ref.PLANES:
        ws = presence.passage_workspace(c['shape'], planes)
        ws.fill_(0xFF)
        for shift in (0, 1, 2, 3):
            rasters.append(run_case(c, gpu, planes, shift, ws)[0])
    assert all(torch.equal(rasters[0], r) for r in rasters[1:])
    # the defaults: planes and workspace chosen by the function, no stats, host input
    traj, off = device_case(c, gpu)
    plain = presence.compute_track_passage(traj, c['shape'], c['r2'], offsets=off)
    assert torch.equal(plain, rasters[0])


def test_host_input(gpu):
    from ssrs_amd import presence
    c = ref.case('lengths_r8')
    counts, per_track = presence.compute_track_passage(c['tracks'], c['shape'], c['r2'], cells_per_track=True)
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int32 and per_track.dtype == np.int32
    ref.check(c['name'], counts, per_track)


@pytest.mark.parametrize('name', ['borders_257', 'borders_257_r26', 'lead_7'])
def test_split_calls_accumulate(gpu, name):
    """One call over all tracks equals two calls over a split of them into one raster (the second one's first offset is
    not 0), and what the raster held before is kept."""
    from ssrs_amd import presence
    c = ref.case(name)
    traj, off = device_case(c, gpu)
    cut = len(c['tracks']) * 2 // 5
    pattern = ((np.arange(c['shape'][0] * c['shape'][1], dtype=np.uint32).reshape(c['shape']) * 2654435761) | 1).view(np.int32)
    acc = torch.from_numpy(pattern.copy()).to(gpu)
    ws = presence.passage_workspace(c['shape'], 2)
    _, first = presence.compute_track_passage(traj, c['shape'], c['r2'], offsets=off[:cut + 1], counts=acc,
                                              cells_per_track=True, planes=2, workspace=ws)
    _, second = presence.compute_track_passage(traj, c['shape'], c['r2'], offsets=off[cut:], counts=acc,
                                               cells_per_track=True, planes=2, workspace=ws)
    ref.check(c['name'], acc.cpu().numpy(), torch.cat([first, second]).cpu().numpy(), before=pattern)
    one = presence.compute_track_passage(traj, c['shape'], c['r2'], offsets=off, planes=2, workspace=ws)
    assert torch.equal(one, acc - torch.from_numpy(pattern).to(gpu))
    with pytest.raises(ValueError, match='workspace'):                                   # too small for 8 planes
        presence.compute_track_passage(traj, c['shape'], c['r2'], offsets=off, planes=8, workspace=ws)


@pytest.mark.parametrize('name', ['borders_97', 'empty_tracks', 'pingpong_41', 'misaligned_lead', 'outside', 'memset_path',
                                  'shape_1x1', 'shape_40x1'])
def test_r2_zero_is_track_occupancy(gpu, name):
    """The same buffers through ssrs_track_occupancy and through ssrs_track_passage with r2 = 0: equal rasters and equal
    cells per track."""
    from ssrs_amd import presence
    import test_gpu_occupancy
    c = occupancy_ref.case(name)
    traj, off = test_gpu_occupancy.device_case(c, gpu)
    for planes in ref.PLANES:
        occ, occ_cells = presence.compute_track_occupancy(traj, c['shape'], offsets=off, cells_per_track=True, planes=planes)
        pas, pas_cells = presence.compute_track_passage(traj, c['shape'], 0, offsets=off, cells_per_track=True, planes=planes)
        assert torch.equal(occ, pas) and torch.equal(occ_cells, pas_cells)
    occupancy_ref.check(name, pas.cpu().numpy(), pas_cells.cpu().numpy())


def test_turbines_on_cell_centres_count_the_same_tracks(gpu):
    """K8 at 40 turbines that stand on cell centres (Turbines.cell_coordinates' frame: x along columns, y along rows, in
    cells from the centre of cell (0, 0)) against the passage counts at those cells, on in-raster tracks of 37 x 53.
    K8's test is dx*dx + dy*dy <= radius_cells * radius_cells in f64, and passage_r2 is the floor of that square:
      - the f64 sqrt(26) squares to 25.999999999999996, so it is r2 = 25 for both (a point at squared distance 26 is
        outside K8's disk as well);
      - the next f64 above it squares to 26.000000000000007: r2 = 26, the first disk that holds (5, 1)."""
    from ssrs_amd import presence, turbines
    shape = (37, 53)
    tracks = ref.walks(77, shape, np.random.default_rng(77).integers(0, 60, 90))
    assert all(((t >= 0) & (t < np.array(shape))).all() for t in tracks)
    c = dict(tracks=tracks, lead=0)
    traj, off = device_case(c, gpu)
    rng = np.random.default_rng(5)
    cells = rng.choice(shape[0] * shape[1], 40, replace=False)
    rr, cc = cells // shape[1], cells % shape[1]
    rr[:4], cc[:4] = (0, 0, 36, 36), (0, 52, 0, 52)                              # the corners: clipped disks
    xy = np.stack([cc, rr], 1).astype(np.float64)
    root = float(np.sqrt(26.))
    seen = {}
    for radius_cells in (root, float(np.nextafter(root, 6.))):
        r2 = presence.passage_r2(radius_cells, 1.)
        hits, _ = turbines.turbine_encounters(traj, off, xy, radius_cells, shape)
        per_turbine, _ = turbines.encounter_counts(hits, 40)
        counts = presence.compute_track_passage(traj, shape, r2, offsets=off)
        want = ref.passage(tracks, shape, r2)[0]
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), want)
        assert np.array_equal(per_turbine.cpu().numpy(), want[rr, cc].astype(np.int64)), r2
        seen[r2] = want[rr, cc]
    assert sorted(seen) == [25, 26] and not np.array_equal(seen[25], seen[26]) and int(seen[26].max()) > 1


DIRTY_CASES = ('basic_1x1_r3', 'basic_1x9_r83', 'basic_9x1_r26', 'basic_5x3_r35', 'basic_37x53_r26', 'basic_70x130_r25',
               'lengths_r26', 'borders_33', 'borders_257_r26', 'memset_path', 'lead_7', 'straight_1024', 'pingpong_4096')


@pytest.mark.parametrize('fill', FILLS, ids=[str(f) for f in FILLS])
def test_on_dirty_guarded_memory(gpu, fill):
    """As tests/test_gpu_dirty_memory.py: every tensor of the call (the workspace from torch.empty among them) in an arena
    of zeros, of 0xFF, and of what the case before left behind (two passes in one arena); the guards intact after every
    case, and the restatement's integers, so the same as on clean memory."""
    with dirty(fill) as arena:
        for _ in range(2 if fill == 'leavings' else 1):
            for name in DIRTY_CASES:
                for planes, shift in ((1, 0), (8, 3)):
                    run_case(ref.case(name), gpu, planes, shift)
                arena.assert_clean()
        assert arena.buffers and not arena.passed, (len(arena.buffers), arena.passed)
        if fill == 'leavings':
            assert arena.reused > 0, 'no buffer was handed out again'


KEY = ('s10d270', 0)
STEM = 's10d270_d0_t75_fluidflow_r0'


def test_simulator_end_to_end(gpu, tmp_path):
    from ssrs_amd import Config, Simulator, presence
    cfg = Config(run_name='pas', out_dir=str(tmp_path), sim_seed=1, region_width_km=(5., 4.), resolution=100.,
                 track_count=64, track_start_region=(1, 4, 0.2, 0.6), track_direction=0., track_passage_radius=250.,
                 save_tracks=True)
    sim = Simulator(cfg, terrain='synthetic')
    assert sim.gridsize == (40, 50) and presence.passage_r2(250., 100.) == 6
    with pytest.raises(ValueError, match='no track passage'):
        sim.compute_passage_map()
    sim.simulate_tracks()
    with open(os.path.join(sim.mode_data_dir, f'{STEM}_tracks.pkl'), 'rb') as f:
        tracks = pickle.load(f)
    assert len(tracks) == 64
    want, want_cells = ref.passage(tracks, (40, 50), 6)
    assert int(want.max()) > 1 and int(want.sum()) == int(want_cells.sum(dtype=np.int64))
    saved = np.load(os.path.join(sim.mode_data_dir, f'{STEM}_passage.npy'))
    assert saved.dtype == np.int32 and saved.shape == (40, 50) and np.array_equal(saved.view(np.uint32), want)
    kept = sim.track_passage_counts[KEY]
    assert isinstance(kept, np.ndarray) and kept.dtype == np.int32 and np.array_equal(kept, saved)
    share = sim.compute_passage_map()
    assert share.dtype == np.float32 and np.array_equal(share, (want / 64).astype(np.float32))
    assert share.max() <= 1. and share.min() >= 0.
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_passage.npy')), share)

    # switched off: no passage file, and the histogram and the tracks are the plain run's
    plain = Simulator(replace(cfg, run_name='p', track_passage_radius=0.), terrain='synthetic')
    plain.simulate_tracks()
    assert plain.track_passage_counts == {}
    assert not [f for f in os.listdir(plain.mode_data_dir) if 'passage' in f]
    assert torch.equal(plain._presence_counts[KEY], sim._presence_counts[KEY])
    with open(os.path.join(plain.mode_data_dir, f'{STEM}_tracks.pkl'), 'rb') as f:
        plain_tracks = pickle.load(f)
    assert len(plain_tracks) == 64 and all(np.array_equal(a, b) for a, b in zip(plain_tracks, tracks))
    with pytest.raises(ValueError, match='no track passage'):
        plain.compute_passage_map()
