"""Turbine encounters on the device (K8): which tracks came within R cells of which turbine, and at which step first.
The expected values are a brute-force NumPy evaluation of the header's expression, (c - xt)**2 + (r - yt)**2 <= R * R,
over ALL (point, turbine) pairs; every comparison is exact -- bitmaps, counts and first steps."""
import os
import pickle
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, COLS = 70, 90                         # 3 x 3 bins of 32 x 32 cells, neither side a multiple of 32
LENGTHS = [1, 1, 0, 2, 63, 64, 65, 255, 256, 257, 1000, 4097] + [3] * 300
RADII = [0., 0.5, 1.0, float(np.sqrt(2.)), 2.5, 5.0, 40.0]


def _walk(rng, n, start=None):
    """A random walk of n cells inside the raster, int16 (n, 2) [row, col]."""
    pos = np.array([rng.integers(0, ROWS), rng.integers(0, COLS)]) if start is None else np.array(start)
    steps = rng.integers(-1, 2, (n, 2))
    steps[:1] = 0
    out = pos + np.cumsum(steps, 0)
    # reflect at the raster's edges
    for ax, hi in ((0, ROWS - 1), (1, COLS - 1)):
        v = np.abs(out[:, ax]) % (2 * hi)
        out[:, ax] = np.where(v > hi, 2 * hi - v, v)
    return out.astype(np.int16)


def _synthetic():
    rng = np.random.default_rng(12)
    tracks = [_walk(rng, n) for n in LENGTHS]
    # turbine 0 sits on the centre of cell (row 20, col 30): its four neighbours are exactly on the circle of radius 1, the
    # offsets (3, 4) and (4, -3) exactly on the circle of radius 5, the diagonal neighbours inside sqrt(2)'s (2 < 2.0000000000000004)
    tracks[10][100:108] = [[20, 31], [20, 29], [21, 30], [19, 30], [23, 34], [24, 27], [21, 31], [19, 29]]
    tracks[11][:3] = [[20, 30], [25, 30], [20, 35]]           # distance 0 and exactly 5 along the axes
    # short tracks that begin ON turbines 1 .. 7 (a first step of 0, several tracks per wave span)
    for k, (r, c) in enumerate([(50, 40), (51, 41), (10, 60), (45, 15), (46, 17), (35, 89), (30, 0)]):
        tracks[20 + 3 * k] = _walk(rng, 3, (r, c))
    xy = np.zeros((70, 2))
    xy[:9] = [[30., 20.],              # a cell centre
              [40.5, 50.5],            # a cell corner
              [60., 10.], [60., 10.],  # two at the same position
              [15., 45.], [17., 46.],  # overlapping disks
              [89., 35.],              # on the raster's east edge
              [-2., 30.],              # outside, reaches in from radius 2 on
              [-200., -200.]]          # reaches nothing at any radius here
    xy[9:, 0] = rng.uniform(-5., COLS + 4., 61)
    xy[9:, 1] = rng.uniform(-5., ROWS + 4., 61)
    xy[9:40] = np.round(xy[9:40] * 2.) / 2.                   # many of them on centres, edges and corners of cells
    return tracks, xy


def _pack(tracks):
    off = np.concatenate(([0], np.cumsum([len(t) for t in tracks]))).astype(np.int64)
    traj = np.concatenate(tracks).astype(np.int16) if len(tracks) else np.zeros((0, 2), np.int16)
    return traj, off


def brute_force(traj, off, xy, radius):
    """(bitmap uint32 (ntracks, words), tracks_per_turbine int64, turbines_per_track int32, first_step int32)."""
    r, c = traj[:, 0].astype(np.int64), traj[:, 1].astype(np.int64)
    xt, yt = xy[None, :, 0], xy[None, :, 1]
    inside = (c[:, None] - xt) ** 2 + (r[:, None] - yt) ** 2 <= radius * radius          # (points, nturb)
    n, nturb = off.size - 1, xy.shape[0]
    words = (nturb + 31) // 32
    enc = np.zeros((n, words * 32), dtype=bool)
    first = np.full(n, -1, dtype=np.int32)
    for k in range(n):
        seg = inside[off[k]:off[k + 1]]
        enc[k, :nturb] = seg.any(0)
        where = np.nonzero(seg.any(1))[0]
        if where.size:
            first[k] = where[0]
    weights = (1 << np.arange(32, dtype=np.uint64))
    bitmap = (enc.reshape(n, words, 32) * weights).sum(2).astype(np.uint32)
    return bitmap, enc[:, :nturb].sum(0).astype(np.int64), enc[:, :nturb].sum(1).astype(np.int32), first


def check(got_hits, got_first, traj, off, xy, radius):
    from ssrs_amd import turbines as tb
    bitmap, per_turbine, per_track, first = brute_force(traj, off, xy, radius)
    hits = got_hits.cpu().numpy().view(np.uint32)
    assert np.array_equal(hits, bitmap), np.argwhere(hits != bitmap)[:8]
    got = got_first.cpu().numpy()
    assert np.array_equal(got, first), np.argwhere(got != first)[:8]
    a, b = tb.encounter_counts(got_hits, xy.shape[0])
    assert a.dtype == torch.int64 and b.dtype == torch.int32
    assert np.array_equal(a.cpu().numpy(), per_turbine) and np.array_equal(b.cpu().numpy(), per_track)
    return bitmap, per_turbine, first


@pytest.fixture(scope='module')
def synthetic(gpu):
    tracks, xy = _synthetic()
    traj, off = _pack(tracks)
    return dict(traj=traj, off=off, xy=xy, traj_dev=torch.from_numpy(traj).to(gpu), off_dev=torch.from_numpy(off).to(gpu))


@pytest.mark.parametrize('nturb', [1, 33, 70])
@pytest.mark.parametrize('radius', RADII)
def test_synthetic_trajectories_against_brute_force(synthetic, nturb, radius):
    from ssrs_amd import turbines as tb
    s = synthetic
    xy = s['xy'][:nturb]
    hits, first = tb.turbine_encounters(s['traj_dev'], s['off_dev'], xy, radius, (ROWS, COLS))
    assert tuple(hits.shape) == (len(LENGTHS), (nturb + 31) // 32) and hits.dtype == torch.int32
    bitmap, per_turbine, first_ref = check(hits, first, s['traj'], s['off'], xy, radius)
    if nturb == 70:
        # the cases the issue names are really in the data
        assert per_turbine[8] == 0 and (per_turbine[2] == per_turbine[3])
        assert per_turbine[0] >= (2 if radius >= 1. else 1) and per_turbine[6] >= 1
        assert (per_turbine[7] >= 1) == (radius >= 2.)                        # the one outside reaches in from 2 cells on
        assert first_ref[2] == -1 and (first_ref == 0).sum() >= 5            # the empty track; tracks that start on a turbine
    if radius in (1.0, 5.0) and nturb == 1:
        t10 = s['traj'][s['off'][10]:s['off'][11]].astype(np.float64)
        d2 = (t10[:, 1] - 30.) ** 2 + (t10[:, 0] - 20.) ** 2
        assert (d2 == radius * radius).any()                                  # points exactly ON the circle, and they count
        assert bitmap[10, 0] == 1


def test_unaligned_buffer_and_caller_bins(synthetic, gpu):
    """A trajectory buffer that is only 4-byte aligned takes the scalar loads; cull lists given by the caller (numpy or
    device tensors) give the same bitmap as the ones built inside; a list that omits a turbine loses its hits."""
    from ssrs_amd import turbines as tb
    s = synthetic
    xy, radius = s['xy'], 2.5
    shifted = torch.cat([torch.zeros((1, 2), dtype=torch.int16, device=gpu), s['traj_dev']])[1:]
    assert shifted.data_ptr() % 16 == 4
    hits, first = tb.turbine_encounters(shifted, s['off_dev'], xy, radius, (ROWS, COLS))
    check(hits, first, s['traj'], s['off'], xy, radius)
    bins = tb.build_bins(xy, radius, (ROWS, COLS))
    for given in (bins, tuple(torch.from_numpy(b).to(gpu) for b in bins)):
        h2, f2 = tb.turbine_encounters(s['traj_dev'], s['off_dev'], xy, radius, (ROWS, COLS), bins=given)
        assert torch.equal(h2, hits) and torch.equal(f2, first)
    lists = [bins[1][bins[0][b]:bins[0][b + 1]] for b in range(bins[0].size - 1)]
    lists = [items[items != 0] for items in lists]
    without0 = (np.concatenate(([0], np.cumsum([items.size for items in lists]))).astype(np.int32),
                np.concatenate(lists).astype(np.int32))
    h3, _ = tb.turbine_encounters(s['traj_dev'], s['off_dev'], xy, radius, (ROWS, COLS), bins=without0)
    want = hits.clone()
    want[:, 0] &= ~1
    assert torch.equal(h3, want) and not torch.equal(h3, hits)
    with pytest.raises(ValueError, match='bin_start'):
        tb.turbine_encounters(s['traj_dev'], s['off_dev'], xy, radius, (ROWS, COLS), bins=(bins[0][:-1], bins[1]))
    with pytest.raises(ValueError):
        tb.turbine_encounters(s['traj_dev'], s['off_dev'], xy, -1., (ROWS, COLS))


def test_a_track_trapped_inside_a_disk(gpu):
    """200 000 points that alternate between two cells inside a disk (what a trap cell of a solved 10 m field does to a
    track), short tracks before and after: one run, exact results."""
    from ssrs_amd import turbines as tb
    rng = np.random.default_rng(4)
    trap = np.empty((200_000, 2), dtype=np.int16)
    trap[0::2], trap[1::2] = (20, 30), (20, 31)
    trap[:7] = [[14, 30], [15, 30], [16, 30], [17, 30], [18, 30], [19, 30], [20, 30]]       # walks in: first step 4 at R = 2.5
    tracks = [_walk(rng, 3) for _ in range(5)] + [_walk(rng, 3, (20, 30))] + [trap] + [_walk(rng, 3, (21, 31))] + \
        [_walk(rng, 3) for _ in range(5)]
    traj, off = _pack(tracks)
    xy = np.array([[30., 20.], [31.5, 20.5], [60., 60.]])
    hits, first = tb.turbine_encounters(torch.from_numpy(traj).to(gpu), torch.from_numpy(off).to(gpu), xy, 2.5, (ROWS, COLS))
    bitmap, per_turbine, first_ref = check(hits, first, traj, off, xy, 2.5)
    assert bitmap[6, 0] == 3 and first_ref[6] == 4 and first_ref[5] == 0 and first_ref[7] == 0


def test_accumulation_over_calls_and_slices(synthetic, gpu):
    """Tracks [0, k) and [k, n) as two calls into slices of one hits / first_step equal one call; a second call over the
    same tracks changes nothing (hits are ORed, first steps min-ed)."""
    from ssrs_amd import turbines as tb
    s = synthetic
    xy, radius, n = s['xy'], 2.5, len(LENGTHS)
    one_h, one_f = tb.turbine_encounters(s['traj_dev'], s['off_dev'], xy, radius, (ROWS, COLS))
    for k in (9, 11, 150):                         # inside the long tracks; inside the run of short ones
        hits = torch.zeros((n, 3), dtype=torch.int32, device=gpu)
        first = torch.full((n,), -1, dtype=torch.int32, device=gpu)
        tb.turbine_encounters(s['traj_dev'], s['off_dev'][:k + 1], xy, radius, (ROWS, COLS), hits=hits[:k], first_step=first[:k])
        assert not hits[k:].any() and (first[k:] == -1).all()
        tb.turbine_encounters(s['traj_dev'], s['off_dev'][k:], xy, radius, (ROWS, COLS), hits=hits[k:], first_step=first[k:])
        assert torch.equal(hits, one_h) and torch.equal(first, one_f)
    again_h, again_f = tb.turbine_encounters(s['traj_dev'], s['off_dev'], xy, radius, (ROWS, COLS),
                                             hits=one_h.clone(), first_step=one_f.clone())
    assert torch.equal(again_h, one_h) and torch.equal(again_f, one_f)
    # turbines of a second call are ORed into the same bitmap: [0, 33) then all 70 is all 70
    part_h, part_f = tb.turbine_encounters(s['traj_dev'], s['off_dev'], np.concatenate([xy[:33], np.full((37, 2), -1e6)]),
                                           radius, (ROWS, COLS))
    both_h, both_f = tb.turbine_encounters(s['traj_dev'], s['off_dev'], xy, radius, (ROWS, COLS), hits=part_h, first_step=part_f)
    assert torch.equal(both_h, one_h) and torch.equal(both_f, one_f)


def test_iter_device_chunks_serves_the_encounters(gpu):
    """The smoke inputs with a pool too small to record and a budget too small for one tensor: iter_device_chunks() hands
    over the replay ranges on the device; they concatenate to tracks(), and the encounters computed range by range into
    slices of one bitmap equal those of the run that holds its trajectory tensor."""
    from ssrs_amd import layers, movmodel
    from ssrs_amd import turbines as tb
    from ssrs_amd.synthetic import synthetic_dem
    from oracle import ssrs_oracle as orc
    rows, cols, res = 96, 128, 100.
    oro, _ = layers.updraft_from_dem(synthetic_dem((rows, cols), res), res, 10., 270., threshold=0.75)
    upd = orc.get_above_threshold_speed(oro, 0.75)
    pot = orc.solve_potential(upd, 0.)
    rng = np.random.default_rng(0)
    starts = np.stack([rng.integers(1, 12, 256), rng.integers(0, cols, 256)], 1)
    whole = movmodel.simulate_tracks(0., starts, (rows, cols), 1, 1., upd, pot, seed=30, want_tracks=True)
    assert whole.traj is not None
    one = list(whole.iter_device_chunks())
    assert len(one) == 1 and one[0][:2] == (0, 256) and one[0][2] is whole.traj and one[0][3] is whole.offsets
    ranged = movmodel.simulate_tracks(0., starts, (rows, cols), 1, 1., upd, pot, seed=30, want_tracks=True,
                                      record_pool_bytes=4096, traj_budget_bytes=16 * 1024)
    assert ranged.traj is None
    ref_tracks = whole.tracks()
    xy = np.stack([rng.uniform(0., cols - 1., 40), rng.uniform(0., rows - 1., 40)], 1)
    hits = torch.zeros((256, 2), dtype=torch.int32, device=gpu)
    first = torch.full((256,), -1, dtype=torch.int32, device=gpu)
    nchunks, nxt = 0, 0
    for t0, t1, traj, off in ranged.iter_device_chunks():
        assert t0 == nxt and t1 > t0 and traj.is_cuda and off.is_cuda and traj.dtype == torch.int16 and off.dtype == torch.int64
        assert int(off[0]) == 0 and off.numel() == t1 - t0 + 1 and int(off[-1]) == traj.shape[0]
        got = list(movmodel.TrackBatch.host_tracks(traj, off))
        assert len(got) == t1 - t0 and all(np.array_equal(a, b) for a, b in zip(got, ref_tracks[t0:t1]))
        tb.turbine_encounters(traj, off, xy, 3.0, (rows, cols), hits=hits[t0:t1], first_step=first[t0:t1])
        nchunks, nxt = nchunks + 1, t1
    assert nxt == 256 and nchunks >= 2
    h1, f1 = tb.turbine_encounters(whole.traj, whole.offsets, xy, 3.0, (rows, cols))
    assert torch.equal(hits, h1) and torch.equal(first, f1) and bool(h1.any())
    check(h1, f1, whole.traj.cpu().numpy(), whole.offsets.cpu().numpy(), xy, 3.0)


def _turbine_table():
    # 60 x 80 cells at 100 m from (0, 0): bounds (0, 0, 7900, 5900); the tracks start in rows 2 .. 6 and head north
    return dict(x=[2000., 3050., 4000., 5000., 5500., 6010., 9000., 4000.],
                y=[700., 900., 1500., 800., 1250., 2000., 1000., 2000.],
                p_name=['A', 'A', 'A', 'B', 'B', 'B', 'B', 'A'],
                t_hh=[80., 80., 50., 80., 80., 80., 80., 30.],         # the seventh lies outside, the eighth is too low
                t_rd=[100.] * 8)


def test_simulator_end_to_end(gpu, tmp_path, capsys):
    from ssrs_amd import Simulator
    from oracle import ssrs_oracle as orc
    from test_gpu_simulator import make_config
    cfg = make_config(tmp_path, turbine_encounter_radius=150.)
    sim = Simulator(cfg, terrain='synthetic', turbines=_turbine_table())
    assert len(sim.turbines) == 6 and list(sim.turbines.get_project_names()) == ['A', 'B']
    sim.simulate_tracks()
    key = ('s10d270', 0)
    stem = os.path.join(sim.mode_data_dir, 's10d270_d0_t75_fluidflow_r0')
    with open(f'{stem}_tracks.pkl', 'rb') as f:
        tracks = pickle.load(f)
    assert len(tracks) == 200
    traj, off = _pack(tracks)
    xy = sim.turbines.cell_coordinates(sim.bounds, 100.)
    assert np.array_equal(xy, np.array([[20., 7.], [30.5, 9.], [40., 15.], [50., 8.], [55., 12.5], [60.1, 20.]]))
    _, per_turbine, per_track, first = brute_force(traj, off, xy, 1.5)
    assert per_turbine.sum() > 0 and (per_turbine > 0).sum() >= 3              # the run does meet turbines
    enc = sim.turbine_encounters[key]
    assert enc['tracks_per_turbine'].dtype == np.int64 and np.array_equal(enc['tracks_per_turbine'], per_turbine)
    assert enc['turbines_per_track'].dtype == np.int32 and np.array_equal(enc['turbines_per_track'], per_track)
    assert enc['first_step'].dtype == np.int32 and np.array_equal(enc['first_step'], first)
    saved = np.load(f'{stem}_turbine_encounters.npy')
    assert saved.dtype == np.int64 and np.array_equal(saved, per_turbine)
    share = sim.compute_turbine_encounters()
    assert share.dtype == np.float64 and np.array_equal(share, np.mean([per_turbine / 200.], axis=0))
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'summary_turbine_encounters.npy')), share)

    # the same run without the pickle: the trajectories are still produced on the device, the encounters are the same
    quiet = Simulator(replace(cfg, run_name='q', save_tracks=False), terrain='synthetic', turbines=_turbine_table())
    quiet.simulate_tracks()
    assert not [f for f in os.listdir(quiet.mode_data_dir) if f.endswith('.pkl')]
    for name in ('tracks_per_turbine', 'turbines_per_track', 'first_step'):
        assert np.array_equal(quiet.turbine_encounters[key][name], enc[name]), name
    assert torch.equal(quiet._presence_counts[key], sim._presence_counts[key])
    assert np.array_equal(quiet.compute_turbine_encounters(), share)

    # ---- the wind-plant map: the ladder at krad = int(2.7) = 2, cropped to the project's turbines +- pad
    counts = np.zeros((60, 80), dtype=np.int64)
    np.add.at(counts, (traj[:, 0].astype(int), traj[:, 1].astype(int)), 1)
    window, (r0, r1, c0, c1) = sim.compute_windplant_presence_map('A', radius=270., pad=500.)
    # project A inside the bounds: x 2000 .. 4000, y 700 .. 1500 -> centres 100 c in [1500, 4500], 100 r in [200, 2000]
    assert (r0, r1, c0, c1) == (2, 21, 15, 46)
    sm = orc.smooth_presence_from_counts(counts, 2)
    sm = sm / sm.max()
    sm = sm / sm.max()
    assert window.dtype == np.float32 and window.shape == (19, 31)
    np.testing.assert_allclose(window, (sm / sm.max())[2:21, 15:46], rtol=1e-6, atol=1e-7)
    assert np.array_equal(np.load(os.path.join(sim.mode_data_dir, 'presence_A.npy')), window)
    assert not os.path.exists(os.path.join(sim.mode_data_dir, 'summary_presence.npy'))
    rounded = sim.compute_presence_map(radius=270.)                            # krad = round(2.7) = 3: another map
    assert not np.allclose(rounded[2:21, 15:46], window, rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError, match='nowhere'):
        sim.compute_windplant_presence_map('nowhere')
    capsys.readouterr()
    sim.plot_windplant_presence_map('B', radius=270., pad=500.)
    assert os.path.exists(os.path.join(sim.mode_data_dir, 'presence_B.npy'))
    assert 'no-op' not in capsys.readouterr().out

    # ---- without turbines nothing changes: the stub's line, no encounters, and the error that says why
    plain = Simulator(replace(cfg, run_name='p', turbine_encounter_radius=0.), terrain='synthetic')
    assert plain.turbines is None
    capsys.readouterr()
    plain.plot_windplant_presence_map('A')
    assert 'plot_windplant_presence_map: plotting is outside the hot-path scope of this build (no-op)' in capsys.readouterr().out
    with pytest.raises(ValueError, match='no turbine encounters'):
        plain.compute_turbine_encounters()


def test_raster_too_large_for_the_lds_mask(gpu):
    """20 000 x 20 000 cells are 625 x 625 = 390 625 bins, more than the 262 144 whose occupied-bin mask fits LDS: the
    kernel reads bin_start per point instead.  Aligned and unaligned buffer, points all over the raster and around the
    turbines, a point outside the raster (it encounters nothing)."""
    from ssrs_amd import turbines as tb
    rows = cols = 20000
    rng = np.random.default_rng(21)
    xy = np.array([[17000., 15000.], [17003.5, 15002.5], [19999., 19999.], [0., 0.], [31.5, 19000.2], [-3., 8000.]])
    tracks = []
    for n in (1, 0, 300, 64, 257, 5, 5, 5, 700):
        t = np.stack([rng.integers(0, rows, n), rng.integers(0, cols, n)], 1)
        near = rng.random(n) < 0.5                      # half of the points within a few cells of some turbine
        which = xy[rng.integers(0, len(xy), n)]
        t[near, 0] = np.clip(np.round(which[near, 1]) + rng.integers(-4, 5, near.sum()), 0, rows - 1)
        t[near, 1] = np.clip(np.round(which[near, 0]) + rng.integers(-4, 5, near.sum()), 0, cols - 1)
        tracks.append(t.astype(np.int16))
    traj, off = _pack(tracks)
    for radius in (0., 3.0):
        for shift in (0, 1):
            dev = torch.cat([torch.zeros((shift, 2), dtype=torch.int16, device=gpu), torch.from_numpy(traj).to(gpu)])[shift:]
            hits, first = tb.turbine_encounters(dev, torch.from_numpy(off).to(gpu), xy, radius, (rows, cols))
            _, per_turbine, _ = check(hits, first, traj, off, xy, radius)
            assert (per_turbine > 0).sum() >= (4 if radius else 1)
    # a point outside the raster (row 20000 of a raster declared 20000 rows high is one past the end) encounters nothing
    out = np.array([[15000, 17000], [20000, 17000]], dtype=np.int16)
    hits, first = tb.turbine_encounters(torch.from_numpy(out).to(gpu), torch.tensor([0, 1, 2], device=gpu), np.array([[17000., 20000.]]),
                                        5000., (rows, cols))
    assert hits.cpu().numpy().view(np.uint32).tolist() == [[1], [0]] and first.cpu().numpy().tolist() == [0, -1]


def test_more_spans_than_the_minimum_per_wave(gpu):
    """7e6 points: more than 1536 blocks x 4 waves x 4 spans x 256 points, so every wave walks more than the minimum number
    of spans and the grid is full.  One 3e6-point track, 2600 of 1000 points, 20 000 of 7 and one of 1.3e6."""
    from ssrs_amd import turbines as tb
    lengths = [3_000_000] + [1000] * 2600 + [7] * 20_000 + [1_300_000]
    assert sum(lengths) > 1536 * 4 * 4 * 256
    rng = np.random.default_rng(6)
    walk = _walk(rng, sum(lengths))
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    xy = np.array([[30., 20.], [40.5, 50.5], [88., 68.], [-2., 30.]])
    hits, first = tb.turbine_encounters(torch.from_numpy(walk).to(gpu), torch.from_numpy(off).to(gpu), xy, 2.5, (ROWS, COLS))
    # brute force, vectorised over the tracks (none is empty): any() per track and the first point inside any disk
    r, c = walk[:, 0].astype(np.float64), walk[:, 1].astype(np.float64)
    inside = (c[:, None] - xy[None, :, 0]) ** 2 + (r[:, None] - xy[None, :, 1]) ** 2 <= 2.5 * 2.5
    enc = np.logical_or.reduceat(inside, off[:-1], axis=0)
    bitmap = (enc * (1 << np.arange(4))).sum(1).astype(np.uint32)[:, None]
    idx = np.where(inside.any(1), np.arange(walk.shape[0]), np.iinfo(np.int64).max)
    first_idx = np.minimum.reduceat(idx, off[:-1])
    first_ref = np.where(enc.any(1), first_idx - off[:-1], -1).astype(np.int32)
    assert np.array_equal(hits.cpu().numpy().view(np.uint32), bitmap)
    assert np.array_equal(first.cpu().numpy(), first_ref)
    per_turbine, per_track = tb.encounter_counts(hits, 4)
    assert np.array_equal(per_turbine.cpu().numpy(), enc.sum(0)) and np.array_equal(per_track.cpu().numpy(), enc.sum(1))
    assert enc[0].all() or enc[0, :3].all()                      # the long tracks do meet turbines
