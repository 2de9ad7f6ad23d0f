"""K22 on the MI355X: movmodel.score_tracks_profile (ssrs_tracks_score_profile through the C ABI) against K21 on the same
device -- every integer equal, no tolerance: the same arithmetic from the same header -- and against tests/score_ref.py
looped over the grid (the counts exactly, S within one unit per SCORED move, score_ref.s_bound_ok); on dirty, guarded
memory; on a side stream; movmodel.fit_tracks on the reference's own runs; and Simulator.fit_tracks."""
import dataclasses
import os
import pickle

import numpy as np
import pytest
import torch

import score_profile_ref as pref
import score_ref as ref
import stream_order
from dirty_memory import dirty
from test_gpu_score import place

pytestmark = pytest.mark.gpu

MEMORIES, NUS = pref.DEVICE_GRID
CASES = ('7x9_m8_nu1', '12x40_upd_m3', '12x40_drw_m8_nu0.5', 'huge_potential', 'nan_updraft', 'tiny_updraft', 'g7_m8')


def placed(c, device, tracks=None, lead=None, shift=None):
    """(traj on the device at the case's placement, offsets on the device)."""
    traj, offsets = ref.flat(c['tracks'] if tracks is None else tracks, c['lead'] if lead is None else lead)
    return place(traj, c['shift'] if shift is None else shift, device), torch.from_numpy(offsets).to(device)


def profile(c, device, memories=MEMORIES, nus=NUS, **kw):
    from ssrs_amd import movmodel
    view, off = placed(c, device, **kw)
    return movmodel.score_tracks_profile(view, c['shape'], c['move_dirn'], memories, nus, c['updraft'], c['potential'], offsets=off)


def k21(c, device, memory, nu, **kw):
    """K21's rows under (memory, nu), int64 numpy (ntracks, 6)."""
    from ssrs_amd import movmodel
    view, off = placed(c, device, **kw)
    return movmodel.score_tracks(view, c['shape'], c['move_dirn'], memory, nu, c['updraft'], c['potential'], offsets=off,
                                 want_p=False, want_status=False).rows.cpu().numpy()


@pytest.mark.parametrize('name', CASES)
def test_profile_equals_k21_integer_for_integer(gpu, name):
    """profile.row(m, nu) is score_tracks(..., m, nu).rows in all six columns, on dirty, guarded memory under both fills."""
    c = ref.case(name)
    want = {(m, nu): k21(c, gpu, m, nu) for m in MEMORIES for nu in set(NUS)}
    for fill in (0xFF, 'leavings'):
        with dirty(fill) as arena:
            got = profile(c, gpu)
            assert got.rows.dtype == torch.int64 and tuple(got.rows.shape) == (len(c['tracks']), len(MEMORIES), len(NUS), 6)
            assert got.memories == MEMORIES and got.nus.tolist() == list(NUS)
            for (m, nu), rows in want.items():
                assert np.array_equal(got.row(m, nu), rows), (fill, m, nu)
            assert np.array_equal(got.host_rows()[:, :, 2], got.host_rows()[:, :, 4])      # nu = 1 twice
            arena.assert_clean()
            assert arena.buffers


@pytest.mark.parametrize('name', CASES)
def test_profile_against_the_reference_definition(gpu, name):
    c = ref.case(name)
    pref.check(profile(c, gpu).host_rows(), pref.expected(c, MEMORIES, NUS))


def test_independence_of_placement_order_and_chunking(gpu):
    """Every placement of traj and remainder of the first offset; one call equals two calls over two halves; a permutation
    of the tracks permutes the rows; a second run gives identical integers."""
    c = ref.case('g7_m8')
    tracks = c['tracks']
    n = len(tracks)
    whole = profile(c, gpu).host_rows()
    pref.check(whole, pref.expected(c, MEMORIES, NUS))
    with dirty(0xFF) as arena:
        for shift in range(4):
            for lead in ((0, 1, 2, 3, 6) if shift == 0 else (c['lead'],)):
                assert np.array_equal(profile(c, gpu, shift=shift, lead=lead).host_rows(), whole), (shift, lead)
        arena.assert_clean()
    halves = [profile(c, gpu, tracks=tracks[:n // 2]).host_rows(), profile(c, gpu, tracks=tracks[n // 2:], lead=2, shift=3).host_rows()]
    assert np.array_equal(np.concatenate(halves), whole)
    order = np.random.default_rng(3).permutation(n)
    assert np.array_equal(profile(c, gpu, tracks=[tracks[k] for k in order], shift=1).host_rows(), whole[order])
    assert np.array_equal(profile(c, gpu).host_rows(), whole)
    # the list form equals the tensor form; memories come sorted and de-duplicated; the order of the nus is the caller's
    from ssrs_amd import movmodel
    listed = movmodel.score_tracks_profile(tracks, c['shape'], c['move_dirn'], (8, 3, 1, 3), (2., .5), c['updraft'], c['potential'])
    assert listed.memories == (1, 3, 8)
    assert np.array_equal(listed.host_rows(), whole[:, [0, 2, 4]][:, :, [3, 1]])
    empty = movmodel.score_tracks_profile([], c['shape'], 0., (1, 2), (1.,))
    assert tuple(empty.rows.shape) == (0, 2, 1, 6)
    none = movmodel.score_tracks_profile([np.zeros((0, 2), dtype=np.int16)] * 3, c['shape'], 0., (1, 2), (1.,))
    assert tuple(none.rows.shape) == (3, 2, 1, 6) and not none.rows.any()


def test_long_tracks_and_many_segments(gpu):
    """A track across eight blocks, forty tracks inside one block, empty tracks between them."""
    rng = np.random.default_rng(8)
    c = ref.case('g7_m1')
    tracks = [ref.forward(2000, ref.G7_SHAPE, rng)] + [ref.forward(13, ref.G7_SHAPE, rng) for _ in range(40)] + \
        [np.zeros((0, 2), dtype=np.int16)] * 3 + [ref.forward(600, ref.G7_SHAPE, rng)]
    memories, nus = (1, 2, 3, 4, 8), (1., .5)
    with dirty(0xFF) as arena:
        got = profile(c, gpu, memories, nus, tracks=tracks, lead=1, shift=2)
        pref.check(got.host_rows(), pref.expected(c, memories, nus, tracks))
        arena.assert_clean()
    for m, nu in ((1, 1.), (8, .5)):
        assert np.array_equal(got.row(m, nu), k21(c, gpu, m, nu, tracks=tracks, lead=1, shift=2))


def test_every_launch_goes_to_the_callers_stream(gpu):
    """include/ssrs_score_profile.h is outside the glob that tests/test_gpu_stream_order.py parses, so the contract is
    pinned here, as tests/test_gpu_score.py pins K21's: traj holds zeros; on the side stream a delay and then the copy of
    the real points are enqueued, on the null stream a longer delay; score_tracks_profile runs on the side stream, which
    alone is synchronised.  A read-back, a memset or a launch on another stream reads the zeros or is overtaken; a launch
    on the null stream runs after the consumer has read its rows."""
    from ssrs_amd import movmodel
    side, _ = stream_order.side_stream()
    assert side is not None, f'none of {stream_order.CANDIDATES} fresh streams separates from the null stream'
    c = ref.case('g7_m1')
    memories, nus = (1, 3), (1., .5, 1.)
    want = pref.expected(c, memories, nus)
    traj, offsets = ref.flat(c['tracks'], 0)
    real = torch.from_numpy(traj).to(gpu)
    held = torch.zeros_like(real)
    off = torch.from_numpy(offsets).to(gpu)
    upd = torch.from_numpy(c['updraft']).to(gpu)
    pot = torch.from_numpy(c['potential']).to(gpu)
    stream_order.cycles_per_ms()
    torch.cuda.synchronize()
    try:
        stream_order.delay(torch.cuda.default_stream(), 4 * stream_order.DELAY_MS)
        a, b = stream_order.delay(side, timed=True)
        with torch.cuda.stream(side):
            held.copy_(real)
            res = movmodel.score_tracks_profile(held, c['shape'], c['move_dirn'], memories, nus, upd, pot, offsets=off)
            got = res.host_rows()                          # (a blocking copy on the side stream: it alone is waited for)
            side.synchronize()
        pref.check(got, want)
        assert a.elapsed_time(b) >= stream_order.DELAY_MS
    finally:
        torch.cuda.synchronize()


def test_the_limits_eight_memories_thirty_two_nus(gpu):
    c = ref.case('7x9_m1_nu1')
    memories, nus = tuple(range(1, 9)), np.linspace(0., 3.875, 32)
    assert nus[8] == 1.
    with dirty(0xFF) as arena:
        got = profile(c, gpu, memories, nus)
        arena.assert_clean()
    assert tuple(got.rows.shape) == (len(c['tracks']), 8, 32, 6)
    for m, k in ((1, 0), (8, 31), (4, 8), (6, 19)):
        assert np.array_equal(got.row(m, nus[k]), k21(c, gpu, m, float(nus[k]))), (m, k)


# ------------------------------------------------------------------------------------------------ the fit
# the reference's own runs (tests/golden/g7_tracks.npz), their first 24 tracks: what they were generated with, and what the
# oracle in numpy gives on memories (1, 2, 3, 4) x np.linspace(0, 2, 9) with zero_bits = inf: (memory, nu, bits)
FIT_MEMORIES, FIT_NUS = (1, 2, 3, 4), np.linspace(0., 2., 9)
FIT_TABLE = {'ff_m3': (3, 1.0, 2211.2), 'ff_m1_nu05': (1, 0.5, 3120.3), 'ff_d135_m2': (2, 1.25, 1396.7)}
_fit_cases = {}


def fit_case(tag):
    """(a case like score_ref's on the tag's first 24 tracks, its expected TrackProfile in numpy), computed once."""
    from ssrs_amd import movmodel
    if tag not in _fit_cases:
        tracks, dirn, _, _, upd, pot = ref.g7_case(tag)
        c = dict(name='fit_' + tag, shape=ref.G7_SHAPE, move_dirn=dirn, updraft=upd, potential=pot, tracks=tracks[:24])
        _fit_cases[tag] = (c, movmodel.TrackProfile(pref.expected(c, FIT_MEMORIES, FIT_NUS), FIT_MEMORIES, FIT_NUS))
    return _fit_cases[tag]


def fit(c, device, **kw):
    from ssrs_amd import movmodel
    return movmodel.fit_tracks(c['tracks'], c['shape'], c['move_dirn'], c['updraft'], c['potential'], memories=FIT_MEMORIES,
                               nus=FIT_NUS, **kw)


@pytest.mark.parametrize('tag', sorted(FIT_TABLE))
def test_fit_gives_back_what_the_reference_ran_with(gpu, tag):
    """One round on the grid: the device's best memory, best nu, bits and forbidden-move counts are the numpy oracle's,
    which are the table's."""
    c, want = fit_case(tag)
    moves = sum(len(t) - 1 for t in c['tracks'])
    memory, nu, bits = want.best()
    assert (memory, nu) == FIT_TABLE[tag][:2] and abs(bits - FIT_TABLE[tag][2]) <= .05
    # the runner-up is further away than the device can differ (one unit of 2^-32 bit per move either way; the gap is
    # 5.5, 17.2 and 0.24 bits)
    totals = np.sort(want.total_bits().reshape(-1))
    assert totals[1] - totals[0] > 2 * moves * 2. ** -32
    # at nu = 0 every combination costs moves * log2(9), to the rounding of s_j: all nine cells get 1 / 9, a forbidden one too
    assert (np.abs(want.total_bits()[:, 0] - moves * np.log2(9.)) <= moves * 2. ** -32).all() and not want.forbidden()[:, 0].any()
    if tag == 'ff_m3':                                     # only the true memory forbids none of the 2153 moves
        assert moves == 2153 and want.forbidden()[:, 4].tolist() == [4, 1, 0, 75]
    got = fit(c, gpu, rounds=1)
    last = got.profiles[-1]
    assert len(got.profiles) == 1 and got.memory == memory and got.nu == nu and not got.at_edge
    scored = int(last.row(memory, nu)[:, 1].sum())
    print(f'{tag}: memory {got.memory}, nu {got.nu}, bits {got.bits!r} (expected {bits!r}), scored {scored}')
    assert abs(got.bits - bits) <= scored * 2. ** -32
    assert np.array_equal(last.forbidden(), want.forbidden())
    pref.check(last.host_rows(), want.host_rows())
    # one round: the bracket is one spacing of the grid, inside nu's two neighbours, around or beside nu
    assert got.nu_hi - got.nu_lo == 2 / 8 and nu - 2 / 8 <= got.nu_lo <= nu <= got.nu_hi <= nu + 2 / 8
    # a price per forbidden move: the totals of the excluded memories turn finite and equal the formula
    excluded = ~np.isfinite(last.total_bits())
    assert excluded.any() and np.array_equal(excluded, want.forbidden() > 0)
    priced = last.total_bits(zero_bits=20.)
    total = last.host_rows().sum(0)
    assert np.isfinite(priced).all()
    assert np.array_equal(priced, total[..., 0] / 2. ** 32 + 20. * (total[..., 2] + total[..., 5]))
    assert np.array_equal(priced[~excluded], last.total_bits()[~excluded])


def numpy_zoom(c, rounds):
    """The fit restated on score_ref: (memory, nu) after `rounds` rounds of the zoom.  pow(0, nu) is 0 for every nu > 0, so
    a memory that forbids a move on round 1's grid forbids it on every later grid, whose nus are positive: those
    memories stay out (inf) without being evaluated again, which keeps this restatement to seconds."""
    nus, memories = FIT_NUS, FIT_MEMORIES
    for _ in range(rounds):
        total = pref.expected(c, memories, nus).sum(0)
        bits = np.where(total[..., 2] + total[..., 5] > 0, np.inf, total[..., 0] / 2. ** 32)
        a, b = np.unravel_index(int(np.argmin(bits)), bits.shape)
        memory, nu = memories[a], float(nus[b])
        memories = tuple(m for k, m in enumerate(memories) if not (total[k, nus > 0., 2] + total[k, nus > 0., 5]).any())
        nus = np.linspace(nus[max(b - 1, 0)], nus[min(b + 1, len(nus) - 1)], len(nus))
        assert nus[0] > 0.
    return memory, nu


@pytest.mark.parametrize('tag', sorted(FIT_TABLE))
def test_fit_three_rounds_zoom_on_the_same_memory(gpu, tag):
    """Three rounds: the numpy restatement's memory and nu; the last bracket is (2 / 8) * 2 / 8 * 2 / 8 = 0.015625 wide, the
    spacing of round 3's grid -- the closing profile at the two midpoints beside nu picks that half of the two spacings
    between nu's neighbours -- and holds the smallest of the oracle's totals on a grid four times finer between those
    neighbours, as convexity in nu says it must."""
    c, want = fit_case(tag)
    got = fit(c, gpu, rounds=3)
    memory, nu = numpy_zoom(c, 3)
    print(f'{tag}: memory {got.memory}, nu {got.nu!r} in [{got.nu_lo!r}, {got.nu_hi!r}]; numpy: memory {memory}, nu {nu!r}')
    assert len(got.profiles) == 3 and got.memory == memory == want.best()[0]
    assert got.nu_lo <= nu <= got.nu_hi and got.nu_lo <= got.nu <= got.nu_hi
    assert got.nu_hi - got.nu_lo == (2 / 8) * 2 / 8 * 2 / 8
    assert all(p.memories == FIT_MEMORIES and p.nus.size == 9 for p in got.profiles)
    assert got.bits <= got.profiles[0].best()[2]           # (a zoom's grid holds the best nu of the grid before)
    assert got.closing.memories == FIT_MEMORIES and got.closing.nus.tolist() == [got.nu - 2. ** -7, got.nu + 2. ** -7]
    fine = np.linspace(nu - 2. ** -6, nu + 2. ** -6, 9)
    bits = pref.expected(c, (memory,), fine).sum(0)[0, :, 0] / 2. ** 32
    print(f'{tag}: the oracle on the finer grid {bits.tolist()}')
    assert got.nu_lo <= fine[int(np.argmin(bits))] <= got.nu_hi


# ------------------------------------------------------------------------------------------------ the simulator
def test_simulator_fits_its_own_tracks(gpu, tmp_path):
    """The 50 x 60 synthetic uniform case of test_gpu_score.test_simulator_scores_its_own_tracks, both movement models: the
    file holds what was returned, every rows_total[a, b] is the summed file of score_tracks under that pair, the fitted
    memory forbids no move, metres in give the same fit as cells in, and the run's Config is as it was."""
    from ssrs_amd import Config, Simulator
    base = dict(out_dir=str(tmp_path), sim_seed=11, region_width_km=(6., 5.), resolution=100., track_count=24,
                track_start_region=(1, 5, 0.2, 0.6), track_direction=0., track_dirn_restrict=2)
    config_of = lambda sim: {f.name: getattr(sim, f.name) for f in dataclasses.fields(Config)}
    for model in ('fluidflow', 'drw'):
        sim = Simulator(Config(run_name=f'fit_{model}', movement_model=model, **base), terrain='synthetic')
        assert sim.gridsize == (50, 60)
        sim.simulate_tracks()
        case_id = sim.case_ids[0]
        with open(sim._get_tracks_fname(case_id, 0, sim.mode_data_dir) + '.pkl', 'rb') as f:
            tracks = pickle.load(f)
        before = config_of(sim)
        nus = np.linspace(0., 2., 5)
        got = sim.fit_tracks(tracks, nus=nus, rounds=2)
        assert repr(config_of(sim)) == repr(before) and sim.track_dirn_restrict == 2
        last = got.profiles[-1]
        saved = dict(np.load(os.path.join(sim.mode_data_dir, f'{sim._get_id_string(case_id, 0)}_track_fit.npz')))
        assert sorted(saved) == ['bits', 'memories', 'memory', 'nu', 'nu_hi', 'nu_lo', 'nus', 'rows_total']
        assert (int(saved['memory']), float(saved['nu']), float(saved['bits'])) == (got.memory, got.nu, got.bits)
        assert (float(saved['nu_lo']), float(saved['nu_hi'])) == (got.nu_lo, got.nu_hi) and got.nu_lo <= got.nu <= got.nu_hi
        assert saved['memories'].tolist() == [1, 2, 3, 4] == list(last.memories) and np.array_equal(saved['nus'], last.nus)
        assert saved['rows_total'].dtype == np.int64 and np.array_equal(saved['rows_total'], last.host_rows().sum(0))
        assert len(got.profiles) == 2 and np.array_equal(got.profiles[0].nus, nus)
        assert not last.row(got.memory, got.nu)[:, [2, 5]].any() and np.isfinite(got.bits)
        # the cells' centres in projected metres give the same fit.  Of the tracks whose every move is a unit move, that is:
        # a start on row 1 is relocated by two rows during the burn-in, the pickle then holds a jump of up to three rows, a
        # NOT_A_MOVE as cells, which the line walk of xy=True fills with moves the bird did not make (a step back among
        # them, which every memory forbids).  Starts are spread over rows 1 .. 6, so most tracks have none
        from ssrs_amd import movmodel
        clean = [t for t in tracks if np.array_equal(movmodel.rasterize_track(t[:, 0], t[:, 1]), t)]
        print(f'{model}: {len(clean)} of {len(tracks)} tracks hold unit moves only')
        assert len(clean) >= len(tracks) // 2
        west, south = float(sim.bounds[0]), float(sim.bounds[1])
        metres = [np.stack([west + t[:, 1] * 100., south + t[:, 0] * 100.], 1) for t in clean]
        cells = sim.fit_tracks(clean, nus=nus, rounds=2)
        again = sim.fit_tracks(metres, case_id, 0, xy=True, nus=nus, rounds=2)
        assert (again.memory, again.nu, again.bits) == (cells.memory, cells.nu, cells.bits) and np.isfinite(again.bits)
        assert np.array_equal(again.profiles[-1].host_rows(), cells.profiles[-1].host_rows())
        with pytest.raises(ValueError, match='case_id'):
            sim.fit_tracks(tracks, 'no_such_case')
        # every pair of the last round against the file that score_tracks writes under it
        for a, memory in enumerate(last.memories):
            for b, nu in enumerate(last.nus):
                sim.track_dirn_restrict, sim.track_stochastic_nu = memory, float(nu)
                sim.score_tracks(tracks)
                rows = np.load(os.path.join(sim.mode_data_dir, f'{sim._get_id_string(case_id, 0)}_track_scores.npy'))
                assert np.array_equal(rows.sum(0), saved['rows_total'][a, b]), (model, memory, nu)
