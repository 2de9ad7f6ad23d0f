"""K21 on the MI355X: movmodel.score_tracks (ssrs_tracks_score through the C ABI) against tests/score_ref.py, the
definition on the oracle's functions, on dirty, guarded memory; on the stepper's own tracks; on a side stream; and through
Simulator.score_tracks.  status, the counts and (nu in {0, 1}) p are compared exactly, S within one unit per SCORED move
(score_ref.s_bound_ok: derived from log2's error, not measured), p for other nu within RTOL_NU."""
import os
import pickle

import numpy as np
import pytest
import torch

import score_ref as ref
import stream_order
from dirty_memory import dirty

pytestmark = pytest.mark.gpu

# pow() is not reproducible across libms (test_gpu_tracks.test_nu_half_within_tolerance says the same of the stepper), so for
# nu outside {0, 1} p is compared with a relative bound: 8 x the largest relative difference to score_ref measured on these
# cases on the MI355X (profiles/track_score.md), the margin RTOL_AMP takes over its measured value.
RTOL_NU_MEASURED = 4.1858240471795136e-16       # the largest over the four nu cases (7x9_m1_nu2); under two ulp of p
RTOL_NU = 8 * RTOL_NU_MEASURED                   # 3.35e-15


def place(traj, shift, device):
    """traj (int16 (n, 2)) on the device at an address 4 * shift bytes past a 16-byte boundary."""
    raw = torch.zeros((traj.shape[0] + 12, 2), dtype=torch.int16, device=device)
    start = (-raw.data_ptr() % 16) // 4 + 4 + shift
    view = raw[start:start + traj.shape[0]]
    view.copy_(torch.from_numpy(traj))
    assert view.data_ptr() % 16 == 4 * (shift % 4) and view.is_contiguous()
    return view


def run(c, device, tracks=None, lead=None, shift=None, smap=True, cmap=True, **kw):
    """score_tracks on case c from a placed device tensor -> (dict like score_ref.score's, the TrackScores)."""
    from ssrs_amd import movmodel
    traj, offsets = ref.flat(c['tracks'] if tracks is None else tracks, c['lead'] if lead is None else lead)
    view = place(traj, c['shift'] if shift is None else shift, device)
    off = torch.from_numpy(offsets).to(device)
    res = movmodel.score_tracks(view, c['shape'], c['move_dirn'], c['memory'], c['nu'], c['updraft'], c['potential'],
                                offsets=off, surprisal_map=smap, scored_map=cmap, **kw)
    return host(res, offsets), res


def host(res, offsets):
    lo, hi = int(offsets[0]), int(offsets[-1])
    return dict(p=None if res.p is None else res.p.cpu().numpy()[lo:hi],
                status=None if res.status is None else res.status.cpu().numpy()[lo:hi],
                rows=res.rows.cpu().numpy(),
                surprisal_map=None if res.surprisal_map is None else res.surprisal_map.cpu().numpy(),
                scored_map=None if res.scored_map is None else res.scored_map.cpu().numpy().astype(np.int64))


def nu_difference(got, want):
    """The largest relative difference of p over the SCORED moves."""
    scored = want['status'] == ref.SCORED
    if not scored.any():
        return 0.
    return float(np.max(np.abs(got['p'][scored] - want['p'][scored]) / want['p'][scored]))


def check(c, got, want):
    if got['status'] is not None:
        assert np.array_equal(got['status'], want['status'])
    if got['p'] is not None:
        if c['nu'] in (0., 1.):
            assert np.array_equal(got['p'].view(np.uint64), want['p'].view(np.uint64)), 'p is bit-equal for nu in {0, 1}'
        else:
            rest = want['status'] != ref.SCORED
            assert np.array_equal(got['p'][rest].view(np.uint64), want['p'][rest].view(np.uint64))
            worst = nu_difference(got, want)
            print(f"{c['name']}: nu = {c['nu']:g}, largest relative difference of p {worst:.3e} (RTOL_NU {RTOL_NU:.3e})")
            assert worst <= RTOL_NU
    assert np.array_equal(got['rows'][:, 1:], want['rows'][:, 1:])
    assert ref.s_bound_ok(got['rows'], want['rows'])
    if c['nu'] not in (0., 1.):
        return                                             # (the maps of these cases follow p's own differences)
    if got['scored_map'] is not None:
        assert np.array_equal(got['scored_map'], want['scored_map'])
        assert int(got['rows'][:, 1].sum()) == int(got['scored_map'].sum())
    if got['surprisal_map'] is not None:
        assert (np.abs(got['surprisal_map'] - want['surprisal_map']) <= want['scored_map']).all()
        assert int(got['rows'][:, 0].sum()) == int(got['surprisal_map'].sum())


@pytest.mark.parametrize('name', ref.case_names())
def test_cases_on_dirty_guarded_memory(gpu, name):
    c = ref.case(name)
    want = ref.expected(c)
    for fill in (0xFF, 'leavings'):
        with dirty(fill) as arena:
            got, _ = run(c, gpu)
            check(c, got, want)
            arena.assert_clean()
            assert arena.buffers
    if c['nu'] == 0.:
        evaluated = np.isin(want['status'], (ref.SCORED, ref.ZERO, ref.UNDEFINED))
        assert evaluated.sum() > 100 and (got['p'][evaluated] == 1. / 9.).all()


def test_nu_cases_checksums(gpu):
    """For nu outside {0, 1} the device's own S and maps still add up: the two checksums."""
    for name in ('7x9_m2_nu0.5', '7x9_m1_nu2', '12x40_drw_m8_nu0.5', 'g7_m3_nu2'):
        c = ref.case(name)
        got, _ = run(c, gpu)
        assert int(got['rows'][:, 0].sum()) == int(got['surprisal_map'].sum())
        assert int(got['rows'][:, 1].sum()) == int(got['scored_map'].sum()) > 0
        assert np.array_equal(got['scored_map'], ref.expected(c)['scored_map'])


@pytest.mark.parametrize('name', ['7x9_m8_nu1', '12x40_upd_m3', 'g7_m8'])
def test_every_placement_and_output(gpu, name):
    """traj at 0, 4, 8 and 12 bytes past a 16-byte boundary, first offsets of every remainder modulo 4, and the optional
    outputs left out one by one."""
    c = ref.case(name)
    want = ref.expected(c)
    with dirty(0xFF) as arena:
        for shift in range(4):
            for lead in ((0, 1, 2, 3, 6) if shift == 0 else (c['lead'],)):
                check(c, run(c, gpu, shift=shift, lead=lead)[0], want)
        check(c, run(c, gpu, want_p=False)[0], want)
        check(c, run(c, gpu, want_status=False)[0], want)
        check(c, run(c, gpu, smap=None, cmap=None)[0], want)
        check(c, run(c, gpu, smap=None)[0], want)
        arena.assert_clean()


def test_list_of_tracks_and_host_views(gpu):
    """The list form (what TrackBatch.tracks() and the pickle give) equals the tensor form; loglik, bits_per_move, counts."""
    from ssrs_amd import movmodel
    c = ref.case('g7_m1')
    want = ref.expected(c)
    res = movmodel.score_tracks(c['tracks'], c['shape'], c['move_dirn'], c['memory'], c['nu'], c['updraft'], c['potential'],
                                surprisal_map=True, scored_map=True)
    off = res.offsets.cpu().numpy()
    assert off[0] == 0 and np.array_equal(np.diff(off), [len(t) for t in c['tracks']])
    check(c, host(res, off), want)
    rows = res.host_rows()
    assert np.allclose(res.loglik(), -np.log(2.) * rows[:, 0] / 2. ** 32, rtol=0, atol=0)
    scored = rows[:, 1] > 0
    assert np.array_equal(res.bits_per_move()[scored], rows[scored, 0] / 2. ** 32 / rows[scored, 1])
    assert np.isnan(res.bits_per_move()[~scored]).all() and (~scored).any()
    assert {k: v.tolist() for k, v in res.counts().items()} == \
        {name: want['rows'][:, k].tolist() for k, name in enumerate(ref.COLUMNS) if k > 0}
    # no tracks, and tracks without points: nothing to do
    empty = movmodel.score_tracks([], c['shape'], 0.)
    assert empty.rows.shape == (0, 6) and empty.p.numel() == 0
    none = movmodel.score_tracks([np.zeros((0, 2), dtype=np.int16)] * 3, c['shape'], 0.)
    assert none.rows.shape == (3, 6) and not none.rows.any()
    with pytest.raises(ValueError, match='whole history'):
        movmodel.score_tracks(c['tracks'], c['shape'], 0., memory_parameter=0)
    with pytest.raises(ValueError, match='memory_parameter = 9'):
        movmodel.score_tracks(c['tracks'], c['shape'], 0., memory_parameter=9)
    with pytest.raises(ValueError, match='potential_field needs updraft_field'):
        movmodel.score_tracks(c['tracks'], c['shape'], 0., potential_field=c['potential'])


def test_independence_of_order_and_chunking(gpu):
    """One call, two calls over two halves, a permuted order, with the maps accumulated across the calls: identical
    integers, the maps included."""
    c = ref.case('g7_m8')
    tracks = c['tracks']
    n = len(tracks)
    whole, _ = run(c, gpu)
    smap = torch.zeros(c['shape'], dtype=torch.int64, device=gpu)
    cmap = torch.zeros(c['shape'], dtype=torch.int32, device=gpu)
    first, _ = run(c, gpu, tracks=tracks[:n // 2], smap=smap, cmap=cmap)
    second, res = run(c, gpu, tracks=tracks[n // 2:], smap=smap, cmap=cmap, lead=2, shift=3)
    assert res.surprisal_map is smap and res.scored_map is cmap
    assert np.array_equal(np.concatenate([first['rows'], second['rows']]), whole['rows'])
    assert np.array_equal(np.concatenate([first['p'], second['p']]).view(np.uint64), whole['p'].view(np.uint64))
    assert np.array_equal(second['surprisal_map'], whole['surprisal_map']) and np.array_equal(second['scored_map'], whole['scored_map'])
    order = np.random.default_rng(3).permutation(n)
    mixed, _ = run(c, gpu, tracks=[tracks[k] for k in order], shift=1)
    assert np.array_equal(mixed['rows'], whole['rows'][order])
    assert np.array_equal(mixed['surprisal_map'], whole['surprisal_map']) and np.array_equal(mixed['scored_map'], whole['scored_map'])
    again, _ = run(c, gpu)
    for key in ('rows', 'surprisal_map', 'scored_map', 'status'):
        assert np.array_equal(again[key], whole[key])


def test_long_tracks_and_many_segments(gpu):
    """A track across eight blocks, forty tracks inside one block, empty tracks between them."""
    rng = np.random.default_rng(8)
    c = ref.case('g7_m1')
    tracks = [ref.forward(2000, ref.G7_SHAPE, rng)] + [ref.forward(13, ref.G7_SHAPE, rng) for _ in range(40)] + \
        [np.zeros((0, 2), dtype=np.int16)] * 3 + [ref.forward(600, ref.G7_SHAPE, rng)]
    with dirty(0xFF) as arena:
        check(c, run(c, gpu, tracks=tracks, lead=1, shift=2)[0], ref.expected(c, tracks))
        arena.assert_clean()


@pytest.mark.parametrize('tag', ['ff_m1', 'drw_d250_m3'])
def test_the_steppers_own_tracks_score_on_every_move(gpu, golden, tag):
    """simulate_tracks on G7's inputs, scored from the batch's own device tensors: every move is SCORED, and the rows are
    score_ref's on the golden trajectories (which the stepper reproduces)."""
    from ssrs_amd import movmodel
    g = golden('g7_tracks.npz')
    tracks, dirn, mem, nu, upd, pot = ref.g7_case(tag)
    starts = np.stack([g['start_rows'], g['start_cols']], 1)
    batch = movmodel.simulate_tracks(dirn, starts, ref.G7_SHAPE, mem, nu, upd, pot, seed=int(g['seed']), want_tracks=True)
    assert batch.traj is not None and int(batch.offsets[-1]) == sum(len(t) for t in tracks)
    res = movmodel.score_tracks(batch.traj, ref.G7_SHAPE, dirn, mem, nu, upd, pot, offsets=batch.offsets)
    want = ref.score(tracks, ref.G7_SHAPE, dirn, mem, nu, upd, pot)
    status = res.status.cpu().numpy()
    assert np.array_equal(status, want['status']) and set(status.tolist()) == {ref.SCORED, ref.LAST}
    assert np.array_equal(res.p.cpu().numpy().view(np.uint64), want['p'].view(np.uint64))
    rows = res.host_rows()
    assert np.array_equal(rows[:, 1:], want['rows'][:, 1:]) and ref.s_bound_ok(rows, want['rows'])
    assert np.array_equal(rows[:, 1], batch.lengths.cpu().numpy() - 1)


def test_every_launch_goes_to_the_callers_stream(gpu):
    """include/ssrs_score.h is outside the glob that tests/test_gpu_stream_order.py parses, so the contract is pinned here.
    traj holds zeros; on the side stream a delay and then the copy of the real points are enqueued, on the null stream a
    longer delay; score_tracks runs on the side stream, which alone is synchronised.  A read-back or a launch on another
    stream reads the zeros; a launch on the null stream runs after the consumer has read its outputs."""
    from ssrs_amd import movmodel
    side, _ = stream_order.side_stream()
    assert side is not None, f'none of {stream_order.CANDIDATES} fresh streams separates from the null stream'
    c = ref.case('g7_m1')
    want = ref.expected(c)
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
            res = movmodel.score_tracks(held, c['shape'], c['move_dirn'], c['memory'], c['nu'], upd, pot, offsets=off,
                                        surprisal_map=True, scored_map=True)
            got = host(res, offsets)                       # (blocking copies on the side stream: it alone is waited for)
            side.synchronize()
        check(c, got, want)
        assert a.elapsed_time(b) >= stream_order.DELAY_MS
    finally:
        torch.cuda.synchronize()


def test_simulator_scores_its_own_tracks(gpu, tmp_path):
    """A 50 x 60 synthetic uniform case: the pickled tracks of the run's own simulate_tracks all score; the file is the
    returned rows; metres in, the same cells out; with movement_model = 'drw' every p is the normalised masked prior."""
    from ssrs_amd import Config, Simulator
    base = dict(out_dir=str(tmp_path), sim_seed=11, region_width_km=(6., 5.), resolution=100., track_count=24,
                track_start_region=(1, 5, 0.2, 0.6), track_direction=0., track_dirn_restrict=2)
    for model in ('fluidflow', 'drw'):
        sim = Simulator(Config(run_name=f'score_{model}', movement_model=model, **base), terrain='synthetic')
        assert sim.gridsize == (50, 60)
        sim.simulate_tracks()
        case_id = sim.case_ids[0]
        with open(sim._get_tracks_fname(case_id, 0, sim.mode_data_dir) + '.pkl', 'rb') as f:
            tracks = pickle.load(f)
        assert len(tracks) == 24 and all(t.dtype == np.int16 for t in tracks)
        scores = sim.score_tracks(tracks)
        rows = scores.host_rows()
        assert np.array_equal(rows[:, 1], [len(t) - 1 for t in tracks]) and not rows[:, 2:].any() and rows[:, 1].sum() > 200
        saved = np.load(os.path.join(sim.mode_data_dir, f'{sim._get_id_string(case_id, 0)}_track_scores.npy'))
        assert saved.dtype == np.int64 and saved.shape == (24, 6) and np.array_equal(saved, rows)
        assert np.isfinite(scores.loglik()).all() and (scores.loglik() < 0).all()
        if model == 'drw':
            want = ref.score(tracks, sim.gridsize, 0., 2, 1.)
            assert np.array_equal(scores.p.cpu().numpy().view(np.uint64), want['p'].view(np.uint64))
            assert np.array_equal(rows[:, 1:], want['rows'][:, 1:]) and ref.s_bound_ok(rows, want['rows'])
        # the cells' centres in projected metres, every third fix: the line walk fills the gaps with unit moves
        west, south = float(sim.bounds[0]), float(sim.bounds[1])
        metres = [np.stack([west + t[::3, 1] * 100., south + t[::3, 0] * 100.], 1) for t in tracks]
        thinned = sim.score_tracks(metres, case_id, 0, xy=True)
        counts = thinned.counts()
        # (a start on row 1 is relocated by two rows while j <= burnin = 5, and a step along that row is then no unit move)
        assert (counts['not_a_move'] <= 6).all() and not counts['out'].any() and counts['scored'].sum() > 100
        assert int(thinned.offsets[-1]) >= sum(len(m) for m in metres)
        with pytest.raises(ValueError, match='case_id'):
            sim.score_tracks(tracks, 'no_such_case')
