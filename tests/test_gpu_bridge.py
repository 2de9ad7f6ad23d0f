"""K23 on the MI355X: movmodel.score_gaps (ssrs_tracks_bridge through the C ABI) against tests/bridge_ref.py, the unconfined
definition on the oracle's functions, on dirty, guarded memory; against K21 on the device for gaps of one move; against
itself by Chapman-Kolmogorov; over orders and chunks; on a side stream; and through Simulator.score_fixes.  Statuses are
compared exactly, g and arrivals bit for bit at nu in {0, 1} and within bridge_ref.bound(n) elsewhere (derived from K21's
bound on pow and the roundings of a step, not measured)."""
import math
import os
import pickle

import numpy as np
import pytest
import torch

import bridge_ref as ref
import score_ref as sref
import stream_order
from dirty_memory import dirty

pytestmark = pytest.mark.gpu


def host(res):
    return dict(g=res.g.cpu().numpy(), status=res.status.cpu().numpy(), surprisal=res.surprisal.cpu().numpy(),
                arrivals=None if res.arrivals is None else res.arrivals.cpu().numpy(), p=res.p())


def run(c, jobs=None, want_arrivals=True):
    from ssrs_amd import movmodel
    res = movmodel.score_gaps(c['jobs'] if jobs is None else jobs, c['shape'], c['move_dirn'], c['nu'], c['updraft'],
                              c['potential'], want_arrivals=want_arrivals)
    return host(res), res


@pytest.mark.parametrize('name', ref.case_names())
def test_cases_on_dirty_guarded_memory(gpu, name):
    c = ref.case(name)
    want = ref.expected(c)
    for fill in (0xFF, 'leavings'):
        with dirty(fill) as arena:
            got, res = run(c)
            ref.check(c, got, want, say=print)
            arena.assert_clean()
            assert arena.buffers
        assert ref.same_bits(got['p'], ref.sum9(got['g'].T))
        counts = np.bincount(want['status'], minlength=5)
        assert res.counts() == {name: int(counts[k]) for k, name in enumerate(('scored', 'zero', 'too_long', 'out', 'undefined'))}


def one_move_jobs(tracks, shape):
    """For every point past the burn-in of 8-connected tracks the job of the move that leaves it, with the move that
    arrived as the incoming state (4 after a gap, a rest or a start) -> (jobs, the point's index in the flat trajectory)."""
    burnin = int(min(shape) / 10)
    jobs, at, base = [], [], 0
    for track in tracks:
        pts = [(int(r), int(c)) for r, c in track]
        for i in range(burnin + 2, len(pts) - 1):
            d = (pts[i][0] - pts[i - 1][0], pts[i][1] - pts[i - 1][1])
            jobs.append(pts[i] + (ref.state_of(d) if sref.unit(d) else 4,) + pts[i + 1] + (1,))
            at.append(base + i)
        base += len(pts)
    return np.array(jobs, dtype=np.int32).reshape(-1, 6), np.array(at, dtype=np.int64)


@pytest.mark.parametrize('name', ['7x9_nu1', '7x9_nu0', '7x9_nu0.5', '7x9_nu2', '12x40_drw_d250_nu0.5', '12x40_ff_nu2', 'g7_nu1',
                                  'huge_potential'])
def test_one_move_is_k21_on_the_device(gpu, name):
    """n = 1: P equals score_tracks' p bit for bit at every nu -- the same device function on the same operands -- and the
    statuses correspond (a jump is K21's NOT_A_MOVE and a ZERO gap)."""
    from ssrs_amd import movmodel
    c = ref.case(name)
    rng = np.random.default_rng(31)
    tracks = [sref.walk(300, c['shape'], rng), sref.forward(200, c['shape'], rng), sref.walk(120, c['shape'], rng, rim=False)] + \
        sref.hand_made(c['shape'])
    k21 = movmodel.score_tracks(tracks, c['shape'], c['move_dirn'], 1, c['nu'], c['updraft'], c['potential'])
    jobs, at = one_move_jobs(tracks, c['shape'])
    assert len(jobs) > 500
    got, _ = run(c, jobs)
    p, status = k21.p.cpu().numpy()[at], k21.status.cpu().numpy()[at]
    maps = {sref.SCORED: ref.SCORED, sref.ZERO: ref.ZERO, sref.UNDEFINED: ref.UNDEFINED, sref.OUT: ref.OUT, sref.NOT_A_MOVE: ref.ZERO}
    inside = (jobs[:, 3] >= 0) & (jobs[:, 3] < c['shape'][0]) & (jobs[:, 4] >= 0) & (jobs[:, 4] < c['shape'][1])
    assert np.array_equal(got['status'], [maps[int(s)] if ok else ref.OUT for s, ok in zip(status, inside)])   # (a jump off the raster)
    assert ref.same_bits(got['p'], p) and ref.same_bits(got['arrivals'][:, 0], p)
    assert (status == sref.SCORED).sum() > 100 and len(set(jobs[:, 2].tolist())) == 9
    scored = status == sref.SCORED
    assert (np.abs(got['surprisal'][scored] - np.array([sref.surprisal(v) for v in p[scored]])) <= 1).all()


@pytest.mark.parametrize('name', ['7x9_nu0', '7x9_nu0.5', '12x40_ff_nu2', 'g7_nu1'])
def test_chapman_kolmogorov_through_the_api(gpu, name):
    """P_n(A -> B) against the sum over the states (x, d) after k moves of g_k(A -> x)[d] * P_{n-k}((x, d) -> B), every
    factor from score_gaps: the bound is bridge_ref.bound for n + 1 steps (n steps on either side and the product)."""
    c = ref.case(name)
    rows, cols = c['shape']
    want = ref.expected(c)
    picked = [j for j, st in zip(c['jobs'], want['status']) if st == ref.SCORED and 3 <= j[5] <= 16][:3]
    assert len(picked) == 3
    done = 0
    for ra, ca, s, rb, cb, n in (tuple(int(v) for v in j) for j in picked):
        for k in sorted({1, n // 2, n - 1}):
            cells = [(r, c_) for r in range(max(ra - k, 0), min(ra + k, rows - 1) + 1)
                     for c_ in range(max(ca - k, 0), min(ca + k, cols - 1) + 1)]
            first, _ = run(c, np.array([(ra, ca, s, r, c_, k) for r, c_ in cells], dtype=np.int32), want_arrivals=False)
            states = [(x, d, first['g'][i, d]) for i, x in enumerate(cells) for d in range(9) if first['g'][i, d] != 0.]
            second, _ = run(c, np.array([x + (d,) + (rb, cb, n - k) for x, d, _ in states], dtype=np.int32), want_arrivals=False)
            whole, _ = run(c, np.array([(ra, ca, s, rb, cb, n)], dtype=np.int32), want_arrivals=False)
            parts = math.fsum(m * p for (_, _, m), p in zip(states, second['p']))
            rel = abs(parts - whole['p'][0]) / whole['p'][0]
            print(f'{name}: n = {n}, k = {k}, {len(states)} states: relative difference {rel:.3e} (bound {ref.bound(n + 1):.3e})')
            assert whole['status'][0] == ref.SCORED and rel <= ref.bound(n + 1)
            done += 1
    assert done >= 4


def test_order_and_chunking(gpu):
    """Permuted jobs give permuted outputs bit for bit; 600 jobs (more than the CUs) equal the same jobs in three calls;
    no job and one job."""
    c = ref.case('12x40_ff_nu2')
    rng = np.random.default_rng(6)
    jobs = c['jobs'][rng.integers(0, len(c['jobs']), 600)]
    with dirty(0xFF) as arena:
        whole, _ = run(c, jobs)
        order = rng.permutation(600)
        mixed, _ = run(c, jobs[order])
        parts = [run(c, jobs[lo:hi])[0] for lo, hi in ((0, 1), (1, 257), (257, 600))]
        none, res = run(c, jobs[:0])
        arena.assert_clean()
    ref.check(c, whole, ref.score(c, jobs), jobs=jobs)
    for key in ('g', 'arrivals', 'p'):
        assert ref.same_bits(mixed[key], whole[key][order]), key
        assert ref.same_bits(np.concatenate([p[key] for p in parts]), whole[key]), key
    for key in ('status', 'surprisal'):
        assert np.array_equal(mixed[key], whole[key][order]) and np.array_equal(np.concatenate([p[key] for p in parts]), whole[key])
    assert none['g'].shape == (0, 9) and none['arrivals'].shape == (0, 32) and res.total_bits() == 0. and \
        res.counts() == dict.fromkeys(('scored', 'zero', 'too_long', 'out', 'undefined'), 0)


def test_every_launch_goes_to_the_callers_stream(gpu):
    """include/ssrs_bridge.h is outside the glob that tests/test_gpu_stream_order.py parses, so the contract is pinned here,
    as tests/test_gpu_score.py does for K21.  The jobs tensor holds zeros (every job TOO_LONG); on the side stream a delay and
    then the copy of the real jobs are enqueued, on the null stream a longer delay; score_gaps runs on the side stream, which
    alone is synchronised.  The scan, its read-back or the gaps' launch on another stream read the zeros; a launch on the
    null stream runs after the consumer has read its outputs."""
    from ssrs_amd import movmodel
    side, _ = stream_order.side_stream()
    assert side is not None, f'none of {stream_order.CANDIDATES} fresh streams separates from the null stream'
    c = ref.case('g7_nu1')
    want = ref.expected(c)
    real = torch.from_numpy(c['jobs']).to(gpu)
    held = torch.zeros_like(real)
    upd = torch.from_numpy(c['updraft']).to(gpu)
    pot = torch.from_numpy(c['potential']).to(gpu)
    stream_order.cycles_per_ms()
    torch.cuda.synchronize()
    try:
        stream_order.delay(torch.cuda.default_stream(), 4 * stream_order.DELAY_MS)
        a, b = stream_order.delay(side, timed=True)
        with torch.cuda.stream(side):
            held.copy_(real)
            res = movmodel.score_gaps(held, c['shape'], c['move_dirn'], c['nu'], upd, pot, want_arrivals=True)
            got = host(res)                                # (blocking copies on the side stream: it alone is waited for)
            side.synchronize()
        ref.check(c, got, want)
        assert a.elapsed_time(b) >= stream_order.DELAY_MS
    finally:
        torch.cuda.synchronize()


def test_simulator_scores_the_gaps_of_its_own_tracks(gpu, tmp_path):
    """A 50 x 60 synthetic uniform case with track_dirn_restrict = 1: the run's own tracks past their burn-in (6 points, where
    the stepper relocates and a pair of fixes may be further apart than its moves), thinned by 4 with the true numbers of
    moves: every gap is SCORED, the file is the returned arrays, and the total is score_gaps' on the same jobs."""
    from ssrs_amd import Config, Simulator, movmodel
    base = dict(out_dir=str(tmp_path), sim_seed=11, region_width_km=(6., 5.), resolution=100., track_count=24,
                track_start_region=(1, 5, 0.2, 0.6), track_direction=0., track_dirn_restrict=1)
    for model in ('fluidflow', 'drw'):
        sim = Simulator(Config(run_name=f'bridge_{model}', movement_model=model, **base), terrain='synthetic')
        assert sim.gridsize == (50, 60)
        sim.simulate_tracks()
        case_id = sim.case_ids[0]
        with open(sim._get_tracks_fname(case_id, 0, sim.mode_data_dir) + '.pkl', 'rb') as f:
            tracks = [t[6:] for t in pickle.load(f)]
        thin = [movmodel.thin_track(t, 4) for t in tracks]
        fixes, moves = [t[0] for t in thin], [t[1] for t in thin]
        scores = sim.score_fixes(fixes, moves)
        ngaps = sum(len(m) for m in moves)
        assert ngaps > 100 and scores.counts() == dict(scored=ngaps, zero=0, too_long=0, out=0, undefined=0)
        saved = np.load(os.path.join(sim.mode_data_dir, f'{sim._get_id_string(case_id, 0)}_gap_scores.npy'))
        assert saved.dtype == np.int64 and saved.shape == (ngaps, 4)
        assert np.array_equal(saved[:, 0], np.repeat(np.arange(24), [len(m) for m in moves]))
        assert np.array_equal(saved[:, 1], np.concatenate([np.arange(len(m)) for m in moves]))
        assert not saved[:, 2].any() and np.array_equal(saved[:, 3], scores.surprisal.cpu().numpy())
        jobs = np.concatenate([movmodel.fix_gaps(f, m)[0] for f, m in zip(fixes, moves)])
        assert np.array_equal(jobs, scores.jobs.cpu().numpy())
        fields = sim._score_inputs('score_fixes', [], case_id, 0, False)[3]
        direct = movmodel.score_gaps(jobs, sim.gridsize, sim.track_direction, sim.track_stochastic_nu, fields[0], fields[1])
        assert direct.total_bits() == scores.total_bits() and 0. < scores.total_bits() < np.inf
        # metres in: the cells' centres round to the same cells, and are not joined by a line
        west, south = float(sim.bounds[0]), float(sim.bounds[1])
        metres = [np.stack([west + f[:, 1] * 100., south + f[:, 0] * 100.], 1) for f in fixes]
        again = sim.score_fixes(metres, moves, case_id, 0, xy=True)
        assert np.array_equal(again.jobs.cpu().numpy(), jobs) and again.total_bits() == scores.total_bits()
        with pytest.raises(ValueError, match='case_id'):
            sim.score_fixes(fixes, moves, 'no_such_case')
    sim = Simulator(Config(run_name='bridge_m2', movement_model='drw', **dict(base, track_dirn_restrict=2)), terrain='synthetic')
    with pytest.raises(ValueError, match='track_dirn_restrict = 2'):
        sim.score_fixes([np.zeros((2, 2), dtype=np.int64)])
