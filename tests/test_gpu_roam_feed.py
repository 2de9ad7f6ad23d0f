"""The roaming stepper with feeder waves (k_step_roam<REV, 256, true>, SSRS_TRACKS_ROAM_FEED): a second wave per SIMD
computes the Philox blocks and hands the uniforms over through a ring in LDS.  Whoever supplies a pair's uniforms -- the
feeder, or the stepping wave itself when a slot is not there in time -- lengths, end cells and the uint32 histogram are
the C oracle's, bit for bit.  The set-ups are those of tests/test_gpu_tracks.py; the oracle runs once per set-up.

SSRS_TRACKS_ROAM_FEED: unset / 1 feeders on, 0 the kernel without them, 2 the feeders skip every odd trip (so that fed
trips and the stepping wave's own Philox alternate deterministically)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FEED_MODES = [None, '0', '2']


@contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check(res, ref, feed, tag, wide=False, may_not_roam=False):
    st = res.stats
    assert np.array_equal(res.lengths.cpu().numpy(), ref['lengths']), (tag, feed)
    assert np.array_equal(res.ends.cpu().numpy(), ref['ends']), (tag, feed)
    assert np.array_equal(res.hist.cpu().numpy().view(np.uint32), ref['hist']), (tag, feed)
    fed, own = st['roam_fed_wave_pairs'], st['roam_own_wave_pairs']
    print(tag, 'feed', feed, 'launches', st['roam_launches'], 'wide', st['roam_wide_launches'],
          'pairs', st['roam_wave_pairs'], 'fed', fed, 'own', own)
    assert fed + own == st['roam_wave_pairs'], (tag, feed, st)
    if may_not_roam and st['roam_launches'] == 0:
        assert st['roam_wave_pairs'] == 0, (tag, feed, st)
        return
    assert st['roam_launches'] > 0, (tag, feed, st)
    if wide:
        # (a scattered batch makes one narrow launch before its first deal: with the width forced it takes no feeders either)
        assert st['roam_wide_launches'] > 0 and fed == 0, (tag, feed, st)
    elif feed == '0':
        assert fed == 0, (tag, feed, st)
    elif feed == '2':
        assert fed > 0 and own > 0, (tag, feed, st)
    else:
        assert fed > 0, (tag, feed, st)


# ---- case 1: launches of two trips -- priming, DONE after two trips, lanes that never step
@pytest.fixture(scope='module', params=[0., 315.])
def ring_case(request):
    from oracle import c_oracle
    dirn = request.param
    rows, cols = 9, 150
    rng = np.random.default_rng(int(dirn) + 5)
    upd = np.abs(rng.normal(0.8, 0.6, (rows, cols)))
    pot = (1000. * (1 - np.arange(rows)[:, None] / (rows - 1.)) + rng.normal(0, 30., (rows, cols))).astype(np.float32)
    n = 9000
    ring_r = rng.choice([0, 1, rows - 2, rows - 1], n)
    ring_c = rng.choice([0, 1, cols - 2, cols - 1], n)
    on_row = rng.random(n) < 0.7
    starts = np.stack([np.where(on_row, ring_r, rng.integers(0, rows, n)),
                       np.where(on_row, rng.integers(0, cols, n), ring_c)], 1)
    ref = c_oracle.simulate_tracks(dirn, starts, (rows, cols), 1, 1., upd, pot, seed=11, want_traj=False)
    return dirn, (rows, cols), upd, pot, starts, ref


@pytest.mark.parametrize('feed', FEED_MODES)
def test_two_trip_launches_from_the_boundary_rows(gpu, ring_case, feed):
    from ssrs_amd import movmodel
    dirn, shape, upd, pot, starts, ref = ring_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed):
        res = movmodel.simulate_tracks(dirn, starts, shape, 1, 1., upd, pot, seed=11, steps_per_launch=16,
                                       use_table=True, thr=True, scattered=True)
    _check(res, ref, feed, f'ring{int(dirn)}')


# ---- case 2: waves that run a launch out because a lane waits for its release; blk0 of late lanes
@pytest.fixture(scope='module')
def release_case():
    from oracle import c_oracle
    rng = np.random.default_rng(355781144)
    rows, cols = int(rng.integers(5, 400)), int(rng.integers(5, 500))
    assert rng.random() >= 0.15
    n = int(rng.choice([1, 7, 64, 65, 300, 2000, 9000, 20000]))
    dirn = float(rng.choice([0., 45., 90., 135., 180., 225., 270., 315., rng.uniform(0, 360)]))
    kind = rng.choice(['rough', 'smooth', 'flat', 'speckle', 'nan', 'wells', 'scales'])
    assert (rows, cols, n, dirn, str(kind)) == (10, 213, 9000, 315., 'scales')
    upd = np.abs(rng.normal(0.8, 0.6, (rows, cols)))
    ramp = 1000. * (1 - np.arange(rows)[:, None] / max(rows - 1., 1.))
    pot = (ramp + rng.normal(0, rng.choice([0.01, 1.0, 30.0]), (rows, cols))).astype(np.float32)
    upd = upd * 10. ** rng.uniform(-9, 39, upd.shape)
    upd[rng.random((rows, cols)) < 0.01] = np.inf
    band = 10. ** rng.integers(-44, 8, rows // 8 + 1).astype(np.float64)
    pot = (pot.astype(np.float64) * np.repeat(band, 8)[:rows, None]).astype(np.float32)
    starts = np.stack([rng.integers(0, rows, n), rng.integers(0, cols, n)], 1)
    s = int(rng.integers(0, 2**31))
    ref = c_oracle.simulate_tracks(dirn, starts, (rows, cols), 1, 1., upd, pot, seed=s, want_traj=False)
    return dirn, (rows, cols), upd, pot, starts, s, ref


@pytest.mark.parametrize('feed', FEED_MODES)
def test_launches_while_tracks_wait_for_their_release(gpu, release_case, feed):
    from ssrs_amd import movmodel
    dirn, shape, upd, pot, starts, s, ref = release_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed):
        res = movmodel.simulate_tracks(dirn, starts, shape, 1, 1., upd, pot, seed=s, steps_per_launch=16,
                                       use_table=True, thr=True, scattered=True)
    _check(res, ref, feed, 'release')


# ---- case 3: full lists, mixed windows, the stop flag ending launches early; 3b: wide launches take no feeders
@pytest.fixture(scope='module')
def pits_case():
    from oracle import c_oracle
    from test_gpu_tracks import _random_field_case
    rows, cols = 300, 2200
    upd, pot = _random_field_case(rows, cols, 9)
    pot = pot.copy()
    rr, cc = np.arange(rows)[:, None], np.arange(cols)[None, :]
    for c0 in (300, 1100, 1900):                               # three pits side by side
        pot -= (900. * np.exp(-((rr - 120) ** 2 / (2. * 12. ** 2) + (cc - c0) ** 2 / (2. * 260. ** 2)))).astype(np.float32)
    rng = np.random.default_rng(3)
    n = 8192
    starts = np.stack([rng.integers(2, 10, n), rng.integers(5, cols - 5, n)], 1)
    cap = 5000
    ref = c_oracle.simulate_tracks(0., starts, (rows, cols), 1, 1., upd, pot, seed=6, max_moves=cap, want_traj=False)
    assert (ref['lengths'] - 1 >= cap).mean() > 0.5
    return (rows, cols), upd, pot, starts, cap, ref


@pytest.mark.parametrize('scattered', [False, True])
@pytest.mark.parametrize('feed', FEED_MODES)
def test_full_lists_and_the_stop_flag(gpu, pits_case, feed, scattered):
    from ssrs_amd import movmodel
    shape, upd, pot, starts, cap, ref = pits_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed, SSRS_TRACKS_FIXED_STEPS='1'):
        res = movmodel.simulate_tracks(0., starts, shape, 1, 1., upd, pot, seed=6, use_table=True, thr=True,
                                       max_moves=cap, steps_per_launch=64, scattered=scattered)
    _check(res, ref, feed, f'pits{int(scattered)}')


@pytest.mark.parametrize('scattered', [False, True])
@pytest.mark.parametrize('feed', FEED_MODES)
def test_wide_launches_take_no_feeders(gpu, pits_case, feed, scattered):
    from ssrs_amd import movmodel
    shape, upd, pot, starts, cap, ref = pits_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed, SSRS_TRACKS_FIXED_STEPS='1', SSRS_TRACKS_ROAM_WIDTH='2'):
        res = movmodel.simulate_tracks(0., starts, shape, 1, 1., upd, pot, seed=6, use_table=True, thr=True,
                                       max_moves=cap, steps_per_launch=64, scattered=scattered)
    _check(res, ref, feed, f'pits{int(scattered)}w2', wide=True)


# ---- case 4: long launches, where the ring wraps many times
@pytest.fixture(scope='module')
def wells_case():
    from oracle import c_oracle
    from test_gpu_tracks import _random_field_case
    rows, cols = 700, 1100
    upd, pot = _random_field_case(rows, cols, 5)
    pot = pot.copy()
    rr, cc = np.arange(rows)[:, None], np.arange(cols)[None, :]
    for r0, c0, w in ((200, 300, 14.), (330, 820, 18.), (340, 330, 10.), (520, 600, 16.)):
        pot -= (700. * np.exp(-((rr - r0) ** 2 + (cc - c0) ** 2) / (2. * w ** 2))).astype(np.float32)
    rng = np.random.default_rng(77)
    n = 20000
    starts = np.stack([rng.integers(2, 12, n), rng.integers(5, cols - 5, n)], 1)
    cap = 9000
    ref = c_oracle.simulate_tracks(0., starts, (rows, cols), 1, 1., upd, pot, seed=4, max_moves=cap, want_traj=False)
    assert (ref['lengths'] - 1 >= cap).mean() > 0.05
    return (rows, cols), upd, pot, starts, cap, ref


@pytest.mark.parametrize('growing', [False, True])
@pytest.mark.parametrize('feed', FEED_MODES)
def test_long_launches_wrap_the_ring(gpu, wells_case, feed, growing):
    from ssrs_amd import movmodel
    shape, upd, pot, starts, cap, ref = wells_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed, SSRS_TRACKS_FIXED_STEPS=None if growing else '1'):
        res = movmodel.simulate_tracks(0., starts, shape, 1, 1., upd, pot, seed=4, use_table=True, thr=True,
                                       max_moves=cap, steps_per_launch=128)
    # (launches that grow finish this batch before the host's policy turns to the roaming kernel: no pair is counted then,
    # and the run checks the integers alone, as the growing run of test_block_windows_for_batches_that_roam_basins does)
    _check(res, ref, feed, f'wells{int(growing)}', may_not_roam=growing)


def test_hand_over_word_is_the_top_halves_of_words_x_and_z(gpu):
    """What a feeder writes per pair, (x & 0xFFFF0000) | (z >> 16), from the written-out rounds against the four words of
    rocRAND's engine on the device, and those against the Random123-pinned oracle."""
    from ssrs_amd import movmodel
    from oracle.philox import philox4x32_10
    rng = np.random.default_rng(2)
    n = 4096
    track = rng.integers(0, 2**63, n, dtype=np.uint64)
    blk = rng.integers(0, 3_750_001, n, dtype=np.uint64)
    track[:8] = [0, 1, 2**32 - 1, 2**32, 2**32 + 1, 2**40 + 12345, 2**63 + 5, 2**64 - 1]
    track[8:1024] += np.uint64(2**32)                          # (ids above 2^32 in bulk, too)
    blk[:8] = [0, 1, 2, 3, 3_750_000, 3_749_999, 65535, 65536]
    for seed in (0, 30, 2**64 - 1, 0x123456789ABCDEF):
        packed, words = movmodel.roam_pair_words(seed, track, blk)
        assert np.array_equal(packed, (words[:, 0] & np.uint32(0xFFFF0000)) | (words[:, 2] >> np.uint32(16)))
        s = int(seed) & 0xFFFFFFFFFFFFFFFF
        want = philox4x32_10(blk & np.uint64(0xFFFFFFFF), blk >> np.uint64(32), track & np.uint64(0xFFFFFFFF),
                             track >> np.uint64(32), s & 0xFFFFFFFF, s >> 32)
        for j in range(4):
            assert np.array_equal(words[:, j].astype(np.uint64), np.asarray(want[j], dtype=np.uint64)), (seed, j)
