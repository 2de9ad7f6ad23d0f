"""The roaming stepper's trip, with its housekeeping dealt over the shadows of its four gathers (k_step_roam): the stop
flag asked for behind the first gather, the look ahead and the stop test behind the first two, the ring behind the third.
Whatever the layout, lengths, end cells and the uint32 histogram are the C oracle's, bit for bit -- with feeder waves,
without them, with every odd trip on the stepping wave's own Philox, and with the stop flag on and off.

The set-ups and their oracle runs are the fixtures of tests/test_gpu_roam_feed.py.  stats['roam_stopped_waves'] counts the
waves that left a launch because its stop flag was up: the flag must still end launches, and never without it."""
import numpy as np
import pytest

from test_gpu_roam_feed import _env, FEED_MODES, ring_case, release_case, pits_case, wells_case  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

NO_STOP = [None, '1']


def _check(res, ref, tag, no_stop, must_stop=False):
    st = res.stats
    assert np.array_equal(res.lengths.cpu().numpy(), ref['lengths']), tag
    assert np.array_equal(res.ends.cpu().numpy(), ref['ends']), tag
    assert np.array_equal(res.hist.cpu().numpy().view(np.uint32), ref['hist']), tag
    print(tag, 'launches', st['roam_launches'], 'wide', st['roam_wide_launches'], 'pairs', st['roam_wave_pairs'],
          'fed', st['roam_fed_wave_pairs'], 'own', st['roam_own_wave_pairs'], 'stopped waves', st['roam_stopped_waves'])
    assert st['roam_launches'] > 0, (tag, st)
    assert st['roam_fed_wave_pairs'] + st['roam_own_wave_pairs'] == st['roam_wave_pairs'], (tag, st)
    if no_stop:
        assert st['roam_stopped_waves'] == 0, (tag, st)
    elif must_stop:
        assert st['roam_stopped_waves'] > 0, (tag, st)


@pytest.mark.parametrize('no_stop', NO_STOP)
@pytest.mark.parametrize('feed', FEED_MODES)
def test_launches_of_two_trips(gpu, ring_case, feed, no_stop):
    from ssrs_amd import movmodel
    dirn, shape, upd, pot, starts, ref = ring_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed, SSRS_TRACKS_NO_ROAM_STOP=no_stop):
        res = movmodel.simulate_tracks(dirn, starts, shape, 1, 1., upd, pot, seed=11, steps_per_launch=16,
                                       use_table=True, thr=True, scattered=True)
    _check(res, ref, f'ring{int(dirn)} feed {feed} no_stop {no_stop}', no_stop)


@pytest.mark.parametrize('no_stop', NO_STOP)
@pytest.mark.parametrize('feed', FEED_MODES)
def test_lanes_that_wait_for_their_release(gpu, release_case, feed, no_stop):
    from ssrs_amd import movmodel
    dirn, shape, upd, pot, starts, s, ref = release_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed, SSRS_TRACKS_NO_ROAM_STOP=no_stop):
        res = movmodel.simulate_tracks(dirn, starts, shape, 1, 1., upd, pot, seed=s, steps_per_launch=16,
                                       use_table=True, thr=True, scattered=True)
    _check(res, ref, f'release feed {feed} no_stop {no_stop}', no_stop)


@pytest.mark.parametrize('no_stop', NO_STOP)
@pytest.mark.parametrize('scattered', [False, True])
@pytest.mark.parametrize('feed', FEED_MODES)
def test_full_lists_and_the_stop_flag(gpu, pits_case, feed, scattered, no_stop):
    from ssrs_amd import movmodel
    shape, upd, pot, starts, cap, ref = pits_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed, SSRS_TRACKS_FIXED_STEPS='1', SSRS_TRACKS_NO_ROAM_STOP=no_stop):
        res = movmodel.simulate_tracks(0., starts, shape, 1, 1., upd, pot, seed=6, use_table=True, thr=True,
                                       max_moves=cap, steps_per_launch=64, scattered=scattered)
    _check(res, ref, f'pits{int(scattered)} feed {feed} no_stop {no_stop}', no_stop, must_stop=True)


@pytest.mark.parametrize('no_stop', NO_STOP)
@pytest.mark.parametrize('scattered', [False, True])
@pytest.mark.parametrize('feed', FEED_MODES)
def test_full_lists_in_wide_blocks(gpu, pits_case, feed, scattered, no_stop):
    from ssrs_amd import movmodel
    shape, upd, pot, starts, cap, ref = pits_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed, SSRS_TRACKS_FIXED_STEPS='1', SSRS_TRACKS_ROAM_WIDTH='2',
              SSRS_TRACKS_NO_ROAM_STOP=no_stop):
        res = movmodel.simulate_tracks(0., starts, shape, 1, 1., upd, pot, seed=6, use_table=True, thr=True,
                                       max_moves=cap, steps_per_launch=64, scattered=scattered)
    _check(res, ref, f'pits{int(scattered)}w2 feed {feed} no_stop {no_stop}', no_stop, must_stop=True)
    assert res.stats['roam_wide_launches'] > 0 and res.stats['roam_fed_wave_pairs'] == 0, res.stats


@pytest.mark.parametrize('no_stop', NO_STOP)
@pytest.mark.parametrize('feed', FEED_MODES)
def test_long_launches_wrap_the_ring(gpu, wells_case, feed, no_stop):
    from ssrs_amd import movmodel
    shape, upd, pot, starts, cap, ref = wells_case
    with _env(SSRS_TRACKS_ROAM_FEED=feed, SSRS_TRACKS_FIXED_STEPS='1', SSRS_TRACKS_NO_ROAM_STOP=no_stop):
        res = movmodel.simulate_tracks(0., starts, shape, 1, 1., upd, pot, seed=4, use_table=True, thr=True,
                                       max_moves=cap, steps_per_launch=128)
    _check(res, ref, f'wells feed {feed} no_stop {no_stop}', no_stop)
