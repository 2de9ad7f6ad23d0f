"""Periodic shuffles of a settled roaming batch deal into the windows of the last scan: no k_wander_windows, no live count
read back (TrackPolicy::scan_windows, TrackRun::wander_sort).  Whatever the interval of the shuffles, with feeder waves and
without, in narrow and in wide blocks, lengths, end cells and the uint32 histogram are the C oracle's, bit for bit, and
the shuffles made fewer window scans than there were sorts.  SSRS_TRACKS_NO_SHUFFLE_REUSE brings every scan back.

The set-up and its oracle run are the pits_case fixture of tests/test_gpu_roam_feed.py (300 x 2 200, three pits side by
side, 8 192 tracks, 5 000 moves at most, launches of 64 steps)."""
import numpy as np
import pytest

from test_gpu_roam_feed import _env, pits_case  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def _run(pits_case, scattered=True, **env):
    from ssrs_amd import movmodel
    shape, upd, pot, starts, cap, ref = pits_case
    with _env(SSRS_TRACKS_FIXED_STEPS='1', **env):
        res = movmodel.simulate_tracks(0., starts, shape, 1, 1., upd, pot, seed=6, use_table=True, thr=True,
                                       max_moves=cap, steps_per_launch=64, scattered=scattered)
    st = res.stats
    print(env, 'scattered', scattered, 'launches', st['roam_launches'], 'wide', st['roam_wide_launches'], 'sorts', st['wander_sorts'],
          'shuffles', st['roam_shuffles'], 'window scans', st['window_scans'])
    assert np.array_equal(res.lengths.cpu().numpy(), ref['lengths']), env
    assert np.array_equal(res.ends.cpu().numpy(), ref['ends']), env
    assert np.array_equal(res.hist.cpu().numpy().view(np.uint32), ref['hist']), env
    assert st['roam_launches'] > 0 and st['roam_shuffles'] > 0, (env, st)
    # every sort that is no shuffle looks for its windows
    assert st['window_scans'] >= st['wander_sorts'] - st['roam_shuffles'] > 0, (env, st)
    return st


@pytest.mark.parametrize('feed', [None, '0'])
@pytest.mark.parametrize('shuffle', ['1', '4'])
def test_shuffles_scan_no_windows(gpu, pits_case, shuffle, feed):
    st = _run(pits_case, SSRS_TRACKS_ROAM_SHUFFLE=shuffle, SSRS_TRACKS_ROAM_FEED=feed)
    assert st['window_scans'] < st['wander_sorts'], st
    assert st['roam_wide_launches'] == 0 and (st['roam_fed_wave_pairs'] > 0) == (feed is None), st


@pytest.mark.parametrize('shuffle', ['1', '4'])
def test_shuffles_of_a_wide_deal_scan_no_windows(gpu, pits_case, shuffle):
    st = _run(pits_case, SSRS_TRACKS_ROAM_SHUFFLE=shuffle, SSRS_TRACKS_ROAM_WIDTH='2')
    assert st['window_scans'] < st['wander_sorts'], st
    assert st['roam_wide_launches'] > 0, st


def test_shuffles_of_a_batch_that_came_as_a_front(gpu, pits_case):
    st = _run(pits_case, scattered=False, SSRS_TRACKS_ROAM_SHUFFLE='1')
    assert st['window_scans'] < st['wander_sorts'], st


def test_every_sort_scans_with_the_reuse_switched_off(gpu, pits_case):
    st = _run(pits_case, SSRS_TRACKS_ROAM_SHUFFLE='1', SSRS_TRACKS_NO_SHUFFLE_REUSE='1')
    assert st['window_scans'] == st['wander_sorts'], st
