"""Flight time (K16), the parts that need no device: the oracle of tests/flight_time_ref.py on moves worked by hand, the
wind's components on the host, the scalars' checks, the argument checks of flight.compute_track_times, the Config fields
and where they stand, and the random inputs of the device's windinfo test."""
import math
from dataclasses import fields

import numpy as np
import pytest
import torch

from ssrs_amd import Config, Simulator, flight

import flight_time_ref as ref

P = ref.DEFAULT                                           # 15 m/s, at least 1 m/s, 10 m cells


def test_oracle_on_moves_worked_by_hand():
    # still air: 10 m at 15 m/s = 666 666.67 us, rounded; the same for a rest, whatever the wind
    assert ref.move_dt(P, 1, 0, 0, 0) == ref.move_dt(P, 0, -1, 0, 0) == 666_667
    assert ref.move_dt(P, 0, 0, 9_999, -20_000) == 666_667
    # the air moves +row at 10 m/s: downwind 25 m/s is exactly 400 000 us, upwind 5 m/s is 2 s
    assert ref.move_dt(P, 1, 0, 10_000, 0) == 400_000
    assert ref.move_dt(P, -1, 0, 10_000, 0) == 2_000_000 == ref.move_dt(P, 0, 1, 0, -10_000)
    # a pure cross wind of 10 m/s: sqrt(225e6 - 100e6) = 11 180.3 -> 11 180 mm/s, from either side and along either axis
    assert math.isqrt(125_000_000) == 11_180
    want = (10 ** 10 + 5_590) // 11_180
    assert want == 894_454
    assert ref.move_dt(P, 1, 0, 0, 10_000) == ref.move_dt(P, 1, 0, 0, -10_000) == ref.move_dt(P, 0, -1, -10_000, 0) == want
    # a diagonal is 14 142 mm: still air, the 10 m/s wind along it (7 071 on each axis: a = 10 000, no cross wind), and
    # across it (a = 0, b = 14 142, cross2 = 99 998 082, sqrt(125 001 918) -> 11 180)
    assert (10_000 * ref.SQRT2_16 + 32768) >> 16 == 14_142
    assert ref.move_dt(P, 1, 1, 0, 0) == 942_800
    assert ref.move_dt(P, 1, 1, 7_071, 7_071) == (14_142 * 10 ** 6 + 12_500) // 25_000 == 565_680
    assert ref.move_dt(P, -1, -1, 7_071, 7_071) == (14_142 * 10 ** 6 + 2_500) // 5_000
    assert ref.move_dt(P, 1, -1, 7_071, 7_071) == (14_142 * 10 ** 6 + 5_590) // 11_180 == 1_264_937
    # the bird cannot hold the heading (cross wind above va), or makes less than gmin: gmin = 1 m/s, 10 s a cell
    assert ref.move_dt(P, 1, 0, 0, 20_000) == ref.move_dt(P, 1, 0, -14_500, 0) == 10_000_000
    assert ref.move_dt(P, 1, 0, -14_000, 0) == 10_000_000 and ref.move_dt(P, 1, 0, -13_999, 0) == (10 ** 10 + 500) // 1_001
    # the cap: 1 km cells at 1 mm/s
    assert ref.move_dt((15_000, 1, 10 ** 6), 1, 0, 0, 20_000) == ref.CAP == 2 ** 31 - 1


def test_oracle_sums_and_the_cases_cover_what_they_claim():
    tracks = [np.array([(1, 1), (1, 2), (2, 3), (2, 3), (-1, -1), (2, 3)], dtype=np.int16), np.zeros((0, 2), dtype=np.int16),
              np.array([(0, 0)], dtype=np.int16), np.array([(3, 3), (0, 3)], dtype=np.int16)]
    wr = np.zeros((4, 4), dtype=np.int32)
    wc = np.zeros((4, 4), dtype=np.int32)
    wr[3, 3] = -10_000                                     # the jump (3, 3) -> (0, 3) is ONE move, downwind
    masked = np.concatenate(tracks).copy()
    masked[[1, 3]] = -1
    out = ref.flight_times(tracks, wr, wc, (4, 4), P, masked)
    assert out['dt'].tolist() == [666_667, 942_800, 666_667, 0, 0, 0, 0, 400_000, 0]
    assert out['times'].tolist() == [[2_276_134, 666_667 + 666_667], [0, 0], [0, 0], [400_000, 400_000]]
    assert out['time_hist'][1, 1] == 666_667 and out['time_hist'][1, 2] == 942_800 and out['time_hist'][2, 3] == 666_667
    assert out['time_hist'][3, 3] == 400_000 and out['time_hist'].sum() == 2_676_134
    assert out['band_time_hist'][1, 2] == 0 and out['band_time_hist'].sum() == 1_733_334
    # the shared raster: NaN cells (still air), stalls, ground speeds below gmin, and the cap in its case
    c = ref.case('lengths')
    assert ((c['wr'] == 0) & (c['wc'] == 0)).sum() > 100
    assert (np.abs(c['wr']) > P[0]).any() and (np.abs(c['wc']) > P[0]).any()
    assert (c['wr'][5, 5], c['wc'][5, 5]) == (-10 ** 6, 0) and (c['wr'][6, 6], c['wc'][6, 6]) == (0, 14_500)
    assert (ref.expected('traps')['dt'] == 10_000_000).any()
    cap = ref.expected('cap')['dt']
    assert cap[0] == ref.CAP and cap[2] < ref.CAP and int(ref.expected('cap')['times'][0, 0]) > 2 ** 32
    assert {0, 1} <= set(ref.expected('fast_fine')['dt'].tolist())
    for name in ref.CASE_IDS:
        npoints = sum(len(t) for t in ref.case(name)['tracks'])
        assert npoints <= 30_000 and ref.expected(name)['dt'].shape == (npoints,)
    assert sum(len(t) > 0 for t in ref.case('short_300')['tracks'][:260]) > 256          # more tracks in a tile than slots


def test_wind_components_on_the_host():
    # a westerly (from 270) of 10 m/s moves the air east: +row on DEM-only terrain, +col with geographic layers
    assert flight.wind_pair(10., 270., 'row_east') == (10_000, 0)
    assert flight.wind_pair(10., 270., 'row_north') == (0, 10_000)
    # a northerly moves it south
    assert flight.wind_pair(10., 0., 'row_north') == (-10_000, 0) and flight.wind_pair(10., 0., 'row_east') == (0, -10_000)
    assert flight.wind_pair(10., 45., 'row_east') == (-7_071, -7_071)
    assert flight.wind_pair(float('nan'), 45.) == (0, 0) == flight.wind_pair(10., float('nan'))
    assert flight.wind_pair(5000., 45.) == (-2 ** 20, -2 ** 20) and flight.wind_pair(-5000., 45.) == (2 ** 20, 2 ** 20)
    rng = np.random.default_rng(0)
    for ws, wd in zip(rng.uniform(0., 40., 50), rng.uniform(-400., 800., 50)):
        for axes in ('row_east', 'row_north'):
            wr, wc = ref.windinfo(np.array([ws]), np.array([wd]), axes)
            assert flight.wind_pair(ws, wd, axes) == (int(wr[0]), int(wc[0]))
    with pytest.raises(ValueError, match='ray_axes'):
        flight.wind_pair(10., 0., 'row_south')
    with pytest.raises(ValueError, match='ray_axes'):
        flight.wind_cellinfo(np.zeros((2, 2)), np.zeros((2, 2)), 'row_south')


def test_time_params():
    p = flight.time_params(10., 15., 1.)
    assert (p.va, p.gmin, p.res_mm) == P
    p = flight.time_params(0.001, 1048.576, 0.001)
    assert (p.va, p.gmin, p.res_mm) == (2 ** 20, 1, 1)
    p = flight.time_params(1000., 15., 15.)
    assert (p.va, p.gmin, p.res_mm) == (15_000, 15_000, 10 ** 6)
    for kw, text in ((dict(airspeed=0.), 'airspeed'), (dict(airspeed=1048.58), 'airspeed'), (dict(airspeed=float('nan')), 'airspeed'),
                     (dict(min_groundspeed=0.), 'min_groundspeed'), (dict(min_groundspeed=15.001), 'min_groundspeed'),
                     (dict(min_groundspeed=float('inf')), 'min_groundspeed'), (dict(resolution=0.), 'resolution'),
                     (dict(resolution=1000.001), 'resolution'), (dict(resolution='x'), 'resolution')):
        with pytest.raises(ValueError, match=text):
            flight.time_params(**dict(dict(resolution=10., airspeed=15., min_groundspeed=1.), **kw))


def test_argument_checks_need_no_device():
    kw = dict(resolution=10., airspeed=15., wind=(10., 270.))
    good = [np.zeros((3, 2), dtype=np.int16)]
    for bad in ([np.zeros((3, 2), dtype=np.int32)], [np.zeros((3, 3), dtype=np.int16)], [np.zeros(6, dtype=np.int16)]):
        with pytest.raises(ValueError, match=r'expected int16 \(n, 2\)'):
            flight.compute_track_times(bad, (4, 4), **kw)
    with pytest.raises(ValueError, match='offsets'):
        flight.compute_track_times(good, (4, 4), offsets=np.array([0, 3]), **kw)
    with pytest.raises(ValueError, match='offsets'):
        flight.compute_track_times(torch.zeros((3, 2), dtype=torch.int16), (4, 4), **kw)
    with pytest.raises(ValueError, match='tracks is'):
        flight.compute_track_times(torch.zeros((3, 2), dtype=torch.int32), (4, 4), offsets=np.array([0, 3]), **kw)
    with pytest.raises(ValueError, match='masked'):
        flight.compute_track_times(good, (4, 4), masked=np.zeros((2, 2), dtype=np.int16), **kw)
    with pytest.raises(ValueError, match='masked'):
        flight.compute_track_times(good, (4, 4), masked=np.zeros((3, 2), dtype=np.int32), **kw)
    for wind in (10., (1., 2., 3.), torch.zeros((4, 4, 2), dtype=torch.int64), torch.zeros((4, 5, 2), dtype=torch.int32),
                 np.zeros((4, 4, 2), dtype=np.int32), ('a', 'b')):
        with pytest.raises(ValueError, match='wind'):
            flight.compute_track_times(good, (4, 4), **dict(kw, wind=wind))
    with pytest.raises(ValueError, match='ray_axes'):
        flight.compute_track_times(good, (4, 4), ray_axes='row_up', **kw)
    with pytest.raises(ValueError, match='min_groundspeed'):
        flight.compute_track_times(good, (4, 4), min_groundspeed=16., **kw)
    for name in ('time_hist', 'band_time_hist'):
        with pytest.raises(ValueError, match=name):
            flight.compute_track_times(good, (4, 4), masked=good[0], **{name: torch.zeros((4, 4), dtype=torch.int64)}, **kw)


def test_config_fields():
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    assert cfg.flight_time is False and cfg.flight_min_groundspeed == 1.
    names = [f.name for f in fields(Config)]
    at = names.index('rotor_clearance')
    assert names[at + 1:at + 3] == ['flight_time', 'flight_min_groundspeed']
    build = list(dict(_SECTIONS)['MI355X build'])
    at = build.index('rotor_clearance')
    assert build[at + 1:at + 3] == ['flight_time', 'flight_min_groundspeed'] and build[-1] == 'turbine_encounter_radius'
    text = str(Config(flight_time=True, flight_min_groundspeed=2.5)).split(':::: MI355X build')[1]
    assert 'flight_time = True' in text and 'flight_min_groundspeed = 2.5' in text
    assert 'flight_time = False' in str(cfg) and 'flight_min_groundspeed = 1.0' in str(cfg)


def test_simulator_refuses_bad_flight_time_settings(tmp_path):
    for kw, text in ((dict(flight_min_groundspeed=0.), 'min_groundspeed'), (dict(flight_min_groundspeed=15.5), 'min_groundspeed'),
                     (dict(flight_airspeed=2000.), 'airspeed'), (dict(resolution=2000.), 'resolution')):
        with pytest.raises(ValueError, match=text):
            Simulator(Config(out_dir=str(tmp_path), flight_time=True, **kw), terrain='synthetic')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=lambda d: d.__name__)
def test_windinfo_inputs_keep_the_exemptions_rare(dtype):
    """The inputs tests/test_gpu_flight_time.py gives ssrs_flight_windinfo: fewer than 1 % of the components lie within
    1e-6 of a half-integer before rounding, where the device's sin and cos may round the other way."""
    ws, wd = ref.windinfo_inputs(dtype)
    assert ws.dtype == dtype and ws.shape == ref.SHAPE and np.isnan(ws).any() and np.isnan(wd).any()
    exempt = ref.windinfo_exempt(ws, wd, 'row_east') | ref.windinfo_exempt(ws, wd, 'row_north')
    assert exempt.mean() < 0.01
    wr, wc = ref.windinfo(ws, wd)
    assert (np.abs(wr) == 2 ** 20).any() and ((wr == 0) & (wc == 0)).any()
