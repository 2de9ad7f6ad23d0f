"""Flight height (K14), the parts that need no device: the Config fields and where they stand, the metre-to-millimetre
conversion, the argument checks of ssrs_amd/flight.py, the library's refusals, the oracle on cases counted by hand, and
compute_rotor_presence_map before any run."""
import ctypes as C
import os
from dataclasses import fields

import numpy as np
import pytest
import torch

from ssrs_amd import Config, Simulator, flight

import altitude_ref as ref

NEW = ['flight_height', 'flight_height_start', 'flight_height_floor', 'flight_height_ceiling', 'flight_airspeed',
       'flight_sink_rate', 'rotor_zone']


def test_config_fields():
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    assert [getattr(cfg, n) for n in NEW] == [False, 100., 10., 1000., 15., -1., (30., 150.)]
    names = [f.name for f in fields(Config)]
    at = names.index('track_occupancy')
    assert names[at + 1:at + 8] == NEW
    build = list(dict(_SECTIONS)['MI355X build'])
    at = build.index('track_occupancy')
    assert build[at + 1:at + 8] == NEW
    assert build.index('rotor_zone') < build.index('turbine_encounter_radius') == len(build) - 1
    text = str(Config(flight_height=True, rotor_zone=(20., 90.))).split(':::: MI355X build')[1]
    assert 'flight_height = True' in text and 'rotor_zone = (20.0, 90.0)' in text
    assert 'flight_height = False' in str(cfg)


def test_metres_to_millimetres():
    assert flight.to_mm(100.) == 100_000 and flight.to_mm(0.0005) == 0 and flight.to_mm(0.0015) == 2       # int(round())
    assert flight.to_mm(-12.3456) == -12346 and flight.to_mm(30) == 30_000
    assert flight.to_mm(2147483.647) == 2 ** 31 - 1 and flight.to_mm(-2147483.648) == -2 ** 31
    for bad in (2147483.648, -2147483.649, float('inf'), float('nan')):
        with pytest.raises((ValueError, OverflowError)):
            flight.to_mm(bad)
    p = flight.height_params(100., 10., 1000., (30., 150.))
    assert (p.start, p.floor, p.ceil, p.band_lo, p.band_hi) == ref.DEFAULT
    with pytest.raises(ValueError, match='floor'):
        flight.height_params(100., 10.001, 10., (30., 150.))
    with pytest.raises(ValueError, match='band'):
        flight.height_params(100., 10., 1000., (150., 30.))
    with pytest.raises(ValueError, match='band'):
        flight.height_params(100., 10., 1000., 30.)
    flight.height_params(100., 10., 10., (30., 30.))                       # (equal ends are a band and a clamp)


def test_argument_checks_need_no_device():
    kw = dict(start=100., floor=10., ceil=1000., band=(30., 150.))
    info = torch.zeros((4, 4, 2), dtype=torch.int32)
    good = [np.zeros((3, 2), dtype=np.int16)]
    for bad in ([np.zeros((3, 2), dtype=np.int32)], [np.zeros((3, 3), dtype=np.int16)], [np.zeros(6, dtype=np.int16)]):
        with pytest.raises(ValueError, match=r'expected int16 \(n, 2\)'):
            flight.compute_track_altitudes(bad, info, (4, 4), **kw)
    pts = torch.zeros((3, 2), dtype=torch.int16)
    with pytest.raises(ValueError, match='needs offsets'):
        flight.compute_track_altitudes(pts, info, (4, 4), **kw)
    with pytest.raises(ValueError, match=r'expected int16 \(points, 2\)'):
        flight.compute_track_altitudes(pts.to(torch.int32), info, (4, 4), offsets=torch.tensor([0, 3]), **kw)
    with pytest.raises(ValueError, match='offsets must be int64'):
        flight.compute_track_altitudes(pts, info, (4, 4), offsets=torch.tensor([0, 3], dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match='offsets goes with a device tensor'):
        flight.compute_track_altitudes(good, info, (4, 4), offsets=np.array([0, 3]), **kw)
    for bad in (info.to(torch.int64), info[:, :, 0], torch.zeros((4, 5, 2), dtype=torch.int32), np.zeros((4, 4, 2), dtype=np.int32)):
        with pytest.raises(ValueError, match='cellinfo'):
            flight.compute_track_altitudes(good, bad, (4, 4), **kw)
    with pytest.raises(ValueError, match='band_hist'):
        flight.compute_track_altitudes(good, info, (4, 4), band_hist=torch.zeros((4, 4), dtype=torch.int32), **kw)   # not on the device
    with pytest.raises(ValueError, match='workspace'):
        flight.compute_track_altitudes(good, info, (4, 4), workspace=np.zeros(256, dtype=np.uint8), **kw)
    with pytest.raises(ValueError, match='floor'):
        flight.compute_track_altitudes(good, info, (4, 4), **dict(kw, floor=2000.))
    with pytest.raises(ValueError, match='band'):
        flight.compute_track_altitudes(good, info, (4, 4), **dict(kw, band=(3., 2.)))
    with pytest.raises(TypeError):
        flight.compute_track_altitudes(good, info, (4, 4))                                   # the heights have no defaults
    for bad in (dict(resolution=0.), dict(airspeed=0.), dict(airspeed=-1.), dict(sink=float('nan'))):
        with pytest.raises(ValueError, match='altitude_cellinfo'):
            flight.altitude_cellinfo(np.zeros((4, 4)), np.zeros((4, 4)), **dict(dict(resolution=10., airspeed=15., sink=1.), **bad))


def test_oracle_on_cases_counted_by_hand():
    assert [ref.diagonal_step(v) for v in (1, 3, 1001, -1, -3, -1001, 2 ** 26, -2 ** 26)] == \
        [1, 4, 1416, -1, -4, -1416, 94906368, -94906368]
    climb = np.array([[1001, -3], [5, 7]], dtype=np.int32)
    elev = np.array([[0, 2000], [ref.SENTINEL, 500]], dtype=np.int32)
    # (0,0)->(0,1): 1001 - 2000;  (0,1)->(1,0): diagonal -4, nodata ahead: no terrain;  (1,0)->(1,1): 5, nodata behind;
    # (1,1)->(3,3): outside: 0;  (3,3)->(0,0): 0
    track = np.array([[0, 0], [0, 1], [1, 0], [1, 1], [3, 3], [0, 0]], dtype=np.int16)
    assert ref.moves(track, climb, elev, (2, 2)) == [-999, -4, 5, 0, 0]
    out = ref.altitude([track, track[:0], track[4:5]], climb, elev, (2, 2), (1000, 0, 1003, 0, 1))
    assert out['alt'].tolist() == [1000, 1, 0, 5, 5, 5, 1000]
    assert out['traj_band'].tolist() == [[-1, -1], [0, 1], [1, 0], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]
    assert out['band_hist'].tolist() == [[0, 1], [1, 0]]
    assert out['in_band'].tolist() == [2, 0, 0]
    assert out['h_min'].tolist() == [0, 2 ** 31 - 1, 1000] and out['h_max'].tolist() == [1000, -2 ** 31, 1000]
    w = np.array([[np.nan, 1.75, 0.75 + 0.5 / 6250.]], dtype=np.float64)
    z = np.array([[1.0005, np.nan, 3e6]], dtype=np.float64)
    c, e = ref.cellinfo(w, z, 100., 16., 0.75)
    assert c.tolist() == [[-4688, 6250, 0]] and e.tolist() == [[1000, ref.SENTINEL, 2 ** 30]]
    for case in ref.CASES:
        assert all(t.dtype == np.int16 and t.ndim == 2 and t.shape[1] == 2 for t in case['tracks']), case['name']
    T = ref.TILE
    assert [len(t) for t in ref.case('lengths')['tracks']] == [0, 1, 2, T - 1, T, T + 1, 3 * T + 5]
    assert ref.expected('pinned_ceiling')['h_max'][0] == ref.DEFAULT[2] and ref.expected('pinned_floor')['h_min'][0] == ref.DEFAULT[1]
    assert (ref.expected('ceiling_then_floor')['h_min'][0], ref.expected('ceiling_then_floor')['h_max'][0]) == ref.DEFAULT[1:3]
    wide = ref.expected('beyond_int32')
    assert wide['h_max'][0] > 1_800_000_000 and wide['h_min'][0] == -2 ** 31 and wide['alt'][120] < -2_000_000_000
    assert 0 < ref.expected('band_1mm')['in_band'].sum() < ref.expected('band_all')['in_band'].sum()
    assert ref.expected('band_none')['in_band'].sum() == 0
    assert total_points() < 120_000


def total_points():
    return sum(len(t) for c in ref.CASES for t in c['tracks'])


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ssrs_hip.h')).read()
    assert f'#define SSRS_ALTITUDE_TILE {ref.TILE}' in header and _native.SSRS_ALTITUDE_TILE == flight.TILE == ref.TILE
    assert lib.ssrs_track_altitude_workspace_bytes(0) == 256
    assert lib.ssrs_track_altitude_workspace_bytes(10 ** 8) == -(-(10 ** 8 // ref.TILE + 2) * 24 // 256) * 256
    assert C.sizeof(_native.SsrsAltitudeParams) == 20
    raw = (C.c_char * 128)()
    buf = C.c_void_p((C.addressof(raw) + 15) // 16 * 16)
    odd = lambda k: C.c_void_p(buf.value + k)
    good = dict(traj=buf, off=buf, ntracks=1, info=buf, rows=2, cols=2, params=ref.DEFAULT, tb=buf, ws=buf, nbytes=256)
    bad = [dict(traj=None), dict(off=None), dict(info=None), dict(params=None), dict(ws=None), dict(rows=0), dict(rows=32768),
           dict(cols=0), dict(cols=32768), dict(ntracks=-1), dict(ntracks=2 ** 31), dict(traj=odd(2)), dict(tb=odd(2)),
           dict(info=odd(4)), dict(ws=odd(8)), dict(params=(0, 2, 1, 0, 0)), dict(params=(0, 1, 2, 1, 0)), dict(nbytes=255)]
    for kw in bad:
        a = dict(good, **kw)
        p = None if a['params'] is None else C.byref(_native.SsrsAltitudeParams(*a['params']))
        rc = lib.ssrs_track_altitude(a['traj'], a['off'], a['ntracks'], a['info'], a['rows'], a['cols'], p, None, None, a['tb'],
                                     None, None, None, a['ws'], a['nbytes'], None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_track_altitude' in lib.ssrs_last_error(), kw
    # (no tracks: nothing to do, whatever the other arguments point at)
    p = C.byref(_native.SsrsAltitudeParams(*ref.DEFAULT))
    assert lib.ssrs_track_altitude(buf, buf, 0, buf, 2, 2, p, None, None, None, None, None, None, buf, 256, None) == _native.SSRS_OK
    for kw in (dict(w=None), dict(z=None), dict(out=None), dict(rows=0), dict(cols=32768), dict(wt=2), dict(out=odd(4))):
        a = dict(dict(w=buf, z=buf, out=buf, rows=2, cols=2, wt=0), **kw)
        rc = lib.ssrs_altitude_cellinfo(a['w'], a['wt'], a['z'], 1, a['rows'], a['cols'], 0.75, 1., a['out'], None)
        assert rc == _native.SSRS_ERR_INVALID and b'ssrs_altitude_cellinfo' in lib.ssrs_last_error(), kw


def test_rotor_presence_map_before_any_run_raises():
    sim = object.__new__(Simulator)
    sim.rotor_presence_counts = {}
    with pytest.raises(ValueError, match='flight_height=True'):
        sim.compute_rotor_presence_map()


def test_simulator_refuses_bad_flight_settings(tmp_path):
    for kw, text in ((dict(flight_airspeed=0.), 'flight_airspeed'), (dict(rotor_zone=(150., 30.)), 'rotor_zone'),
                     (dict(flight_height_floor=2000.), 'floor'), (dict(flight_sink_rate=float('nan')), 'flight_sink_rate')):
        with pytest.raises(ValueError, match=text):
            Simulator(Config(out_dir=str(tmp_path), flight_height=True, **kw), terrain='synthetic')
