"""Rotor transits (K18), the parts that need no device: the numpy restatement against hand-computed integers, the cull
lists against every transit the brute force accepts, rotor_disks and rotor_axes, the Config fields and the constructor's
refusals, the third header against the binding, and the library's argument errors."""
import ctypes as C
import os
import re
from dataclasses import fields

import numpy as np
import pytest

from ssrs_amd import Config, Simulator
from ssrs_amd import turbines as tb

import test_native_abi as abi
import transit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ssrs_hip_transits.h')


# ------------------------------------------------------------------------------------------------ the restatement
def group_transits(group):
    """int64 (nturb, 2) of the planted tracks of one group alone, on the planted ground and turbines."""
    c = ref.case('planted')
    tracks = [(p, a) for p, a, g in ref.planted_tracks() if g == group]
    assert tracks
    mini = dict(c, tracks=[p for p, _ in tracks], alts=[a for _, a in tracks], lead=0, tail=0, shift=0)
    return ref.compute(mini)


def only(res, **want):
    """The transits of the named turbines are as given and no other of the planted eleven has any."""
    t = res['transits']
    for name in ('A', 'B', 'C2', 'NAN_REACH', 'NEG_REACH', 'NAN_XY', 'NAN_AXIS', 'DIAG', 'OUTSIDE', 'BIG_HI', 'BIG_LO'):
        assert t[getattr(ref, name)].tolist() == list(want.get(name, (0, 0))), (name, t[getattr(ref, name)].tolist())


def test_a_turbine_between_two_rows():
    """A at (30, 20.5), reach 3, axis (0, 1): (20, c) -> (21, c) starts downwind (s_0 = -0.5 < 0), so it goes against the
    wind, and hits for c = 27 .. 33, the edge included; C2 at (31, 20.5), reach 5, holds all nine columns."""
    res = group_transits('between_rows')
    only(res, A=(0, 7), C2=(0, 9))
    hit = res['bitmap'][:, 0] & 1
    assert hit.tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0]                       # c = 26 .. 34
    only(group_transits('between_rows_back'), A=(7, 0), C2=(9, 0))


def test_a_turbine_on_a_row():
    """B at (30, 20): 19 -> 20 -> 21 is ONE transit (the point on the plane is upwind), 20 -> 19 is one with the wind,
    20 -> 21 alone and a move along the plane are none.  The same moves through A and C2, whose plane is at 20.5."""
    res = group_transits('on_a_row')
    only(res, B=(1, 1), A=(0, 2), C2=(0, 2))
    assert (res['bitmap'][:, 0] >> ref.B & 1).tolist() == [1, 1, 0, 0]


def test_heights_at_the_edge_and_a_millimetre_beyond():
    only(group_transits('height_edge'), A=(0, 2), C2=(0, 4))
    res = group_transits('height_edge')
    assert (res['bitmap'][:, 0] & 1).tolist() == [1, 0, 1, 0]


def test_interpolated_height_sums_beyond_int32_and_what_is_no_move():
    res = group_transits('diagonal')                                          # 0.75 cells at the plane hits, 1.25 misses
    only(res, DIAG=(0, 1))
    assert (res['bitmap'][:, 0] >> ref.DIAG & 1).tolist() == [1, 0]
    only(group_transits('beyond_int32'), BIG_HI=(0, 1))
    for group in ('end_begin', 'jump', 'outside_end', 'nodata_end'):
        only(group_transits(group))
    only(group_transits('reaching_in'), OUTSIDE=(0, 2))
    only(group_transits('last'), A=(1, 0), C2=(1, 0))


def test_pingpong_lead_tail_and_cuts():
    base, ping = ref.expected('planted')['transits'], ref.expected('pingpong')['transits']
    # the walk that the ping-pong replaces had its own transits; what the 4096 moves add is 2048 a direction at least
    assert (ping[[ref.A, ref.C2]] >= 2048).all() and (ping[[ref.A, ref.C2]] <= base[[ref.A, ref.C2]] + 2048).all()
    c = ref.case('pingpong')
    alone = ref.compute(dict(c, tracks=[c['tracks'][11]], alts=[c['alts'][11]]))
    assert alone['transits'][ref.A].tolist() == alone['transits'][ref.C2].tolist() == [2048, 2048]
    # lead and tail points and every cut change nothing
    for name in ref.DEVICE_IDS:
        if name.startswith(('lead_', 'cuts')):
            assert np.array_equal(ref.expected(name)['transits'], base), name
    assert np.array_equal(ref.expected('pingpong_shift_3')['transits'], ping)
    cuts = ref.case('cuts')
    assert len(cuts['tracks'][0]) == 256 and all(len(t) == 4 for t in cuts['tracks'][1:65])
    # ... though reading them as moves would: the lead point and the first point are a transit of A
    c = ref.case('lead_5_shift_1')
    traj, alt, off = ref.flat(c)
    wrong = ref.brute_force(traj, alt, np.array([off[1] - 1, off[2]]), c['elev'], c['xy'], c['reach'], c['hub'], c['axis'], c['shape'])
    assert wrong['transits'][ref.A].sum() == 1
    wrong = ref.brute_force(traj, alt, np.array([off[-2], off[-1] + 1]), c['elev'], c['xy'], c['reach'], c['hub'], c['axis'], c['shape'])
    assert wrong['transits'][ref.A].sum() == ref.compute(dict(c, tracks=c['tracks'][-1:], alts=c['alts'][-1:], lead=0, tail=0))['transits'][ref.A].sum() + 1


def test_quotient_form_decides_the_same():
    """u_0 + t (u_1 - u_0) with t = s_0 / (s_0 - s_1), the form with the division, on the random case."""
    c = ref.case('random')
    traj, alt, off = ref.flat(c)
    k, _, dirn = ref.move_matrix(traj, alt, off[1:], c['elev'], c['xy'], c['reach'], c['hub'], c['axis'], c['shape'])
    r0, c0, r1, c1 = (traj[k, 0].astype(float), traj[k, 1].astype(float), traj[k + 1, 0].astype(float), traj[k + 1, 1].astype(float))
    e = c['elev'].astype(np.int64)
    z0 = e[traj[k, 0], traj[k, 1]] + alt[k]
    z1 = e[traj[k + 1, 0], traj[k + 1, 1]] + alt[k + 1]
    xt, yt, ax, ay = c['xy'][None, :, 0], c['xy'][None, :, 1], c['axis'][None, :, 0], c['axis'][None, :, 1]
    s0 = ax * (c0[:, None] - xt) + ay * (r0[:, None] - yt)
    s1 = ax * (c1[:, None] - xt) + ay * (r1[:, None] - yt)
    u0 = ax * (r0[:, None] - yt) - ay * (c0[:, None] - xt)
    u1 = ax * (r1[:, None] - yt) - ay * (c1[:, None] - xt)
    h0, h1 = (z0[:, None] - c['hub'][None, :]) / ref.MM, (z1[:, None] - c['hub'][None, :]) / ref.MM
    with np.errstate(invalid='ignore', divide='ignore'):
        t = s0 / (s0 - s1)
        u, h = u0 + t * (u1 - u0), h0 + t * (h1 - h0)
        hit = ((s0 < 0) != (s1 < 0)) & (u * u + h * h <= c['reach'][None, :] ** 2)
    assert np.array_equal(hit, dirn >= 0) and hit.sum() >= 150


# ------------------------------------------------------------------------------------------------ the cull
@pytest.mark.parametrize('name', ['random', 'planted', 'pingpong'])
def test_every_transit_is_in_the_list_of_its_first_points_bin(name):
    c = ref.case(name)
    traj, alt, off = ref.flat(c)
    k, _, dirn = ref.move_matrix(traj, alt, off[1:], c['elev'], c['xy'], c['reach'], c['hub'], c['axis'], c['shape'])
    start, items = ref.bins(c)
    nbc = -(-c['shape'][1] // 32)
    move, turbine = np.nonzero(dirn >= 0)
    assert move.size >= 150
    worst = 0.
    for m, t in zip(move, turbine):
        r, col = int(traj[k[m], 0]), int(traj[k[m], 1])
        b = (r >> 5) * nbc + (col >> 5)
        assert t in items[start[b]:start[b + 1]], (m, t)
        worst = max(worst, float(np.hypot(col - c['xy'][t, 0], r - c['xy'][t, 1]) - c['reach'][t]))
    assert worst <= np.sqrt(2.) + 1e-9 < ref.CULL_MARGIN


# ------------------------------------------------------------------------------------------------ disks and axes
def test_rotor_disks_and_axes():
    dem = np.arange(20, dtype=np.float64).reshape(4, 5) * 10.
    dem[2, 3] = np.nan
    table = tb.Turbines(dict(x=[100., 300., 140., 260.], y=[100., 200., 251., 0.], t_hh=[80., 90.5, 100., np.nan],
                             t_rd=[100., 120., np.nan, 90.]), min_hubheight=0.)
    assert len(table) == 3                                                    # (a NaN hub height does not pass the filter)
    xy, reach, hub, n_empty = tb.rotor_disks(table, dem, (0., 0., 400., 300.), 100., clearance=10.)
    assert xy.tolist() == [[1., 1.], [3., 2.], [1.4, 2.51]]
    assert reach[0] == 0.6 and np.isnan(reach[1:]).all() and n_empty == 2     # (nodata under the second, no t_rd for the third)
    assert hub.dtype == np.int32 and hub.tolist() == [60_000 + 80_000, 0, 0]
    cyl_reach, _ = tb.rotor_geometry(table, dem, (0., 0., 400., 300.), 100., clearance=10.)
    assert np.array_equal(reach, cyl_reach, equal_nan=True)
    tall = tb.Turbines(dict(x=[0.], y=[0.], t_hh=[100.], t_rd=[1.]))
    tall.columns['t_hh'] = np.array([3e6])                                    # (past the constructor's filter: 3e9 mm)
    assert tb.rotor_disks(tall, np.zeros((2, 2)), (0., 0., 100., 100.), 100.)[2].tolist() == [2 ** 31 - 1]
    with pytest.raises(ValueError, match='t_hh'):
        tb.rotor_disks(tb.Turbines(dict(x=[0.], y=[0.], t_rd=[1.])), np.zeros((2, 2)), (0., 0., 100., 100.), 100.)

    west = tb.rotor_axes(270., 'row_north')
    assert west.shape == (1, 2) and west.dtype == np.float64 and np.abs(west - [[-1., 0.]]).max() <= 1e-15
    assert np.abs(tb.rotor_axes(270., 'row_east') - [[0., -1.]]).max() <= 1e-15
    assert tb.rotor_axes(270., 'row_north', 3).shape == (3, 2) and tb.rotor_axes([0., 90.], 'row_north').shape == (2, 2)
    assert np.abs(tb.rotor_axes([0., 90.], 'row_north') - [[0., 1.], [1., 0.]]).max() <= 1e-15
    assert np.isnan(tb.rotor_axes([np.nan, 0.], 'row_north')[0]).all()
    with pytest.raises(ValueError, match='directions'):
        tb.rotor_axes([0., 90.], 'row_north', 3)
    # a bird flying east through a rotor that faces a westerly transits with the wind
    flat = dict(elev=np.zeros((5, 9), dtype=np.int32), xy=np.array([[4.5, 2.]]), reach=np.array([2.]),
                hub=np.array([0], dtype=np.int32), axis=west, shape=(5, 9))
    east = ref.brute_force(np.array([[2, 3], [2, 4], [2, 5], [2, 6]], dtype=np.int16), np.zeros(4, dtype=np.int32),
                           np.array([0, 4]), flat['elev'], flat['xy'], flat['reach'], flat['hub'], flat['axis'], flat['shape'])
    assert east['transits'].tolist() == [[1, 0]]


# ------------------------------------------------------------------------------------------------ Config
def test_config_fields_their_slot_and_section():
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    assert cfg.rotor_transits is False and cfg.rotor_yaw == -1.
    names = [f.name for f in fields(Config)]
    at = names.index('track_passage_radius')
    assert names[at + 1:at + 3] == ['rotor_transits', 'rotor_yaw']
    section = list(dict(_SECTIONS)['MI355X build'])
    at = section.index('track_passage_radius')
    assert section[at + 1:at + 3] == ['rotor_transits', 'rotor_yaw']
    text = str(Config(rotor_transits=True, rotor_yaw=90.)).split(':::: MI355X build')[1]
    assert 'rotor_transits = True' in text and 'rotor_yaw = 90.0' in text


def _turbines(**drop):
    cols = dict(x=[1500., 2500.], y=[700., 900.], t_hh=[80., 90.], t_rd=[100., 110.])
    return {k: v for k, v in cols.items() if k not in drop}


def test_constructor_refusals(tmp_path):
    """Each missing prerequisite by name, before any raster is computed (no GPU here)."""
    base = dict(run_name='t', out_dir=str(tmp_path), region_width_km=(8., 6.), resolution=100., track_count=10, sim_seed=1,
                rotor_transits=True)
    good = dict(flight_height=True, rotor_geometry='turbine')
    for kw, turbines, match in ((dict(good, flight_height=False), _turbines(), 'needs flight_height=True'),
                                (dict(good, rotor_geometry='band'), _turbines(), "needs rotor_geometry='turbine'"),
                                (good, None, 'needs turbines'),
                                (good, _turbines(t_hh=1), 'needs turbines with t_hh'),
                                (good, _turbines(t_rd=1), 'needs turbines with t_rd'),
                                (dict(good, rotor_yaw=float('nan')), _turbines(), 'rotor_yaw')):
        with pytest.raises(ValueError, match=match) as err:
            Simulator(Config(**base, **kw), terrain='synthetic', turbines=turbines)
        assert 'rotor_transits' in str(err.value) or 'rotor_yaw' in str(err.value)
    # (flight_time is no prerequisite: with everything else in place the constructor goes on to the rasters, which need
    # the device -- not tried here.)  Off, nothing is asked for
    sim = object.__new__(Simulator)
    sim.rotor_transits, sim.turbine_rotor_transits = False, {}
    sim._check_rotor_transits(None)
    with pytest.raises(ValueError, match='rotor_transits=True'):
        sim.compute_turbine_rotor_transits()


# ------------------------------------------------------------------------------------------------ the third header
def header_text():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def transit_prototypes():
    """{name: (restype, [argtypes])} of ssrs_hip_transits.h, by the parsing rules of test_native_abi.declared_prototypes."""
    code = '\n'.join(line for line in header_text().splitlines() if not line.lstrip().startswith('#'))
    protos = {}
    for ret, name, params in re.findall(r'([A-Za-z_][\w\s\*]*?)\b(ssrs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', code):
        ret = ' '.join(ret.replace('*', ' * ').split())
        assert ret in abi.RETURNS, f'{name}: return type {ret!r} is not in the binding\'s vocabulary'
        argtypes = []
        for param in [' '.join(p.split()) for p in params.split(',')]:
            if '*' in param:
                argtypes.append(C.c_void_p)
                continue
            ctype, _, pname = param.rpartition(' ')
            assert ctype in abi.SCALARS and re.fullmatch(r'[A-Za-z_]\w*', pname), f'{name}: parameter {param!r}'
            argtypes.append(abi.SCALARS[ctype])
        assert name not in protos, f'{name} declared twice'
        protos[name] = (abi.RETURNS[ret], argtypes)
    return protos


def test_transit_prototypes_match_their_header():
    from ssrs_amd import _native
    lib = _native.lib()
    protos = transit_prototypes()
    assert sorted(protos) == sorted(_native.TRANSIT_PROTOTYPES) == ['ssrs_rotor_transits']
    restype, argtypes = protos['ssrs_rotor_transits']
    fn = lib.ssrs_rotor_transits
    assert list(fn.argtypes) == argtypes and fn.restype is restype
    assert _native.ROTOR_TRANSITS_ARGTYPES == argtypes and len(argtypes) == 18 and argtypes[11] is C.c_double
    assert '#include "ssrs_hip.h"' in open(HEADER).read()
    found = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SSRS_ROTOR_TRANSIT_[A-Z0-9_]+)[ \t]+(\d+)[ \t]*$', header_text(), flags=re.M))
    assert found == {'SSRS_ROTOR_TRANSIT_LDS_TURBINES': '7680'} and _native.ROTOR_TRANSIT_LDS_TURBINES == 7680
    # the first header and its mirror are as they were
    assert not set(_native.TRANSIT_PROTOTYPES) & (set(_native.PROTOTYPES) | set(_native.PASSAGE_PROTOTYPES))
    assert 'ssrs_rotor_transits' not in _native.EXPORTS and len(abi.declared_functions()) == 79
    assert lib.ssrs_version() == 109


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    buf = (C.c_char * 64)()
    assert C.addressof(buf) % 8 == 0
    odd = lambda n: C.c_void_p(C.addressof(buf) + n)
    names = ('traj', 'off', 'ntracks', 'alt', 'info', 'rows', 'cols', 'xy', 'reach', 'hub', 'axis', 'mm', 'nturb', 'bin_start',
             'bin_items', 'hits', 'transits')
    good = dict(dict.fromkeys(names, buf), ntracks=1, rows=2, cols=2, mm=1000., nturb=1)
    bad = [(b'NULL', {name: None}) for name in names if good[name] is buf] + \
          [(b'ntracks', dict(ntracks=-1)), (b'ntracks', dict(ntracks=2 ** 31)), (b'nturb', dict(nturb=0)), (b'nturb', dict(nturb=8193)),
           (b'raster', dict(rows=0)), (b'raster', dict(cols=32768)), (b'4-byte aligned', dict(traj=odd(2))),
           (b'4-byte aligned', dict(alt=odd(2))), (b'cellinfo', dict(info=odd(4))), (b'8-byte aligned', dict(transits=odd(4))),
           (b'8-byte aligned', dict(axis=odd(4))), (b'hub', dict(hub=odd(2))), (b'mm_per_cell', dict(mm=0.)),
           (b'mm_per_cell', dict(mm=-1.)), (b'mm_per_cell', dict(mm=float('nan'))), (b'mm_per_cell', dict(mm=float('inf')))]
    assert len(bad) == 12 + 16
    for text, kw in bad:
        a = dict(good, **kw)
        rc = lib.ssrs_rotor_transits(*(a[name] for name in names), None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_rotor_transits' in lib.ssrs_last_error() and text in lib.ssrs_last_error(), (kw, lib.ssrs_last_error())
    assert bytes(buf) == bytes(64)
    # (no tracks: nothing to do, whatever the other arguments point at)
    assert lib.ssrs_rotor_transits(*(dict(good, ntracks=0)[name] for name in names), None) == _native.SSRS_OK
    assert bytes(buf) == bytes(64)
