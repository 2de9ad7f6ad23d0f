"""Collision risk (K19), the parts that need no device: Band's table against an independent evaluation and its exact
properties, the 1-D model's disk mean against its closed form, the classes, the planted rings of tests/collision_ref.py
against hand-computed integers, the Config fields and the constructor's refusals, the fourth header against the binding,
and the library's argument errors."""
import ctypes as C
import math
import os
import re
from dataclasses import fields

import numpy as np
import pytest

from ssrs_amd import Config, Simulator
from ssrs_amd import turbines as tb

import collision_ref as ref
import test_native_abi as abi
import transit_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ssrs_hip_collision.h')
BIRD = dict(speed=15., bird_length=0.85, bird_wingspan=2.1)


def table_of(rows, clearance=0., flapping=False, model_3d=True, profile=ref.PROFILE, **bird):
    """band_collision_table of turbines given as rows [R, rpm, max chord, pitch, blades]."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    return tb.band_collision_table(rows[:, 0], clearance, rows[:, 1:], flapping=flapping, model_3d=model_3d,
                                   chord_profile=profile, **dict(BIRD, **bird))


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('flapping, model_3d, clearance', [(False, True, 10.), (True, True, 0.), (False, False, 2.5)])
def test_table_against_an_independent_evaluation(flapping, model_3d, clearance):
    """turbines.band_collision_table (numpy, vectorised) against collision_ref.band_rows (plain Python, one radius at a
    time) at the 256 area midpoints.  The bound is ONE unit of 2^-32: both evaluate the same formula in f64, where p 2^32 <=
    2^32 carries an absolute rounding error of a few 2^-21 at most, so the two rint() can differ by one and no more."""
    rows = [(50., 12., 4., 15., 3.), (40., 15.5, 3.2, 10., 3.), (63., 9., 4.5, 20., 2.)]
    cls, table, classes = table_of(rows, clearance, flapping, model_3d)
    assert cls.tolist() == [0, 1, 2] and table.shape == (3, 2, 256) and table.dtype == np.uint32 and cls.dtype == np.int32
    for c, (R, rpm, chord, pitch, blades) in enumerate(rows):
        assert classes[c].tolist() == [R, R + clearance, rpm, chord, pitch, blades]
        want = ref.band_rows(R, R + clearance, rpm, chord, pitch, blades, 15., 0.85, 2.1, flapping, model_3d)
        assert np.abs(table[c].astype(np.int64) - want.astype(np.int64)).max() <= 1
        assert (want > 0).sum() >= 300                                       # (it is no table of zeros)
    # ring k's entry is p at r = reach sqrt((k + 0.5) / 256)
    p = tb.band_probability(60. * math.sqrt(100.5 / 256.), 50., 12., 4., 15., 3., 15., 0.85, 2.1, chord_profile=ref.PROFILE)
    assert table_of(rows[:1], 10.)[1][0, 1, 100] == int(np.rint(float(p) * 2. ** 32))


def test_exact_properties_of_the_table():
    row = (50., 12., 4., 15., 3.)
    _, table, _ = table_of([row], clearance=10.)
    # zero past the blade tip: ring k is past it when its midpoint 60 sqrt((k + 0.5) / 256) > 50
    past = 60. * np.sqrt((np.arange(256) + 0.5) / 256.) > 50.
    assert 70 < past.sum() < 90 and (table[0][:, past] == 0).all() and (table[0][:, ~past] > 0).all()
    # zero for no blades, no rotation, no speed
    for kw in (dict(rows=[(50., 12., 4., 15., 0.)]), dict(rows=[(50., 0., 4., 15., 3.)]), dict(rows=[row], speed=0.)):
        assert (table_of(kw.pop('rows'), **kw)[1] == 0).all()
    # clipped to [0, 1]: a slow bird in front of a fast rotor with many blades is hit for sure, and 1 is stored as 2^32 - 1
    _, sure, _ = table_of([(50., 60., 4., 15., 12.)], speed=1.)
    assert sure.max() == 2 ** 32 - 1 and (sure == 2 ** 32 - 1).sum() > 100
    # the two directions differ only through the sign: |+c sin + a c cos| against |-c sin + a c cos|, the same body term
    r = np.linspace(10., 50., 99)
    kw = dict(chord_profile=ref.PROFILE)
    up = tb.band_probability(r, *row, 15., 0.85, 2.1, upwind=True, **kw)
    down = tb.band_probability(r, *row, 15., 0.85, 2.1, upwind=False, **kw)
    flat = tb.band_probability(r, *row, 15., 0.85, 2.1, model_3d=False, **kw)
    omega = 2. * np.pi * 12. / 60.
    chord = 4. * np.interp(r / 50., np.arange(1, 21) * 0.05, ref.PROFILE)
    alpha, gamma, scale = 15. / (r * omega), np.deg2rad(15.), 3. * omega / (2. * np.pi * 15.)
    assert np.allclose(up - flat, scale * np.abs(chord * np.sin(gamma) + alpha * chord * np.cos(gamma)), rtol=0, atol=1e-14)
    assert np.allclose(down - flat, scale * np.abs(-chord * np.sin(gamma) + alpha * chord * np.cos(gamma)), rtol=0, atol=1e-14)
    assert (up >= down).all() and (up > down).sum() >= 90                    # (flying upwind is the riskier way)
    assert (table[0, 1] >= table[0, 0]).all()                                # [c, 1] is against the wind: the formula's +
    # K = 0 makes it independent of chord and pitch, and of the direction
    one = table_of([(50., 12., 4., 15., 3.)], model_3d=False)[1]
    other = table_of([(50., 12., 1.5, 40., 3.)], model_3d=False, profile=[1.] * 20)[1]
    assert np.array_equal(one, other) and np.array_equal(one[0, 0], one[0, 1])
    # the profile is a parameter: twice the chord, twice the swept term
    double = tb.band_probability(r, 50., 12., 8., 15., 3., 15., 0.85, 2.1, **kw)
    assert np.allclose(double - flat, 2. * (up - flat), rtol=0, atol=1e-14)
    for bad in ([1.] * 19, [1.] * 19 + [-0.1]):
        with pytest.raises(ValueError, match='chord profile'):
            tb.band_probability(r, *row, 15., 0.85, 2.1, chord_profile=bad)


def test_disk_mean_of_the_1d_model_against_its_closed_form():
    """K = 0: p(r) = min(1, b W F / (2 pi r)) inside r* = v / (Omega beta) and B = b Omega L / (2 pi v) outside.  In s = r^2 /
    R^2, which the equal-area rings cut into 256 equal cells, that is f(s) = min(1, A / sqrt(s)) for s < s* = (r* / R)^2 with
    A = b W F / (2 pi R), and B beyond, whose integral over [0, 1] is A^2 + 2 A (sqrt(s*) - A) + B (1 - s*) when A^2 <= s* <=
    1.  The table's mean is the midpoint rule with h = 1 / 256.  On a cell the rule's value and the integral both lie between
    h inf f and h sup f, so the rule is off by at most h (sup f - inf f) a cell, h TV(f) in all; f falls from 1 to F B at s*
    and steps to B there: TV = (1 - F B) + |B - F B|.  Each entry is rounded to 2^-32, half a unit at most.  The bound is
    that sum, derived here and not from the table."""
    b, R, rpm, v, L, W = 3., 50., 12., 15., 0.85, 2.1
    omega = 2. * math.pi * rpm / 60.
    for flapping in (False, True):
        F = 1. if flapping else 2. / math.pi
        A, B = b * W * F / (2. * math.pi * R), b * omega * L / (2. * math.pi * v)
        s_star = (v / (omega * L / W) / R) ** 2
        assert A * A < s_star < 1. and B < 1.
        integral = A * A + 2. * A * (math.sqrt(s_star) - A) + B * (1. - s_star)
        bound = ((1. - F * B) + abs(B - F * B)) / 256. + 2. ** -33
        _, table, _ = table_of([(R, rpm, 4., 15., b)], flapping=flapping, model_3d=False)
        for dirn in (0, 1):
            mean = float(table[0, dirn].astype(np.float64).sum()) / 256. / 2. ** 32
            print(f'flapping={flapping} dirn={dirn}: table mean {mean:.6f}, closed form {integral:.6f}, bound {bound:.6f}')
            assert abs(mean - integral) <= bound
        assert 0.02 < integral < 0.2


def test_classes():
    rows = [(50., 12., 4., 15., 3.), (40., 12., 4., 15., 3.), (50., 12., 4., 15., 3.), (50., np.nan, 4., 15., 3.),
            (np.nan, 12., 4., 15., 3.), (40., 12., 4., 15., 3.), (50., 12., 4., 15., 2.)]
    cls, table, classes = table_of(rows, clearance=5.)
    assert cls.tolist() == [0, 1, 0, -1, -1, 1, 2] and table.shape == (3, 2, 256) and classes.shape == (3, 6)
    assert classes[:, 0].tolist() == [50., 40., 50.] and classes[:, 1].tolist() == [55., 45., 55.]
    # without a valid turbine: one row of zeros (the library asks for nclass >= 1)
    cls, table, classes = table_of([(np.nan, 12., 4., 15., 3.)])
    assert cls.tolist() == [-1] and table.shape == (1, 2, 256) and not table.any() and classes.shape == (0, 6)
    # the parameters come from the turbine columns where the table carries them
    fleet = tb.Turbines(dict(x=[0., 1., 2.], y=[0., 0., 0.], t_rd=[100., 100., 80.], t_rpm=[12., 14., 12.],
                             t_blades=[3, 3, 2]), min_hubheight=0.)
    params = tb.band_parameters(fleet, blades=5, rpm=99., max_chord=4., pitch=15.)
    assert params.tolist() == [[12., 4., 15., 3.], [14., 4., 15., 3.], [12., 4., 15., 2.]]
    plain = tb.Turbines(dict(x=[0., 1.], y=[0., 0.]), min_hubheight=0.)
    assert tb.band_parameters(plain, 3, 12., 4., 15.).tolist() == [[12., 4., 15., 3.]] * 2


# ------------------------------------------------------------------------------------------------ the planted rings
def test_planted_rings_by_hand():
    """Every planted track's transits of the main turbine, in move order, as (direction, ring) worked out by hand in
    collision_ref._ring_tracks; the turbines that share its place see the same; the one with no reach only its own hub."""
    c = ref.case('rings')
    res = ref.expected('rings')
    planted = ref._ring_tracks()
    for j, (_, _, name, want) in enumerate(planted):
        for t in (ref.T_MAIN, ref.T_OTHER, ref.T_NOCLASS, ref.T_PASTCLASS):
            got = [(d, k) for track, turbine, d, k in res['rings'] if track == j and turbine == t]
            assert got == want, (j, name, t, got[:4], want[:4])
    zero = [(track, d, k) for track, turbine, d, k in res['rings'] if turbine == ref.T_ZERO]
    first = [j for j, (_, _, name, _) in enumerate(planted) if name == 'zero_reach'][0]
    assert zero == [(first, 1, 0)]
    assert not [1 for _, turbine, _, _ in res['rings'] if turbine == ref.T_FAR]
    # the sums by hand: classes 0 and 1 for the two that count, nothing for class -1 and the class past the table
    table = c['table'].astype(np.int64)
    want = np.zeros((6, 2), dtype=np.int64)
    per_track = np.zeros(len(planted), dtype=np.int64)
    for j, (_, _, _, rings) in enumerate(planted):
        for d, k in rings:
            want[ref.T_MAIN, d] += table[0, d, k]
            want[ref.T_OTHER, d] += table[1, d, k]
            per_track[j] += table[0, d, k] + table[1, d, k]
    want[ref.T_ZERO, 1] = table[0, 1, 0]
    per_track[first] += table[0, 1, 0]
    assert np.array_equal(res['risk'], want) and np.array_equal(res['track_risk'], per_track)
    assert res['transits'][ref.T_NOCLASS].tolist() == res['transits'][ref.T_MAIN].tolist() == [1199, 1218]
    assert np.array_equal(ref.expected('rings_shift_3')['risk'], want)
    # the transits are K18's own
    for name in ('rings', 'planted', 'pingpong'):
        assert np.array_equal(ref.expected(name)['transits'], tref.compute(ref.case(name))['transits'])
    ping = ref.expected('pingpong')
    assert ping['risk'][tref.A].min() > 2 ** 40 and ping['risk'][tref.DIAG].sum() == 0 < ping['transits'][tref.DIAG].sum()
    assert ping['risk'].sum() == ping['track_risk'].sum()


# ------------------------------------------------------------------------------------------------ Config
def test_config_fields_their_slot_and_section():
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    new = ['collision_risk', 'bird_length', 'bird_wingspan', 'bird_flight', 'collision_avoidance', 'collision_model_3d',
           'rotor_blades', 'rotor_rpm', 'rotor_max_chord', 'rotor_pitch', 'rotor_chord_profile']
    assert [getattr(cfg, n) for n in new] == [False, 0.85, 2.1, 'gliding', 0., True, 3, 12., 4., 15., ref.PROFILE]
    names = [f.name for f in fields(Config)]
    at = names.index('rotor_yaw')
    assert names[at + 1:at + 12] == new
    section = list(dict(_SECTIONS)['MI355X build'])
    at = section.index('rotor_yaw')
    assert section[at + 1:at + 12] == new and section[-1] == 'turbine_encounter_radius'
    text = str(Config(collision_risk=True, bird_flight='flapping', rotor_rpm=14.5)).split(':::: MI355X build')[1]
    assert 'collision_risk = True' in text and 'bird_flight = flapping' in text and 'rotor_rpm = 14.5' in text
    assert 'rotor_chord_profile = (0.73, 0.79' in text


def _turbines(**drop):
    cols = dict(x=[1500., 2500.], y=[700., 900.], t_hh=[80., 90.], t_rd=[100., 110.])
    return {k: v for k, v in cols.items() if k not in drop}


def test_constructor_refusals(tmp_path):
    """Each missing prerequisite and each impossible bird or rotor by name, before any raster is computed (no GPU here)."""
    base = dict(run_name='t', out_dir=str(tmp_path), region_width_km=(8., 6.), resolution=100., track_count=10, sim_seed=1,
                collision_risk=True)
    good = dict(flight_height=True, rotor_geometry='turbine')
    for kw, turbines, match in ((dict(good, flight_height=False), _turbines(), 'needs flight_height=True'),
                                (dict(good, rotor_geometry='band'), _turbines(), "needs rotor_geometry='turbine'"),
                                (good, None, 'needs turbines'),
                                (good, _turbines(t_hh=1), 'needs turbines with t_hh'),
                                (good, _turbines(t_rd=1), 'needs turbines with t_rd'),
                                (dict(good, rotor_yaw=float('nan')), _turbines(), 'rotor_yaw'),
                                (dict(good, bird_length=0.), _turbines(), 'bird_length'),
                                (dict(good, bird_wingspan=float('nan')), _turbines(), 'bird_wingspan'),
                                (dict(good, bird_flight='soaring'), _turbines(), 'bird_flight'),
                                (dict(good, collision_avoidance=1.5), _turbines(), 'collision_avoidance'),
                                (dict(good, collision_avoidance=-0.1), _turbines(), 'collision_avoidance'),
                                (dict(good, rotor_blades=-1), _turbines(), 'rotor_blades'),
                                (dict(good, rotor_rpm=float('inf')), _turbines(), 'rotor_rpm'),
                                (dict(good, rotor_max_chord=-4.), _turbines(), 'rotor_max_chord'),
                                (dict(good, rotor_pitch=float('nan')), _turbines(), 'rotor_pitch'),
                                (dict(good, rotor_chord_profile=(1.,) * 19), _turbines(), 'rotor_chord_profile')):
        with pytest.raises(ValueError, match=match) as err:
            Simulator(Config(**base, **kw), terrain='synthetic', turbines=turbines)
        assert 'collision_risk' in str(err.value) or 'rotor_yaw' in str(err.value)
    # off, nothing is asked for: not even a sensible bird
    sim = object.__new__(Simulator)
    sim.collision_risk, sim.turbine_collision_risk, sim.bird_length = False, {}, -1.
    sim._check_collision_risk(None)
    with pytest.raises(ValueError, match='collision_risk=True'):
        sim.compute_turbine_collision_risk()


# ------------------------------------------------------------------------------------------------ the fourth header
def header_text():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def collision_prototypes():
    """{name: (restype, [argtypes])} of ssrs_hip_collision.h, by the parsing rules of test_native_abi.declared_prototypes."""
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


def test_collision_prototypes_match_their_header():
    from ssrs_amd import _native
    lib = _native.lib()
    protos = collision_prototypes()
    assert sorted(protos) == sorted(_native.COLLISION_PROTOTYPES) == ['ssrs_rotor_collision_risk']
    restype, argtypes = protos['ssrs_rotor_collision_risk']
    fn = lib.ssrs_rotor_collision_risk
    assert list(fn.argtypes) == argtypes and fn.restype is restype
    assert _native.argtypes('ssrs_rotor_collision_risk') == argtypes == _native.ROTOR_COLLISION_RISK_ARGTYPES
    # ssrs_rotor_transits' arguments, then cls, table, nclass, risk, track_risk, and the stream last
    assert len(argtypes) == 23 and argtypes[:17] == _native.ROTOR_TRANSITS_ARGTYPES[:17] and argtypes[19] is C.c_int
    assert _native.COLLISION_PROTOTYPES['ssrs_rotor_collision_risk'] == \
        _native.TRANSIT_PROTOTYPES['ssrs_rotor_transits'][:-1] + 'ppippp'
    assert '#include "ssrs_hip_transits.h"' in open(HEADER).read()
    found = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SSRS_[A-Z0-9_]+)[ \t]+(\d+)[ \t]*$', header_text(), flags=re.M))
    assert found == {'SSRS_COLLISION_RINGS': '256', 'SSRS_ROTOR_COLLISION_LDS_TURBINES': '2560'}
    assert _native.COLLISION_RINGS == tb.COLLISION_RINGS == 256 and _native.ROTOR_COLLISION_LDS_TURBINES == 2560
    # a group of its own: the other headers and their mirrors are as they were
    others = set(_native.PROTOTYPES) | set(_native.PASSAGE_PROTOTYPES) | set(_native.TRANSIT_PROTOTYPES)
    assert not set(_native.COLLISION_PROTOTYPES) & others and list(_native.TRANSIT_PROTOTYPES) == ['ssrs_rotor_transits']
    assert 'ssrs_rotor_collision_risk' not in _native.EXPORTS and len(abi.declared_functions()) == 79
    assert lib.ssrs_version() == 109


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    buf = (C.c_char * 64)()
    assert C.addressof(buf) % 8 == 0
    odd = lambda n: C.c_void_p(C.addressof(buf) + n)
    names = ('traj', 'off', 'ntracks', 'alt', 'info', 'rows', 'cols', 'xy', 'reach', 'hub', 'axis', 'mm', 'nturb', 'bin_start',
             'bin_items', 'hits', 'transits', 'cls', 'table', 'nclass', 'risk', 'track_risk')
    good = dict(dict.fromkeys(names, buf), ntracks=1, rows=2, cols=2, mm=1000., nturb=1, nclass=1)
    bad = [(b'NULL', {name: None}) for name in names if good[name] is buf and name != 'track_risk'] + \
          [(b'ntracks', dict(ntracks=-1)), (b'nturb', dict(nturb=0)), (b'nturb', dict(nturb=8193)),
           (b'raster', dict(rows=0)), (b'4-byte aligned', dict(traj=odd(2))), (b'8-byte aligned', dict(transits=odd(4))),
           (b'mm_per_cell', dict(mm=0.)),
           (b'nclass', dict(nclass=0)), (b'nclass', dict(nclass=-3)), (b'4-byte aligned', dict(cls=odd(2))),
           (b'4-byte aligned', dict(table=odd(1))), (b'8-byte aligned', dict(risk=odd(4))),
           (b'8-byte aligned', dict(track_risk=odd(4))), (b'8-byte aligned', dict(track_risk=odd(1)))]
    assert len(bad) == 15 + 14
    for text, kw in bad:
        a = dict(good, **kw)
        rc = lib.ssrs_rotor_collision_risk(*(a[name] for name in names), None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_rotor_collision_risk' in lib.ssrs_last_error() and text in lib.ssrs_last_error(), \
            (kw, lib.ssrs_last_error())
    assert bytes(buf) == bytes(64)
    # (no tracks: nothing to do, whatever the other arguments point at; track_risk may be NULL)
    for kw in (dict(ntracks=0), dict(ntracks=0, track_risk=None)):
        assert lib.ssrs_rotor_collision_risk(*(dict(good, **kw)[name] for name in names), None) == _native.SSRS_OK
    assert bytes(buf) == bytes(64)
