"""K20 on the host, without a GPU: the fifth header against its binding, the library's argument refusals, the Config
fields and the constructor's refusals, the window statement of include/ssrs_hip_sites.h by a brute force over ALL sites, and
a hand-made case whose rings are known."""
import ctypes as C
import os
import re
from dataclasses import fields

import numpy as np
import pytest

from ssrs_amd import Config, Simulator
from ssrs_amd import turbines as tb

import collision_ref as cref
import site_ref as ref
import test_native_abi as abi
import transit_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ssrs_hip_sites.h')


# ------------------------------------------------------------------------------------------------ the fifth header
def header_text():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def site_prototypes():
    """{name: (restype, [argtypes])} of ssrs_hip_sites.h, by the parsing rules of test_native_abi.declared_prototypes."""
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


def test_site_prototypes_match_their_header():
    from ssrs_amd import _native
    lib = _native.lib()
    protos = site_prototypes()
    assert sorted(protos) == sorted(_native.SITE_PROTOTYPES) == ['ssrs_site_collision_risk']
    restype, argtypes = protos['ssrs_site_collision_risk']
    fn = lib.ssrs_site_collision_risk
    assert list(fn.argtypes) == argtypes and fn.restype is restype
    assert _native.argtypes('ssrs_site_collision_risk') == argtypes == _native.SITE_COLLISION_RISK_ARGTYPES
    # the chunk and the raster as ssrs_rotor_transits takes them, then the class, the axis, the table, and the stream last
    assert len(argtypes) == 16 and argtypes[:7] == _native.ROTOR_TRANSITS_ARGTYPES[:7]
    assert argtypes[7] is C.c_double and argtypes[8] is C.c_int and argtypes[10] is C.c_int and argtypes[11] is C.c_double
    assert '#include "ssrs_hip_collision.h"' in open(HEADER).read()
    found = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SSRS_[A-Z0-9_]+)[ \t]+([\d.]+)[ \t]*$', header_text(), flags=re.M))
    assert found == {'SSRS_SITE_MAX_REACH': '62.0'}
    assert _native.SITE_MAX_REACH == tb.SITE_MAX_REACH == 62.
    # a group of its own: the other headers and their mirrors are as they were
    others = set(_native.PROTOTYPES) | set(_native.PASSAGE_PROTOTYPES) | set(_native.TRANSIT_PROTOTYPES) | \
        set(_native.COLLISION_PROTOTYPES)
    assert not set(_native.SITE_PROTOTYPES) & others and list(_native.COLLISION_PROTOTYPES) == ['ssrs_rotor_collision_risk']
    assert 'ssrs_site_collision_risk' not in _native.EXPORTS and len(abi.declared_functions()) == 79
    assert lib.ssrs_version() == 109


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    buf = (C.c_char * 64)()
    assert C.addressof(buf) % 8 == 0
    odd = lambda n: C.c_void_p(C.addressof(buf) + n)
    names = ('traj', 'off', 'ntracks', 'alt', 'info', 'rows', 'cols', 'reach', 'hub_mm', 'axis', 'per_cell', 'mm', 'table',
             'transits', 'risk')
    good = dict(dict.fromkeys(names, buf), ntracks=1, rows=2, cols=2, reach=4., hub_mm=90000, per_cell=0, mm=1000.)
    nan, inf = float('nan'), float('inf')
    bad = [(b'NULL', {name: None}) for name in names if good[name] is buf and name != 'transits'] + \
          [(b'ntracks', dict(ntracks=-1)), (b'raster', dict(rows=0)), (b'raster', dict(cols=0)), (b'raster', dict(cols=-5)),
           (b'raster', dict(rows=32768)), (b'4-byte aligned', dict(traj=odd(2))), (b'4-byte aligned', dict(alt=odd(1))),
           (b'8-byte aligned', dict(info=odd(4))), (b'8-byte aligned', dict(axis=odd(4))), (b'4-byte aligned', dict(table=odd(2))),
           (b'8-byte aligned', dict(transits=odd(4))), (b'8-byte aligned', dict(risk=odd(4))),
           (b'mm_per_cell', dict(mm=0.)), (b'mm_per_cell', dict(mm=-1000.)), (b'mm_per_cell', dict(mm=nan)),
           (b'mm_per_cell', dict(mm=inf)), (b'reach', dict(reach=62.5)), (b'reach', dict(reach=inf)),
           # the refusals come before the reach that has nothing to do
           (b'NULL', dict(reach=nan, risk=None)), (b'mm_per_cell', dict(reach=-1., mm=0.))]
    assert len(bad) == 7 + 20
    for text, kw in bad:
        a = dict(good, **kw)
        rc = lib.ssrs_site_collision_risk(*(a[name] for name in names), None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_site_collision_risk' in lib.ssrs_last_error() and text in lib.ssrs_last_error(), (kw, lib.ssrs_last_error())
    assert bytes(buf) == bytes(64)
    # nothing to do, whatever the other arguments point at: no tracks, a NaN or negative reach; transits may be NULL
    for kw in (dict(ntracks=0), dict(ntracks=0, transits=None), dict(reach=nan), dict(reach=-0.5), dict(reach=-inf, transits=None)):
        assert lib.ssrs_site_collision_risk(*(dict(good, **kw)[name] for name in names), None) == _native.SSRS_OK
    assert bytes(buf) == bytes(64)


# ------------------------------------------------------------------------------------------------ Config and Simulator
def test_config_fields_their_slot_and_section():
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    new = ['site_collision_risk', 'site_hub_height', 'site_rotor_diameter']
    assert [getattr(cfg, n) for n in new] == [False, 90., 120.]
    names = [f.name for f in fields(Config)]
    at = names.index('rotor_chord_profile')
    assert names[at + 1:at + 4] == new
    section = list(dict(_SECTIONS)['MI355X build'])
    at = section.index('rotor_chord_profile')
    assert section[at + 1:at + 4] == new and section[-1] == 'turbine_encounter_radius'
    text = str(Config(site_collision_risk=True, site_hub_height=105.5)).split(':::: MI355X build')[1]
    assert 'site_collision_risk = True' in text and 'site_hub_height = 105.5' in text and 'site_rotor_diameter = 120.0' in text


def test_constructor_refusals(tmp_path):
    """Each missing prerequisite and each impossible class, bird or rotor by name, before any raster is computed (no GPU
    here); no turbines and no rotor_geometry are asked for."""
    base = dict(run_name='t', out_dir=str(tmp_path), region_width_km=(8., 6.), resolution=100., track_count=10, sim_seed=1,
                site_collision_risk=True)
    good = dict(flight_height=True)
    for kw, match in ((dict(good, flight_height=False), 'needs flight_height=True'),
                      (dict(good, site_hub_height=0.), 'site_hub_height'),
                      (dict(good, site_hub_height=float('nan')), 'site_hub_height'),
                      (dict(good, site_rotor_diameter=-120.), 'site_rotor_diameter'),
                      (dict(good, site_rotor_diameter=float('inf')), 'site_rotor_diameter'),
                      (dict(good, rotor_clearance=float('nan')), 'rotor_clearance'),
                      (dict(good, site_rotor_diameter=12000., rotor_clearance=250.), r'\(12000 / 2 \+ 250\) / 100 = 62.5 cells'),
                      (dict(good, rotor_yaw=float('nan')), 'rotor_yaw'),
                      (dict(good, bird_length=0.), 'bird_length'),
                      (dict(good, bird_wingspan=float('nan')), 'bird_wingspan'),
                      (dict(good, bird_flight='soaring'), 'bird_flight'),
                      (dict(good, collision_avoidance=1.5), 'collision_avoidance'),
                      (dict(good, rotor_blades=-1), 'rotor_blades'),
                      (dict(good, rotor_rpm=float('inf')), 'rotor_rpm'),
                      (dict(good, rotor_max_chord=-4.), 'rotor_max_chord'),
                      (dict(good, rotor_pitch=float('nan')), 'rotor_pitch'),
                      (dict(good, rotor_chord_profile=(1.,) * 19), 'rotor_chord_profile')):
        with pytest.raises(ValueError, match=match) as err:
            Simulator(Config(**base, **kw), terrain='synthetic')
        assert 'site_collision_risk' in str(err.value) or 'rotor_yaw' in str(err.value)
    # the checks are collision_risk's own, factored: the same refusal under its name
    with pytest.raises(ValueError, match=r'bird_flight.*\(collision_risk\)'):
        Simulator(Config(**dict(base, site_collision_risk=False, collision_risk=True), flight_height=True,
                         rotor_geometry='turbine', bird_flight='soaring'), terrain='synthetic',
                  turbines=dict(x=[1500.], y=[700.], t_hh=[80.], t_rd=[100.]))
    # off, nothing is asked for: not even a sensible class
    sim = object.__new__(Simulator)
    sim.site_collision_risk, sim.site_collision_risk_sums, sim.site_hub_height = False, {}, -1.
    sim._check_site_collision_risk()
    assert sim._resolve_site_class() is None
    with pytest.raises(ValueError, match='site_collision_risk=True'):
        sim.compute_site_collision_risk_map()


def test_the_class_of_a_run_is_collision_risks_class():
    """The table of the candidate class is band_collision_table's row of a fleet of that class, and reach and hub_mm are
    rotor_disks' numbers."""
    sim = object.__new__(Simulator)
    for name, value in vars(Config(site_collision_risk=True, flight_height=True, resolution=50., site_hub_height=87.5,
                                   site_rotor_diameter=130., rotor_clearance=5., bird_flight='flapping')).items():
        setattr(sim, name, value)
    sim._check_site_collision_risk()
    reach, hub_mm, table = sim._resolve_site_class()
    assert reach == (65. + 5.) / 50. and hub_mm == 87500 and table.shape == (2, 256) and table.dtype == np.uint32
    cfg = Config()
    _, want, classes = tb.band_collision_table(np.array([65., 65.]), 5., np.array([[cfg.rotor_rpm, cfg.rotor_max_chord,
                                               cfg.rotor_pitch, cfg.rotor_blades]] * 2), cfg.flight_airspeed, cfg.bird_length,
                                               cfg.bird_wingspan, True, True, cfg.rotor_chord_profile)
    assert classes.shape == (1, 6) and np.array_equal(table, want[0]) and table.max() > 0


# ------------------------------------------------------------------------------------------------ the window statement
def _window_case():
    """A 12 x 16 raster with random walks of unit moves and, planted, the diagonal moves whose second point lies on the
    plane of a site W columns away."""
    shape = (12, 16)
    rng = np.random.default_rng(12)
    tracks, alts = [], []
    for _ in range(12):
        p = [(int(rng.integers(0, 12)), int(rng.integers(0, 16)))]
        for _ in range(60):
            r, c = p[-1]
            p.append((min(11, max(0, r + int(rng.integers(-1, 2)))), min(15, max(0, c + int(rng.integers(-1, 2))))))
        tracks.append(np.array(p, dtype=np.int16))
        alts.append(rng.integers(20_000, 90_000, len(p)).astype(np.int32))
    planted = [[(4, 2), (5, 3)], [(6, 13), (5, 12)]]
    for p in planted:
        tracks.append(np.array(p, dtype=np.int16))
        alts.append(np.full(2, ref.LEVEL, dtype=np.int32))
    return dict(name='window', shape=shape, tracks=tracks, alts=alts, elev=np.full(shape, ref.GROUND, dtype=np.int32), lead=0,
                tail=0, shift=0), len(tracks) - len(planted)


@pytest.mark.parametrize('reach', [4.0, 0.65, 2.25])
def test_window_statement(reach):
    """Full brute force over ALL sites: every transited site lies within W of the move's first point; the planted diagonal
    move (r, c) -> (r + 1, c + 1) meets the plane of row r + 1 at its second point, column c + 1, so the site at column
    c + 1 + floor(reach) is transited from W = floor(reach) + 1 columns away when reach + 1.5 does not pass the next
    integer (4.0 and 2.25; not 0.65): W is attained, and a window of W - 1 would lose that transit."""
    c, first_planted = _window_case()
    W = ref.window(reach)
    traj, alt, offsets = tref.flat(c)
    off = offsets[1:]
    every = ref.brute_force(traj, alt, off, c['elev'], reach, ref.LEVEL, ref.PLANE, ref.TABLE, c['shape'], every_site=True)
    # (the restriction of the oracle drops nothing)
    near = ref.brute_force(traj, alt, off, c['elev'], reach, ref.LEVEL, ref.PLANE, ref.TABLE, c['shape'])
    assert np.array_equal(every['transits'], near['transits']) and np.array_equal(every['risk'], near['risk'])
    assert every['transits'].sum() > 100
    # the moves in brute-force order: one track here, so rings' first entry is the track; find the move through its points
    k, r0, c0 = ref.first_points(traj, alt, off, c['elev'], c['shape'])
    _, dirn, _ = cref.ring_matrix(traj, alt, off, c['elev'], *ref.site_turbines(c['elev'], reach, ref.LEVEL, ref.PLANE), c['shape'])
    move, site = np.nonzero(dirn >= 0)
    dist = np.maximum(np.abs(site // 16 - r0[move]), np.abs(site % 16 - c0[move]))
    assert move.size == every['transits'].sum() and dist.max() <= W
    if reach in (4.0, 2.25):
        far = dist == W
        assert far.any(), 'W is attained'
        # the planted move (4, 2) -> (5, 3): the site of row 5 at column 3 + floor(reach)
        want = (5, 3 + int(reach))
        assert every['transits'][want][1] >= 1 and want[1] - 2 == W
        assert (np.stack([site // 16, site % 16], 1)[far] == want).all(1).any()


# ------------------------------------------------------------------------------------------------ by hand
@pytest.mark.parametrize('col', [30, 4, 85])
def test_hand_made_rings(col):
    """A move (19, c) -> (20, c) at hub height with the axis along +row and reach 4 transits exactly the sites
    (20, c - 4 .. c + 4), against the wind, at lateral offsets -4 .. 4: lhs / rhs = offset^2 / 16."""
    shape = ref.SHAPE
    elev = np.full(shape, ref.GROUND, dtype=np.int32)
    traj = np.array([(19, col), (20, col)], dtype=np.int16)
    alt = np.full(2, ref.LEVEL, dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    table = np.arange(512, dtype=np.uint32).reshape(2, 256) * 1000 + 7
    res = ref.brute_force(traj, alt, off, elev, 4.0, ref.LEVEL, ref.PLANE, table, shape, every_site=True)
    want = np.zeros(shape + (2,), dtype=np.int64)
    want[20, col - 4:col + 5, 1] = 1
    assert np.array_equal(res['transits'], want)
    rings = [255, 144, 64, 16, 0, 16, 64, 144, 255]
    assert [(t, s, d, k) for t, s, d, k in res['rings']] == [(0, 20 * shape[1] + col - 4 + j, 1, k) for j, k in enumerate(rings)]
    assert res['risk'][20, col - 4:col + 5, 1].tolist() == [int(table[1, k]) for k in rings] and res['risk'][..., 0].sum() == 0
