"""Track passage (K17), the parts that need no device: the numpy restatement against the definition itself, r2 from
metres, the second header against the binding, the library's refusals, the Config field and the constructor's checks."""
import ctypes as C
import os
import re
from dataclasses import fields

import numpy as np
import pytest
import torch

from ssrs_amd import Config, Simulator, presence

import occupancy_ref
import passage_ref as ref
import test_native_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'ssrs_hip_passage.h')


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_a_hand_made_case():
    tracks = [np.array([[0, 0], [5, 5]], dtype=np.int16),                        # (5, 5) is outside a 2 x 3 raster
              np.array([[1, 2]], dtype=np.int16), np.zeros((0, 2), dtype=np.int16)]
    counts, per_track = ref.passage(tracks, (2, 3), 1)
    assert counts.tolist() == [[1, 1, 1], [1, 1, 1]] and per_track.tolist() == [3, 3, 0]
    counts, per_track = ref.passage(tracks, (2, 3), 2)
    assert counts.tolist() == [[1, 2, 1], [1, 2, 1]] and per_track.tolist() == [4, 4, 0]
    assert [len(ref.disk(r2)) for r2 in (0, 1, 2, 4, 5, 8, 9, 25, 26)] == [1, 5, 9, 13, 21, 25, 29, 81, 89]
    assert (5, 1) in ref.disk(26) and (5, 1) not in ref.disk(25)
    # (the plus of r2 = 1 after any unit move: three of its five cells are new)
    assert ref.crescent_sizes(0) == [1] * 8 and ref.crescent_sizes(1) == [3] * 8
    for c in ref.CASES:
        assert all(t.dtype == np.int16 and t.ndim == 2 and t.shape[1] == 2 for t in c['tracks']), c['name']
        assert 0 <= c['r2'] <= 255 * 255 and c['shape'] in ref.RASTERS + ((11, 1030),)
    assert {c['r2'] for c in ref.CASES} >= set(ref.R2S) | {3, 83, 35}


SMALL = [c['name'] for c in ref.CASES if c['name'].startswith('basic_') and c['shape'][0] * c['shape'][1] <= 15]


@pytest.mark.parametrize('name', SMALL)
def test_restatement_is_the_definition(name):
    """Every cell measured against every point, on the rasters of at most 15 cells (all radii, the all-covering one too)."""
    c = ref.case(name)
    counts, per_track = ref.brute(c['tracks'], c['shape'], c['r2'])
    assert np.array_equal(counts, ref.expected(name)[0]) and np.array_equal(per_track, ref.expected(name)[1])


def test_restatement_is_the_definition_on_a_larger_raster():
    c = ref.case('lead_2')
    counts, per_track = ref.brute(c['tracks'][:12], c['shape'], 26)
    got = ref.passage(c['tracks'][:12], c['shape'], 26)
    assert np.array_equal(counts, got[0]) and np.array_equal(per_track, got[1])


@pytest.mark.parametrize('name', ['borders_33', 'empty_tracks', 'outside', 'shape_1x40', 'shape_1x1', 'memset_path'])
def test_r2_zero_is_the_occupancy_reference(name):
    c = occupancy_ref.case(name)
    counts, per_track = ref.passage(c['tracks'], c['shape'], 0)
    assert np.array_equal(counts, occupancy_ref.expected(name)[0]) and np.array_equal(per_track, occupancy_ref.expected(name)[1])


# ------------------------------------------------------------------------------------------------ r2 from metres
def test_passage_r2():
    """floor((R / resolution)^2) in f64, no epsilon: exact squares and either side of them."""
    assert presence.passage_r2(0., 10.) == 0
    assert presence.passage_r2(50., 10.) == 25 and presence.passage_r2(30., 10.) == 9 and presence.passage_r2(2550., 10.) == 65025
    assert presence.passage_r2(np.nextafter(50., 0.), 10.) == 24 and presence.passage_r2(np.nextafter(50., 100.), 10.) == 25
    assert presence.passage_r2(51., 10.) == 26                                   # 5.1^2 = 26.01
    assert presence.passage_r2(50.9, 10.) == 25                                  # 5.09^2 = 25.9
    assert presence.passage_r2(25., 10.) == 6 and presence.passage_r2(9.99, 10.) == 0 and presence.passage_r2(10., 10.) == 1
    # sqrt(26) cells: the f64 square of the f64 root is what the floor sees (no epsilon)
    root = float(np.sqrt(26.))
    assert presence.passage_r2(root * 1., 1.) == int(np.floor(root * root))
    for radius, resolution in ((-1., 10.), (float('nan'), 10.), (2551., 10.), (np.nextafter(2550., 3000.), 10.), (float('inf'), 10.)):
        with pytest.raises(ValueError) as err:
            presence.passage_r2(radius, resolution)
        assert repr(float(radius)) in str(err.value) and repr(float(resolution)) in str(err.value)
    with pytest.raises(ValueError, match='resolution'):
        presence.passage_r2(10., 0.)


# ------------------------------------------------------------------------------------------------ the second header
def header_text():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def passage_prototypes():
    """{name: (restype, [argtypes])} of ssrs_hip_passage.h, by the parsing rules of test_native_abi.declared_prototypes."""
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


def test_passage_prototypes_match_their_header():
    from ssrs_amd import _native
    lib = _native.lib()
    protos = passage_prototypes()
    assert sorted(protos) == sorted(_native.PASSAGE_PROTOTYPES) == ['ssrs_track_passage', 'ssrs_track_passage_workspace_bytes']
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
    assert _native.PASSAGE_ARGTYPES == protos['ssrs_track_passage'][1] and len(_native.PASSAGE_ARGTYPES) == 13
    assert '#include "ssrs_hip.h"' in open(HEADER).read()


def test_passage_constants_match_their_header():
    from ssrs_amd import _native
    found = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SSRS_PASSAGE_[A-Z0-9_]+)[ \t]+(\d+)[ \t]*$', header_text(), flags=re.M))
    assert found == {'SSRS_PASSAGE_MAX_PLANES': '8', 'SSRS_PASSAGE_MAX_RADIUS': '255'}
    assert _native.PASSAGE_MAX_PLANES == presence.MAX_PASSAGE_PLANES == 8
    assert _native.PASSAGE_MAX_RADIUS == presence.MAX_PASSAGE_RADIUS == 255
    assert not [n for n in vars(_native) if n.startswith('SSRS_PASSAGE')]


def test_the_first_header_keeps_its_79_exports():
    from ssrs_amd import _native
    names = abi.declared_functions()
    assert len(names) == 79 and sorted(_native.EXPORTS) == names
    assert not set(_native.PASSAGE_PROTOTYPES) & set(_native.PROTOTYPES)
    assert _native.lib().ssrs_version() == 109


# ------------------------------------------------------------------------------------------------ refusals
def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    assert lib.ssrs_track_passage_workspace_bytes(97, 131, 3) == -(-97 * 131 * 4 * 3 // 256) * 256
    assert lib.ssrs_track_passage_workspace_bytes(8, 8, 1) == 256
    for bad in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (-1, 8, 1)):
        assert lib.ssrs_track_passage_workspace_bytes(*bad) == 0
    buf = (C.c_char * 64)()
    good = dict(traj=buf, off=buf, ntracks=1, rows=2, cols=2, r2=4, planes=1, counts=buf, per_track=None, stats=None, ws=buf,
                nbytes=256)
    bad = [(b'NULL', dict(traj=None)), (b'NULL', dict(off=None)), (b'NULL', dict(counts=None)), (b'NULL', dict(ws=None)),
           (b'planes', dict(planes=0)), (b'planes', dict(planes=9)), (b'planes', dict(planes=-1)),
           (b'raster', dict(rows=0)), (b'raster', dict(rows=32768)), (b'raster', dict(cols=0)), (b'raster', dict(cols=32768)),
           (b'r2', dict(r2=-1)), (b'r2', dict(r2=255 * 255 + 1)), (b'r2', dict(r2=2 ** 40)),
           (b'ntracks', dict(ntracks=-1)), (b'ntracks', dict(ntracks=2 ** 31)),
           (b'4-byte aligned', dict(traj=C.c_void_p(C.addressof(buf) + 2))),
           (b'workspace', dict(nbytes=255)), (b'workspace', dict(rows=8, cols=8, planes=2, nbytes=256))]
    for text, kw in bad:
        a = dict(good, **kw)
        rc = lib.ssrs_track_passage(a['traj'], a['off'], a['ntracks'], a['rows'], a['cols'], a['r2'], a['planes'], a['counts'],
                                    a['per_track'], a['stats'], a['ws'], a['nbytes'], None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_track_passage' in lib.ssrs_last_error() and text in lib.ssrs_last_error(), kw
    assert bytes(buf) == bytes(64)
    # (no tracks: nothing to do, whatever the other arguments point at; the largest radius is accepted)
    assert lib.ssrs_track_passage(buf, buf, 0, 2, 2, 255 * 255, 8, buf, None, None, buf, 256, None) == _native.SSRS_OK


def test_argument_checks_need_no_device():
    good = [np.zeros((3, 2), dtype=np.int16)]
    for bad in ([np.zeros((3, 2), dtype=np.int32)], [np.zeros((3, 3), dtype=np.int16)], [np.zeros(6, dtype=np.int16)]):
        with pytest.raises(ValueError, match=r'expected int16 \(n, 2\)'):
            presence.compute_track_passage(bad, (4, 4), 1)
    for r2 in (-1, 255 * 255 + 1, 2.0, None, True):
        with pytest.raises(ValueError, match='r2'):
            presence.compute_track_passage(good, (4, 4), r2)
    for planes in (0, 9, -1):
        with pytest.raises(ValueError, match='planes'):
            presence.compute_track_passage(good, (4, 4), 1, planes=planes)
    pts = torch.zeros((3, 2), dtype=torch.int16)
    with pytest.raises(ValueError, match='needs offsets'):
        presence.compute_track_passage(pts, (4, 4), 1)
    with pytest.raises(ValueError, match=r'expected int16 \(points, 2\)'):
        presence.compute_track_passage(pts.to(torch.int32), (4, 4), 1, offsets=torch.tensor([0, 3]))
    with pytest.raises(ValueError, match='offsets must be int64'):
        presence.compute_track_passage(pts, (4, 4), 1, offsets=torch.tensor([0, 3], dtype=torch.int32))
    with pytest.raises(ValueError, match='offsets goes with a device tensor'):
        presence.compute_track_passage(good, (4, 4), 1, offsets=np.array([0, 3]))
    with pytest.raises(ValueError, match='stats must be'):
        presence.compute_track_passage(good, (4, 4), 1, stats=torch.zeros(2, dtype=torch.int64))      # (a host tensor)


# ------------------------------------------------------------------------------------------------ Config
def test_config_field_and_constructor_checks(tmp_path):
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    assert cfg.track_passage_radius == 0.
    assert 'track_passage_radius' in [f.name for f in fields(Config)]
    assert 'track_passage_radius' in dict(_SECTIONS)['MI355X build']
    assert 'track_passage_radius = 0.0' in str(cfg).split(':::: MI355X build')[1]
    assert 'track_passage_radius = 250.0' in str(Config(track_passage_radius=250.)).split(':::: MI355X build')[1]
    base = dict(run_name='t', out_dir=str(tmp_path), region_width_km=(8., 6.), resolution=100., track_count=10, sim_seed=1)
    # refused before any raster is computed (no GPU here)
    for radius in (-1., float('nan')):
        with pytest.raises(ValueError, match='track_passage_radius'):
            Simulator(Config(**base, track_passage_radius=radius), terrain='synthetic')
    with pytest.raises(ValueError, match='25600.0.*100.0'):                      # 256 cells
        Simulator(Config(**base, track_passage_radius=25600.), terrain='synthetic')


def test_passage_map_before_any_run_raises():
    sim = object.__new__(Simulator)
    sim.track_passage_counts = {}
    with pytest.raises(ValueError, match='track_passage_radius'):
        sim.compute_passage_map()
