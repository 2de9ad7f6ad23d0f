"""K23 on the host, without a GPU: include/ssrs_bridge.h against its binding, the library's argument refusals, and
movmodel.fix_gaps / thin_track / score_gaps' own refusals on planted sequences."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bridge_ref as ref
import test_native_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 'ssrs_bridge.h'


def bridge_prototypes():
    """{name: (restype, [argtypes])} of ssrs_bridge.h, by the parsing rules of test_native_abi.declared_prototypes."""
    protos = {}
    for ret, name, params in re.findall(abi.PROTOTYPE, abi.header_code(HEADER)):
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


def test_bridge_prototype_matches_its_header():
    from ssrs_amd import _native
    lib = _native.lib()
    protos = bridge_prototypes()
    assert sorted(protos) == sorted(_native.BRIDGE_PROTOTYPES) == ['ssrs_tracks_bridge']
    restype, argtypes = protos['ssrs_tracks_bridge']
    fn = lib.ssrs_tracks_bridge
    assert list(fn.argtypes) == argtypes and fn.restype is restype
    assert _native.argtypes('ssrs_tracks_bridge') == argtypes == _native.BRIDGE_ARGTYPES
    assert len(argtypes) == 10 and argtypes[4] is C.c_int64 and all(a is C.c_void_p for k, a in enumerate(argtypes) if k != 4)
    text = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "ssrs_hip.h"' in text
    # the last parameter is the stream, by the name the stream contract looks for
    assert re.search(r'void \*stream\);', text)
    found = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SSRS_BRIDGE_[A-Z0-9_]+)[ \t]+(\d+)', text, flags=re.M))
    assert found == {'SSRS_BRIDGE_SCORED': '0', 'SSRS_BRIDGE_ZERO': '1', 'SSRS_BRIDGE_TOO_LONG': '2', 'SSRS_BRIDGE_OUT': '3',
                     'SSRS_BRIDGE_UNDEFINED': '4', 'SSRS_BRIDGE_MAX_MOVES': '32', 'SSRS_BRIDGE_JOB': '6'}
    assert (_native.BRIDGE_SCORED, _native.BRIDGE_ZERO, _native.BRIDGE_TOO_LONG, _native.BRIDGE_OUT, _native.BRIDGE_UNDEFINED) == \
        (ref.SCORED, ref.ZERO, ref.TOO_LONG, ref.OUT, ref.UNDEFINED) == tuple(range(5))
    assert (_native.BRIDGE_MAX_MOVES, _native.BRIDGE_JOB) == (ref.MAX_MOVES, 6) == (32, 6)
    # the gap statuses that K21 has too carry K21's numbers, so that one table reads both
    assert (_native.BRIDGE_SCORED, _native.BRIDGE_ZERO, _native.BRIDGE_OUT, _native.BRIDGE_UNDEFINED) == \
        (_native.SCORE_SCORED, _native.SCORE_ZERO, _native.SCORE_OUT, _native.SCORE_UNDEFINED)
    # a group of its own: disjoint from every other group, which are as they were
    groups = {name: getattr(_native, name) for name in dir(_native) if name.endswith('PROTOTYPES')}
    assert len(groups) == 8 and 'BRIDGE_PROTOTYPES' in groups
    for name, group in groups.items():
        if name != 'BRIDGE_PROTOTYPES':
            assert not set(group) & set(_native.BRIDGE_PROTOTYPES), name
    assert 'ssrs_tracks_bridge' not in _native.EXPORTS and len(abi.declared_functions()) == 79
    assert lib.ssrs_version() == 109
    # outside the glob of the stream contract's parse (tests/test_gpu_bridge.py pins the stream itself)
    assert not HEADER.startswith('ssrs_hip')


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    buf = (C.c_char * 64)()
    assert C.addressof(buf) % 8 == 0
    odd = lambda n: C.c_void_p(C.addressof(buf) + n)
    prm = _native.SsrsTrackParams()
    assert lib.ssrs_track_params_init(C.byref(prm), 24, 30, 1, 1.0) == 0

    alive = []

    def params(**kw):
        q = _native.SsrsTrackParams()
        alive.append(q)
        C.memmove(C.byref(q), C.byref(prm), C.sizeof(prm))
        for k, v in kw.items():
            setattr(q, k, v)
        return C.cast(C.pointer(q), C.c_void_p)

    names = ('params', 'updraft', 'potential', 'jobs', 'ngaps', 'g', 'status', 'surprisal', 'arrivals')
    good = dict(dict.fromkeys(names, buf), params=params(), ngaps=1)
    nan = float('nan')
    bad = [(b'NULL', dict(params=None)), (b'NULL', dict(jobs=None)), (b'NULL', dict(g=None)), (b'NULL', dict(status=None)),
           (b'NULL', dict(surprisal=None)),
           (b'potential needs an updraft', dict(updraft=None)),
           (b'ngaps', dict(ngaps=-1)), (b'ngaps', dict(ngaps=2 ** 31)),
           (b'raster', dict(params=params(rows=2))), (b'raster', dict(params=params(cols=2))),
           (b'raster', dict(params=params(rows=32768))), (b'raster', dict(params=params(cols=-4))),
           (b'memory_parameter = 0 is not supported', dict(params=params(memory_parameter=0))),
           (b'memory_parameter = 2 is not supported', dict(params=params(memory_parameter=2))),
           (b'memory_parameter = -1', dict(params=params(memory_parameter=-1))),
           (b'scaling_parameter', dict(params=params(scaling_parameter=-0.5))),
           (b'scaling_parameter', dict(params=params(scaling_parameter=nan))),
           (b'jobs must be 4-byte aligned', dict(jobs=odd(2))), (b'8-byte aligned', dict(g=odd(4))),
           (b'8-byte aligned', dict(surprisal=odd(4))), (b'8-byte aligned', dict(arrivals=odd(4))),
           # the refusals come before the call that has nothing to do
           (b'NULL', dict(ngaps=0, g=None)), (b'memory_parameter = 3', dict(ngaps=0, params=params(memory_parameter=3)))]
    for text, kw in bad:
        a = dict(good, **kw)
        rc = lib.ssrs_tracks_bridge(*(a[name] for name in names), None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_tracks_bridge' in lib.ssrs_last_error() and text in lib.ssrs_last_error(), (kw, lib.ssrs_last_error())
    assert bytes(buf) == bytes(64)
    # nothing to do, whatever the other arguments point at; arrivals may be NULL, both fields too
    for kw in (dict(ngaps=0), dict(ngaps=0, arrivals=None), dict(ngaps=0, updraft=None, potential=None),
               dict(ngaps=0, potential=None), dict(ngaps=0, params=params(scaling_parameter=0., rows=3, cols=32767))):
        assert lib.ssrs_tracks_bridge(*(dict(good, **kw)[name] for name in names), None) == _native.SSRS_OK
    assert bytes(buf) == bytes(64)


def test_python_refusals_need_no_gpu():
    from ssrs_amd import movmodel
    jobs = np.array([[3, 3, 4, 4, 4, 2]], dtype=np.int32)
    with pytest.raises(ValueError, match=r'jobs of shape \(1, 5\)'):
        movmodel.score_gaps(jobs[:, :5], (24, 30), 0.)
    with pytest.raises(ValueError, match=r'jobs of shape \(6,\)'):
        movmodel.score_gaps(jobs[0], (24, 30), 0.)
    with pytest.raises(ValueError, match='integer array'):
        movmodel.score_gaps(jobs.astype(np.float64), (24, 30), 0.)
    with pytest.raises(ValueError, match='does not fit int32'):
        movmodel.score_gaps(jobs.astype(np.int64) * 2 ** 31, (24, 30), 0.)
    with pytest.raises(ValueError, match='scaling_parameter = -1'):
        movmodel.score_gaps(jobs, (24, 30), 0., -1.)
    with pytest.raises(ValueError, match='scaling_parameter = nan'):
        movmodel.score_gaps(jobs, (24, 30), 0., float('nan'))
    with pytest.raises(ValueError, match='integer cells'):
        movmodel.fix_gaps(np.array([[1.5, 2.], [3., 4.]]))
    with pytest.raises(ValueError, match='3 moves for 2 pairs'):
        movmodel.fix_gaps([(1, 1), (2, 2), (3, 3)], [1, 1, 1])
    with pytest.raises(ValueError, match='does not fit int32'):
        movmodel.fix_gaps([(1, 1), (2 ** 40, 2)])
    with pytest.raises(ValueError, match='every = 0'):
        movmodel.thin_track([(1, 1), (2, 2)], 0)


def test_fix_gaps_on_planted_sequences():
    from ssrs_amd import movmodel
    # unit pairs, a repeated cell, a long pair, a jump: incoming after a unit move and after a gap
    fixes = [(5, 5), (6, 5), (6, 6), (6, 6), (7, 7), (9, 12), (10, 12), (50, 12), (50, 13)]
    jobs, pair = movmodel.fix_gaps(fixes)
    assert jobs.dtype == np.int32 and pair.dtype == np.int64
    assert jobs.tolist() == [[5, 5, 4, 6, 5, 1],          # the first pair: no last move
                             [6, 5, 7, 6, 6, 1],          # after the unit move (1, 0): state 7
                             [6, 6, 4, 7, 7, 1],          # after the repeated cell, which is left out: 4
                             [7, 7, 8, 9, 12, 5],         # after the unit move (1, 1): 8; 5 moves, the Chebyshev distance
                             [9, 12, 4, 10, 12, 1],       # after a gap: 4
                             [10, 12, 7, 50, 12, 40],     # longer than 32: kept, to come back TOO_LONG
                             [50, 12, 4, 50, 13, 1]]
    assert pair.tolist() == [0, 1, 3, 4, 5, 6, 7]
    # with moves: the repeated cell is kept with its number; a single move between cells that are further apart, or a unit
    # pair flown in more than one move, is no unit move
    moves = [1, 1, 3, 2, 5, 1, 40, 1]
    jobs, pair = movmodel.fix_gaps(np.array(fixes, dtype=np.int16), moves)
    assert pair.tolist() == list(range(8)) and jobs[:, 5].tolist() == moves
    assert jobs[:, 2].tolist() == [4, 7, 5, 4, 4, 4, 7, 4]
    assert jobs[:, [0, 1]].tolist() == [list(f) for f in fixes[:-1]] and jobs[:, [3, 4]].tolist() == [list(f) for f in fixes[1:]]
    jobs, _ = movmodel.fix_gaps(fixes[:3], [1, 0])
    assert jobs.tolist() == [[5, 5, 4, 6, 5, 1], [6, 5, 7, 6, 6, 0]]
    # (a single move that cannot join its cells is kept, and arrives nowhere: ZERO)
    assert movmodel.fix_gaps([(5, 5), (8, 5), (9, 5)], [1, 1])[0].tolist() == [[5, 5, 4, 8, 5, 1], [8, 5, 4, 9, 5, 1]]
    # every unit move gives its own state
    for k in range(9):
        d = ref.DELTAS[k]
        got = movmodel.fix_gaps([(5, 5), (5 + d[0], 5 + d[1]), (9, 9)], [1, 4])[0]
        assert got[1, 2] == k and got[0, 2] == 4
    # nothing to pair
    for empty in ([], [(3, 3)], np.zeros((0, 2), dtype=np.int64), [(3, 3), (3, 3)]):
        jobs, pair = movmodel.fix_gaps(empty)
        assert jobs.shape == (0, 6) and jobs.dtype == np.int32 and pair.shape == (0,)
    assert 'lower bound' in movmodel.fix_gaps.__doc__ and 'not an estimate' in movmodel.fix_gaps.__doc__


def test_thin_track_keeps_every_nth_point_and_the_last():
    from ssrs_amd import movmodel
    track = np.array([(r, 2 * r) for r in range(11)], dtype=np.int16)
    for every, idx in ((1, list(range(11))), (2, [0, 2, 4, 6, 8, 10]), (4, [0, 4, 8, 10]), (5, [0, 5, 10]), (16, [0, 10]),
                       (10, [0, 10])):
        fixes, moves = movmodel.thin_track(track, every)
        assert fixes.tolist() == track[idx].tolist() and moves.tolist() == np.diff(idx).tolist() and moves.sum() == 10
    fixes, moves = movmodel.thin_track(track[:1], 3)
    assert fixes.tolist() == [[0, 0]] and moves.shape == (0,)
    fixes, moves = movmodel.thin_track(track[:0], 3)
    assert fixes.shape == (0, 2) and moves.shape == (0,)
    # the reference's own tracks, thinned: fix_gaps gives the jobs bridge_ref builds from the full track with incoming 4,
    # except after a unit pair
    tracks = ref.sref.g7_case('ff_m1')[0]
    for track in tracks[:4]:
        cut = track[10:]
        for every in (2, 5, 16, 32):
            jobs, pair = movmodel.fix_gaps(*movmodel.thin_track(cut, every))
            want = np.array(ref.thinned(cut, every, 0, False)).reshape(-1, 6)
            assert np.array_equal(jobs[:, [0, 1, 3, 4, 5]], want[:, [0, 1, 3, 4, 5]]) and pair.tolist() == list(range(len(want)))
            after_unit = np.r_[False, want[:-1, 5] == 1]
            assert (jobs[~after_unit, 2] == 4).all()


def test_simulator_refuses_without_a_gpu():
    """score_fixes names the run's track_dirn_restrict before it touches a field."""
    from ssrs_amd import simulator

    class Run:
        track_dirn_restrict = 3
    with pytest.raises(ValueError, match=r'score_fixes: track_dirn_restrict = 3 is not supported'):
        simulator.Simulator.score_fixes(Run(), [np.zeros((2, 2), dtype=np.int64)])
