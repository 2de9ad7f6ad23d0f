"""K21 on the host, without a GPU: include/ssrs_score.h against its binding, the library's argument refusals,
movmodel.rasterize_track, and tests/score_ref.py -- the definition on the oracle's functions -- on the reference's own
tracks (tests/golden/g7_tracks.npz) and on oracle tracks whose burn-in relocation really happens."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import ssrs_oracle as orc

import score_ref as ref
import test_native_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 'ssrs_score.h'


# ------------------------------------------------------------------------------------------------ the header
def score_prototypes():
    """{name: (restype, [argtypes])} of ssrs_score.h, by the parsing rules of test_native_abi.declared_prototypes."""
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


def test_score_prototype_matches_its_header():
    from ssrs_amd import _native
    lib = _native.lib()
    protos = score_prototypes()
    assert sorted(protos) == sorted(_native.SCORE_PROTOTYPES) == ['ssrs_tracks_score']
    restype, argtypes = protos['ssrs_tracks_score']
    fn = lib.ssrs_tracks_score
    assert list(fn.argtypes) == argtypes and fn.restype is restype
    assert _native.argtypes('ssrs_tracks_score') == argtypes == _native.SCORE_ARGTYPES
    assert len(argtypes) == 12 and argtypes[5] is C.c_int64 and all(a is C.c_void_p for k, a in enumerate(argtypes) if k != 5)
    text = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "ssrs_hip.h"' in text
    # the last parameter is the stream, by the name the stream contract looks for
    assert re.search(r'void \*stream\);', text)
    found = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SSRS_SCORE_[A-Z0-9_]+)[ \t]+(\d+)', text, flags=re.M))
    assert found == {'SSRS_SCORE_SCORED': '0', 'SSRS_SCORE_ZERO': '1', 'SSRS_SCORE_NOT_A_MOVE': '2', 'SSRS_SCORE_OUT': '3',
                     'SSRS_SCORE_UNDEFINED': '4', 'SSRS_SCORE_LAST': '5', 'SSRS_SCORE_MAX_MEMORY': '8', 'SSRS_SCORE_ROW': '6'}
    assert (_native.SCORE_SCORED, _native.SCORE_ZERO, _native.SCORE_NOT_A_MOVE, _native.SCORE_OUT, _native.SCORE_UNDEFINED,
            _native.SCORE_LAST) == (ref.SCORED, ref.ZERO, ref.NOT_A_MOVE, ref.OUT, ref.UNDEFINED, ref.LAST) == tuple(range(6))
    assert (_native.SCORE_MAX_MEMORY, _native.SCORE_ROW) == (8, 6)
    # a group of its own: the other headers and their mirrors are as they were
    others = set(_native.PROTOTYPES) | set(_native.PASSAGE_PROTOTYPES) | set(_native.TRANSIT_PROTOTYPES) | \
        set(_native.COLLISION_PROTOTYPES) | set(_native.SITE_PROTOTYPES)
    assert not set(_native.SCORE_PROTOTYPES) & others
    assert 'ssrs_tracks_score' not in _native.EXPORTS and len(abi.declared_functions()) == 79
    assert lib.ssrs_version() == 109
    # outside the glob of the stream contract's parse (tests/test_gpu_score.py pins the stream itself)
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

    names = ('params', 'updraft', 'potential', 'traj', 'off', 'ntracks', 'p', 'status', 'rows', 'smap', 'cmap')
    good = dict(dict.fromkeys(names, buf), params=params(), ntracks=1)
    nan = float('nan')
    bad = [(b'NULL', dict(params=None)), (b'NULL', dict(traj=None)), (b'NULL', dict(off=None)), (b'NULL', dict(rows=None)),
           (b'potential needs an updraft', dict(updraft=None)),
           (b'ntracks', dict(ntracks=-1)), (b'ntracks', dict(ntracks=2 ** 31)),
           (b'raster', dict(params=params(rows=2))), (b'raster', dict(params=params(cols=2))),
           (b'raster', dict(params=params(rows=32768))), (b'raster', dict(params=params(cols=-4))),
           (b'memory_parameter = 0 (the whole history)', dict(params=params(memory_parameter=0))),
           (b'memory_parameter = 9', dict(params=params(memory_parameter=9))),
           (b'memory_parameter = -1', dict(params=params(memory_parameter=-1))),
           (b'scaling_parameter', dict(params=params(scaling_parameter=-0.5))),
           (b'scaling_parameter', dict(params=params(scaling_parameter=nan))),
           (b'traj must be 4-byte aligned', dict(traj=odd(2))), (b'8-byte aligned', dict(p=odd(4))),
           (b'8-byte aligned', dict(rows=odd(4))), (b'8-byte aligned', dict(smap=odd(4))),
           (b'scored_map must be 4-byte aligned', dict(cmap=odd(2))),
           # the refusals come before the call that has nothing to do
           (b'NULL', dict(ntracks=0, rows=None)), (b'memory_parameter = 0', dict(ntracks=0, params=params(memory_parameter=0)))]
    for text, kw in bad:
        a = dict(good, **kw)
        rc = lib.ssrs_tracks_score(*(a[name] for name in names), None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_tracks_score' in lib.ssrs_last_error() and text in lib.ssrs_last_error(), (kw, lib.ssrs_last_error())
    assert bytes(buf) == bytes(64)
    # nothing to do, whatever the other arguments point at; every optional output may be NULL, both fields too
    for kw in (dict(ntracks=0), dict(ntracks=0, p=None, status=None, smap=None, cmap=None),
               dict(ntracks=0, updraft=None, potential=None), dict(ntracks=0, potential=None),
               dict(ntracks=0, params=params(scaling_parameter=0., memory_parameter=8, rows=3, cols=32767))):
        assert lib.ssrs_tracks_score(*(dict(good, **kw)[name] for name in names), None) == _native.SSRS_OK
    assert bytes(buf) == bytes(64)


def test_python_refusals_need_no_gpu():
    from ssrs_amd import movmodel
    with pytest.raises(ValueError, match=r'memory_parameter = 0 \(the whole history\) is not supported'):
        movmodel.score_tracks([np.zeros((2, 2), dtype=np.int16)], (24, 30), 0., memory_parameter=0)


# ------------------------------------------------------------------------------------------------ rasterize_track
def test_rasterize_track_gives_unit_moves_and_keeps_the_ends():
    from ssrs_amd import movmodel
    rng = np.random.default_rng(4)
    for n in (1, 2, 3, 40):
        r = np.cumsum(rng.normal(0., 3., n)) + 50.
        c = np.cumsum(rng.normal(0., 5., n)) + 60.
        cells = movmodel.rasterize_track(r, c)
        assert cells.dtype == np.int16 and cells.ndim == 2 and cells.shape[1] == 2
        assert tuple(cells[0]) == (int(np.rint(r[0])), int(np.rint(c[0])))
        assert tuple(cells[-1]) == (int(np.rint(r[-1])), int(np.rint(c[-1])))
        d = np.abs(np.diff(cells.astype(int), axis=0))
        assert (d.max(1) == 1).all() if len(d) else n == 1 or len(cells) == 1
        # every fix's cell is on the path, in order
        at = 0
        for fr, fc in zip(np.rint(r), np.rint(c)):
            hits = np.nonzero((cells[at:, 0] == fr) & (cells[at:, 1] == fc))[0]
            assert hits.size, (fr, fc)
            at += int(hits[0])
    # the formula by hand: (0, 0) -> (2, 5): N = 5, rows (2 i 2 + 5) // 10 = 0, 1, 1, 2, 2
    assert movmodel.rasterize_track([0., 2.], [0., 5.]).tolist() == [[0, 0], [0, 1], [1, 2], [1, 3], [2, 4], [2, 5]]
    assert movmodel.rasterize_track([0., -2.], [0., -5.]).tolist() == [[0, 0], [0, -1], [-1, -2], [-1, -3], [-2, -4], [-2, -5]]
    # repeated fixes in one cell are dropped; an empty track stays empty
    assert movmodel.rasterize_track([3.2, 2.9, 3.4, 3.6], [7., 7.1, 6.8, 7.]).tolist() == [[3, 7], [4, 7]]
    assert movmodel.rasterize_track([], []).shape == (0, 2)
    with pytest.raises(ValueError):
        movmodel.rasterize_track([0., np.nan], [0., 1.])
    with pytest.raises(ValueError):
        movmodel.rasterize_track([0., 40000.], [0., 1.])


# ------------------------------------------------------------------------------------------------ the reference's own tracks
G7_MOVES = {'ff_m1': 5837, 'ff_m3': 5515, 'ff_d135_m2': 3704, 'drw_m1': 5448, 'drw_d250_m3': 1528, 'ff_m1_nu05': 6127}
G7_SMALLEST_P = {'ff_m1': 0.007737588161701856, 'ff_m3': 0.034221178346260005, 'ff_d135_m2': 0.027359774240134423,
                 'drw_m1': 0.2928932188134524, 'drw_d250_m3': 0.13101013500492273}


@pytest.mark.parametrize('tag', ref.G7_TAGS)
def test_the_references_own_tracks_score_on_every_move(tag):
    """Every move the reference made has a positive probability under the definition: SCORED and nothing else, as many as
    sum(lengths - 1); the smallest p of the nu = 1 cases is the oracle's."""
    tracks, dirn, mem, nu, upd, pot = ref.g7_case(tag)
    res = ref.score(tracks, ref.G7_SHAPE, dirn, mem, nu, upd, pot)
    moves = sum(len(t) - 1 for t in tracks)
    assert moves == G7_MOVES[tag]
    counts = np.bincount(res['status'], minlength=6)
    assert counts[ref.SCORED] == moves and counts[ref.LAST] == len(tracks) == 64 and counts.sum() == moves + 64
    assert np.array_equal(res['rows'][:, 1], [len(t) - 1 for t in tracks]) and not res['rows'][:, 2:].any()
    if tag in G7_SMALLEST_P:
        assert res['p'][res['status'] == ref.SCORED].min() == G7_SMALLEST_P[tag]
    assert res['rows'][:, 0].sum() == res['surprisal_map'].sum() and res['scored_map'].sum() == moves
    # the burn-in relocation happened in these runs (starts on rows 0 and 1), or the first deltas would not be moves
    assert any(t[0][0] <= 1 for t in tracks)


@pytest.mark.parametrize('memory, nu, fluid', [(1, 1., True), (3, 1., True), (8, 1., False), (2, .5, True)])
def test_oracle_tracks_from_the_edges_score_on_every_move(memory, nu, fluid):
    """Oracle tracks on a 24 x 30 raster (burnin 2) started on row 0, row 1, column 0 and the far edges: the first three
    points are relocated before they move, and every move still scores."""
    shape = (24, 30)
    rng = np.random.default_rng(24 + memory)
    upd, pot = ref.fields(shape, rng) if fluid else (None, None)
    starts = [(0, 7), (1, 12), (9, 0), (23, 11), (22, 4), (12, 29), (5, 28), (0, 0), (23, 29), (1, 1)]
    tracks = ref.oracle_tracks(shape, 0., memory, nu, upd, pot, rng, starts=starts)
    relocated = 0
    for start, track in zip(starts, tracks):
        assert tuple(track[0]) == start and len(track) >= 2
        relocated += int(max(abs(int(track[1][0]) - start[0]), abs(int(track[1][1]) - start[1])) > 1)
        res = ref.score([track], shape, 0., memory, nu, upd, pot)
        assert (res['status'][:-1] == ref.SCORED).all() and res['status'][-1] == ref.LAST
        assert res['rows'][0, 1] == len(track) - 1
    assert all(orc.move_away_from_boundary(*s, *shape) != s for s in starts)
    assert relocated >= 3                                  # (a relocation by 2 and a move back by 1 looks like a unit move)


def test_reference_definition_by_hand():
    """drw, heading 0, memory 1 on a 24 x 30 raster: after a move north (+row) the mask leaves the three cells ahead, and
    the prior's lobe is cos(45 deg), 1, cos(45 deg): p = 1 / (1 + sqrt 2) ahead, sqrt(.5) / (1 + sqrt 2) diagonal."""
    prior = ref.prior_of(0.)
    assert prior[7] == 1. and prior[4] == 0. and abs(prior[6] - np.sqrt(.5)) < 1e-15
    track = np.array([(10, 10), (11, 10), (12, 10), (13, 11), (13, 11), (12, 11), (20, 20), (21, 20)], dtype=np.int16)
    p, st, base = ref.score_track(track, (24, 30), prior, 1, 1.)
    assert st.tolist() == [ref.SCORED, ref.SCORED, ref.SCORED, ref.ZERO, ref.ZERO, ref.NOT_A_MOVE, ref.SCORED, ref.LAST]
    assert abs(p[1] - 1. / (1. + np.sqrt(2.))) < 1e-15 and abs(p[2] - np.sqrt(.5) / (1. + np.sqrt(2.))) < 1e-15
    # the move after the jump is scored with a fresh memory: the same p as the track's first move north
    assert p[6] == p[0]
    assert ref.surprisal(0.5) == 2 ** 32 and ref.surprisal(1.) == 0 and ref.surprisal(2. ** -1074) == 1074 * 2 ** 32
    # nu = 0: every evaluated cell, a rest included, gets exactly 1 / 9
    p0, st0, _ = ref.score_track(track, (24, 30), prior, 1, 0.)
    assert (p0[[0, 1, 2, 3, 4, 6]] == 1. / 9.).all() and st0[3] == ref.SCORED and st0[5] == ref.NOT_A_MOVE
