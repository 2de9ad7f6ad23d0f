"""K22 on the host, without a GPU: include/ssrs_score_profile.h against its binding, the library's and the Python layer's
refusals, TrackProfile.total_bits and .best on hand-made rows, and the zoom rule of movmodel.fit_tracks against a stub
profile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_native_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 'ssrs_score_profile.h'
EXPORT = 'ssrs_tracks_score_profile'
SCALARS = dict(abi.SCALARS, int32_t=C.c_int32)


# ------------------------------------------------------------------------------------------------ the header
def test_profile_prototype_matches_its_header():
    from ssrs_amd import _native
    lib = _native.lib()
    protos = {}
    for ret, name, params in re.findall(abi.PROTOTYPE, abi.header_code(HEADER)):
        ret = ' '.join(ret.replace('*', ' * ').split())
        argtypes = []
        for param in [' '.join(p.split()) for p in params.split(',')]:
            if '*' in param:
                argtypes.append(C.c_void_p)
                continue
            ctype, _, pname = param.rpartition(' ')
            assert ctype in SCALARS and re.fullmatch(r'[A-Za-z_]\w*', pname), f'{name}: parameter {param!r}'
            argtypes.append(SCALARS[ctype])
        assert name not in protos, f'{name} declared twice'
        protos[name] = (abi.RETURNS[ret], argtypes)
    assert sorted(protos) == sorted(_native.PROFILE_PROTOTYPES) == [EXPORT]
    restype, argtypes = protos[EXPORT]
    fn = getattr(lib, EXPORT)
    assert list(fn.argtypes) == argtypes and fn.restype is restype is C.c_int
    assert _native.argtypes(EXPORT) == argtypes == _native.PROFILE_ARGTYPES
    assert len(argtypes) == 12 and [k for k, a in enumerate(argtypes) if a is not C.c_void_p] == [5, 7, 9]
    assert argtypes[5] is C.c_int64 and argtypes[7] is argtypes[9] is C.c_int32
    text = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert '#include "ssrs_hip.h"' in text
    # the last parameter is the stream, by the name the stream contract looks for
    assert re.search(r'void \*stream\);', text)
    found = dict(re.findall(r'^[ \t]*#[ \t]*define[ \t]+(SSRS_PROFILE_[A-Z0-9_]+)[ \t]+(\d+)', text, flags=re.M))
    assert found == {'SSRS_PROFILE_MAX_MEMORIES': '8', 'SSRS_PROFILE_MAX_NUS': '32'}
    assert (_native.PROFILE_MAX_MEMORIES, _native.PROFILE_MAX_NUS) == (8, 32)
    # a group of its own: the other headers and their mirrors are as they were
    others = set(_native.PROTOTYPES) | set(_native.PASSAGE_PROTOTYPES) | set(_native.TRANSIT_PROTOTYPES) | \
        set(_native.COLLISION_PROTOTYPES) | set(_native.SITE_PROTOTYPES) | set(_native.SCORE_PROTOTYPES)
    assert not set(_native.PROFILE_PROTOTYPES) & others
    assert EXPORT not in _native.EXPORTS and len(abi.declared_functions()) == 79
    assert lib.ssrs_version() == 109
    # outside the glob of the stream contract's parse (tests/test_gpu_score_profile.py pins the stream itself)
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

    def ints(*v):
        alive.append((C.c_int32 * len(v))(*v))
        return C.cast(alive[-1], C.c_void_p)

    def doubles(*v):
        alive.append((C.c_double * len(v))(*v))
        return C.cast(alive[-1], C.c_void_p)

    names = ('params', 'updraft', 'potential', 'traj', 'off', 'ntracks', 'memories', 'nmem', 'nus', 'nnu', 'rows')
    good = dict(dict.fromkeys(names, buf), params=params(), ntracks=1, memories=ints(1, 2, 3, 8), nmem=4,
                nus=doubles(0., 1., .5, 1.), nnu=4)
    nan = float('nan')
    nine = ints(*range(1, 10))
    many = doubles(*([1.] * 33))
    bad = [(b'NULL', dict(params=None)), (b'NULL', dict(traj=None)), (b'NULL', dict(off=None)), (b'NULL', dict(rows=None)),
           (b'NULL', dict(memories=None)), (b'NULL', dict(nus=None)),
           (b'potential needs an updraft', dict(updraft=None)),
           (b'ntracks', dict(ntracks=-1)), (b'ntracks', dict(ntracks=2 ** 31)),
           (b'raster', dict(params=params(rows=2))), (b'raster', dict(params=params(cols=32768))),
           (b'nmem = 0', dict(nmem=0)), (b'nmem = 9', dict(memories=nine, nmem=9)), (b'nmem = -1', dict(nmem=-1)),
           (b'memories[0] = 0', dict(memories=ints(0, 1), nmem=2)), (b'whole history', dict(memories=ints(0), nmem=1)),
           (b'memories[1] = 9', dict(memories=ints(8, 9), nmem=2)),
           (b'ascend strictly (memories[2] = 2 after 2)', dict(memories=ints(1, 2, 2), nmem=3)),
           (b'ascend strictly (memories[1] = 1 after 3)', dict(memories=ints(3, 1), nmem=2)),
           (b'nnu = 0', dict(nnu=0)), (b'nnu = 33', dict(nus=many, nnu=33)),
           (b'nus[1] = -0.5', dict(nus=doubles(1., -.5), nnu=2)), (b'nus[0] = nan', dict(nus=doubles(nan), nnu=1)),
           (b'burnin', dict(params=params(burnin=-1))),
           (b'traj must be 4-byte aligned', dict(traj=odd(2))), (b'rows must be 8-byte aligned', dict(rows=odd(4))),
           # the refusals come before the call that has nothing to do
           (b'NULL', dict(ntracks=0, rows=None)), (b'nnu = 0', dict(ntracks=0, nnu=0))]
    for text, kw in bad:
        a = dict(good, **kw)
        rc = getattr(lib, EXPORT)(*(a[name] for name in names), None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert EXPORT.encode() in lib.ssrs_last_error() and text in lib.ssrs_last_error(), (kw, lib.ssrs_last_error())
    assert bytes(buf) == bytes(64)
    # nothing to do, whatever the other arguments point at; both fields may be NULL; memory_parameter and
    # scaling_parameter are not read; the largest grid
    for kw in (dict(ntracks=0), dict(ntracks=0, updraft=None, potential=None), dict(ntracks=0, potential=None),
               dict(ntracks=0, params=params(scaling_parameter=nan, memory_parameter=0, rows=3, cols=32767)),
               dict(ntracks=0, memories=ints(*range(1, 9)), nmem=8, nus=doubles(*np.linspace(0., 4., 32)), nnu=32)):
        assert getattr(lib, EXPORT)(*(dict(good, **kw)[name] for name in names), None) == _native.SSRS_OK
    assert bytes(buf) == bytes(64)


def test_python_refusals_need_no_gpu():
    from ssrs_amd import movmodel
    tracks = [np.zeros((2, 2), dtype=np.int16)]
    for memories, nus, text in (((0, 1), (1.,), r'whole history'), ((1, 9), (1.,), r'outside \[1, 8\]'), ((), (1.,), 'empty'),
                                ((1,), (), r'0 nus'), ((1,), [1.] * 33, r'33 nus'), ((1,), (1., -1.), 'not negative'),
                                ((1,), (np.nan,), 'not NaN')):
        with pytest.raises(ValueError, match=text):
            movmodel.score_tracks_profile(tracks, (24, 30), 0., memories, nus)
        with pytest.raises(ValueError, match=text):
            movmodel.fit_tracks(tracks, (24, 30), 0., memories=memories, nus=nus)
    with pytest.raises(ValueError, match='rounds = 0'):
        movmodel.fit_tracks(tracks, (24, 30), 0., rounds=0)
    mem, nu = movmodel._profile_grid((3, 1, 3, 2), (2., 0., 2.))
    assert mem.tolist() == [1, 2, 3] and mem.dtype == np.int32 and nu.tolist() == [2., 0., 2.]


# ------------------------------------------------------------------------------------------------ total_bits and best
def rows_of(S, zero, undefined=None):
    """Rows (1, nmem, nnu, 6) with the given S (units of 2^-32 bit), zero and undefined counts."""
    S = np.asarray(S, dtype=np.int64)
    rows = np.zeros((1,) + S.shape + (6,), dtype=np.int64)
    rows[0, ..., 0], rows[0, ..., 2] = S, zero
    rows[0, ..., 5] = 0 if undefined is None else undefined
    rows[0, ..., 1] = 10
    return rows


def test_total_bits_and_best_on_hand_made_rows():
    from ssrs_amd import movmodel
    one = 2 ** 32
    # two tracks add; nus out of order; memory 2 forbids one move at nu = 1 (zero) and one at nu = .5 (undefined)
    rows = np.concatenate([rows_of([[5 * one, 3 * one, 4 * one], [one, 2 * one, one // 2]], [[0, 0, 0], [1, 0, 0]],
                                   [[0, 0, 0], [0, 0, 1]]),
                           rows_of([[one, one, one], [0, 0, 0]], 0)])
    prof = movmodel.TrackProfile(rows, (1, 2), (1., 2., .5))
    assert prof.host_rows() is prof.host_rows() and prof.host_rows().shape == (2, 2, 3, 6)
    assert np.array_equal(prof.total_bits(), [[6., 4., 5.], [np.inf, 2., np.inf]])          # 0 * inf is 0
    assert np.array_equal(prof.total_bits(zero_bits=20.), [[6., 4., 5.], [21., 2., 20.5]])
    assert np.array_equal(prof.total_bits(zero_bits=0.), [[6., 4., 5.], [1., 2., .5]])
    assert prof.best() == (2, 2., 2.) and prof.best(zero_bits=0.) == (2, .5, .5)
    assert np.array_equal(prof.row(2, .5), rows[:, 1, 2]) and np.array_equal(prof.forbidden(), [[0, 0, 0], [1, 0, 1]])
    with pytest.raises(ValueError, match='nu 3'):
        prof.row(1, 3.)
    with pytest.raises(ValueError, match='memory 4'):
        prof.row(4, 1.)
    # ties: ascending memory first, then ascending nu, whatever the order the nus came in
    tie = movmodel.TrackProfile(rows_of([[7 * one, 2 * one, 2 * one], [2 * one, 2 * one, 9 * one]], 0), (1, 3), (4., 2., 1.))
    assert tie.best() == (1, 1., 2.)
    tie = movmodel.TrackProfile(rows_of([[7 * one, 7 * one, 7 * one], [2 * one, 2 * one, 9 * one]], 0), (1, 3), (4., 2., 1.))
    assert tie.best() == (3, 2., 2.)
    assert movmodel.TrackProfile(rows_of([[one, one]], 0), (2,), (1., 1.)).row(2, 1.)[0, 0] == one
    # every combination forbids a move: the error names the fewest and where
    shut = movmodel.TrackProfile(rows_of([[one, one], [one, one]], [[4, 3], [2, 1]], [[0, 0], [0, 1]]), (1, 2), (1., .5))
    with pytest.raises(ValueError, match=r'the fewest, 2, under memory 2 and nu 0\.5 '):
        shut.best()                                        # (ascending nu: 0.5 comes first; 1 zero + 1 undefined = 2 = the other)
    assert shut.best(zero_bits=1.) == (2, .5, 3.)
    with pytest.raises(ValueError, match='rows of shape'):
        movmodel.TrackProfile(rows, (1, 2, 3), (1., 2., .5))


# ------------------------------------------------------------------------------------------------ the zoom
def test_fit_zooms_between_the_neighbours_of_the_best_nu(monkeypatch):
    """score_tracks_profile replaced by a stub whose total is (nu - target)^2 bits for memory 2 and more for the others:
    the grids of the rounds, the closing profile, the bracket, at_edge, and the bound at an end of the grid."""
    from ssrs_amd import movmodel
    seen = []

    def stub(target):
        def profile(tracks, grid_shape, move_dirn, memories, nus, updraft_field=None, potential_field=None, *, offsets=None):
            mem, nu = movmodel._profile_grid(memories, nus)
            seen.append((mem.tolist(), nu.copy()))
            S = np.rint(((nu[None, :] - target) ** 2 + (mem[:, None] != 2)) * 2. ** 32).astype(np.int64)
            return movmodel.TrackProfile(rows_of(S, 0), mem.tolist(), nu)
        return profile

    monkeypatch.setattr(movmodel, 'score_tracks_profile', stub(1.3))
    fit = movmodel.fit_tracks(None, (24, 30), 0., memories=(3, 1, 2), nus=np.linspace(0., 2., 9))
    assert [m for m, _ in seen] == [[1, 2, 3]] * 4 and len(fit.profiles) == 3           # three rounds and the closing profile
    assert np.array_equal(seen[0][1], np.linspace(0., 2., 9)) and np.array_equal(seen[1][1], np.linspace(1., 1.5, 9))
    assert np.array_equal(seen[2][1], np.linspace(1.25, 1.375, 9))                         # 1.3125 is round 2's best
    assert (fit.memory, fit.nu) == (2, 1.296875) and not fit.at_edge
    # the closing profile at the midpoints beside nu: neither is lower, the minimum lies between them, one spacing wide
    assert seen[3][1].tolist() == [1.2890625, 1.3046875] and fit.closing.nus.tolist() == seen[3][1].tolist()
    assert (fit.nu_lo, fit.nu_hi) == (1.2890625, 1.3046875) and fit.nu_hi - fit.nu_lo == (2 / 8) * 2 / 8 * 2 / 8
    assert fit.bits == fit.profiles[-1].total_bits()[1, 3] and abs(fit.bits - (1.296875 - 1.3) ** 2) < 2. ** -32
    # the default grid and one round; a grid that comes unsorted is bracketed on its sorted values
    del seen[:]
    fit = movmodel.fit_tracks(None, (24, 30), 0., rounds=1)
    assert np.array_equal(seen[0][1], np.linspace(0., 4., 17)) and seen[0][0] == [1, 2, 3, 4] and len(seen) == 2
    assert (fit.nu, fit.nu_lo, fit.nu_hi) == (1.25, 1.125, 1.375)
    fit = movmodel.fit_tracks(None, (24, 30), 0., nus=(2., 0., 1.5, 1.), rounds=2)
    assert (fit.profiles[0].best()[1], seen[-2][1].tolist()) == (1.5, np.linspace(1., 2., 4).tolist())
    # a midpoint lower than the best grid nu moves the bracket to its side; nu and bits stay the grid's
    for target, bracket in ((1.15, (1., 1.25)), (1.36, (1.25, 1.5))):
        monkeypatch.setattr(movmodel, 'score_tracks_profile', stub(target))
        fit = movmodel.fit_tracks(None, (24, 30), 0., nus=np.linspace(0., 2., 9), rounds=1)
        assert (fit.nu, fit.nu_lo, fit.nu_hi) == (1.25,) + bracket and fit.nu_lo <= target <= fit.nu_hi
        assert fit.bits == fit.profiles[0].best()[2]
    # the best nu at the grid's largest: it is itself the bound, the zoom is one-sided and says so
    monkeypatch.setattr(movmodel, 'score_tracks_profile', stub(5.))
    del seen[:]
    fit = movmodel.fit_tracks(None, (24, 30), 0., nus=np.linspace(0., 2., 9), rounds=2)
    assert fit.at_edge and np.array_equal(seen[1][1], np.linspace(1.75, 2., 9)) and (fit.nu, fit.nu_lo, fit.nu_hi) == (2., 1.984375, 2.)
    # ... and at the smallest, which is no edge in that sense
    monkeypatch.setattr(movmodel, 'score_tracks_profile', stub(-1.))
    fit = movmodel.fit_tracks(None, (24, 30), 0., nus=np.linspace(0., 2., 9), rounds=2)
    assert not fit.at_edge and (fit.nu, fit.nu_lo, fit.nu_hi) == (0., 0., .015625)
    # a grid of one nu has no neighbours and no closing profile
    fit = movmodel.fit_tracks(None, (24, 30), 0., nus=(1.,), rounds=2)
    assert (fit.nu, fit.nu_lo, fit.nu_hi, fit.closing) == (1., 1., 1., None)
