"""K22 without a GPU: ssrs_amd/csrc/score_profile.hip compiled with g++ against tests/hip_host_stub under
-ffp-contract=off and run on the CPU, as test_score_emulation.py does for K21 (whose stub additions, placement and
parameter helpers it borrows).  The kernel's own code runs here as it stands -- the stage, the searches, the one walk back
with its masks per memory, the reuse of the nu-free half, the per-nu half, the grouped segmented scan and the 64-bit adds
-- and is held to score_ref.score looped over the grid (score_profile_ref.expected) on every case of score_ref.cases().
What it does not cover: the device's own arithmetic, blocks that run at the same time, and speed."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import score_profile_ref as pref
import score_ref as ref
from test_score_emulation import ERR_CPP, EXTRA_H, ROOT, params_of, place, ptr


def build(work):
    """The CPU build of score_profile.hip in `work`, bound by the library's own prototype."""
    from ssrs_amd import _native
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'score_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'libscore_profile_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include',
                    str(work / 'score_emu_extra.h'), '-x', 'c++', os.path.join(csrc, 'score_profile.hip'),
                    str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_blocks.restype = C.c_longlong
    L.ssrs_tracks_score_profile.argtypes = _native.PROFILE_ARGTYPES
    return L


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    return build(tmp_path_factory.mktemp('score_profile_emu'))


def call(L, c, memories, nus, tracks=None, shift=None, lead=None, fill=0xDEAD):
    """One call on case c (its own tracks, or `tracks`) into `rows` filled with `fill` -> int64 (ntracks, nmem, nnu, 6)."""
    traj, offsets = ref.flat(c['tracks'] if tracks is None else tracks, c['lead'] if lead is None else lead)
    ntracks = offsets.size - 1
    owner, traj_v = place(traj, c['shift'] if shift is None else shift)
    rows = np.full((ntracks, len(memories), len(nus), 6), fill, dtype=np.uint64)
    upd = None if c['updraft'] is None else np.ascontiguousarray(c['updraft'], dtype=np.float64)
    pot = None if c['potential'] is None else np.ascontiguousarray(c['potential'], dtype=np.float32)
    prm = params_of(c)
    prm.memory_parameter, prm.scaling_parameter = -3, float('nan')      # ignored
    mem = np.asarray(memories, dtype=np.int32)
    nu = np.asarray(nus, dtype=np.float64)
    before = owner.copy()
    rc = L.ssrs_tracks_score_profile(C.cast(C.byref(prm), C.c_void_p), ptr(upd), ptr(pot), ptr(traj_v), ptr(offsets), ntracks,
                                     ptr(mem), len(memories), ptr(nu), len(nus), ptr(rows), None)
    assert rc == 0, L.ssrs_last_error()
    assert np.array_equal(owner, before)
    return rows.view(np.int64)


@pytest.mark.parametrize('name', ref.case_names())
def test_emulated_case_on_every_grid(emu, name):
    """Every case under every grid, into dirty rows."""
    c = ref.case(name)
    for memories, nus in pref.GRIDS:
        pref.check(call(emu, c, memories, nus), pref.expected(c, memories, nus))


def test_grids_cover_what_they_are_for():
    """The memories differ where they should (a longer memory forbids more), every evaluated status occurs, and a combination
    equals K21's own expectation at the case's parameters."""
    c = ref.case('g7_m8')
    want = pref.expected(c, (1, 2, 3, 8), (0., 1., .5, 2., 1.))
    zero = want[..., 2].sum(0)
    # nu = 1: the masks are running ANDs, so never fewer with a longer memory, and more in the end; nu = 0: none
    assert (np.diff(zero[:, 1]) >= 0).all() and zero[3, 1] > zero[0, 1] and not zero[:, 0].any()
    assert np.array_equal(want[:, :, 1], want[:, :, 4]) and np.array_equal(want[:, 3, 1], ref.expected(c)['rows'])
    assert (want[:, :, 2, 0] != want[:, :, 3, 0]).any()
    assert pref.expected(ref.case('huge_potential'), (1, 2), (1.,))[..., 5].sum() > 0
    assert (want[..., 3].sum() > 0) and (want[..., 4].sum() > 0)


@pytest.mark.parametrize('name', ['7x9_m8_nu1', '12x40_upd_m3', 'g7_m8'])
def test_emulated_every_placement(emu, name):
    """traj at 0, 4, 8 and 12 bytes past a 16-byte boundary, every first offset modulo 4, rows dirty in two ways."""
    c = ref.case(name)
    memories, nus = pref.GRIDS[0]
    want = pref.expected(c, memories, nus)
    for shift in range(4):
        for lead in ((0, 1, 2, 3, 6) if shift == 0 else (c['lead'],)):
            pref.check(call(emu, c, memories, nus, shift=shift, lead=lead, fill=2 ** 64 - 1 if shift % 2 else 0xDEAD), want)


def test_emulated_independence(emu):
    """One call, two calls over two halves, a permuted order, a second run: the same integers (the same log2 on every path
    here); the order of the nus permutes the columns."""
    c = ref.case('g7_m8')
    tracks = c['tracks']
    n = len(tracks)
    memories, nus = (1, 3, 8), (.5, 1., 2.)
    whole = call(emu, c, memories, nus)
    halves = [call(emu, c, memories, nus, tracks=tracks[:n // 2]), call(emu, c, memories, nus, tracks=tracks[n // 2:], lead=2)]
    assert np.array_equal(np.concatenate(halves), whole)
    order = np.random.default_rng(3).permutation(n)
    assert np.array_equal(call(emu, c, memories, nus, tracks=[tracks[k] for k in order], shift=1), whole[order])
    assert np.array_equal(call(emu, c, memories, nus), whole)
    assert np.array_equal(call(emu, c, memories, (2., .5, 1., 2.)), whole[:, :, [2, 0, 1, 2]])
    assert np.array_equal(call(emu, c, (3,), (1.,)), whole[:, 1:2, 1:2])


def test_emulated_blocks_and_long_tracks(emu):
    """A track of 2000 points crosses eight blocks: its rows are the sums of eight segments; 40 tracks of 13 points put
    twenty segments into one block.  Five combinations: a full group of four and a group of one."""
    rng = np.random.default_rng(8)
    c = ref.case('g7_m1')
    tracks = [ref.forward(2000, ref.G7_SHAPE, rng)] + [ref.forward(13, ref.G7_SHAPE, rng) for _ in range(40)] + \
        [np.zeros((0, 2), dtype=np.int16)] * 3 + [ref.forward(600, ref.G7_SHAPE, rng)]
    memories, nus = (1, 2, 3, 4, 8), (1.,)
    want = pref.expected(c, memories, nus, tracks)
    before = emu.emu_blocks()
    pref.check(call(emu, c, memories, nus, tracks=tracks, lead=1, shift=2), want)
    assert emu.emu_blocks() - before >= 12 and (want[0, :, 0, 1:3].sum(1) == 1999).all() and want[0, 0, 0, 1] > 256


def test_emulated_nothing_to_do_touches_nothing(emu):
    c = ref.case('7x9_m1_nu1')
    traj, _ = ref.flat(c['tracks'], 2)
    rows = np.full((4, 2, 2, 6), 9, dtype=np.uint64)
    prm = params_of(c)
    mem, nu = np.array([1, 2], dtype=np.int32), np.array([1., .5])
    before = emu.emu_launches()
    for off, n in ((np.array([5], dtype=np.int64), 0), (np.array([5, 5, 5, 5], dtype=np.int64), 3)):
        rc = emu.ssrs_tracks_score_profile(C.cast(C.byref(prm), C.c_void_p), None, None, ptr(traj), ptr(off), n, ptr(mem), 2,
                                           ptr(nu), 2, ptr(rows), None)
        assert rc == 0
    assert emu.emu_launches() == before and (rows == 9).all()
