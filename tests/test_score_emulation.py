"""K21 without a GPU: ssrs_amd/csrc/score.hip compiled with g++ against tests/hip_host_stub under -ffp-contract=off and run
on the CPU, as test_site_emulation.py does for K20.  The kernel cooperates through __shared__ and __syncthreads() only, so
its own code runs here as it stands: the stage and its 16-byte and point-by-point loads, the two binary searches, the
look-back, the restated weights, masks and probability sequence, the segmented scan and the 64-bit adds -- on the cases of
tests/score_ref.py, which tests/test_gpu_score.py runs on the device.  What it does not cover: the device's own arithmetic
(the f64 operations, log2 and pow are the host's here), blocks that run at the same time, and speed."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ERR_CPP = '''#include "common.h"
namespace ssrs {
char *error_buffer() { static thread_local char buf[512] = ""; return buf; }
int set_error(int code, const char *fmt, ...)
{ va_list ap; va_start(ap, fmt); vsnprintf(error_buffer(), 512, fmt, ap); va_end(ap); return code; }
}
extern "C" const char *ssrs_last_error(void) { return ssrs::error_buffer(); }
extern "C" long long emu_launches(void) { return emu_launch_count; }
extern "C" long long emu_blocks(void) { return emu_block_count; }
'''
# what the kernel uses beyond the stub: the vector type, the atomics (the threads of a block are OS threads), the copies and
# the memset; launches and blocks are counted
EXTRA_H = '''#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
struct alignas(16) uint4 { uint32_t x, y, z, w; };
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
constexpr int hipMemcpyDeviceToHost = 2;
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline long long emu_launch_count = 0, emu_block_count = 0;
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \\
    (++emu_launch_count, emu_block_count += dim3(grid).x, emu_launch(grid, block, [&] { kernel(__VA_ARGS__); }))
'''


def build(work):
    """The CPU build of score.hip in `work`, bound by the library's own prototype."""
    from ssrs_amd import _native
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'score_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'libscore_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include',
                    str(work / 'score_emu_extra.h'), '-x', 'c++', os.path.join(csrc, 'score.hip'),
                    str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_blocks.restype = C.c_longlong
    L.ssrs_tracks_score.argtypes = _native.SCORE_ARGTYPES
    return L


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    return build(tmp_path_factory.mktemp('score_emu'))


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def place(values, shift):
    """`values` (4 bytes a row) copied to an address `shift` rows past a 16-byte boundary.  Returns (owner, view)."""
    raw = np.zeros((values.shape[0] + 12,) + values.shape[1:], dtype=values.dtype)
    start = (-raw.ctypes.data % 16) // 4 + 4 + shift
    view = raw[start:start + values.shape[0]]
    view[:] = values
    assert (view.ctypes.data % 16) == 4 * (shift % 4)
    return raw, view


def params_of(c):
    from ssrs_amd import movmodel
    p = movmodel.make_track_params(c['shape'], c['move_dirn'], c['memory'], c['nu'])
    assert [p.prior[k] for k in range(9)] == ref.prior_of(c['move_dirn'])
    assert p.burnin == int(min(c['shape']) / 10)
    return p


def call(L, c, tracks=None, offsets=None, traj=None, shift=None, lead=None, want_p=True, want_status=True, maps=None,
         want_maps=True):
    """One call on case c (its own tracks, or `tracks`; or a ready traj with offsets).  Returns a dict like score_ref.score's,
    the uint64 results as int64."""
    if traj is None:
        traj, offsets = ref.flat(c['tracks'] if tracks is None else tracks, c['lead'] if lead is None else lead)
    ntracks = offsets.size - 1
    owner, traj_v = place(traj, c['shift'] if shift is None else shift)
    npts = traj.shape[0]
    p = np.full(npts, -7., dtype=np.float64)
    status = np.full(npts, 99, dtype=np.uint8)
    rows = np.full((ntracks, 6), 0xDEAD, dtype=np.uint64)
    if maps is None:
        maps = (np.zeros(c['shape'], dtype=np.uint64), np.zeros(c['shape'], dtype=np.uint32))
    upd = None if c['updraft'] is None else np.ascontiguousarray(c['updraft'], dtype=np.float64)
    pot = None if c['potential'] is None else np.ascontiguousarray(c['potential'], dtype=np.float32)
    prm = params_of(c)
    rc = L.ssrs_tracks_score(C.cast(C.byref(prm), C.c_void_p), ptr(upd), ptr(pot), ptr(traj_v), ptr(offsets), ntracks,
                             ptr(p) if want_p else None, ptr(status) if want_status else None, ptr(rows),
                             ptr(maps[0]) if want_maps else None, ptr(maps[1]) if want_maps else None, None)
    assert rc == 0, L.ssrs_last_error()
    lo, hi = int(offsets[0]), int(offsets[-1])
    # nothing outside the chunk's points is written
    outside = np.r_[0:lo, hi:npts]
    assert (p[outside] == -7.).all() and (status[outside] == 99).all()
    assert want_p or (p == -7.).all()
    assert want_status or (status == 99).all()
    return dict(p=p[lo:hi], status=status[lo:hi], rows=rows.view(np.int64), surprisal_map=maps[0].view(np.int64),
                scored_map=maps[1].astype(np.int64))


def check(c, got, want, maps=True, p=True, status=True):
    assert not status or np.array_equal(got['status'], want['status'])
    if not p:
        pass
    elif c['nu'] in (0., 1.):
        assert np.array_equal(got['p'].view(np.uint64), want['p'].view(np.uint64)), 'p is bit-equal for nu in {0, 1}'
    else:                                                  # (the same libm on both sides here; the device test has the bound)
        assert np.allclose(got['p'], want['p'], rtol=1e-12, atol=0., equal_nan=True)
    assert np.array_equal(got['rows'][:, 1:], want['rows'][:, 1:])
    assert ref.s_bound_ok(got['rows'], want['rows'])
    if maps:
        assert np.array_equal(got['scored_map'], want['scored_map'])
        assert abs(int(got['surprisal_map'].sum()) - int(want['surprisal_map'].sum())) <= int(want['rows'][:, 1].sum())
        assert (np.abs(got['surprisal_map'] - want['surprisal_map']) <= want['scored_map']).all()
        # the two checksums
        assert int(got['rows'][:, 0].sum()) == int(got['surprisal_map'].sum())
        assert int(got['rows'][:, 1].sum()) == int(got['scored_map'].sum())


@pytest.mark.parametrize('name', ref.case_names())
def test_emulated_case(emu, name):
    c = ref.case(name)
    check(c, call(emu, c), ref.expected(c))


def test_cases_cover_what_they_are_for():
    """Every status occurs; the corners of the fields do what their names say."""
    seen = np.zeros(6, dtype=np.int64)
    for c in ref.cases():
        seen += np.bincount(ref.expected(c)['status'], minlength=6)
    assert (seen > 0).all()
    assert (ref.expected(ref.case('huge_potential'))['status'] == ref.UNDEFINED).sum() > 0
    e = ref.expected(ref.case('7x9_m1_nu0'))
    evaluated = np.isin(e['status'], (ref.SCORED, ref.ZERO, ref.UNDEFINED))
    assert evaluated.sum() > 300 and (e['p'][evaluated] == 1. / 9.).all() and (e['status'][evaluated] == ref.SCORED).all()
    e = ref.expected(ref.case('huge_potential_nu0'))
    assert (e['p'][np.isin(e['status'], (ref.SCORED, ref.ZERO, ref.UNDEFINED))] == 1. / 9.).all()
    # a flat potential: every weight is 0, the masked prior decides
    c = ref.case('flat_potential')
    e = ref.expected(c)
    drw = ref.score(c['tracks'], c['shape'], c['move_dirn'], c['memory'], c['nu'])
    assert np.array_equal(e['p'], drw['p']) and (e['status'] == ref.SCORED).sum() > 100
    # every oracle track of a case scores on every move, the relocated first moves included
    for name in ('7x9_m1_nu1', '7x9_m8_nu1', '12x40_upd_m3', '12x40_drw_d250_m3', '12x40_drw_m8_nu0.5'):
        c = ref.case(name)
        for track in c['tracks'][-8:]:
            st = ref.expected(c, [track])['status']
            assert len(track) >= 2 and (st[:-1] == ref.SCORED).all() and st[-1] == ref.LAST, name


@pytest.mark.parametrize('name', ['7x9_m8_nu1', '12x40_upd_m3', 'g7_m8'])
def test_emulated_every_placement(emu, name):
    """traj at 0, 4, 8 and 12 bytes past a 16-byte boundary, every first offset modulo 4, and the outputs one by one."""
    c = ref.case(name)
    want = ref.expected(c)
    for shift in range(4):
        for lead in ((0, 1, 2, 3, 6) if shift == 0 else (c['lead'],)):
            check(c, call(emu, c, shift=shift, lead=lead), want)
    check(c, call(emu, c, want_p=False), want, p=False)
    check(c, call(emu, c, want_status=False), want, status=False)
    check(c, call(emu, c, want_maps=False), want, maps=False)


def test_emulated_independence(emu):
    """One call, two calls over two halves, a permuted order, with the maps accumulated across the calls: the same integers.
    (The same log2 on every path here, so the sums are equal, not only within the bound.)"""
    c = ref.case('g7_m8')
    tracks = c['tracks']
    n = len(tracks)
    whole = call(emu, c)
    maps = (np.zeros(c['shape'], dtype=np.uint64), np.zeros(c['shape'], dtype=np.uint32))
    halves = [call(emu, c, tracks=tracks[:n // 2], maps=maps), call(emu, c, tracks=tracks[n // 2:], maps=maps, lead=2)]
    assert np.array_equal(np.concatenate([h['rows'] for h in halves]), whole['rows'])
    assert np.array_equal(np.concatenate([h['p'] for h in halves]).view(np.uint64), whole['p'].view(np.uint64))
    assert np.array_equal(maps[0].view(np.int64), whole['surprisal_map']) and np.array_equal(maps[1], whole['scored_map'])
    order = np.random.default_rng(3).permutation(n)
    mixed = call(emu, c, tracks=[tracks[k] for k in order], shift=1)
    assert np.array_equal(mixed['rows'], whole['rows'][order])
    assert np.array_equal(mixed['surprisal_map'], whole['surprisal_map']) and np.array_equal(mixed['scored_map'], whole['scored_map'])
    # maps that start non-zero are added to
    maps = (np.full(c['shape'], 2 ** 62 - 3, dtype=np.uint64), np.full(c['shape'], 7, dtype=np.uint32))
    call(emu, c, maps=maps)
    assert np.array_equal(maps[0].view(np.int64) - (2 ** 62 - 3), whole['surprisal_map'])
    assert np.array_equal(maps[1].astype(np.int64) - 7, whole['scored_map'])
    # a track cut in two inside: the pieces overlap by memory + 1 points ... is NOT the same (the burn-in counts from each
    # piece's start); what is the same is a chunk of whole tracks taken out of a longer offsets array
    traj, offsets = ref.flat(tracks, 4)
    part = call(emu, c, traj=traj, offsets=np.ascontiguousarray(offsets[3:9]))
    assert np.array_equal(part['rows'], whole['rows'][3:8])


def test_emulated_blocks_and_long_tracks(emu):
    """A track of 2000 points crosses eight blocks: its row is the sum of eight segments; 40 tracks of 13 points put twenty
    segments into one block."""
    rng = np.random.default_rng(8)
    c = ref.case('g7_m1')
    tracks = [ref.forward(2000, ref.G7_SHAPE, rng)] + [ref.forward(13, ref.G7_SHAPE, rng) for _ in range(40)] + \
        [np.zeros((0, 2), dtype=np.int16)] * 3 + [ref.forward(600, ref.G7_SHAPE, rng)]
    want = ref.expected(c, tracks)
    before = emu.emu_blocks()
    check(c, call(emu, c, tracks=tracks, lead=1, shift=2), want)
    assert emu.emu_blocks() - before >= 12 and want['rows'][0, 1:3].sum() == 1999 and want['rows'][0, 1] > 256


def test_emulated_nothing_to_do_touches_nothing(emu):
    c = ref.case('7x9_m1_nu1')
    traj, offsets = ref.flat(c['tracks'], 2)
    p = np.full(traj.shape[0], -7.)
    rows = np.full((4, 6), 9, dtype=np.uint64)
    prm = params_of(c)
    before = emu.emu_launches()
    for off, n in ((np.array([5], dtype=np.int64), 0), (np.array([5, 5, 5, 5], dtype=np.int64), 3)):
        rc = emu.ssrs_tracks_score(C.cast(C.byref(prm), C.c_void_p), None, None, ptr(traj), ptr(off), n, ptr(p), None, ptr(rows),
                                   None, None, None)
        assert rc == 0
    assert emu.emu_launches() == before and (p == -7.).all() and (rows == 9).all()
