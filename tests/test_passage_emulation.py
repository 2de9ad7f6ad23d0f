"""K17 without a GPU: ssrs_amd/csrc/passage.hip compiled with g++ against tests/hip_host_stub and run on the CPU, as
test_occupancy_emulation.py does for K13.  The kernel uses no cross-lane intrinsic, so its own code runs here as it
stands: the half-widths in LDS, whole disks and crescents and their clipping, the predecessor across the lane and span
cuts, the memo, the race for a bit (the threads of a block are OS threads), both ways of clearing and a workspace that is
never clean -- on the cases of tests/passage_ref.py, which tests/test_gpu_passage.py runs on the device."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import passage_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SSRS_ERR_INVALID = -1
ERR_CPP = '''#include "common.h"
namespace ssrs {
char *error_buffer() { static thread_local char buf[512] = ""; return buf; }
int set_error(int code, const char *fmt, ...)
{ va_list ap; va_start(ap, fmt); vsnprintf(error_buffer(), 512, fmt, ap); va_end(ap); return code; }
}
extern "C" const char *ssrs_last_error(void) { return ssrs::error_buffer(); }
extern "C" long long emu_launches(void) { return emu_launch_count; }
extern "C" long long emu_memsets(void) { return emu_memset_count; }
'''
# what this kernel uses beyond the stub: the 16-byte vector, atomics (the threads of a block are OS threads), the L2 load
# and the copies; launches and memsets are counted, so that the clearing path can be seen
EXTRA_H = '''#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <class T> inline T atomicOr(T *p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
#define __HIP_MEMORY_SCOPE_AGENT 4
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, order)
constexpr int hipMemcpyDeviceToHost = 2;
inline long long emu_launch_count = 0, emu_memset_count = 0;
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { ++emu_memset_count; memset(p, v, n); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemcpy2DAsync(void *d, size_t dpitch, const void *s, size_t spitch, size_t width, size_t height, int,
                                   hipStream_t)
{ for (size_t i = 0; i < height; ++i) memcpy((char *)d + i * dpitch, (const char *)s + i * spitch, width);
  return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \\
    (++emu_launch_count, emu_launch(grid, block, [&] { kernel(__VA_ARGS__); }))
'''


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    from ssrs_amd import _native
    work = tmp_path_factory.mktemp('passage_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'passage_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'libpassage_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include', str(work / 'passage_emu_extra.h'),
                    '-x', 'c++', os.path.join(csrc, 'passage.hip'), str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_memsets.restype = C.c_longlong
    L.ssrs_track_passage_workspace_bytes.restype = C.c_size_t
    L.ssrs_track_passage_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.ssrs_track_passage.argtypes = _native.PASSAGE_ARGTYPES
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def place(traj, shift):
    """`traj` copied to an address `shift` points (4 bytes each) past a 16-byte boundary; the points around it are
    in-raster, so that a kernel that counted them would show.  Returns (the owner of the memory, the view)."""
    raw = np.zeros((traj.shape[0] + 12, 2), dtype=np.int16)
    assert raw.ctypes.data % 4 == 0
    start = (-raw.ctypes.data % 16) // 4 + 4 + shift
    view = raw[start:start + traj.shape[0]]
    view[:] = traj
    assert view.shape[0] == 0 or (view.ctypes.data % 16) == 4 * (shift % 4)
    return raw, view


_workspaces = {}


def dirty_workspace(L, shape, planes):
    """One workspace per (raster, planes) for the whole module: 0xFF at first, then whatever the case before left in it.
    No test cleans it."""
    key = (shape, planes)
    if key not in _workspaces:
        nbytes = L.ssrs_track_passage_workspace_bytes(shape[0], shape[1], planes)
        assert nbytes == -(-shape[0] * shape[1] * 4 * planes // 256) * 256
        _workspaces[key] = np.full(nbytes // 4, 0xFFFFFFFF, dtype=np.uint32)
    return _workspaces[key]


def call(L, shape, r2, planes, traj, off, counts, per_track=None, stats=None, shift=0, ws=None):
    """off: the offsets the call gets (a slice of a longer vector).  Returns (launches, memsets)."""
    owner, view = place(traj, shift)
    off = np.ascontiguousarray(off)
    ws = dirty_workspace(L, shape, planes) if ws is None else ws
    before = L.emu_launches(), L.emu_memsets()
    rc = L.ssrs_track_passage(ptr(view), ptr(off), off.size - 1, shape[0], shape[1], r2, planes, ptr(counts),
                              ptr(per_track), ptr(stats), ptr(ws), ws.nbytes, None)
    assert rc == 0, L.ssrs_last_error()
    return L.emu_launches() - before[0], L.emu_memsets() - before[1]


def run_case(L, c, planes, shift=0, ws=None):
    traj, off = ref.flat(c)
    counts = np.zeros(c['shape'], dtype=np.uint32)
    per_track = np.zeros(len(c['tracks']), dtype=np.uint32)
    stats = np.zeros(2, dtype=np.uint64)
    work = call(L, c['shape'], c['r2'], planes, traj, off[1:], counts, per_track, stats, shift=shift, ws=ws)
    return counts, per_track, stats, work


@pytest.mark.parametrize('planes', ref.PLANES)
@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_emulated_case(emu, c, planes):
    """Aligned and at the three misaligned placements, on a workspace that holds 0xFF or another case's leavings."""
    paths = ref.clearing_paths(c, planes)
    for shift in (0, 1, 2, 3):
        counts, per_track, stats, (launches, memsets) = run_case(emu, c, planes, shift)
        ref.check(c['name'], counts, per_track)
        assert int(stats[1]) == int(counts.sum(dtype=np.int64))
        assert int(stats[0]) >= int(stats[1])
        # one set kernel a round with points, and before it a memset or the unset walk of the round before
        assert (launches, memsets) == (len(paths) + paths.count('unset'), paths.count('memset'))


def test_both_clearing_paths_are_taken():
    """The cases above go through both: the short tracks of a 70 x 130 raster are unset, the long ones of 5 x 3 memset."""
    assert ref.clearing_paths(ref.case('borders_257'), 1) == ['memset'] + ['unset'] * 8
    assert ref.clearing_paths(ref.case('borders_257_r26'), 1) == ['memset'] + ['unset'] * 8
    assert ref.clearing_paths(ref.case('borders_257'), 8) == ['memset', 'memset']      # (a 1-track round against 1 plane)
    assert ref.clearing_paths(ref.case('borders_33'), 1) == ['memset', 'unset']
    assert ref.clearing_paths(ref.case('memset_path'), 1) == ['memset', 'memset']


def test_emulated_clearing_choice_does_not_matter(emu):
    """The same tracks at a radius where the rule picks the unset walk and at planes where it picks the memset, each on a
    workspace of 0xFF and on one of zeros: four times the restatement's integers."""
    c = ref.case('borders_33')
    for planes, want in ((1, ['memset', 'unset']), (3, ['memset'])):
        assert ref.clearing_paths(c, planes) == want
        for fill in (0xFFFFFFFF, 0):
            ws = np.full(emu.ssrs_track_passage_workspace_bytes(*c['shape'], planes) // 4, fill, dtype=np.uint32)
            counts, per_track, _, _ = run_case(emu, c, planes, ws=ws)
            ref.check(c['name'], counts, per_track)


def test_emulated_no_per_track_no_stats(emu):
    c = ref.case('lengths_r8')
    traj, off = ref.flat(c)
    counts = np.zeros(c['shape'], dtype=np.uint32)
    call(emu, c['shape'], c['r2'], 3, traj, off[1:], counts)
    assert np.array_equal(counts, ref.expected(c['name'])[0])


@pytest.mark.parametrize('planes', ref.PLANES)
def test_emulated_accumulation(emu, planes):
    """Two calls on disjoint track sets into one `counts` equal one call on the union, and what `counts`,
    `cells_per_track` and `stats` held before is kept."""
    c = ref.case('borders_257')
    traj, off = ref.flat(c)
    off = off[1:]
    pattern = (np.arange(c['shape'][0] * c['shape'][1], dtype=np.uint32).reshape(c['shape']) * 2654435761) | 1
    counts = pattern.copy()
    per_track = np.full(257, 5, dtype=np.uint32)
    stats = np.array([7, 11], dtype=np.uint64)
    call(emu, c['shape'], c['r2'], planes, traj, off[:101], counts, per_track[:100], stats)
    call(emu, c['shape'], c['r2'], planes, traj, off[100:], counts, per_track[100:], stats)      # (its first offset is not 0)
    ref.check(c['name'], counts, per_track - 5, before=pattern)
    assert int(stats[1]) - 11 == int(ref.expected(c['name'])[0].sum(dtype=np.int64))


def test_emulated_r2_zero_is_occupancy(emu):
    import occupancy_ref
    for name in ('borders_33', 'empty_tracks', 'outside', 'shape_1x40'):
        c = occupancy_ref.case(name)
        traj, off = occupancy_ref.flat(c)
        counts = np.zeros(c['shape'], dtype=np.uint32)
        per_track = np.zeros(len(c['tracks']), dtype=np.uint32)
        stats = np.zeros(2, dtype=np.uint64)
        call(emu, c['shape'], 0, 3, traj, off[1:], counts, per_track, stats)
        occupancy_ref.check(name, counts, per_track)


def test_emulated_work_bounds(emu):
    """stats[0] at r2 = 25: a unit move costs a crescent, not a disk, and the memo leaves a ping-pong two crescents a
    lane.  |D| and the largest crescent come from the restatement's offset list."""
    ndisk, ncres = len(ref.disk(25)), max(ref.crescent_sizes(25))
    assert ndisk == 81 and 11 <= ncres and ndisk > 4 * ncres          # (a crescent has a cell a row at least)
    c = ref.case('straight_1024')
    n = len(c['tracks'][0]) - 1
    counts, per_track, stats, _ = run_case(emu, c, 1)
    ref.check(c['name'], counts, per_track)
    assert n == 1024 and int(stats[0]) <= ndisk + n * ncres           # (whole disks: about n * ndisk)
    c = ref.case('pingpong_4096')
    n = len(c['tracks'][0])
    counts, per_track, stats, _ = run_case(emu, c, 1)
    ref.check(c['name'], counts, per_track)
    assert n == 4096 and int(stats[0]) <= ndisk + (n // 4) * ncres    # (no memo: n crescents)
    assert int(stats[0]) >= ndisk + 2 * min(ref.crescent_sizes(25))   # the first lane's two, at least


def test_emulated_nothing_to_do_touches_nothing(emu):
    shape = (37, 53)
    ws = np.full(emu.ssrs_track_passage_workspace_bytes(*shape, 2) // 4, 0xA5A5A5A5, dtype=np.uint32)
    counts = np.full(shape, 9, dtype=np.uint32)
    per_track = np.full(3, 9, dtype=np.uint32)
    stats = np.full(2, 9, dtype=np.uint64)
    traj = np.zeros((0, 2), dtype=np.int16)
    assert call(emu, shape, 4, 2, traj, np.array([5], dtype=np.int64), counts, per_track, stats, ws=ws) == (0, 0)
    assert call(emu, shape, 4, 2, traj, np.array([5, 5, 5, 5], dtype=np.int64), counts, per_track, stats, ws=ws) == (0, 0)
    assert (counts == 9).all() and (per_track == 9).all() and (stats == 9).all() and (ws == 0xA5A5A5A5).all()
