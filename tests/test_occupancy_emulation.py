"""K13 without a GPU: ssrs_amd/csrc/occupancy.hip compiled with g++ against tests/hip_host_stub and run on the CPU, as
test_allen_emulation.py does for K12.  The kernel uses no cross-lane intrinsic, so its own code runs here as it stands:
the rounds and their bits and planes, the offsets staged per round, the binary search and the walk over empty tracks and
track ends inside a lane's four points, the aligned and the point-by-point loads, the test-before-set and the race for a
bit (the threads of a block are OS threads), both clearing paths and the zero workspace -- on the cases of
tests/occupancy_ref.py, which tests/test_gpu_occupancy.py runs on the device."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import occupancy_ref as ref

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
extern "C" long long emu_blocks(void) { return emu_block_count; }
'''
# what this kernel uses beyond the stub: the 16-byte vector, atomics (the threads of a block are OS threads), the L2 load
# and the copies; launches and blocks are counted, so that the grid sizing can be seen
EXTRA_H = '''#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <class T> inline T atomicOr(T *p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
#define __HIP_MEMORY_SCOPE_AGENT 4
#define __HIP_MEMORY_SCOPE_SYSTEM 5
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, order)
inline int __popc(unsigned v) { return __builtin_popcount(v); }
constexpr int hipMemcpyDeviceToHost = 2;
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemcpy2DAsync(void *d, size_t dpitch, const void *s, size_t spitch, size_t width, size_t height, int,
                                   hipStream_t)
{ for (size_t i = 0; i < height; ++i) memcpy((char *)d + i * dpitch, (const char *)s + i * spitch, width);
  return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline long long emu_launch_count = 0, emu_block_count = 0;
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \\
    (++emu_launch_count, emu_block_count += dim3(grid).x, emu_launch(grid, block, [&] { kernel(__VA_ARGS__); }))
'''


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    from ssrs_amd import _native
    work = tmp_path_factory.mktemp('occupancy_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'occupancy_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'liboccupancy_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include', str(work / 'occupancy_emu_extra.h'),
                    '-x', 'c++', os.path.join(csrc, 'occupancy.hip'), str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_blocks.restype = C.c_longlong
    L.ssrs_track_occupancy_workspace_bytes.restype = C.c_size_t
    L.ssrs_track_occupancy_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.ssrs_track_occupancy.argtypes = _native.OCCUPANCY_ARGTYPES
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def place(traj, shift):
    """`traj` copied to an address `shift` points (4 bytes each) past a 16-byte boundary; the points around it are
    in-raster, so that a kernel that counted them would show.  Returns (the owner of the memory, the view)."""
    raw = np.full((traj.shape[0] + 12, 2), 3, dtype=np.int16)
    assert raw.ctypes.data % 4 == 0
    start = (-raw.ctypes.data % 16) // 4 + 4 + shift
    view = raw[start:start + traj.shape[0]]
    view[:] = traj
    assert view.shape[0] == 0 or (view.ctypes.data % 16) == 4 * (shift % 4)
    return raw, view


class Call:
    """One workspace and its buffers for a raster: calls chain on it, and it must be zero after each."""

    def __init__(self, L, shape, planes):
        self.L, self.shape, self.planes = L, shape, planes
        self.nbytes = L.ssrs_track_occupancy_workspace_bytes(shape[0], shape[1], planes)
        assert self.nbytes == -(-shape[0] * shape[1] * 4 * planes // 256) * 256
        self.ws = np.zeros(self.nbytes // 4, dtype=np.uint32)

    def __call__(self, traj, off, counts, per_track=None, shift=0):
        """off: the offsets the call gets (a slice of a longer vector).  Returns (launches, blocks)."""
        owner, view = place(traj, shift)
        off = np.ascontiguousarray(off)
        before = self.L.emu_launches(), self.L.emu_blocks()
        rc = self.L.ssrs_track_occupancy(ptr(view), ptr(off), off.size - 1, self.shape[0], self.shape[1], self.planes,
                                         ptr(counts), ptr(per_track), ptr(self.ws), self.nbytes, None)
        assert rc == 0, self.L.ssrs_last_error()
        assert not self.ws.any(), 'the workspace is not zero after the call'
        return self.L.emu_launches() - before[0], self.L.emu_blocks() - before[1]


def run_case(L, c, planes, call=None):
    traj, off = ref.flat(c)
    call = call or Call(L, c['shape'], planes)
    counts = np.zeros(c['shape'], dtype=np.uint32)
    per_track = np.zeros(len(c['tracks']), dtype=np.uint32)
    work = call(traj, off[1:], counts, per_track, shift=c['shift'])
    return counts, per_track, work


@pytest.mark.parametrize('planes', ref.PLANES)
@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_emulated_case(emu, c, planes):
    counts, per_track, (launches, blocks) = run_case(emu, c, planes)
    ref.check(c['name'], counts, per_track)
    # two launches a round at most (set, and unset or a memset), each sized from the round's points: a wave takes four
    # spans of 256 points at least, so 4096 points fill a block
    paths = ref.clearing_paths(c, planes)
    assert launches == len(paths) + paths.count('unset')
    points = sum(len(t) for t in c['tracks'])
    assert blocks <= launches * (points // 4096 + 2)
    if c['name'] == 'memset_path':
        assert set(paths) == {'memset'}
    if c['name'].startswith('borders_') and c['tracks']:
        assert set(paths) == {'unset'}


def test_emulated_small_round_is_a_small_launch(emu):
    """A round of ~200 points is one block a launch, not K8's 1536."""
    c = ref.case('borders_33')
    assert sum(len(t) for t in c['tracks'][:32]) < 400
    _, _, (launches, blocks) = run_case(emu, c, 1)
    assert (launches, blocks) == (4, 4)


def test_emulated_no_per_track(emu):
    c = ref.case('empty_tracks')
    traj, off = ref.flat(c)
    counts = np.zeros(c['shape'], dtype=np.uint32)
    Call(emu, c['shape'], 3)(traj, off[1:], counts, None)
    assert np.array_equal(counts, ref.expected(c['name'])[0])


@pytest.mark.parametrize('planes', ref.PLANES)
def test_emulated_accumulation(emu, planes):
    """Two calls on disjoint track sets into one `counts` (and one workspace) equal one call on the union, and what
    `counts` held before is kept."""
    c = ref.case('borders_97')
    traj, off = ref.flat(c)
    off = off[1:]
    pattern = (np.arange(c['shape'][0] * c['shape'][1], dtype=np.uint32).reshape(c['shape']) * 2654435761) | 1
    counts = pattern.copy()
    per_track = np.full(97, 5, dtype=np.uint32)
    call = Call(emu, c['shape'], planes)
    call(traj, off[:41], counts, per_track[:40])
    call(traj, off[40:], counts, per_track[40:])                 # (its first offset is not 0)
    ref.check(c['name'], counts, per_track - 5, before=pattern)
    call(traj, off, counts, per_track)                           # once more on the same workspace: everything twice
    assert np.array_equal(counts - pattern, 2 * ref.expected(c['name'])[0])
    assert np.array_equal(per_track - 5, 2 * ref.expected(c['name'])[1])


def test_emulated_nothing_to_do_touches_nothing(emu):
    call = Call(emu, ref.SHAPE, 2)
    counts = np.full(ref.SHAPE, 9, dtype=np.uint32)
    per_track = np.full(3, 9, dtype=np.uint32)
    traj = np.zeros((0, 2), dtype=np.int16)
    assert call(traj, np.array([5], dtype=np.int64), counts, per_track) == (0, 0)               # ntracks == 0
    assert call(traj, np.array([5, 5, 5, 5], dtype=np.int64), counts, per_track) == (0, 0)      # no points
    assert (counts == 9).all() and (per_track == 9).all()


def test_emulated_refusals(emu):
    rows, cols = 8, 8
    traj = np.zeros((16, 2), dtype=np.int16)
    off = np.array([0, 4], dtype=np.int64)
    counts = np.zeros((rows, cols), dtype=np.uint32)
    nbytes = emu.ssrs_track_occupancy_workspace_bytes(rows, cols, 8)
    ws = np.zeros(nbytes // 4, dtype=np.uint32)
    good = dict(traj=ptr(traj), off=ptr(off), ntracks=1, rows=rows, cols=cols, planes=1, counts=ptr(counts),
                per_track=None, ws=ptr(ws), nbytes=nbytes)

    def refused(text, **kw):
        a = dict(good, **kw)
        before = emu.emu_launches()
        rc = emu.ssrs_track_occupancy(a['traj'], a['off'], a['ntracks'], a['rows'], a['cols'], a['planes'], a['counts'],
                                      a['per_track'], a['ws'], a['nbytes'], None)
        msg = emu.ssrs_last_error()
        assert rc == SSRS_ERR_INVALID and text in msg and b'ssrs_track_occupancy' in msg, (rc, msg)
        assert emu.emu_launches() == before and not counts.any() and not ws.any()

    for name in ('traj', 'off', 'counts', 'ws'):
        refused(b'NULL', **{name: None})
    for planes in (0, -1, 9):
        refused(b'planes', planes=planes)
    for kw in (dict(rows=0), dict(rows=32768), dict(cols=0), dict(cols=32768)):
        refused(b'raster', **kw)
    for ntracks in (-1, 2 ** 31):
        refused(b'ntracks', ntracks=ntracks)
    refused(b'4-byte aligned', traj=C.c_void_p(traj.ctypes.data + 2))
    refused(b'workspace', nbytes=255)
    refused(b'workspace', planes=8, nbytes=nbytes - 1)
    assert emu.ssrs_track_occupancy_workspace_bytes(0, 8, 1) == 0
    rc = emu.ssrs_track_occupancy(good['traj'], good['off'], 1, rows, cols, 1, good['counts'], None, good['ws'], nbytes, None)
    assert rc == 0 and counts[0, 0] == 1 and counts.sum() == 1 and not ws.any()
