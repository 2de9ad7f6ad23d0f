"""K20 without a GPU: ssrs_amd/csrc/site_risk.hip compiled with g++ against tests/hip_host_stub under -ffp-contract=off and
run on the CPU, as test_collision_emulation.py does for K19.  The kernel cooperates through __shared__ and __syncthreads()
only, so its own code runs here as it stands: the lanes' runs and the point behind them, the two binary searches and the
walk over empty tracks, the aligned and the point-by-point loads, the window and its clipping, the shared statement of the
test (csrc/rotor_disk.h), the staged table and the 64-bit adds of lanes that meet on one site (the threads of a block are
OS threads) -- on the cases of tests/site_ref.py, which tests/test_gpu_site_risk.py runs on the device.  What it does not
cover: the device's own arithmetic (the f64 operations and the divisions are the host's here), blocks that run at the same
time (they run one after another), and speed."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import site_ref as ref
import transit_ref as tref

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
# what the kernel uses beyond the stub: the vector types, the atomics (the threads of a block are OS threads), the rounding
# intrinsics (plain operations under -ffp-contract=off), the copies; launches and blocks are counted
EXTRA_H = '''#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) int4 { int x, y, z, w; };
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline double __dmul_rn(double a, double b) { return a * b; }
inline double __dadd_rn(double a, double b) { return a + b; }
inline double __dsub_rn(double a, double b) { return a - b; }
constexpr int hipMemcpyDeviceToHost = 2;
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline long long emu_launch_count = 0, emu_block_count = 0;
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \\
    (++emu_launch_count, emu_block_count += dim3(grid).x, emu_launch(grid, block, [&] { kernel(__VA_ARGS__); }))
'''


def build(work):
    """The CPU build of site_risk.hip in `work`, bound by the library's own prototype."""
    from ssrs_amd import _native
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'site_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'libsite_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include',
                    str(work / 'site_emu_extra.h'), '-x', 'c++', os.path.join(csrc, 'site_risk.hip'),
                    str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_blocks.restype = C.c_longlong
    L.ssrs_site_collision_risk.argtypes = _native.SITE_COLLISION_RISK_ARGTYPES
    return L


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    return build(tmp_path_factory.mktemp('site_emu'))


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def place(values, shift):
    """`values` (4 bytes a row) copied to an address `shift` elements past a 16-byte boundary.  Returns (owner, view)."""
    raw = np.zeros((values.shape[0] + 12,) + values.shape[1:], dtype=values.dtype)
    assert raw.ctypes.data % 4 == 0 and (values.shape[0] == 0 or raw[0].nbytes == 4)
    start = (-raw.ctypes.data % 16) // 4 + 4 + shift
    view = raw[start:start + values.shape[0]]
    view[:] = values
    assert view.shape[0] == 0 or (view.ctypes.data % 16) == 4 * (shift % 4)
    return raw, view


def call(L, c, k, off=None, transits=None, risk=None, shift=None, alt_shift=None, want_transits=True, axis=None):
    """One call on case `c` with class `k` over the tracks of `off` (default: all).  axis: a per-cell raster instead of the
    class's own.  Returns (transits, risk) int64 (rows, cols, 2); transits None when not wanted."""
    traj, alt, offsets = tref.flat(c)
    off = np.ascontiguousarray(offsets[1:] if off is None else off)
    ntracks = off.size - 1
    rows, cols = c['shape']
    k = ref.klass(k)
    shift = c['shift'] if shift is None else shift
    o1, traj_v = place(traj, shift)
    o2, alt_v = place(alt, shift if alt_shift is None else alt_shift)
    info = tref.packed(c['elev'])
    ax = np.ascontiguousarray(k['axis'] if axis is None else axis, dtype=np.float64)
    risk = np.zeros((rows, cols, 2), dtype=np.uint64) if risk is None else risk
    if want_transits:
        transits = np.zeros((rows, cols, 2), dtype=np.uint64) if transits is None else transits
    rc = L.ssrs_site_collision_risk(ptr(traj_v), ptr(off), ntracks, ptr(alt_v), ptr(info), rows, cols, k['reach'], k['hub_mm'],
                                    ptr(ax), int(ax.ndim == 3), ref.MM, ptr(ref.TABLE), ptr(transits) if want_transits else None,
                                    ptr(risk), None)
    assert rc == 0, L.ssrs_last_error()
    return transits.astype(np.int64) if want_transits else None, risk.astype(np.int64)


def check(res, out):
    transits, risk = out
    assert transits is None or np.array_equal(transits, res['transits'])
    assert np.array_equal(risk, res['risk'])


@pytest.mark.parametrize('c,k', ref.COMBOS, ids=ref.COMBO_IDS)
def test_emulated_case(emu, c, k):
    res = ref.expected(c, k)
    check(res, call(emu, c, k))
    # the uniform axis equals a per-cell raster filled with that axis
    filled = np.array(np.broadcast_to(np.array(ref.klass(k)['axis']), c['shape'] + (2,)))
    check(res, call(emu, c, k, axis=filled))


def test_cases_are_not_empty():
    """Every class transits something on the planted cases, in both directions; reach 0 only through a hub."""
    for k in ref.CLASS_IDS:
        assert (ref.expected(ref.case('rings'), k)['transits'].sum((0, 1)) > 0).all(), k
    assert ref.expected(ref.case('planted'), 'r65')['transits'].sum() > 10000
    assert all(ref.expected(c, 'r4_col')['transits'].sum() > 0 for c in ref.TINY_CASES[1:])
    assert ref.expected(ref.TINY_CASES[0], 'r4_col')['transits'].sum() == 0         # (a 1 x 1 raster has no move)


@pytest.mark.parametrize('c,k', ref.CELL_COMBOS, ids=ref.CELL_IDS)
def test_emulated_cell_axes(emu, c, k):
    res = ref.expected(c, k, per_cell=True)
    check(res, call(emu, c, k, axis=ref.cell_axes(c['shape'])))
    assert c['shape'] != ref.SHAPE or res['transits'].sum() > 0


@pytest.mark.parametrize('name', ['planted', 'pingpong', 'cuts', 'rings'])
def test_emulated_every_placement(emu, name):
    """Both buffers at the three misaligned placements, the point-by-point path with `alt` alone off the boundary, and the
    same without the counts (transits NULL)."""
    c = ref.case(name)
    res = ref.expected(c, 'r4')
    for shift, alt_shift in ((1, 1), (2, 2), (3, 3), (0, 1), (0, 0)):
        check(res, call(emu, c, 'r4', shift=shift, alt_shift=alt_shift))
    for shift in (0, 1):
        check(res, call(emu, c, 'r4', shift=shift, want_transits=False))


def test_emulated_accumulation_and_chunks(emu):
    """A batch cut into chunks -- inside the long tracks too: a track cut in two overlaps by the point of the cut, so that
    every move is in exactly one chunk -- into outputs that start non-zero (risk at 2^62 - 3) equals one call plus what the
    outputs held."""
    c = ref.case('pingpong')
    res = ref.expected(c, 'r4')
    _, _, offsets = tref.flat(c)
    off = offsets[1:]
    ntracks = off.size - 1
    rows, cols = c['shape']
    transits = np.full((rows, cols, 2), 7, dtype=np.uint64)
    risk = np.full((rows, cols, 2), 2 ** 62 - 3, dtype=np.uint64)
    for lo, hi in ((0, 3), (3, 4), (4, 11)):
        call(emu, c, 'r4', off=off[lo:hi + 1], transits=transits, risk=risk)
    # track 11 is the 4097-point ping-pong: three pieces, each starting at the last point of the one before
    a, b = int(off[11]), int(off[12])
    for lo, hi in ((a, a + 1001), (a + 1000, a + 3002), (a + 3001, b)):
        call(emu, c, 'r4', off=np.array([lo, hi], dtype=np.int64), transits=transits, risk=risk)
    call(emu, c, 'r4', off=off[12:], transits=transits, risk=risk)
    assert ntracks > 12
    assert np.array_equal(transits.astype(np.int64) - 7, res['transits'])
    assert np.array_equal(risk.astype(np.int64) - (2 ** 62 - 3), res['risk'])


def test_emulated_many_moves_on_the_same_sites_and_many_sites(emu):
    """The two ends of the adds.  (The kernel has no table of sites in LDS -- one was built, measured and dropped,
    profiles/site_collision_risk.md -- so there are no two paths to count: every transit is a 64-bit add to its site.)  The
    ping-pong repeats one move inside the reach-6.5 window of a few dozen sites 4096 times, from every lane of two blocks;
    the serpentine walks 6000 distinct moves over a 300 x 300 raster, three blocks, thousands of distinct sites."""
    c = ref.case('pingpong')
    blocks = emu.emu_blocks()
    check(ref.expected(c, 'r65'), call(emu, c, 'r65'))
    assert emu.emu_blocks() - blocks >= 3
    shape = (300, 300)
    pts = []
    for r in range(0, 60):
        cols = range(5, 295) if r % 2 == 0 else range(294, 4, -1)
        pts += [(r + 5, col) for col in cols]
    pts = np.array(pts[:6000], dtype=np.int16)
    rng = np.random.default_rng(5)
    big = dict(name='serpentine', shape=shape, tracks=[pts], alts=[(ref.LEVEL + rng.integers(-200_000, 200_000, len(pts))).astype(np.int32)],
               elev=np.full(shape, ref.GROUND, dtype=np.int32), lead=0, tail=0, shift=0)
    res = ref.compute(big, 'r65')
    assert np.count_nonzero(res['transits'].sum(2)) > 6000
    check(res, call(emu, big, 'r65'))


def test_emulated_nothing_to_do_touches_nothing(emu):
    c = ref.case('rings')
    rows, cols = c['shape']
    transits = np.full((rows, cols, 2), 9, dtype=np.uint64)
    risk = transits.copy()
    before = emu.emu_launches()
    call(emu, c, 'r4', off=np.array([5], dtype=np.int64), transits=transits, risk=risk)
    call(emu, c, 'r4', off=np.array([5, 5, 5, 5], dtype=np.int64), transits=transits, risk=risk)
    # a NaN or negative reach: SSRS_OK, nothing launched
    traj, alt, offsets = tref.flat(c)
    info = tref.packed(c['elev'])
    ax = np.array(ref.PLANE)
    off = np.ascontiguousarray(offsets[1:])
    for reach in (float('nan'), -1., -float('inf')):
        rc = emu.ssrs_site_collision_risk(ptr(traj), ptr(off), off.size - 1, ptr(alt), ptr(info), rows, cols, reach, 0, ptr(ax), 0,
                                          ref.MM, ptr(ref.TABLE), ptr(transits), ptr(risk), None)
        assert rc == 0
    assert emu.emu_launches() == before
    assert (transits == 9).all() and (risk == 9).all()
