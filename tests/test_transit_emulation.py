"""K18 without a GPU: ssrs_amd/csrc/rotor_transits.hip compiled with g++ against tests/hip_host_stub and run on the CPU, as
test_passage_emulation.py does for K17.  The kernel uses no cross-lane intrinsic, so its own code runs here as it stands:
the mask and the counters in dynamic LDS, the lanes' four points and the successor across the lane and span cuts, the
galloping track search over empty tracks and track ends, the aligned and the point-by-point loads, the pending pair and
its hand-overs to LDS and, past the LDS rule's limit, to global memory, the bitmap's memory of the last word (the threads
of a block are OS threads) -- on the cases of tests/transit_ref.py, which tests/test_gpu_rotor_transits.py runs on the
device.  What it does not cover: the device's own arithmetic (the f64 operations are the host's here, under
-ffp-contract=off), blocks that run at the same time (they run one after another), and speed."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import transit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SSRS_ERR_INVALID = -1
LDS_WORDS = 15 * 1024
# The stand-in for dynamic LDS: the stub's `__shared__` is `static`, which `extern __shared__ T name[]` cannot take, so
# the extra header makes it nothing for this file (the kernel has no other __shared__ variable) and the name becomes an
# ordinary array, defined here.  Blocks run one after another, so one array serves.  It is 64 KB of 0xA5 before every
# launch: the launch macro records the bytes asked for, and what lies behind them must still be 0xA5 afterwards.
ERR_CPP = '''#include "common.h"
namespace ssrs {
uint32_t s_trn_lds[16384];
char *error_buffer() { static thread_local char buf[512] = ""; return buf; }
int set_error(int code, const char *fmt, ...)
{ va_list ap; va_start(ap, fmt); vsnprintf(error_buffer(), 512, fmt, ap); va_end(ap); return code; }
}
extern "C" const char *ssrs_last_error(void) { return ssrs::error_buffer(); }
extern "C" long long emu_launches(void) { return emu_launch_count; }
extern "C" long long emu_blocks(void) { return emu_block_count; }
extern "C" long long emu_lds_bytes(void) { return emu_last_lds; }
extern "C" uint32_t *emu_lds(void) { return ssrs::s_trn_lds; }
'''
EXTRA_H = '''#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#undef __shared__
#define __shared__
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) int4 { int x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <class T> inline T atomicOr(T *p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
#define __HIP_MEMORY_SCOPE_AGENT 4
#define __hip_atomic_load(p, order, scope) __atomic_load_n(p, order)
// every operation rounds on its own: plain operations under -ffp-contract=off
inline double __dmul_rn(double a, double b) { return a * b; }
inline double __dadd_rn(double a, double b) { return a + b; }
inline double __dsub_rn(double a, double b) { return a - b; }
constexpr int hipMemcpyDeviceToHost = 2;
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
namespace ssrs { extern uint32_t s_trn_lds[16384]; }
inline long long emu_launch_count = 0, emu_block_count = 0, emu_last_lds = -1;
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \\
    (++emu_launch_count, emu_block_count += dim3(grid).x, emu_last_lds = (long long)(lds), \\
     memset(ssrs::s_trn_lds, 0xA5, sizeof(ssrs::s_trn_lds)), emu_launch(grid, block, [&] { kernel(__VA_ARGS__); }))
'''


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    from ssrs_amd import _native
    work = tmp_path_factory.mktemp('transit_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'transit_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'libtransit_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include',
                    str(work / 'transit_emu_extra.h'), '-x', 'c++', os.path.join(csrc, 'rotor_transits.hip'),
                    str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_blocks.restype = L.emu_lds_bytes.restype = C.c_longlong
    L.emu_lds.restype = C.POINTER(C.c_uint32)
    L.ssrs_rotor_transits.argtypes = _native.ROTOR_TRANSITS_ARGTYPES
    return L


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


def lds_words(shape, nturb):
    """(mask words or 0, turbines with counters in LDS) by the header's rule."""
    nbins = -(-shape[0] // 32) * -(-shape[1] // 32)
    mask_words = (nbins + 31) // 32
    mask = mask_words <= 8192 and mask_words + 2 * nturb <= LDS_WORDS
    return (mask_words if mask else 0), (nturb if mask else min(nturb, 7680))


def call(L, c, off=None, hits=None, transits=None, shift=None, alt_shift=None, bins=None):
    """One call on a case over the tracks of `off` (default: all).  Returns (hits uint32, transits int64)."""
    traj, alt, offsets = ref.flat(c)
    off = np.ascontiguousarray(offsets[1:] if off is None else off)
    ntracks = off.size - 1
    nturb = len(c['reach'])
    shift = c['shift'] if shift is None else shift
    o1, traj_v = place(traj, shift)
    o2, alt_v = place(alt, shift if alt_shift is None else alt_shift)
    info = ref.packed(c['elev'])
    bin_start, bin_items = ref.bins(c) if bins is None else bins
    xy = np.ascontiguousarray(c['xy'], dtype=np.float64)
    reach = np.ascontiguousarray(c['reach'], dtype=np.float64)
    hub = np.ascontiguousarray(c['hub'], dtype=np.int32)
    axis = np.ascontiguousarray(c['axis'], dtype=np.float64)
    hits = np.zeros((ntracks, (nturb + 31) // 32), dtype=np.uint32) if hits is None else hits
    transits = np.zeros((nturb, 2), dtype=np.uint64) if transits is None else transits
    before = L.emu_launches()
    rc = L.ssrs_rotor_transits(ptr(traj_v), ptr(off), ntracks, ptr(alt_v), ptr(info), c['shape'][0], c['shape'][1], ptr(xy),
                               ptr(reach), ptr(hub), ptr(axis), ref.MM, nturb, ptr(bin_start), ptr(bin_items), ptr(hits),
                               ptr(transits), None)
    assert rc == 0, L.ssrs_last_error()
    if L.emu_launches() > before:
        mask_words, cnt = lds_words(c['shape'], nturb)
        asked = L.emu_lds_bytes()
        assert asked == 4 * (mask_words + 2 * cnt) <= 4 * LDS_WORDS
        behind = np.ctypeslib.as_array(L.emu_lds(), shape=(16384,))[asked // 4:]
        assert (behind == 0xA5A5A5A5).all(), 'the kernel wrote past the dynamic LDS it asked for'
    return hits, transits


def check(res, hits, transits):
    assert np.array_equal(hits, res['bitmap'])
    assert np.array_equal(transits.astype(np.int64), res['transits'])


@pytest.mark.parametrize('c', ref.DEVICE_CASES, ids=ref.DEVICE_IDS)
def test_emulated_case(emu, c):
    hits, transits = call(emu, c)
    check(ref.expected(c['name']), hits, transits)


@pytest.mark.parametrize('name', ['planted', 'pingpong', 'cuts'])
def test_emulated_every_placement(emu, name):
    """Both buffers at the three misaligned placements, and the point-by-point path with `alt` alone off the boundary."""
    c = ref.case(name)
    for shift, alt_shift in ((1, 1), (2, 2), (3, 3), (0, 1), (0, 0)):
        hits, transits = call(emu, c, shift=shift, alt_shift=alt_shift)
        check(ref.expected(name), hits, transits)


def test_emulated_accumulation(emu):
    """Calls over disjoint track ranges into one `transits` and the rows of one bitmap equal one call, and what both held
    before is kept."""
    c = ref.case('planted')
    res = ref.expected('planted')
    _, _, offsets = ref.flat(c)
    off = offsets[1:]
    ntracks, nturb = off.size - 1, len(c['reach'])
    hits = np.full((ntracks, 3), 1 << 30, dtype=np.uint32)                 # (bit 30, 62 and 94: the last is no turbine)
    transits = np.full((nturb, 2), 7, dtype=np.uint64)
    for lo, hi in ((0, 9), (9, 10), (10, 12), (12, 200), (200, ntracks)):
        call(emu, c, off=off[lo:hi + 1], hits=hits[lo:hi], transits=transits)
    assert np.array_equal(hits, res['bitmap'] | np.uint32(1 << 30))
    assert np.array_equal(transits.astype(np.int64) - 7, res['transits'])


@pytest.mark.parametrize('nturb', [7679, 7680, 7681, 8192])
def test_emulated_lds_boundary(emu, nturb):
    """Either side of the LDS rule: 7679 turbines keep the mask, 7680 fill the 60 KB with counters, from 7681 on the
    hand-overs of the last ones go to global memory."""
    c = ref.many_turbines(nturb)
    assert lds_words(c['shape'], nturb) == ((1, nturb) if nturb < 7680 else (0, 7680))
    res = ref.compute(c)
    assert res['transits'][nturb - 1].sum() > 0 and (nturb < 7681 or res['transits'][7680].sum() > 0)
    hits, transits = call(emu, c)
    check(res, hits, transits)


def test_emulated_cull_contract(emu):
    """A list that omits a turbine loses its transits; one that names it twice counts them twice."""
    c = ref.case('planted')
    res = ref.expected('planted')
    assert res['transits'][ref.A].sum() > 0
    hits, transits = call(emu, c, bins=ref.edit_bins(ref.bins(c), ref.A, 0))
    want = res['transits'].copy()
    want[ref.A] = 0
    assert np.array_equal(transits.astype(np.int64), want)
    hits, transits = call(emu, c, bins=ref.edit_bins(ref.bins(c), ref.A, 2))
    want = res['transits'].copy()
    want[ref.A] *= 2
    assert np.array_equal(transits.astype(np.int64), want) and np.array_equal(hits, res['bitmap'])


def test_emulated_nothing_to_do_touches_nothing(emu):
    c = ref.case('planted')
    _, _, offsets = ref.flat(c)
    hits = np.full((3, 3), 9, dtype=np.uint32)
    transits = np.full((len(c['reach']), 2), 9, dtype=np.uint64)
    before = emu.emu_launches()
    call(emu, c, off=np.array([5], dtype=np.int64), hits=hits[:0], transits=transits)
    call(emu, c, off=np.array([5, 5, 5, 5], dtype=np.int64), hits=hits, transits=transits)
    assert emu.emu_launches() == before and (hits == 9).all() and (transits == 9).all()
