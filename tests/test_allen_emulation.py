"""K12 without a GPU: ssrs_amd/csrc/allen_thermals.hip compiled with g++ against tests/hip_host_stub and run on the CPU, as
test_smooth_emulation.py does for K11.  This exercises the kernels' own logic -- the table, the staging of a tile's bins
and halo, the acceptance test against the staged region, the ring scan and its stop, the hand-over between the two, ties
across bin and tile borders, the overflow of the list -- on the cases of tests/allen_ref.py, which tests/test_gpu_allen.py
runs on the device."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import allen_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATHS = {'auto': 0, 'lds': 1, 'global': 2}
SSRS_ERR_INVALID = -1
ERR_CPP = '''#include "common.h"
namespace ssrs {
char *error_buffer() { static thread_local char buf[512] = ""; return buf; }
int set_error(int code, const char *fmt, ...)
{ va_list ap; va_start(ap, fmt); vsnprintf(error_buffer(), 512, fmt, ap); va_end(ap); return code; }
}
extern "C" const char *ssrs_last_error(void) { return ssrs::error_buffer(); }
'''
# what this kernel uses beyond the stub: atomics (the threads of a block are OS threads) and the copy of one int
EXTRA_H = '''#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline int atomicMax(int *p, int v)
{ int old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old; }
constexpr int hipMemcpyDeviceToHost = 2;
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
'''


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    from ssrs_amd import _native
    work = tmp_path_factory.mktemp('allen_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'allen_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'liballen_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-fPIC', '-shared', '-pthread',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include', str(work / 'allen_emu_extra.h'),
                    '-x', 'c++', os.path.join(csrc, 'allen_thermals.hip'), str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.ssrs_allen_workspace_bytes.restype = C.c_size_t
    L.ssrs_allen_workspace_bytes.argtypes = [C.c_int]
    L.ssrs_allen_thermal_field.argtypes = _native.ALLEN_FIELD_ARGTYPES
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emu_field(L, case, path='auto', out_dtype=np.float64, expect=0):
    """(field, nearest, table, cells that left the LDS path) of a case of allen_ref.CASES, or the refusal's message."""
    from ssrs_amd.thermals import allen_bins
    rows, cols = case['shape']
    n = case['xt'].size
    zzi, rbar, wtbar, we, below = ref.expected(case['name'])['scalars']
    start, items, bin_m, nbx, nby = allen_bins(case['xt'], case['yt'], case['shape'], case['res'])
    nbytes = L.ssrs_allen_workspace_bytes(n)
    assert nbytes == 256 + (n * 48 + 255) // 256 * 256
    ws = np.zeros(nbytes // 8, dtype=np.uint64)
    out = np.full((rows, cols), np.nan, out_dtype)
    near = np.full((rows, cols), -7, np.int32)
    tab = np.full((n, 6), np.nan)
    arrays = [np.ascontiguousarray(case[k], dtype=np.float64) for k in ('xt', 'yt', 'wgain', 'rgain')]
    rc = L.ssrs_allen_thermal_field(*(ptr(a) for a in arrays), n, ptr(start), ptr(items), bin_m, nbx, nby, rbar, wtbar, zzi,
                                    int(below), we, case['res'], rows, cols, PATHS[path], ptr(out),
                                    int(out_dtype == np.float64), ptr(near), ptr(tab), ptr(ws), nbytes, None)
    assert rc == expect, L.ssrs_last_error()
    return (out, near, tab, int(ws[0])) if rc == 0 else L.ssrs_last_error()


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('case', ref.CASES, ids=ref.CASE_IDS)
def test_emulated_field(emu, case):
    """Every case: the nearest updraft of every cell, the table's bits, the field within the bound, and the same bits on
    the LDS and the global path."""
    name = case['name']
    fld, near, tab, left = emu_field(emu, case, 'auto')
    ref.check_case(name, near, tab, fld)
    glob = emu_field(emu, case, 'global')
    assert glob[3] == 0
    assert all(same_bits(a, b) for a, b in zip((fld, near, tab), glob)), name
    if case['overflow']:
        assert left > 0                                                     # auto fell back ...
        msg = emu_field(emu, case, 'lds', expect=SSRS_ERR_INVALID)          # ... and the forced path is refused
        assert b'does not fit' in msg and b'ssrs_allen_thermal_field' in msg
    elif name != 'tiles':                                                   # (auto IS the LDS path when every list fits)
        lds = emu_field(emu, case, 'lds')
        assert all(same_bits(a, b) for a, b in zip((fld, near, tab), lds[:3])) and lds[3] == left, name
    if name in ('ragged', 'tiles'):
        assert left < fld.size // 2                                         # most cells are settled from the LDS list
    if name == 'clustered':
        assert left > fld.size // 2                                         # far cells cross many empty rings
    if name == 'ragged':                                                    # (on the device: 'tiles' as well)
        f32 = emu_field(emu, case, 'auto', np.float32)[0]
        assert same_bits(f32, fld.astype(np.float32))                       # the f64 value rounded once


def test_emulated_null_nearest_and_table(emu):
    case = ref.CASES[0]
    from ssrs_amd.thermals import allen_bins
    rows, cols = case['shape']
    n = case['xt'].size
    zzi, rbar, wtbar, we, below = ref.expected(case['name'])['scalars']
    start, items, bin_m, nbx, nby = allen_bins(case['xt'], case['yt'], case['shape'], case['res'])
    nbytes = emu.ssrs_allen_workspace_bytes(n)
    ws, out = np.zeros(nbytes // 8, dtype=np.uint64), np.full((rows, cols), np.nan)
    arrays = [np.ascontiguousarray(case[k]) for k in ('xt', 'yt', 'wgain', 'rgain')]
    rc = emu.ssrs_allen_thermal_field(*(ptr(a) for a in arrays), n, ptr(start), ptr(items), bin_m, nbx, nby, rbar, wtbar,
                                      zzi, int(below), we, case['res'], rows, cols, 0, ptr(out), 1, None, None, ptr(ws),
                                      nbytes, None)
    assert rc == 0, emu.ssrs_last_error()
    assert same_bits(out, emu_field(emu, case)[0])
