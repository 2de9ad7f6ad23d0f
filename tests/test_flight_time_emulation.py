"""K16 without a GPU: ssrs_amd/csrc/flight_time.hip compiled with g++ against tests/hip_host_stub and run on the CPU, as
test_altitude_emulation.py does for K14.  The kernel cooperates through __shared__ and __syncthreads() only (no cross-lane
builtin), so its own code runs here as it stands: the move's integer arithmetic with its corrected f64 estimates, the lane
runs and the point behind them, the two binary searches and the walk over empty tracks, the aligned and the point-by-point
loads and stores, the register cache, its evictions and the block's table of cells in LDS, the LDS slots of the per-track
sums and the tracks past them (the threads of a block are OS threads) -- on the cases of tests/flight_time_ref.py, which
tests/test_gpu_flight_time.py runs on the device.  What it does not cover: the device's own arithmetic (sqrt, the f64 division, sin and cos are the host's
here), blocks that run at the same time (they run one after another), and speed."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import flight_time_ref as ref

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
# what the kernels use beyond the stub: the vector types, the atomic add and compare-and-swap (the threads of a block are OS
# threads), the copies and the memset; launches and blocks are counted
EXTRA_H = '''#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) int4 { int x, y, z, w; };
struct alignas(8) int2 { int x, y; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
inline int2 make_int2(int x, int y) { return int2{x, y}; }
template <class T> inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <class T> inline T atomicCAS(T *p, T expected, T v)
{ __atomic_compare_exchange_n(p, &expected, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED); return expected; }
constexpr int hipMemcpyDeviceToHost = 2;
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
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
    work = tmp_path_factory.mktemp('flight_time_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'flight_time_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'libflight_time_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include',
                    str(work / 'flight_time_emu_extra.h'), '-x', 'c++', os.path.join(csrc, 'flight_time.hip'),
                    str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_blocks.restype = C.c_longlong
    L.ssrs_track_time.argtypes = _native.TRACK_TIME_ARGTYPES
    L.ssrs_flight_windinfo.argtypes = _native.FLIGHT_WINDINFO_ARGTYPES
    L.params = _native.SsrsFlightTimeParams
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def place(values, shift, fill):
    """A buffer of values.shape[0] + 12 elements of 4 bytes (rows of `values`' dtype) filled with `fill`, and its view
    that starts `shift` elements past a 16-byte boundary and holds `values`.  Returns (the owner, the view)."""
    raw = np.empty((values.shape[0] + 12,) + values.shape[1:], dtype=values.dtype)
    raw[:] = fill
    assert raw.ctypes.data % 4 == 0 and raw[0].nbytes == 4
    start = (-raw.ctypes.data % 16) // 4 + 4 + shift
    view = raw[start:start + values.shape[0]]
    view[:] = values
    assert view.shape[0] == 0 or (view.ctypes.data % 16) == 4 * (shift % 4)
    return raw, view


WANT_ALL = ref.KEYS
DT_FILL = 123456789


def run(L, c, off=None, want=WANT_ALL, hists=None, uniform=False, use_masked=True):
    """One call on a case.  off: the offsets it gets (default: all tracks).  hists: dict of the two rasters to add to.
    uniform: NULL raster and the case's pair.  Returns (the outputs asked for -- dt as the chunk's points --, launches,
    blocks); what lies around dt must be untouched."""
    traj, offsets, masked = ref.points(c)
    off = np.ascontiguousarray(offsets[1:] if off is None else off)
    ntracks = off.size - 1
    owner, view = place(traj, c['shift'], 3)
    m_owner, m_view = place(masked, c['shift'], 3)
    n = traj.shape[0]
    dt_owner, dt = place(np.full(n, DT_FILL, dtype=np.int32), c['shift'], DT_FILL)
    hists = hists or {k: np.zeros(c['shape'], dtype=np.uint64) for k in ('time_hist', 'band_time_hist')}
    times = np.full((ntracks, 2), 55, dtype=np.int64)
    info = None if uniform else ref.packed(c)
    pair = c['uniform'] if uniform else (12345, -54321)            # (ignored with a raster)
    p = L.params(*c['params'])
    before = L.emu_launches(), L.emu_blocks()
    rc = L.ssrs_track_time(ptr(view), ptr(off), ntracks, ptr(m_view) if use_masked else None, ptr(info), pair[0], pair[1],
                           c['shape'][0], c['shape'][1], C.byref(p),
                           ptr(hists['time_hist']) if 'time_hist' in want else None,
                           ptr(hists['band_time_hist']) if 'band_time_hist' in want else None,
                           ptr(times) if 'times' in want else None, ptr(dt) if 'dt' in want else None, None)
    assert rc == 0, L.ssrs_last_error()
    lo, hi = int(off[0]), int(off[-1])
    inner = np.zeros(n, dtype=bool)
    inner[lo:hi] = True
    assert (dt[~inner] == DT_FILL).all()                   # nothing outside the chunk's points is written
    dt_view = dt[lo:hi].copy()
    dt[:] = DT_FILL
    assert (dt_owner == DT_FILL).all() and (owner[:4] == 3).all() and (m_owner[:4] == 3).all()
    got = dict(hists, times=times, dt=dt_view)
    return {k: got[k] for k in want}, L.emu_launches() - before[0], L.emu_blocks() - before[1]


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_emulated_case(emu, c):
    got, launches, blocks = run(emu, c)
    npoints = sum(len(t) for t in c['tracks'])
    if npoints == 0:
        assert launches == 0 and not got['times'].any()    # (no points: the per-track rows alone are written)
        return
    ref.check(c['name'], got)
    # one launch, a block per tile (a chunk that does not start on a 16-byte boundary of the buffer may take one more)
    tiles = -(-npoints // ref.TILE)
    assert launches == 1 and blocks in (tiles, tiles + 1)
    if c['uniform'] is not None:
        ref.check(c['name'], run(emu, c, uniform=True)[0])


@pytest.mark.parametrize('want', [(), ('time_hist',), ('band_time_hist',), ('times',), ('dt',), ('time_hist', 'times'),
                                  ('band_time_hist', 'dt')], ids=lambda w: '+'.join(w) or 'none')
def test_emulated_optional_outputs(emu, want):
    for name in ('lead_2_shift_1', 'lead_1_shift_0', 'short_300'):
        got, launches, _ = run(emu, ref.case(name), want=want)
        assert launches == 1
        ref.check(name, got)


def test_emulated_without_masked(emu):
    """No masked copy: no point is in the zone, the rest is unchanged."""
    name = 'lengths'
    got, _, _ = run(emu, ref.case(name), want=('time_hist', 'times', 'dt'), use_masked=False)
    want = ref.expected(name)
    assert np.array_equal(got['time_hist'], want['time_hist']) and np.array_equal(got['dt'], want['dt'])
    assert np.array_equal(got['times'][:, 0], want['times'][:, 0]) and not got['times'][:, 1].any()


def test_emulated_accumulation(emu):
    """Two calls into one pair of rasters on disjoint track ranges equal one call on the union, and what the rasters
    held before is kept; the per-track rows of each call are its own tracks'.  Once more: everything twice."""
    name = 'short_300'
    c = ref.case(name)
    off = ref.points(c)[1][1:]
    pattern = (np.arange(ref.SHAPE[0] * ref.SHAPE[1], dtype=np.uint64).reshape(ref.SHAPE) * np.uint64(0x9E3779B97F4A7C15)) | \
        np.uint64(1)
    hists = dict(time_hist=pattern.copy(), band_time_hist=pattern.copy() + np.uint64(5))
    before = {k: v.copy() for k, v in hists.items()}
    a, _, _ = run(emu, c, off=off[:121], want=('time_hist', 'band_time_hist', 'times'), hists=hists)
    b, _, _ = run(emu, c, off=off[120:], want=('time_hist', 'band_time_hist', 'times'), hists=hists)
    ref.check(name, dict(hists, times=np.concatenate([a['times'], b['times']])), before=before)
    run(emu, c, want=('time_hist', 'band_time_hist'), hists=hists)
    ref.check(name, hists, before=before, times=2)


def test_emulated_nothing_to_do(emu):
    traj = np.zeros((4, 2), dtype=np.int16)
    hist = np.full(ref.SHAPE, 9, dtype=np.uint64)
    times = np.full((3, 2), 9, dtype=np.int64)
    dt = np.full(4, 9, dtype=np.int32)
    p = emu.params(*ref.DEFAULT)
    before = emu.emu_launches()

    def call(off):
        rc = emu.ssrs_track_time(ptr(traj), ptr(off), off.size - 1, None, None, 0, 0, ref.SHAPE[0], ref.SHAPE[1], C.byref(p),
                                 ptr(hist), None, ptr(times), ptr(dt), None)
        assert rc == 0, emu.ssrs_last_error()
    call(np.array([2], dtype=np.int64))                                # ntracks == 0: nothing is touched
    assert (times == 9).all()
    call(np.array([2, 2, 2, 2], dtype=np.int64))                       # no points: the rows are zeroed
    assert emu.emu_launches() == before and (hist == 9).all() and (dt == 9).all() and not times.any()


def test_emulated_refusals(emu):
    rows, cols = ref.SHAPE
    traj = np.zeros((16, 2), dtype=np.int16)
    off = np.array([0, 4], dtype=np.int64)
    hist = np.zeros((rows, cols), dtype=np.uint64)
    info = np.zeros((rows, cols, 2), dtype=np.int32)
    dt = np.zeros(16, dtype=np.int32)
    good = dict(traj=ptr(traj), off=ptr(off), ntracks=1, masked=ptr(traj), info=ptr(info), pair=(0, 0), rows=rows, cols=cols,
                params=ref.DEFAULT, hist=ptr(hist), band=ptr(hist), dt=ptr(dt))

    def call(**kw):
        a = dict(good, **kw)
        p = None if a['params'] is None else C.byref(emu.params(*a['params']))
        return emu.ssrs_track_time(a['traj'], a['off'], a['ntracks'], a['masked'], a['info'], a['pair'][0], a['pair'][1],
                                   a['rows'], a['cols'], p, a['hist'], a['band'], None, a['dt'], None)

    def refused(text, **kw):
        before = emu.emu_launches()
        rc = call(**kw)
        msg = emu.ssrs_last_error()
        assert rc == SSRS_ERR_INVALID and text in msg and b'ssrs_track_time' in msg, (rc, msg)
        assert emu.emu_launches() == before and not hist.any() and not dt.any()

    for name in ('traj', 'off', 'params'):
        refused(b'NULL', **{name: None})
    for kw in (dict(rows=0), dict(rows=32768), dict(cols=0), dict(cols=32768)):
        refused(b'raster', **kw)
    for ntracks in (-1, 2 ** 31):
        refused(b'ntracks', ntracks=ntracks)
    refused(b'traj must be 4-byte aligned', traj=C.c_void_p(traj.ctypes.data + 2))
    refused(b'masked must be 4-byte aligned', masked=C.c_void_p(traj.ctypes.data + 2))
    refused(b'windinfo must be 8-byte aligned', info=C.c_void_p(info.ctypes.data + 4))
    refused(b'8-byte aligned', hist=C.c_void_p(hist.ctypes.data + 4))
    refused(b'dt must be 4-byte aligned', dt=C.c_void_p(dt.ctypes.data + 2))
    for params, text in (((0, 1, 10), b'va'), ((2 ** 20 + 1, 1, 10), b'va'), ((15, 0, 10), b'gmin'), ((15, 16, 10), b'gmin'),
                         ((15, 1, 0), b'res_mm'), ((15, 1, 10 ** 6 + 1), b'res_mm')):
        refused(text, params=params)
    refused(b'uniform wind', info=None, pair=(2 ** 20 + 1, 0))
    refused(b'uniform wind', info=None, pair=(0, -2 ** 20 - 1))
    refused(b'band_time_hist needs masked', masked=None)
    refused(b'negative', off=ptr(np.array([-1, 4], dtype=np.int64)))
    refused(b'descends', off=ptr(np.array([4, 0], dtype=np.int64)))
    assert call() == 0 and hist[0, 0] == 2 * 3 * 666_667 and dt.tolist()[:5] == [666_667] * 3 + [0, 0]    # both rasters are `hist`


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=lambda d: d.__name__)
@pytest.mark.parametrize('ray_axes', ['row_north', 'row_east'])
def test_emulated_windinfo(emu, dtype, ray_axes):
    """ssrs_flight_windinfo against numpy on the host's own sin and cos: NaN speed and direction (still air), values
    that clip, infinities."""
    rows, cols = 7, 9
    rng = np.random.default_rng(3)
    ws = rng.uniform(0., 40., (rows, cols))
    wd = rng.uniform(-360., 720., (rows, cols))
    ws[0, :5] = (np.nan, 5., np.nan, 2000., np.inf)
    wd[0, :5] = (10., np.nan, np.nan, 45., 45.)
    wd[1, :5] = (0., 90., 180., 270., 360.)
    wd[2, 0] = np.inf
    ws, wd = np.ascontiguousarray(ws.astype(dtype)), np.ascontiguousarray(wd.astype(dtype))
    wr, wc = ref.windinfo(ws, wd, ray_axes)
    assert (wr[0, :3] == 0).all() and (wc[0, :3] == 0).all() and wr[2, 0] == 0 and wc[2, 0] == 0
    assert wr[0, 3] == wc[0, 3] == wr[0, 4] == wc[0, 4] == -2 ** 20
    out = np.full((rows, cols, 2), 99, dtype=np.int32)
    before = emu.emu_launches()
    axes = {'row_north': 0, 'row_east': 1}[ray_axes]
    rc = emu.ssrs_flight_windinfo(ptr(ws), ptr(wd), int(dtype is np.float64), rows, cols, axes, ptr(out), None)
    assert rc == 0 and emu.emu_launches() == before + 1
    assert np.array_equal(out[..., 0], wr) and np.array_equal(out[..., 1], wc)
    for kw in (dict(ws=None), dict(wd=None), dict(out=None), dict(rows=0), dict(cols=32768), dict(t=2), dict(axes=2)):
        a = dict(dict(ws=ptr(ws), wd=ptr(wd), out=ptr(out), rows=rows, cols=cols, t=0, axes=axes), **kw)
        rc = emu.ssrs_flight_windinfo(a['ws'], a['wd'], a['t'], a['rows'], a['cols'], a['axes'], a['out'], None)
        assert rc == SSRS_ERR_INVALID and b'ssrs_flight_windinfo' in emu.ssrs_last_error(), kw
