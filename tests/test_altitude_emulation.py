"""K14 without a GPU: ssrs_amd/csrc/altitude.hip compiled with g++ against tests/hip_host_stub and run on the CPU, as
test_occupancy_emulation.py does for K13.  The kernels cooperate through __shared__ and __syncthreads() only (no
cross-lane builtin), so their own code runs here as it stands: the operator and its composition, the lane runs, the LDS
scan of a block, the tile operators and the one-block scan of them, the carries, the two binary searches and the walk over
empty tracks, the aligned and the point-by-point loads and stores, the LDS slots of the per-track outputs and the tracks
past them, the merged histogram atomics (the threads of a block are OS threads) -- on the cases of tests/altitude_ref.py,
which tests/test_gpu_altitude.py runs on the device.  What it does not cover: the device's own arithmetic (rint and the
f64 product of ssrs_altitude_cellinfo are the host's here), blocks that run at the same time (they run one after another),
and speed."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import altitude_ref as ref

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
# what these kernels use beyond the stub: the vector types, atomics (the threads of a block are OS threads) and the copies;
# launches and blocks are counted
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
template <class T> inline T atomicMin(T *p, T v)
{ T old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old; }
template <class T> inline T atomicMax(T *p, T v)
{ T old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > old && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  return old; }
constexpr int hipMemcpyDeviceToHost = 2;
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
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
    work = tmp_path_factory.mktemp('altitude_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    (work / 'altitude_emu_extra.h').write_text(EXTRA_H)
    lib = work / 'libaltitude_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-include', str(work / 'altitude_emu_extra.h'),
                    '-x', 'c++', os.path.join(csrc, 'altitude.hip'), str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.emu_launches.restype = L.emu_blocks.restype = C.c_longlong
    L.ssrs_track_altitude_workspace_bytes.restype = C.c_size_t
    L.ssrs_track_altitude_workspace_bytes.argtypes = [C.c_int64]
    L.ssrs_track_altitude.argtypes = _native.ALTITUDE_ARGTYPES
    L.ssrs_altitude_cellinfo.argtypes = _native.ALTITUDE_CELLINFO_ARGTYPES
    L.params = _native.SsrsAltitudeParams
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


WANT_ALL = ('alt', 'band_hist', 'traj_band', 'in_band', 'h_min', 'h_max')


def run(L, c, off=None, want=WANT_ALL, band_hist=None, per_track=None):
    """One call on a case.  off: the offsets it gets (default: all tracks).  Returns (the outputs asked for -- per-point
    ones as the whole buffer without the lead points --, launches, blocks); what lies around the per-point outputs must
    be untouched."""
    traj, offsets = ref.flat(c)
    off = np.ascontiguousarray(offsets[1:] if off is None else off)
    ntracks = off.size - 1
    owner, view = place(traj, c['shift'], 3)
    n = traj.shape[0]
    alt_owner, alt = place(np.full(n, 123456789, dtype=np.int32), c['shift'], 123456789)
    tb_owner, tb = place(np.full((n, 2), 77, dtype=np.int16), c['shift'], 77)
    if band_hist is None:
        band_hist = np.zeros(c['shape'], dtype=np.uint32)
    if per_track is None:
        per_track = {k: np.full(ntracks, 55, dtype=np.int32) for k in ('in_band', 'h_min', 'h_max')}
    nbytes = L.ssrs_track_altitude_workspace_bytes(int(off[-1] - off[0]))
    ws = np.full(nbytes // 8 + 2, -1, dtype=np.int64)
    ws16 = ws[(-ws.ctypes.data % 16) // 8:]
    info = ref.packed(c)
    p = L.params(*c['params'])
    before = L.emu_launches(), L.emu_blocks()
    rc = L.ssrs_track_altitude(ptr(view), ptr(off), ntracks, ptr(info), c['shape'][0], c['shape'][1], C.byref(p),
                               ptr(alt) if 'alt' in want else None, ptr(band_hist) if 'band_hist' in want else None,
                               ptr(tb) if 'traj_band' in want else None,
                               *(ptr(per_track[k]) if k in want else None for k in ('in_band', 'h_min', 'h_max')),
                               ptr(ws16), nbytes, None)
    assert rc == 0, L.ssrs_last_error()
    lo, hi = int(off[0]), int(off[-1])
    # nothing outside the chunk's points is written: not the neighbours' points, not the padding of the buffers
    inner = np.zeros(n, dtype=bool)
    inner[lo:hi] = True
    assert (alt[~inner] == 123456789).all() and (tb[~inner] == 77).all()
    alt_view, tb_view = alt[lo:hi].copy(), tb[lo:hi].copy()
    alt[:], tb[:] = 123456789, 77
    assert (alt_owner == 123456789).all() and (tb_owner == 77).all() and (owner[:4] == 3).all()
    got = dict(alt=alt_view, traj_band=tb_view, band_hist=band_hist, **per_track)
    return {k: got[k] for k in want}, L.emu_launches() - before[0], L.emu_blocks() - before[1]


@pytest.mark.parametrize('c', ref.CASES, ids=ref.CASE_IDS)
def test_emulated_case(emu, c):
    got, launches, blocks = run(emu, c)
    points = sum(len(t) for t in c['tracks'])
    if points == 0:
        assert launches == 0
        assert (got['in_band'] == 55).all()               # (no points: nothing is touched)
        return
    ref.check(c['name'], got)
    # three launches: a block per tile, one block, a block per tile (a chunk that does not start on a 16-byte boundary of
    # the buffer may take one tile more)
    tiles = -(-points // ref.TILE)
    assert launches == 3 and blocks in (2 * tiles + 1, 2 * tiles + 3)


@pytest.mark.parametrize('want', [(), ('alt',), ('band_hist',), ('traj_band',), ('in_band',), ('h_min',), ('h_max',),
                                  ('alt', 'traj_band'), ('band_hist', 'in_band')], ids=lambda w: '+'.join(w) or 'none')
def test_emulated_optional_outputs(emu, want):
    for name in ('lead_2_shift_1', 'lead_1_shift_0'):
        got, launches, _ = run(emu, ref.case(name), want=want)
        assert launches == 3
        ref.check(name, got)


def test_emulated_accumulation(emu):
    """Two calls into one band_hist on disjoint track ranges equal one call on the union, and what the raster held
    before is kept; the per-track vectors of each call are its own tracks'."""
    name = 'short_300'
    c = ref.case(name)
    _, off = ref.flat(c)
    off = off[1:]
    pattern = (np.arange(ref.SHAPE[0] * ref.SHAPE[1], dtype=np.uint32).reshape(ref.SHAPE) * 2654435761) | 1
    hist = pattern.copy()
    a, _, _ = run(emu, c, off=off[:121], want=('band_hist', 'in_band', 'h_min', 'h_max'), band_hist=hist)
    b, _, _ = run(emu, c, off=off[120:], want=('band_hist', 'in_band', 'h_min', 'h_max'), band_hist=hist)
    got = {k: np.concatenate([a[k], b[k]]) for k in ('in_band', 'h_min', 'h_max')}
    ref.check(name, dict(got, band_hist=hist), before=pattern)
    run(emu, c, want=('band_hist',), band_hist=hist)             # once more: everything twice
    assert np.array_equal(hist - pattern, 2 * ref.expected(name)['band_hist'])


def test_emulated_nothing_to_do_touches_nothing(emu):
    c = dict(ref.case('jumps'), tracks=[], lead=0, shift=0)
    traj = np.zeros((4, 2), dtype=np.int16)
    hist = np.full(ref.SHAPE, 9, dtype=np.uint32)
    vec = np.full(3, 9, dtype=np.int32)
    alt = np.full(4, 9, dtype=np.int32)
    ws = np.zeros(64, dtype=np.int64)
    p = emu.params(*ref.DEFAULT)
    before = emu.emu_launches()
    for off in (np.array([2], dtype=np.int64), np.array([2, 2, 2, 2], dtype=np.int64)):        # ntracks == 0; no points
        rc = emu.ssrs_track_altitude(ptr(traj), ptr(off), off.size - 1, ptr(ref.packed(c)), ref.SHAPE[0], ref.SHAPE[1],
                                     C.byref(p), ptr(alt), ptr(hist), None, ptr(vec), ptr(vec), ptr(vec), ptr(ws), 256, None)
        assert rc == 0, emu.ssrs_last_error()
    assert emu.emu_launches() == before and (hist == 9).all() and (vec == 9).all() and (alt == 9).all()


def test_emulated_refusals(emu):
    rows, cols = ref.SHAPE
    traj = np.zeros((16, 2), dtype=np.int16)
    off = np.array([0, 4], dtype=np.int64)
    hist = np.zeros((rows, cols), dtype=np.uint32)
    info = np.zeros((rows, cols, 2), dtype=np.int32)
    tb = np.zeros((16, 2), dtype=np.int16)
    ws = np.zeros(64, dtype=np.int64)
    ws = ws[(-ws.ctypes.data % 16) // 8:]
    assert emu.ssrs_track_altitude_workspace_bytes(0) == 256 and emu.ssrs_track_altitude_workspace_bytes(-1) == 0
    for n in (1, 4096, 4097, 10 ** 8):
        assert emu.ssrs_track_altitude_workspace_bytes(n) == -(-(n // ref.TILE + 2) * 24 // 256) * 256
    good = dict(traj=ptr(traj), off=ptr(off), ntracks=1, info=ptr(info), rows=rows, cols=cols, params=ref.DEFAULT,
                hist=ptr(hist), tb=ptr(tb), ws=ptr(ws), nbytes=256)

    def call(**kw):
        a = dict(good, **kw)
        p = None if a['params'] is None else C.byref(emu.params(*a['params']))
        return emu.ssrs_track_altitude(a['traj'], a['off'], a['ntracks'], a['info'], a['rows'], a['cols'], p, None, a['hist'],
                                       a['tb'], None, None, None, a['ws'], a['nbytes'], None)

    def refused(text, **kw):
        before = emu.emu_launches()
        rc = call(**kw)
        msg = emu.ssrs_last_error()
        assert rc == SSRS_ERR_INVALID and text in msg and b'ssrs_track_altitude' in msg, (rc, msg)
        assert emu.emu_launches() == before and not hist.any() and not tb.any()

    for name in ('traj', 'off', 'info', 'params', 'ws'):
        refused(b'NULL', **{name: None})
    for kw in (dict(rows=0), dict(rows=32768), dict(cols=0), dict(cols=32768)):
        refused(b'raster', **kw)
    for ntracks in (-1, 2 ** 31):
        refused(b'ntracks', ntracks=ntracks)
    refused(b'traj must be 4-byte aligned', traj=C.c_void_p(traj.ctypes.data + 2))
    refused(b'traj_band must be 4-byte aligned', tb=C.c_void_p(tb.ctypes.data + 2))
    refused(b'cellinfo must be 8-byte aligned', info=C.c_void_p(info.ctypes.data + 4))
    refused(b'workspace must be 16-byte aligned', ws=C.c_void_p(ws.ctypes.data + 8))
    refused(b'floor', params=(0, 5, 4, 0, 1))
    refused(b'band_lo', params=(0, 4, 5, 2, 1))
    refused(b'workspace', nbytes=255)
    long_off = np.array([0, 16 * ref.TILE], dtype=np.int64)                       # 18 tiles' worth: 432 bytes -> 512
    refused(b'workspace', off=ptr(long_off), nbytes=256)
    refused(b'negative', off=ptr(np.array([-1, 4], dtype=np.int64)))
    refused(b'descends', off=ptr(np.array([4, 0], dtype=np.int64)))


def test_emulated_good_call_after_refusals(emu):
    """The arguments the refusals vary are a valid call: four points at (0, 0), start height in the band."""
    rows, cols = ref.SHAPE
    traj = np.zeros((16, 2), dtype=np.int16)
    off = np.array([0, 4], dtype=np.int64)
    hist = np.zeros((rows, cols), dtype=np.uint32)
    info = np.zeros((rows, cols, 2), dtype=np.int32)
    ws = np.zeros(64, dtype=np.int64)
    ws = ws[(-ws.ctypes.data % 16) // 8:]
    p = emu.params(*ref.DEFAULT)
    rc = emu.ssrs_track_altitude(ptr(traj), ptr(off), 1, ptr(info), rows, cols, C.byref(p), None, ptr(hist), None, None, None,
                                 None, ptr(ws), 256, None)
    assert rc == 0 and hist[0, 0] == 4 and hist.sum() == 4


@pytest.mark.parametrize('dtypes', [(np.float32, np.float32), (np.float64, np.float32), (np.float32, np.float64),
                                    (np.float64, np.float64)], ids=lambda d: f'{d[0].__name__}-{d[1].__name__}')
def test_emulated_cellinfo(emu, dtypes):
    """ssrs_altitude_cellinfo against numpy: NaN updraft (read as 0), NaN elevation (the sentinel), exact .5 ties (to even,
    both signs), values that clip, infinities."""
    rows, cols = 7, 9
    rng = np.random.default_rng(3)
    w = rng.normal(0.5, 2., (rows, cols))
    z = rng.uniform(-50., 3000., (rows, cols))
    resolution, airspeed, sink = 100., 16., 0.75            # scale = 6250: (w - sink) * scale ties at multiples of 0.00008
    w[0, :6] = sink + np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5]) / 6250.
    w[1, :4] = (np.nan, 1e9, -1e9, np.inf)
    w[1, 4] = -np.inf
    w[2, :3] = (sink + 2. ** 26 / 6250., sink - 2. ** 26 / 6250., sink + (2. ** 26 - 1) / 6250.)
    z[3, :6] = (0.0005, 0.0015, 0.0025, -0.0005, -0.0015, 1234.5675)
    z[4, :5] = (np.nan, 2e6, -2e6, np.inf, -np.inf)
    z[5, :2] = (2. ** 30 / 1000., -(2. ** 30) / 1000.)
    w, z = np.ascontiguousarray(w.astype(dtypes[0])), np.ascontiguousarray(z.astype(dtypes[1]))
    climb, elev = ref.cellinfo(w, z, resolution, airspeed, sink)
    assert climb[1, 0] == np.rint(-sink * 6250.) and climb[1, 1] == 2 ** 26 and climb[1, 2] == -2 ** 26
    assert elev[4, 0] == ref.SENTINEL and elev[4, 1] == 2 ** 30 and elev[4, 2] == -2 ** 30
    if dtypes[0] is np.float64:
        assert climb[0, :6].tolist() == [0, 2, 2, 0, -2, -2]
    out = np.full((rows, cols, 2), 99, dtype=np.int32)
    before = emu.emu_launches()
    rc = emu.ssrs_altitude_cellinfo(ptr(w), int(dtypes[0] is np.float64), ptr(z), int(dtypes[1] is np.float64), rows, cols,
                                    sink, 1000. * resolution / airspeed, ptr(out), None)
    assert rc == 0 and emu.emu_launches() == before + 1
    assert np.array_equal(out[..., 0], climb) and np.array_equal(out[..., 1], elev)
    for kw in (dict(w=None), dict(z=None), dict(out=None), dict(rows=0), dict(cols=32768), dict(wt=2), dict(sink=np.nan)):
        a = dict(dict(w=ptr(w), z=ptr(z), out=ptr(out), rows=rows, cols=cols, wt=0, sink=sink), **kw)
        rc = emu.ssrs_altitude_cellinfo(a['w'], a['wt'], a['z'], 0, a['rows'], a['cols'], a['sink'], 1., a['out'], None)
        assert rc == SSRS_ERR_INVALID and b'ssrs_altitude_cellinfo' in emu.ssrs_last_error(), kw
