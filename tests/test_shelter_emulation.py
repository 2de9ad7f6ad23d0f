"""K9 without a GPU: ssrs_amd/csrc/shelter.hip compiled with g++ against tests/hip_host_stub (one OS thread per GPU
thread, a barrier for __syncthreads) and run on the CPU, judged by tests/shelter_ref.py with the bounds of
test_gpu_shelter.py.  This exercises the kernel's own logic -- tile and halo staging, the in-tile test, the sample
tables and their 256-sample rounds, re-staging between cases of a batch, both paths -- on every machine; the device's
arithmetic is the gpu-marked tests' business."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import shelter_ref as ref
from raster_checks import SLOPE_TOL, check_orograph_cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = (0., 45., 90., 180., 237.3, 270., 315., 359.9)
RASTER_TOL = dict(rtol=1e-11, atol=1e-12)
ERR_CPP = '''#include "common.h"
namespace ssrs {
char *error_buffer() { static thread_local char buf[512] = ""; return buf; }
int set_error(int code, const char *fmt, ...)
{ va_list ap; va_start(ap, fmt); vsnprintf(error_buffer(), 512, fmt, ap); va_end(ap); return code; }
}
extern "C" const char *ssrs_last_error(void) { return ssrs::error_buffer(); }
'''


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    from ssrs_amd import _native as nat
    work = tmp_path_factory.mktemp('shelter_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    lib = work / 'libshelter_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-fPIC', '-shared', '-pthread',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-x', 'c++',
                    os.path.join(csrc, 'shelter.hip'), str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.ssrs_shelter_sx.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                  C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ssrs_updraft_sheltered.argtypes = [C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 8 + \
        [C.c_int, C.POINTER(nat.SsrsShelterParams), C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
         C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def wind_args(wdirn, axes):
    """(B, ur, uc, raster) as layers._wind_direction_args makes them, on the host."""
    if np.ndim(wdirn) <= 1:
        ur, uc = ref.ray_step(np.atleast_1d(np.asarray(wdirn, dtype=np.float64)), axes)
        return ur.size, np.ascontiguousarray(ur), np.ascontiguousarray(uc), None
    wd = np.ascontiguousarray(wdirn if wdirn.ndim == 3 else wdirn[None])
    return wd.shape[0], None, None, wd


def emu_sx(L, z, res, wdirn, dmax, axes, path='auto'):
    from ssrs_amd import _native as nat
    z = np.ascontiguousarray(z)
    rows, cols = z.shape
    batch, ur, uc, wd = wind_args(wdirn, axes)
    tan, deg = np.empty((batch, rows, cols)), np.empty((batch, rows, cols))
    rc = L.ssrs_shelter_sx(ptr(z), int(z.dtype == np.float64), res, ptr(ur), ptr(uc), ptr(wd), dmax, nat.SSRS_RAY_AXES[axes],
                           nat.SSRS_SHELTER_PATH[path], ptr(tan), ptr(deg), rows, cols, batch, None)
    assert rc == 0, L.ssrs_last_error()
    return tan, deg


def emu_updraft(L, z, res, wspeed, wdirn, dmax=500., axes='row_east', path='auto', coeffs=ref.DEFAULT_COEFFS, height=80.):
    from ssrs_amd import _native as nat
    z = np.ascontiguousarray(z)
    rows, cols = z.shape
    batch, ur, uc, wd = wind_args(wdirn, axes)
    ws0 = wd0 = ws = None
    if wd is None:
        ws0 = np.atleast_1d(np.asarray(wspeed, dtype=np.float64))
        wd0 = np.atleast_1d(np.asarray(wdirn, dtype=np.float64))
    else:
        ws = np.ascontiguousarray(wspeed if wspeed.ndim == 3 else wspeed[None])
    prm = nat.SsrsShelterParams(dmax, nat.SSRS_RAY_AXES[axes], nat.SSRS_SHELTER_PATH[path], height, (C.c_double * 7)(*coeffs))
    oro, use = np.empty((batch, rows, cols), np.float32), np.empty((batch, rows, cols))
    rc = L.ssrs_updraft_sheltered(ptr(z), 1, res, ptr(ur), ptr(uc), ptr(ws0), ptr(wd0), ptr(ws), ptr(wd), None, None, 1,
                                  C.byref(prm), 0., 0.75, ptr(oro), ptr(use), None, rows, cols, batch, None)
    assert rc == 0, L.ssrs_last_error()
    return oro, use


def make_dem(shape, hole=True):
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    z = 1500. + 180. * np.sin(r / 7.3) * np.cos(c / 9.1) + 90. * np.sin((r + 2. * c) / 5.7) + 2.5 * r - 1.5 * c
    if hole:
        z[shape[0] // 2 - 1:shape[0] // 2 + 2, shape[1] // 3:shape[1] // 3 + 3] = np.nan
    return z


def wind_raster(shape):
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return 8. + 3. * np.sin(c / 17.) * np.cos(r / 13.), 200. + 110. * np.sin(c / 7. + r / 9.)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize('shape, K', [((20, 23), 5), ((20, 23), 50), ((37, 70), 5)])      # (37, 70): 2 x 2 tiles
def test_emulated_kernel_uniform_wind_bit_identical(emu, shape, K):
    z, res = make_dem(shape), 10.
    for axes in ('row_north', 'row_east'):
        tan, deg = emu_sx(emu, z, res, DIRECTIONS, K * res + 5., axes)
        for b, wdirn in enumerate(DIRECTIONS):
            want = ref.tan_sx(z, res, wdirn, dmax=K * res + 5., ray_axes=axes)
            assert same_bits(tan[b], want), (axes, wdirn)
            np.testing.assert_allclose(deg[b], ref.sx_degrees(want), **SLOPE_TOL)


def test_emulated_kernel_paths_rounds_and_per_cell_wind(emu):
    shape, res = (37, 70), 10.
    z = make_dem(shape)
    ws, wd = wind_raster(shape)
    assert wd.max() - wd.min() > 180.
    for wdirn in (list(DIRECTIONS), wd):
        a = emu_sx(emu, z, res, wdirn, 55., 'row_east', 'lds')
        b = emu_sx(emu, z, res, wdirn, 55., 'row_east', 'global')
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    np.testing.assert_allclose(a[0][0], ref.tan_sx(z, res, wd, dmax=55., ray_axes='row_east'), **RASTER_TOL)
    # K = 300 on a small raster: the global path, and two rounds of the 256-sample table
    z = make_dem((20, 23))
    tan, _ = emu_sx(emu, z, 1., [237.3, 270.], 300.5, 'row_north')
    for b, wdirn in enumerate((237.3, 270.)):
        assert same_bits(tan[b], ref.tan_sx(z, 1., wdirn, dmax=300.5, ray_axes='row_north'))
    _, wd = wind_raster((20, 23))
    tan, _ = emu_sx(emu, z, 1., wd, 300.5, 'row_east')
    np.testing.assert_allclose(tan[0], ref.tan_sx(z, 1., wd, dmax=300.5, ray_axes='row_east'), **RASTER_TOL)
    # an LDS path that cannot hold the halo is refused
    from ssrs_amd import _native as nat
    out = np.empty((1, 20, 23))
    one = np.ones(1)
    rc = emu.ssrs_shelter_sx(ptr(z), 1, 1., ptr(one), ptr(one), None, 300.5, 1, nat.SSRS_SHELTER_PATH['lds'], ptr(out), None,
                             20, 23, 1, None)
    assert rc == nat.SSRS_ERR_INVALID and b'does not fit' in emu.ssrs_last_error()


def test_emulated_kernel_updraft(emu):
    """Neutral coefficients give the original raster, the defaults the reference's adjusted one; a batch over three
    quadrants (the tile is staged again between them) equals three single calls."""
    from oracle import ssrs_oracle as orc
    shape, res = (37, 70), 100.
    z = make_dem(shape)
    slope, aspect = orc.compute_slope_degrees(z, res), orc.compute_aspect_degrees(z, res)
    speeds, dirs = [10., 6., 12.], [45., 237.3, 315.]
    oro, use = emu_updraft(emu, z, res, speeds, dirs)
    plain, _ = emu_updraft(emu, z, res, speeds, dirs, coeffs=ref.NEUTRAL_COEFFS)
    signal = 0
    for b, (s, d) in enumerate(zip(speeds, dirs)):
        w0 = orc.compute_orographic_updraft(s, d, slope, aspect)
        check_orograph_cells(plain[b], w0, s, f'neutral {d:g}')
        want = ref.adjust(w0, ref.tan_sx(z, res, d, dmax=500., ray_axes='row_east'), slope)
        signal += check_orograph_cells(oro[b], want, s, f'improved {d:g}')['signal']
        np.testing.assert_allclose(use[b], orc.get_above_threshold_speed(oro[b], 0.75), rtol=1e-12, atol=1e-15)
        single, _ = emu_updraft(emu, z, res, s, d)
        assert np.array_equal(single[0].view(np.int32), oro[b].view(np.int32))
    assert signal > 0
    ws, wd = wind_raster(shape)
    oro, _ = emu_updraft(emu, z, res, ws, wd)
    w0 = orc.compute_orographic_updraft(ws, wd, slope, aspect)
    want = ref.adjust(w0, ref.tan_sx(z, res, wd, dmax=500., ray_axes='row_east'), slope)
    assert check_orograph_cells(oro[0], want, float(ws.max()), 'per-cell wind')['signal'] > 0
