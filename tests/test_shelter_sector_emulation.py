"""The sector kernel of K9 without a GPU: ssrs_amd/csrc/shelter.hip compiled with g++ against tests/hip_host_stub and run on
the CPU, as test_shelter_emulation.py does for the single ray, judged by tests/shelter_sector_ref.py.  This exercises
k_shelter_sector's own logic -- the halo sized from the M steps of a case and its re-staging, the M K sample table and
its 256-entry rounds, the ray counter and the mean, the launches of a long batch, both paths and the fallback.  On the
CPU every T_m of a uniform wind is the reference's bit for bit (IEEE operations in a fixed order), but atan / tan are the
libm's against numpy's own, an ulp apart: Sx-bar is asked for within rtol 1e-11 / atol 1e-10 and T-bar within rtol 1e-11 /
atol 1e-12, the per-cell bounds of test_gpu_shelter.py, and bit for bit wherever the kernel is compared with itself."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import shelter_ref as ref
import shelter_sector_ref as sref
from raster_checks import check_orograph_cells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RASTER_TOL = dict(rtol=1e-11, atol=1e-12)
SX_TOL = dict(rtol=1e-11, atol=1e-10)
SHAPES = ((70, 45), (33, 65))            # more than one 64 x 32 and 32 x 32 tile in each direction, ragged
W, S, M = 15., 5., 7
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
    work = tmp_path_factory.mktemp('shelter_sector_emu')
    (work / 'err.cpp').write_text(ERR_CPP)
    lib = work / 'libshelter_sector_emu.so'
    csrc = os.path.join(ROOT, 'ssrs_amd', 'csrc')
    subprocess.run(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-fPIC', '-shared', '-pthread',
                    '-I', os.path.join(ROOT, 'tests', 'hip_host_stub'), '-I', csrc, '-x', 'c++',
                    os.path.join(csrc, 'shelter.hip'), str(work / 'err.cpp'), '-o', str(lib)], check=True)
    L = C.CDLL(str(lib))
    L.ssrs_last_error.restype = C.c_char_p
    L.ssrs_shelter_sx_sector.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                         C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p]
    L.ssrs_updraft_sheltered_sector.argtypes = [C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 8 + \
        [C.c_int, C.POINTER(nat.SsrsShelterParams), C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
         C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def wind_args(wdirn, axes, sector, step):
    """(B, ur, uc, raster): the steps of every case's M azimuths, case-major, as layers._wind_direction_args."""
    if np.ndim(wdirn) <= 1:
        cases = np.atleast_1d(np.asarray(wdirn, dtype=np.float64))
        az = np.stack(sref.azimuths(cases, sector, step), axis=1)                    # (B, M)
        ur, uc = ref.ray_step(az.ravel(), axes)
        return cases.size, np.ascontiguousarray(ur), np.ascontiguousarray(uc), None
    wd = np.ascontiguousarray(wdirn if wdirn.ndim == 3 else wdirn[None])
    return wd.shape[0], None, None, wd


def emu_sx(L, z, res, wdirn, dmax, axes, path='auto', sector=W, step=S):
    from ssrs_amd import _native as nat
    z = np.ascontiguousarray(z)
    rows, cols = z.shape
    batch, ur, uc, wd = wind_args(wdirn, axes, sector, step)
    tan, deg = np.empty((batch, rows, cols)), np.empty((batch, rows, cols))
    rc = L.ssrs_shelter_sx_sector(ptr(z), int(z.dtype == np.float64), res, ptr(ur), ptr(uc), ptr(wd), dmax,
                                  nat.SSRS_RAY_AXES[axes], nat.SSRS_SHELTER_PATH[path], sector, step, ptr(tan), ptr(deg),
                                  rows, cols, batch, None)
    assert rc == 0, L.ssrs_last_error()
    return tan, deg


def emu_updraft(L, z, res, wspeed, wdirn, dmax=500., axes='row_east', coeffs=ref.DEFAULT_COEFFS, sector=W, step=S):
    from ssrs_amd import _native as nat
    z = np.ascontiguousarray(z)
    rows, cols = z.shape
    batch, ur, uc, wd = wind_args(wdirn, axes, sector, step)
    ws0 = wd0 = ws = None
    if wd is None:
        ws0 = np.atleast_1d(np.asarray(wspeed, dtype=np.float64))
        wd0 = np.atleast_1d(np.asarray(wdirn, dtype=np.float64))
    else:
        ws = np.ascontiguousarray(wspeed if wspeed.ndim == 3 else wspeed[None])
    prm = nat.SsrsShelterParams(dmax, nat.SSRS_RAY_AXES[axes], 0, 80., (C.c_double * 7)(*coeffs))
    oro, sx = np.empty((batch, rows, cols), np.float32), np.empty((batch, rows, cols))
    rc = L.ssrs_updraft_sheltered_sector(ptr(z), 1, res, ptr(ur), ptr(uc), ptr(ws0), ptr(wd0), ptr(ws), ptr(wd), None, None,
                                         1, C.byref(prm), sector, step, 0., 0.75, ptr(oro), None, ptr(sx), rows, cols,
                                         batch, None)
    assert rc == 0, L.ssrs_last_error()
    return oro, sx


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


@pytest.mark.parametrize('K', [6, 40])           # M K = 42: one round of the table; 280: two, split inside ray 6
@pytest.mark.parametrize('shape', SHAPES)
def test_emulated_sector_uniform_wind(emu, shape, K):
    """Both paths give the same bits, within the bounds of the reference.  355 +- 15 straddles north (column halo on
    both sides), 237.3 is a general direction, 90 +- 15 straddles an axis in the other frame."""
    z, dirs = make_dem(shape), [355., 237.3, 90.]
    for axes in ('row_north', 'row_east'):
        lds = emu_sx(emu, z, 10., dirs, K * 10. + 5., axes, 'lds')
        glob = emu_sx(emu, z, 10., dirs, K * 10. + 5., axes, 'global')
        assert same_bits(lds[0], glob[0]) and same_bits(lds[1], glob[1]), axes
        for b, wdirn in enumerate(dirs):
            tbar, sx = sref.sector_sx(z, 10., wdirn, W, S, dmax=K * 10. + 5., ray_axes=axes)
            np.testing.assert_allclose(lds[1][b], sx, err_msg=f'{axes} {wdirn:g}', **SX_TOL)
            np.testing.assert_allclose(lds[0][b], tbar, err_msg=f'{axes} {wdirn:g}', **RASTER_TOL)
    assert np.abs(lds[1]).max() > 1. and not np.isnan(lds[0]).any()


@pytest.mark.parametrize('shape', SHAPES)
def test_emulated_sector_per_cell_wind(emu, shape):
    """A direction raster over more than half the circle with a NaN in it, over the DEM with the NaN hole: every cell
    within the bounds, the NaN direction gives 0, both paths the same bits.  K = 40: two rounds of the table."""
    z = make_dem(shape)
    _, wd = wind_raster(shape)
    assert wd.max() - wd.min() > 180.
    wd[3, 4] = np.nan
    for K in (6, 40):
        lds = emu_sx(emu, z, 10., wd, K * 10. + 5., 'row_east', 'lds')
        glob = emu_sx(emu, z, 10., wd, K * 10. + 5., 'row_east', 'global')
        assert same_bits(lds[0], glob[0]) and same_bits(lds[1], glob[1])
        tbar, sx = sref.sector_sx(z, 10., wd, W, S, dmax=K * 10. + 5., ray_axes='row_east')
        np.testing.assert_allclose(lds[0][0], tbar, **RASTER_TOL)
        np.testing.assert_allclose(lds[1][0], sx, **SX_TOL)
        assert lds[0][0][3, 4] == 0. and lds[1][0][3, 4] == 0. and not np.isnan(lds[0]).any()


def test_emulated_sector_batch_of_18_equals_single_calls(emu):
    """M = 7: 16 cases per launch, so 18 cases take two launches; the directions walk round the circle, so the halo
    changes from case to case and the tile is staged again."""
    shape, dmax = (33, 65), 65.
    z = make_dem(shape)
    dirs = list(np.linspace(3., 343., 18))
    tan, deg = emu_sx(emu, z, 10., dirs, dmax, 'row_north')
    for b, wdirn in enumerate(dirs):
        one_tan, one_deg = emu_sx(emu, z, 10., wdirn, dmax, 'row_north')
        assert same_bits(tan[b], one_tan[0]) and same_bits(deg[b], one_deg[0]), b
    # a wide sector: M = 61 leaves two cases per launch
    tan, deg = emu_sx(emu, z, 10., [10., 200., 300.], 35., 'row_east', sector=90., step=3.)
    for b, wdirn in enumerate((10., 200., 300.)):
        tbar, sx = sref.sector_sx(z, 10., wdirn, 90., 3., dmax=35., ray_axes='row_east')
        np.testing.assert_allclose(deg[b], sx, **SX_TOL)
        np.testing.assert_allclose(tan[b], tbar, **RASTER_TOL)


def test_emulated_sector_halo_that_does_not_fit_falls_back(emu):
    """K = 120 at 1 m: the sector's halo exceeds the LDS tile for uniform and per-cell wind alike; 'auto' reads global
    memory and gives the forced global path's bits, a forced LDS path is refused.  M K = 840: four rounds."""
    from ssrs_amd import _native as nat
    shape, dmax = (20, 23), 120.5
    z = make_dem(shape)
    _, wd = wind_raster(shape)
    for wdirn in (wd, [237.3, 0.]):
        auto = emu_sx(emu, z, 1., wdirn, dmax, 'row_north')
        glob = emu_sx(emu, z, 1., wdirn, dmax, 'row_north', 'global')
        assert same_bits(auto[0], glob[0]) and same_bits(auto[1], glob[1])
    for b, wdirn in enumerate((237.3, 0.)):
        tbar, sx = sref.sector_sx(z, 1., wdirn, W, S, dmax=dmax, ray_axes='row_north')
        np.testing.assert_allclose(auto[1][b], sx, **SX_TOL)
        np.testing.assert_allclose(auto[0][b], tbar, **RASTER_TOL)
    batch, ur, uc, _ = wind_args([237.3], 'row_north', W, S)
    out = np.empty((1,) + shape)
    for ray_ur, ray_uc, raster in ((ur, uc, None), (None, None, wd)):
        rc = emu.ssrs_shelter_sx_sector(ptr(z), 1, 1., ptr(ray_ur), ptr(ray_uc), ptr(raster), dmax, 0,
                                        nat.SSRS_SHELTER_PATH['lds'], W, S, ptr(out), None, shape[0], shape[1], 1, None)
        assert rc == nat.SSRS_ERR_INVALID and b'does not fit' in emu.ssrs_last_error()


def test_emulated_sector_of_one_ray_is_the_single_ray_kernel(emu):
    """W < S: M = 1 through k_shelter_sector gives k_shelter's bits on every output, uniform and per-cell wind."""
    from ssrs_amd import _native as nat
    emu.ssrs_shelter_sx.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    shape = (33, 65)
    z = make_dem(shape)
    _, wd = wind_raster(shape)
    wd[3, 4] = np.nan
    for wdirn in ([0., 237.3, 270.], wd):
        got = emu_sx(emu, z, 10., wdirn, 65., 'row_east', sector=0., step=5.)
        batch, ur, uc, raster = wind_args(wdirn, 'row_east', 0., 5.)
        tan, deg = np.empty((batch,) + shape), np.empty((batch,) + shape)
        assert emu.ssrs_shelter_sx(ptr(z), 1, 10., ptr(ur), ptr(uc), ptr(raster), 65., 1, 0, ptr(tan), ptr(deg), shape[0],
                                   shape[1], batch, None) == 0
        assert same_bits(got[0], tan) and same_bits(got[1], deg)
    assert nat.SSRS_OK == 0


def test_emulated_sector_updraft(emu):
    """Neutral coefficients give the original raster whatever the sector; the defaults give the reference's adjustment
    by T-bar; a batch equals single calls; per-cell wind."""
    from oracle import ssrs_oracle as orc
    shape, res = (33, 65), 100.
    z = make_dem(shape)
    slope, aspect = orc.compute_slope_degrees(z, res), orc.compute_aspect_degrees(z, res)
    speeds, dirs = [10., 6., 12.], [45., 237.3, 355.]
    oro, sx = emu_updraft(emu, z, res, speeds, dirs)
    plain, _ = emu_updraft(emu, z, res, speeds, dirs, coeffs=ref.NEUTRAL_COEFFS)
    signal = 0
    for b, (s, d) in enumerate(zip(speeds, dirs)):
        w0 = orc.compute_orographic_updraft(s, d, slope, aspect)
        check_orograph_cells(plain[b], w0, s, f'neutral {d:g}')
        tbar, sx_ref = sref.sector_sx(z, res, d, W, S, dmax=500., ray_axes='row_east')
        np.testing.assert_allclose(sx[b], sx_ref, **SX_TOL)
        signal += check_orograph_cells(oro[b], ref.adjust(w0, tbar, slope), s, f'sector {d:g}')['signal']
        single, _ = emu_updraft(emu, z, res, s, d)
        assert np.array_equal(single[0].view(np.int32), oro[b].view(np.int32))
    assert signal > 0
    ws, wd = wind_raster(shape)
    oro, sx = emu_updraft(emu, z, res, ws, wd)
    w0 = orc.compute_orographic_updraft(ws, wd, slope, aspect)
    tbar, sx_ref = sref.sector_sx(z, res, wd, W, S, dmax=500., ray_axes='row_east')
    np.testing.assert_allclose(sx[0], sx_ref, **SX_TOL)
    assert check_orograph_cells(oro[0], ref.adjust(w0, tbar, slope), float(ws.max()), 'per-cell wind')['signal'] > 0
