"""The sector-averaged Sx of K9 on the device: ssrs_shelter_sx_sector / ssrs_updraft_sheltered_sector behind
layers.compute_sx(..., sector=) and layers.orographic_updraft_improved(..., sector=), and Config.orographic_sx_sector
through the Simulator, against the numpy statement in tests/shelter_sector_ref.py (pinned analytically by
test_shelter_sector_host.py).

Bounds: every T_m of a uniform wind is bit-exact by construction, but atan and tan are the device's, and with per-cell
wind so is the ray step: Sx-bar within rtol 1e-11 / atol 1e-10 and T-bar within rtol 1e-11 / atol 1e-12, the per-cell
bounds of test_gpu_shelter.py, over ALL cells.  Wherever the device is compared with itself -- one ray against the
single-ray calls, the LDS path against the global one, neutral coefficients against K1 -- bit for bit.

The DEM values are rounded to f32 first, so that the f32 and the f64 raster of a case share one reference."""
import ctypes as C
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import shelter_ref as ref
import shelter_sector_ref as sref
from raster_checks import check_orograph_cells

pytestmark = pytest.mark.gpu

DIRECTIONS = (0., 45., 180., 237.3, 270., 359.9)
AXES = ('row_north', 'row_east')
SHAPES = ((70, 45), (33, 65))            # more than one 64 x 32 and 32 x 32 tile in each direction, ragged
SECTORS = ((15., 5.), (10., 2.5))        # M = 7 and 9
RASTER_TOL = dict(rtol=1e-11, atol=1e-12)
SX_TOL = dict(rtol=1e-11, atol=1e-10)


def make_dem(shape, hole=True):
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    z = 1500. + 180. * np.sin(r / 7.3) * np.cos(c / 9.1) + 90. * np.sin((r + 2. * c) / 5.7) + 2.5 * r - 1.5 * c
    if hole:
        z[shape[0] // 2 - 1:shape[0] // 2 + 2, shape[1] // 3:shape[1] // 3 + 3] = np.nan
    return z.astype(np.float32).astype(np.float64)


def wind_raster(shape):
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    return 8. + 3. * np.sin(c / 17.) * np.cos(r / 13.), 200. + 110. * np.sin(c / 7. + r / 9.)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def assert_same_bits(got, want, label=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), (f'{label}: {int(bad.sum())} of {bad.size} cells differ; first at {tuple(np.argwhere(bad)[0])}: '
                           f'got {got[bad][0]!r} want {want[bad][0]!r}')


def assert_within_bounds(tan, deg, want_tan, want_deg, label):
    print(f'{label}: largest |Sx-bar - reference| = {np.abs(deg - want_deg).max():.3e} degrees, '
          f'|T-bar - reference| = {np.abs(tan - want_tan).max():.3e}')
    np.testing.assert_allclose(deg, want_deg, err_msg=label, **SX_TOL)
    np.testing.assert_allclose(tan, want_tan, err_msg=label, **RASTER_TOL)


# ------------------------------------------------------------------------------------------------ (a) uniform wind
@pytest.mark.parametrize('sector, step', SECTORS)
@pytest.mark.parametrize('K', [6, 40])           # M K = 42 / 54: one round of the sample table; 280 / 360: two
@pytest.mark.parametrize('shape', SHAPES)
def test_sector_uniform_wind(gpu, shape, K, sector, step):
    """The six directions in one batched call per frame and DEM type."""
    from ssrs_amd import layers
    z, res = make_dem(shape), 10.
    dmax = K * res + 0.5 * res
    for axes in AXES:
        want = [sref.sector_sx(z, res, d, sector, step, dmax=dmax, ray_axes=axes) for d in DIRECTIONS]
        for dem in (z, z.astype(np.float32)):
            tan, deg = layers.compute_sx(dem, res, DIRECTIONS, dmax=dmax, ray_axes=axes, want='both', sector=sector,
                                         sector_step=step)
            assert tan.shape == deg.shape == (len(DIRECTIONS),) + shape and tan.dtype == deg.dtype == np.float64
            for b, wdirn in enumerate(DIRECTIONS):
                assert_within_bounds(tan[b], deg[b], want[b][0], want[b][1], f'{shape} K {K} {axes} {dem.dtype} {wdirn:g}')
    assert np.abs(deg).max() > 1. and not np.isnan(tan).any()
    # a scalar direction gives a (rows, cols) raster, want = 'deg' / 'tan' one of the two
    one = layers.compute_sx(z, res, 359.9, dmax=dmax, ray_axes=axes, sector=sector, sector_step=step)
    assert_same_bits(one, deg[-1])
    one = layers.compute_sx(torch.from_numpy(z).cuda(), res, 359.9, dmax=dmax, ray_axes=axes, want='tan', sector=sector,
                            sector_step=step)
    assert isinstance(one, torch.Tensor)
    assert_same_bits(one.cpu().numpy(), tan[-1])


# ------------------------------------------------------------------------------------------------ (b) per-cell wind
@pytest.mark.parametrize('sector, step', SECTORS)
@pytest.mark.parametrize('shape', SHAPES)
def test_sector_per_cell_wind(gpu, shape, sector, step):
    """The DEM with the NaN hole, a direction raster over more than half the circle with a NaN in it: all cells."""
    from ssrs_amd import layers
    z, res = make_dem(shape), 10.
    _, wd = wind_raster(shape)
    assert wd.max() - wd.min() > 180.
    wd[3, 4] = np.nan
    for K in (6, 40):
        dmax = K * res + 0.5 * res
        for axes in AXES:
            tan, deg = layers.compute_sx(z, res, wd, dmax=dmax, ray_axes=axes, want='both', sector=sector, sector_step=step)
            want_tan, want_deg = sref.sector_sx(z, res, wd, sector, step, dmax=dmax, ray_axes=axes)
            assert_within_bounds(tan, deg, want_tan, want_deg, f'per-cell {shape} K {K} {axes}')
            assert tan[3, 4] == 0. and deg[3, 4] == 0. and not np.isnan(tan).any() and not np.isnan(deg).any()


# ------------------------------------------------------------------------------------------------ (c) one ray
def _sector_call(lib, nat, dem, res, ur, uc, wd, dmax, axes, sector, step, rows, cols, batch):
    tan, deg = (torch.empty((batch, rows, cols), dtype=torch.float64, device='cuda') for _ in range(2))
    nat.check(lib.ssrs_shelter_sx_sector(nat.ptr(dem), 1, C.c_double(res), ur, uc, nat.ptr(wd), C.c_double(dmax),
                                         nat.SSRS_RAY_AXES[axes], 0, C.c_double(sector), C.c_double(step), nat.ptr(tan),
                                         nat.ptr(deg), rows, cols, batch, None))
    torch.cuda.synchronize()
    return tan.cpu().numpy(), deg.cpu().numpy()


def test_sector_of_one_ray_equals_the_single_ray_calls(gpu):
    """W = 0 (and W < S) through the NEW entry points against ssrs_shelter_sx / ssrs_updraft_sheltered: every output,
    bit for bit, uniform and per-cell wind, DEM only and slope / aspect layers."""
    from ssrs_amd import _native as nat, layers
    lib = nat.lib()
    shape, res, dmax, thr = (70, 45), 10., 65., 0.75
    rows, cols = shape
    z = make_dem(shape)
    ws, wd = wind_raster(shape)
    wd[3, 4] = np.nan
    dem = torch.from_numpy(z).cuda()
    ws_d, wd_d = torch.from_numpy(ws).cuda()[None].contiguous(), torch.from_numpy(wd).cuda()[None].contiguous()
    dirs = np.array(DIRECTIONS)
    speeds = np.linspace(5., 11., dirs.size)
    slope, aspect = layers.slope_aspect(dem, res)
    for axes in AXES:
        ur, uc = layers.ray_step(dirs, axes)
        pu, pc = (a.ctypes.data_as(C.c_void_p) for a in (ur, uc))
        old = layers.compute_sx(z, res, dirs, dmax=dmax, ray_axes=axes, want='both')
        for sector, step in ((0., 5.), (4.9, 5.)):
            new = _sector_call(lib, nat, dem, res, pu, pc, None, dmax, axes, sector, step, rows, cols, dirs.size)
            assert_same_bits(new[0], old[0], f'uniform tan {axes}')
            assert_same_bits(new[1], old[1], f'uniform deg {axes}')
        old = layers.compute_sx(z, res, wd, dmax=dmax, ray_axes=axes, want='both')
        new = _sector_call(lib, nat, dem, res, None, None, wd_d, dmax, axes, 0., 5., rows, cols, 1)
        assert_same_bits(new[0][0], old[0], f'per-cell tan {axes}')
        assert_same_bits(new[1][0], old[1], f'per-cell deg {axes}')
    # the updraft: (uniform | per-cell) x (DEM only | layers given)
    for uniform in (True, False):
        for given in (False, True):
            axes = 'row_north' if given else 'row_east'
            kw = dict(slope=slope, aspect=aspect) if given else {}
            old = layers.orographic_updraft_improved(dem, res, speeds if uniform else ws_d, dirs if uniform else wd_d,
                                                     dmax=dmax, threshold=thr, want_sx=True, **kw)
            batch = dirs.size if uniform else 1
            ur, uc = layers.ray_step(dirs, axes)
            ptrs = [a.ctypes.data_as(C.c_void_p) for a in (ur, uc, speeds, dirs)] if uniform else [None] * 4
            prm = nat.SsrsShelterParams(dmax, nat.SSRS_RAY_AXES[axes], 0, 80., (C.c_double * 7)(*ref.DEFAULT_COEFFS))
            oro = torch.empty((batch, rows, cols), dtype=torch.float32, device='cuda')
            use, sx = (torch.empty((batch, rows, cols), dtype=torch.float64, device='cuda') for _ in range(2))
            nat.check(lib.ssrs_updraft_sheltered_sector(
                nat.ptr(dem), 1, C.c_double(res), *ptrs, nat.ptr(None if uniform else ws_d),
                nat.ptr(None if uniform else wd_d), nat.ptr(slope if given else None), nat.ptr(aspect if given else None),
                1, C.byref(prm), C.c_double(0.), C.c_double(5.), C.c_double(0.), C.c_double(thr), nat.ptr(oro), nat.ptr(use),
                nat.ptr(sx), rows, cols, batch, None))
            torch.cuda.synchronize()
            for got, want, name in zip((oro, use, sx), old, ('orograph', 'usable', 'sx')):
                assert_same_bits(got.cpu().numpy(), want.cpu().numpy(), f'{name} uniform={uniform} layers={given}')


# ------------------------------------------------------------------------------------------------ (d) device vs device
@pytest.mark.parametrize('sector, step', SECTORS)
def test_sector_equals_the_mean_of_single_ray_calls(gpu, sector, step):
    """Sx-bar against the mean of M compute_sx(A_m) rasters of the device itself (the unfused route), summed in the
    model's order: the bounds of (a), uniform and per-cell wind."""
    from ssrs_amd import layers
    shape, res, dmax = (70, 45), 10., 405.
    z = make_dem(shape)
    _, wd = wind_raster(shape)
    count = sref.ray_count(sector, step)[1]
    for wdirn in (237.3, 0., wd):
        for axes in AXES:
            acc = np.zeros(shape)
            for a_m in sref.azimuths(wdirn, sector, step):
                acc = acc + layers.compute_sx(z, res, a_m, dmax=dmax, ray_axes=axes)
            tan, deg = layers.compute_sx(z, res, wdirn, dmax=dmax, ray_axes=axes, want='both', sector=sector,
                                         sector_step=step)
            assert_within_bounds(tan, deg, np.tan(acc / float(count) * (np.pi / 180.)), acc / float(count),
                                 f'mean of {count} rays {axes}')


# ------------------------------------------------------------------------------------------------ (e) paths
def test_sector_lds_global_and_fallback_give_equal_bits(gpu):
    from ssrs_amd import layers
    sector = dict(sector=15., sector_step=5.)
    for shape in SHAPES:
        z = make_dem(shape)
        ws, wd = wind_raster(shape)
        for wspeed, wdirn in ((np.linspace(5., 11., len(DIRECTIONS)), list(DIRECTIONS)), (ws, wd)):
            for axes in AXES:
                a = layers.compute_sx(z, 10., wdirn, dmax=405., ray_axes=axes, want='both', path='lds', **sector)
                b = layers.compute_sx(z, 10., wdirn, dmax=405., ray_axes=axes, want='both', path='global', **sector)
                c = layers.compute_sx(z, 10., wdirn, dmax=405., ray_axes=axes, want='both', **sector)
                for x, y, w, name in zip(a, b, c, ('tan', 'deg')):
                    assert_same_bits(x, y, f'{name} {shape} {axes}')
                    assert_same_bits(x, w, f'{name} {shape} {axes} auto')
            a = layers.orographic_updraft_improved(z, 100., wspeed, wdirn, threshold=0.75, want_sx=True, path='lds', **sector)
            b = layers.orographic_updraft_improved(z, 100., wspeed, wdirn, threshold=0.75, want_sx=True, path='global', **sector)
            for x, y, name in zip(a, b, ('orograph', 'usable', 'sx')):
                assert_same_bits(x, y, f'{name} {shape}')
    # K = 120 at 1 m: the sector's halo does not fit, 'auto' reads global memory, a forced LDS path is refused
    z = make_dem((33, 65))
    _, wd = wind_raster((33, 65))
    for wdirn in ([237.3, 0.], wd):
        auto = layers.compute_sx(z, 1., wdirn, dmax=120.5, want='both', **sector)
        glob = layers.compute_sx(z, 1., wdirn, dmax=120.5, want='both', path='global', **sector)
        assert_same_bits(auto[0], glob[0], 'fallback tan')
        assert_same_bits(auto[1], glob[1], 'fallback deg')
        with pytest.raises(ValueError, match='does not fit'):
            layers.compute_sx(z, 1., wdirn, dmax=120.5, path='lds', **sector)
    want_tan, want_deg = sref.sector_sx(z, 1., wd, 15., 5., dmax=120.5)
    assert_within_bounds(auto[0], auto[1], want_tan, want_deg, 'fallback, per-cell wind')
    # 18 uniform cases: two launches (16 cases of 7 rays each travel in the kernel's arguments), halos that change
    many = np.linspace(3., 343., 18)
    tan = layers.compute_sx(z, 10., many, dmax=65., want='tan', **sector)
    for b in range(18):
        assert_same_bits(tan[b], layers.compute_sx(z, 10., float(many[b]), dmax=65., want='tan', **sector), f'case {b} of 18')


# ------------------------------------------------------------------------------------------------ (f) the updraft
def test_sector_updraft(gpu):
    """Neutral coefficients with W = 15: K1's rasters bit for bit.  The default coefficients: the reference's adjustment
    of the oracle's updraft by T-bar."""
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    shape, res, thr = (70, 45), 100., 0.75
    z = make_dem(shape)
    ws, wd = wind_raster(shape)
    sector = dict(sector=15., sector_step=5.)
    neutral = dict(coeffs=ref.NEUTRAL_COEFFS, dmax=550., threshold=thr, **sector)
    for wdirn in (270., 237.3, 0.):
        oro, use = layers.orographic_updraft_improved(z, res, 10., wdirn, **neutral)
        want_oro, want_use = layers.updraft_from_dem(z, res, 10., wdirn, threshold=thr)
        assert_same_bits(oro, want_oro, f'DEM only {wdirn:g}')
        assert_same_bits(use, want_use, f'DEM only, usable {wdirn:g}')
    dem = torch.from_numpy(z).cuda()
    slope, aspect = layers.slope_aspect(dem, res)
    for wspeed, wdirn in ((10., 237.3), ([10., 6.], [270., 45.]), (torch.from_numpy(ws).cuda(), torch.from_numpy(wd).cuda())):
        oro, use = layers.orographic_updraft_improved(dem, res, wspeed, wdirn, slope=slope, aspect=aspect, **neutral)
        want_oro, want_use = layers.orographic_updraft(wspeed, wdirn, slope, aspect, threshold=thr)
        assert_same_bits(oro.cpu().numpy(), want_oro.cpu().numpy(), 'layers given')
        assert_same_bits(use.cpu().numpy(), want_use.cpu().numpy(), 'layers given, usable')
    # the defaults
    slope, aspect = orc.compute_slope_degrees(z, res), orc.compute_aspect_degrees(z, res)
    signal = 0
    for wspeed, wdirn in ((10., 270.), (10., 237.3), (7., 45.), (ws, wd)):
        oro, _, sx = layers.orographic_updraft_improved(z, res, wspeed, wdirn, threshold=thr, want_sx=True, **sector)
        tbar, sx_ref = sref.sector_sx(z, res, wdirn, 15., 5., dmax=500., ray_axes='row_east')
        np.testing.assert_allclose(sx, sx_ref, **SX_TOL)
        w0 = orc.compute_orographic_updraft(wspeed, wdirn, slope, aspect)
        with np.errstate(invalid='ignore'):
            want = ref.adjust(w0, tbar, slope)
        want = np.where(np.isnan(want), 0., want)
        signal += check_orograph_cells(oro, want, float(np.max(wspeed)), f'sector {np.ndim(wdirn)}-d wind')['signal']
    assert signal > 0
    # the sector does something: most cells that carry an updraft differ from the single ray's
    one, _ = layers.orographic_updraft_improved(z, res, 10., 237.3)
    avg, _ = layers.orographic_updraft_improved(z, res, 10., 237.3, **sector)
    assert (avg[one > 0.01] != one[one > 0.01]).mean() > 0.5


# ------------------------------------------------------------------------------------------------ (g) Simulator
def sim_config(tmp_path, **kw):
    from ssrs_amd import Config
    base = Config(run_name='sector', out_dir=str(tmp_path), sim_seed=30, region_width_km=(6., 5.), resolution=100.,
                  track_count=16, track_start_region=(1, 5, 0.2, 0.6), track_direction=0., orographic_model='improved',
                  orographic_sx_sector=15.)
    return replace(base, **kw)


def test_simulator_uniform_mode(gpu, tmp_path):
    from ssrs_amd import Simulator, layers
    sim = Simulator(sim_config(tmp_path), terrain='synthetic')
    assert sim.gridsize == (50, 60)
    dem = sim.get_terrain_elevation()
    oro, _, sx = layers.orographic_updraft_improved(dem, 100., 10., 270., want_sx=True, sector=15.)
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, 's10d270_sx.npy')),
                     layers.compute_sx(dem, 100., 270., sector=15.).astype(np.float32))
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, 's10d270_sx.npy')), sx.astype(np.float32))
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy')), oro)
    assert sim._get_id_string('s10d270', 0) == 's10d270_d0_t75_fluidflow-sx500h80a15s5_r0'
    sim.simulate_tracks()
    assert sorted(os.listdir(sim.mode_data_dir)) == [
        's10d270_d0_t75_fluidflow-sx500h80a15s5_r0_potential.npy', 's10d270_d0_t75_fluidflow-sx500h80a15s5_r0_tracks.pkl',
        's10d270_orograph.npy', 's10d270_sx.npy']
    # W = 0 in the same out_dir / run_name: today's names, and the sector run's potential is not picked up
    sim0 = Simulator(sim_config(tmp_path, orographic_sx_sector=0.), terrain='synthetic')
    assert sim0._get_id_string('s10d270', 0) == 's10d270_d0_t75_fluidflow-sx500h80_r0'
    sim0.simulate_tracks()
    names = sorted(os.listdir(sim0.mode_data_dir))
    assert 's10d270_d0_t75_fluidflow-sx500h80_r0_potential.npy' in names and len(names) == 6
    assert_same_bits(np.load(os.path.join(sim0.mode_data_dir, 's10d270_sx.npy')),
                     layers.compute_sx(dem, 100., 270.).astype(np.float32))
    # a step that is not the default shows in the id
    sim2 = Simulator(sim_config(tmp_path, run_name='fine', orographic_sx_sector=7.5, orographic_sx_step=2.5),
                     terrain='synthetic')
    assert sim2._get_id_string('s10d270') == 's10d270_d0_t75_fluidflow-sx500h80a7.5s2.5'
    assert_same_bits(np.load(os.path.join(sim2.mode_data_dir, 's10d270_sx.npy')),
                     layers.compute_sx(dem, 100., 270., sector=7.5, sector_step=2.5).astype(np.float32))
    # 'original' ignores both fields: today's names and today's bytes
    sim3 = Simulator(sim_config(tmp_path, run_name='original', orographic_model='original'), terrain='synthetic')
    sim3.simulate_tracks()
    assert sorted(os.listdir(sim3.mode_data_dir)) == ['s10d270_d0_t75_fluidflow_r0_potential.npy',
                                                      's10d270_d0_t75_fluidflow_r0_tracks.pkl', 's10d270_orograph.npy']
    plain, _ = layers.updraft_from_dem(dem, 100., 10., 270.)
    assert_same_bits(np.load(os.path.join(sim3.mode_data_dir, 's10d270_orograph.npy')), plain)


def test_simulator_snapshot_mode_with_injected_wind_rasters(gpu, tmp_path):
    from ssrs_amd import Simulator, layers
    ws, wd = wind_raster((50, 60))
    item = dict(datetime=(2010, 6, 17, 13), wspeed=ws, wdirn=wd)
    sim = Simulator(sim_config(tmp_path, sim_mode='snapshot', run_name='snap'), terrain='synthetic', wind=[item])
    case = sim.case_ids[0]
    dem = sim.get_terrain_elevation()
    oro, _, sx = layers.orographic_updraft_improved(dem, 100., ws, wd, want_sx=True, sector=15.)
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, f'{case}_orograph.npy')), oro)
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, f'{case}_sx.npy')), sx.astype(np.float32))
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, f'{case}_sx.npy')),
                     layers.compute_sx(dem, 100., wd, sector=15.).astype(np.float32))
    assert sim._get_id_string(case, 0).endswith('-sx500h80a15s5_r0')
    # and 'original' with W = 15 writes no Sx and today's orograph
    sim2 = Simulator(sim_config(tmp_path, sim_mode='snapshot', run_name='snap_orig', orographic_model='original'),
                     terrain='synthetic', wind=[item])
    assert sorted(os.listdir(sim2.mode_data_dir)) == [f'{case}_orograph.npy']
    assert '-sx' not in sim2._get_id_string(case, 0)
