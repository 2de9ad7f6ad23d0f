"""K9 on the device: ssrs_shelter_sx / ssrs_updraft_sheltered behind layers.compute_sx and
layers.orographic_updraft_improved, and Config.orographic_model = 'improved' through the Simulator, against the numpy
statement of the model in tests/shelter_ref.py (pinned analytically by test_shelter_host.py).

Bounds: with uniform wind the ray step is the host's and every operation of a sample is an IEEE one in a fixed order, so
tan Sx is asked for BIT FOR BIT on every cell.  With per-cell wind the device's sine / cosine of degrees differs from
numpy's by about an ulp, which moves a sample by up to K 2^-52 cells times the DEM's gradient: rtol 1e-11 / atol 1e-12.
Sx in degrees carries the device's atan: raster_checks.SLOPE_TOL.  The adjusted orograph (f32) and the usable updraft
are judged by raster_checks, like the K1 rasters."""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import shelter_ref as ref
from raster_checks import SLOPE_TOL, check_orograph_cells, check_usable

pytestmark = pytest.mark.gpu

DIRECTIONS = (0., 45., 90., 180., 237.3, 270., 315., 359.9)
AXES = ('row_north', 'row_east')
RASTER_TOL = dict(rtol=1e-11, atol=1e-12)


def make_dem(kind, shape):
    rows, cols = shape
    r, c = np.mgrid[0:rows, 0:cols].astype(np.float64)
    z = 1500. + 180. * np.sin(r / 7.3) * np.cos(c / 9.1) + 90. * np.sin((r + 2. * c) / 5.7) + 2.5 * r - 1.5 * c
    if kind == 'plateau':
        z = 1000. + 250. * (np.floor(z / 120.) % 3)                     # flat steps with cliffs between them
    if kind == 'nan':
        z[rows // 2 - 1:rows // 2 + 2, cols // 3:cols // 3 + 3] = np.nan
    return z


def wind_raster(shape, phase=0.):
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    # one full wave across the columns, whatever the shape: 90 .. 310 degrees, more than half the circle
    wd = 200. + 110. * np.sin(2. * np.pi * c / (shape[1] - 1) + r / 29. + phase)
    ws = 8. + 3. * np.sin(c / 17.) * np.cos(r / 13. + phase)
    return ws, wd


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def assert_same_bits(got, want, label=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), (f'{label}: {int(bad.sum())} of {bad.size} cells differ; first at {tuple(np.argwhere(bad)[0])}: '
                           f'got {got[bad][0]!r} want {want[bad][0]!r}')


# ------------------------------------------------------------------------------------------------ Sx
@pytest.mark.parametrize('K', [1, 5, 50])
@pytest.mark.parametrize('shape', [(97, 131), (20, 23)])
def test_sx_uniform_wind_is_bit_identical(gpu, shape, K):
    """All eight directions in one batched call per (DEM, res, frame).  K = 50 on (20, 23): a halo larger than the
    raster."""
    from ssrs_amd import layers
    for kind in ('smooth', 'plateau', 'nan'):
        z = make_dem(kind, shape)
        for res in (10., 100.):
            dmax = K * res + 0.5 * res
            for axes in AXES:
                tan, deg = layers.compute_sx(z, res, DIRECTIONS, dmax=dmax, ray_axes=axes, want='both')
                assert tan.shape == (len(DIRECTIONS),) + shape and tan.dtype == deg.dtype == np.float64
                for b, wdirn in enumerate(DIRECTIONS):
                    want = ref.tan_sx(z, res, wdirn, dmax=dmax, ray_axes=axes)
                    label = f'{kind} {shape} res {res:g} K {K} {axes} {wdirn:g}'
                    assert_same_bits(tan[b], want, label)
                    np.testing.assert_allclose(deg[b], ref.sx_degrees(want), err_msg=label, **SLOPE_TOL)
    # a scalar direction gives a (rows, cols) raster, tensors in give tensors out
    one = layers.compute_sx(torch.from_numpy(z).cuda(), res, 237.3, dmax=dmax, ray_axes='row_east', want='tan')
    assert isinstance(one, torch.Tensor) and tuple(one.shape) == shape
    assert_same_bits(one.cpu().numpy(), ref.tan_sx(z, res, 237.3, dmax=dmax, ray_axes='row_east'))


@pytest.mark.parametrize('K', [1, 5, 50])
@pytest.mark.parametrize('shape', [(97, 131), (20, 23)])
def test_sx_per_cell_wind(gpu, shape, K):
    from ssrs_amd import layers
    _, wd = wind_raster(shape)
    assert wd.max() - wd.min() > 180.
    worst = 0.
    for kind in ('smooth', 'plateau', 'nan'):
        z = make_dem(kind, shape)
        for res in (10., 100.):
            dmax = K * res + 0.5 * res
            for axes in AXES:
                tan, deg = layers.compute_sx(z, res, wd, dmax=dmax, ray_axes=axes, want='both')
                want = ref.tan_sx(z, res, wd, dmax=dmax, ray_axes=axes)
                worst = max(worst, float(np.abs(tan - want).max()))
                np.testing.assert_allclose(tan, want, err_msg=f'{kind} res {res:g} {axes}', **RASTER_TOL)
                np.testing.assert_allclose(deg, ref.sx_degrees(want), rtol=1e-11, atol=1e-10)
    print(f'per-cell wind {shape} K {K}: largest |tan Sx - reference| = {worst:.3e}')
    # a NaN direction (a cell outside the wind samples' hull) sees nothing
    wd_nan = wd.copy()
    wd_nan[3, 4] = np.nan
    tan = layers.compute_sx(z, res, wd_nan, dmax=dmax, ray_axes='row_north', want='tan')
    assert tan[3, 4] == 0. and not np.isnan(tan).any()


def test_lds_and_global_paths_give_equal_bits(gpu):
    """K = 5 with either path forced; K = 200 on (300, 260) does not fit the LDS and takes the global path by itself;
    K = 300 needs two rounds of the sample table."""
    from ssrs_amd import layers
    shape, res, dmax = (97, 131), 10., 55.
    ws, wd = wind_raster(shape)
    for kind in ('smooth', 'nan'):
        z = make_dem(kind, shape)
        for axes in AXES:
            for wdirn in (list(DIRECTIONS), wd):
                a = layers.compute_sx(z, res, wdirn, dmax=dmax, ray_axes=axes, want='both', path='lds')
                b = layers.compute_sx(z, res, wdirn, dmax=dmax, ray_axes=axes, want='both', path='global')
                assert_same_bits(a[0], b[0], f'tan {kind} {axes}')
                assert_same_bits(a[1], b[1], f'deg {kind} {axes}')
        for wspeed, wdirn in (([10.] * 3, [45., 237.3, 315.]), (ws, wd)):
            a = layers.orographic_updraft_improved(z, res, wspeed, wdirn, dmax=dmax, threshold=0.75, want_sx=True, path='lds')
            b = layers.orographic_updraft_improved(z, res, wspeed, wdirn, dmax=dmax, threshold=0.75, want_sx=True, path='global')
            for x, y, name in zip(a, b, ('orograph', 'usable', 'sx')):
                assert_same_bits(x, y, f'{name} {kind}')
    # an f32 DEM is the f64 DEM of the same values
    z32 = make_dem('smooth', shape).astype(np.float32)
    assert_same_bits(layers.compute_sx(z32, res, 237.3, dmax=dmax, want='tan'),
                     layers.compute_sx(z32.astype(np.float64), res, 237.3, dmax=dmax, want='tan'))
    with pytest.raises(ValueError, match='does not fit'):
        layers.compute_sx(z, res, 237.3, dmax=2005., want='tan', path='lds')
    # K = 200: global path
    shape, res, dmax = (300, 260), 10., 2005.
    z = make_dem('smooth', shape)
    tan = layers.compute_sx(z, res, [237.3, 90.], dmax=dmax, ray_axes='row_east', want='tan')
    for b, wdirn in enumerate((237.3, 90.)):
        assert_same_bits(tan[b], ref.tan_sx(z, res, wdirn, dmax=dmax, ray_axes='row_east'), f'K 200 {wdirn:g}')
    _, wd = wind_raster(shape)
    tan = layers.compute_sx(z, res, wd, dmax=dmax, ray_axes='row_north', want='tan')
    want = ref.tan_sx(z, res, wd, dmax=dmax, ray_axes='row_north')
    print(f'per-cell wind {shape} K 200: largest |tan Sx - reference| = {np.abs(tan - want).max():.3e}')
    np.testing.assert_allclose(tan, want, **RASTER_TOL)
    # K = 300: the samples are tabulated 256 at a time, so this takes two rounds of the table
    shape, res, dmax = (20, 23), 1., 300.5
    z = make_dem('nan', shape)
    tan = layers.compute_sx(z, res, [237.3, 270.], dmax=dmax, ray_axes='row_north', want='tan')
    for b, wdirn in enumerate((237.3, 270.)):
        assert_same_bits(tan[b], ref.tan_sx(z, res, wdirn, dmax=dmax, ray_axes='row_north'), f'K 300 {wdirn:g}')
    _, wd = wind_raster(shape)
    np.testing.assert_allclose(layers.compute_sx(z, res, wd, dmax=dmax, want='tan'),
                               ref.tan_sx(z, res, wd, dmax=dmax, ray_axes='row_east'), **RASTER_TOL)


# ------------------------------------------------------------------------------------------------ the updraft
@pytest.mark.parametrize('kind', ['smooth', 'plateau', 'nan'])
def test_neutral_parameters_reproduce_the_original_rasters(gpu, kind):
    """(a, b, c, d, e, f, g) = (0, 0, 1, 1, 0, 0, 0): F_h = F_sx = 1, and the rasters are today's bit for bit."""
    from ssrs_amd import layers
    shape, res, thr = (97, 131), 100., 0.75
    z = make_dem(kind, shape)
    neutral = dict(coeffs=ref.NEUTRAL_COEFFS, dmax=550., threshold=thr)
    for wdirn in (270., 237.3, 0., 45.):
        for min_val in (0., 0.05):
            oro, use = layers.orographic_updraft_improved(z, res, 10., wdirn, min_updraft_val=min_val, **neutral)
            want_oro, want_use = layers.updraft_from_dem(z, res, 10., wdirn, threshold=thr, min_updraft_val=min_val)
            assert_same_bits(oro, want_oro, f'DEM only {wdirn:g}')
            assert_same_bits(use, want_use, f'DEM only, usable {wdirn:g}')
    # slope / aspect layers given: the elementwise kernel's arithmetic, scalar and per-cell wind
    dem = torch.from_numpy(z).cuda()
    slope, aspect = layers.slope_aspect(dem, res)
    ws, wd = wind_raster(shape)
    for wspeed, wdirn in ((10., 237.3), ([10., 6.], [270., 45.]), (torch.from_numpy(ws).cuda(), torch.from_numpy(wd).cuda())):
        oro, use = layers.orographic_updraft_improved(dem, res, wspeed, wdirn, slope=slope, aspect=aspect, **neutral)
        want_oro, want_use = layers.orographic_updraft(wspeed, wdirn, slope, aspect, threshold=thr)
        assert_same_bits(oro.cpu().numpy(), want_oro.cpu().numpy(), 'layers given')
        assert_same_bits(use.cpu().numpy(), want_use.cpu().numpy(), 'layers given, usable')


def reference_updraft(z, res, wspeed, wdirn, dmax, axes, min_val=0., slope=None, aspect=None, **model):
    from oracle import ssrs_oracle as orc
    if slope is None:
        slope, aspect = orc.compute_slope_degrees(z, res), orc.compute_aspect_degrees(z, res)
    w0 = orc.compute_orographic_updraft(wspeed, wdirn, slope, aspect)          # >= 0: its clamp at 0 changes nothing
    T = ref.tan_sx(z, res, wdirn, dmax=dmax, ray_axes=axes)
    with np.errstate(invalid='ignore'):
        w = ref.adjust(w0, T, slope, min_updraft_val=min_val, **model)
    return np.where(np.isnan(w), min_val, w), T                                 # (a NaN wind: the clamp's value)


@pytest.mark.parametrize('kind', ['smooth', 'plateau', 'nan'])
def test_improved_model_against_the_reference(gpu, kind):
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    shape, res, thr, dmax = (97, 131), 100., 0.75, 500.
    z = make_dem(kind, shape)
    signal = 0
    for wdirn in (270., 237.3, 45.):
        oro, use, sx = layers.orographic_updraft_improved(z, res, 10., wdirn, threshold=thr, want_sx=True)
        want, T = reference_updraft(z, res, 10., wdirn, dmax, 'row_east')
        assert oro.dtype == np.float32 and use.dtype == sx.dtype == np.float64
        signal += check_orograph_cells(oro, want, 10., f'improved {kind} {wdirn:g}')['signal']
        want32 = want.astype(np.float32)
        check_usable(use, oro, thr, want32, orc.get_above_threshold_speed(want32, thr), orc)
        np.testing.assert_allclose(sx, ref.sx_degrees(T), **SLOPE_TOL)
    assert signal > 0
    # the model does something: the defaults differ from the original raster on most cells that carry an updraft
    plain, _ = layers.updraft_from_dem(z, res, 10., 237.3)
    got, _ = layers.orographic_updraft_improved(z, res, 10., 237.3)
    assert (got[plain > 0.01] != plain[plain > 0.01]).mean() > 0.9
    # other height / coefficients / clamp; slope and aspect layers given (geographic frame)
    model = dict(height=120., coeffs=(3e-5, 2e-3, 0.9, 0.4, 0.1, -0.05, -0.7))
    slope, aspect = orc.compute_slope_degrees(z, res), orc.compute_aspect_degrees(z, res)
    oro, use = layers.orographic_updraft_improved(z, res, 7., 237.3, slope=slope, aspect=aspect, dmax=350., threshold=thr,
                                                  min_updraft_val=0.02, **model)
    want, _ = reference_updraft(z, res, 7., 237.3, 350., 'row_north', min_val=0.02, slope=slope, aspect=aspect, **model)
    assert check_orograph_cells(oro, want, 7., f'layers given {kind}')['signal'] > 0
    # per-cell wind
    ws, wd = wind_raster(shape)
    oro, use = layers.orographic_updraft_improved(z, res, ws, wd, threshold=thr)
    want, _ = reference_updraft(z, res, ws, wd, dmax, 'row_east')
    assert check_orograph_cells(oro, want, float(ws.max()), f'per-cell wind {kind}')['signal'] > 0
    want32 = want.astype(np.float32)
    check_usable(use, oro, thr, want32, orc.get_above_threshold_speed(want32, thr), orc)


def test_batched_calls_equal_single_calls(gpu):
    """Three uniform cases from three quadrants (the tile is staged again when the upwind side changes) and three wind
    rasters: each equals its own call, bit for bit."""
    from ssrs_amd import layers
    shape, res = (97, 131), 100.
    z = make_dem('nan', shape)
    speeds, dirs = [10., 6., 12.], [45., 237.3, 315.]
    batched = layers.orographic_updraft_improved(z, res, speeds, dirs, threshold=0.75, want_sx=True)
    tan = layers.compute_sx(z, res, dirs, want='tan')
    for b in range(3):
        single = layers.orographic_updraft_improved(z, res, speeds[b], dirs[b], threshold=0.75, want_sx=True)
        for x, y, name in zip(batched, single, ('orograph', 'usable', 'sx')):
            assert x.shape == (3,) + shape and y.shape == shape
            assert_same_bits(x[b], y, f'uniform {name} {b}')
        assert_same_bits(tan[b], layers.compute_sx(z, res, dirs[b], want='tan'), f'uniform tan {b}')
    rasters = [wind_raster(shape, phase) for phase in (0., 1.1, 2.3)]
    ws, wd = np.stack([r[0] for r in rasters]), np.stack([r[1] for r in rasters])
    batched = layers.orographic_updraft_improved(z, res, ws, wd, threshold=0.75, want_sx=True)
    tan = layers.compute_sx(z, res, wd, ray_axes='row_north', want='tan')
    for b in range(3):
        single = layers.orographic_updraft_improved(z, res, ws[b], wd[b], threshold=0.75, want_sx=True)
        for x, y, name in zip(batched, single, ('orograph', 'usable', 'sx')):
            assert_same_bits(x[b], y, f'raster {name} {b}')
        assert_same_bits(tan[b], layers.compute_sx(z, res, wd[b], ray_axes='row_north', want='tan'), f'raster tan {b}')
    # 20 uniform cases: more than one launch's worth of kernel arguments
    many = np.linspace(0., 340., 20)
    tan = layers.compute_sx(z, res, many, dmax=250., want='tan')
    for b in (0, 15, 16, 19):
        assert_same_bits(tan[b], layers.compute_sx(z, res, float(many[b]), dmax=250., want='tan'), f'case {b} of 20')


# ------------------------------------------------------------------------------------------------ Simulator
def sim_config(tmp_path, **kw):
    from ssrs_amd import Config
    base = Config(run_name='shelter', out_dir=str(tmp_path), sim_seed=30, region_width_km=(6., 5.), resolution=100.,
                  track_count=16, track_start_region=(1, 5, 0.2, 0.6), track_direction=0., orographic_model='improved')
    return replace(base, **kw)


def test_simulator_uniform_mode(gpu, tmp_path):
    from ssrs_amd import Simulator, layers
    sim = Simulator(sim_config(tmp_path), terrain='synthetic')
    assert sim.gridsize == (50, 60)
    dem = sim.get_terrain_elevation()
    oro, _, sx = layers.orographic_updraft_improved(dem, 100., 10., 270., want_sx=True)       # DEM only: 'row_east'
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy')), oro)
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, 's10d270_sx.npy')), sx.astype(np.float32))
    assert np.abs(sx).max() > 1.
    assert sim._get_id_string('s10d270', 0) == 's10d270_d0_t75_fluidflow-sx500h80_r0'
    sim.simulate_tracks()
    names = sorted(os.listdir(sim.mode_data_dir))
    assert names == ['s10d270_d0_t75_fluidflow-sx500h80_r0_potential.npy', 's10d270_d0_t75_fluidflow-sx500h80_r0_tracks.pkl',
                     's10d270_orograph.npy', 's10d270_sx.npy']
    assert int(sim._presence_counts[('s10d270', 0)].sum()) > 16
    # injected Slope / Aspect layers are geographic: the ray runs in 'row_north'
    slope, aspect = layers.slope_aspect(dem, 100.)
    sim2 = Simulator(sim_config(tmp_path, run_name='layers', orographic_sx_dmax=350., orographic_height=120.),
                     terrain=dict(Elevation=dem, Slope=slope, Aspect=aspect))
    oro2, _, sx2 = layers.orographic_updraft_improved(dem, 100., 10., 270., slope=slope, aspect=aspect, dmax=350., height=120.,
                                                      ray_axes='row_north', want_sx=True)
    assert_same_bits(np.load(os.path.join(sim2.mode_data_dir, 's10d270_orograph.npy')), oro2)
    assert_same_bits(np.load(os.path.join(sim2.mode_data_dir, 's10d270_sx.npy')), sx2.astype(np.float32))
    assert sim2._get_id_string('s10d270') == 's10d270_d0_t75_fluidflow-sx350h120'
    # 'original': today's names and today's bytes
    sim3 = Simulator(sim_config(tmp_path, run_name='original', orographic_model='original'), terrain='synthetic')
    sim3.simulate_tracks()
    assert sorted(os.listdir(sim3.mode_data_dir)) == ['s10d270_d0_t75_fluidflow_r0_potential.npy',
                                                      's10d270_d0_t75_fluidflow_r0_tracks.pkl', 's10d270_orograph.npy']
    plain, _ = layers.updraft_from_dem(dem, 100., 10., 270.)
    assert_same_bits(np.load(os.path.join(sim3.mode_data_dir, 's10d270_orograph.npy')), plain)


def test_simulator_snapshot_mode_takes_the_wind_rasters(gpu, tmp_path):
    """Scattered wind samples: the per-cell rasters of _wind_rasters go through the sheltered kernel (a lattice would
    too: the fused lattice kernel has no shelter ray)."""
    from ssrs_amd import Simulator, layers
    rng = np.random.default_rng(4)
    gx, gy = np.meshgrid(np.arange(-2., 9., 2.), np.arange(-2., 8., 2.))
    x = (gx + rng.uniform(-0.3, 0.3, gx.shape)).ravel()
    y = (gy + rng.uniform(-0.3, 0.3, gy.shape)).ravel()
    ws = rng.uniform(4., 12., x.size)
    wd = (250. + rng.normal(0., 30., x.size)) % 360.
    item = dict(datetime=(2010, 6, 17, 13), wspeed=ws, wdirn=wd, x_km=x, y_km=y)
    sim = Simulator(sim_config(tmp_path, sim_mode='snapshot', run_name='snap'), terrain='synthetic', wind=[item])
    case = sim.case_ids[0]
    s, d = sim._wind_rasters(sim._wind[0])
    assert not bool(torch.isnan(d).any())
    dem = torch.from_numpy(sim.get_terrain_elevation()).cuda()
    oro, _, sx = layers.orographic_updraft_improved(dem, 100., s, d, want_sx=True)
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, f'{case}_orograph.npy')), oro.cpu().numpy())
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, f'{case}_sx.npy')), sx.to(torch.float32).cpu().numpy())
    # a lattice with 'linear' interpolation bypasses the fused lattice kernel as well
    xk, yk = np.arange(-2., 9., 2.), np.arange(-2., 8., 2.)
    lat = dict(datetime=(2010, 6, 17, 13), wspeed=ws.reshape(gx.shape), wdirn=wd.reshape(gx.shape), x_km=xk, y_km=yk)
    sim2 = Simulator(sim_config(tmp_path, sim_mode='snapshot', run_name='lat'), terrain='synthetic', wind=[lat])
    s, d = sim2._wind_rasters(sim2._wind[0])
    oro, _ = layers.orographic_updraft_improved(dem, 100., s, d)
    assert_same_bits(np.load(os.path.join(sim2.mode_data_dir, f'{case}_orograph.npy')), oro.cpu().numpy())
    assert os.path.exists(os.path.join(sim2.mode_data_dir, f'{case}_sx.npy'))
