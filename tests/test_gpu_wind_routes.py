"""The routes a wind case takes from its resolved form to `<case>_orograph.npy` (and `<case>_r0_thermals.npy`), through
the Simulator: every route's files equal, bit for bit, the library call that route stands for, made here directly.
Nine cases in seasonal mode, so a chunk of 8 and a rest of 1 both occur.  The samples sit on a 3 x 4 lattice from -1 km
to 5 km around the 3 km x 4 km region, so no cell lies outside their hull."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NCASE, CHUNK = 9, 8
GRID, RES = (30, 40), 100.
XK, YK = np.linspace(-1., 5., 4), np.linspace(-1., 5., 3)
_rng = np.random.default_rng(17)
JITTER_DEG = _rng.uniform(-10., 10., (3, 4))                       # the same for every case: a small spread per case
WS = np.stack([np.full((3, 4), 6. + k) for k in range(NCASE)])
WD = np.stack([250. + 5. * k + JITTER_DEG for k in range(NCASE)])
GX, GY = (a.ravel() for a in np.meshgrid(XK, YK))
SX, SY = GX + _rng.uniform(-0.3, 0.3, 12), GY + _rng.uniform(-0.3, 0.3, 12)      # scattered: off the lattice
DATES = [(2010, 6, 1 + k, 13) for k in range(NCASE)]
ROUTES = ('fused lattice', 'lattice, one case on shifted axes', 'lattice, injected slope and aspect', 'lattice nearest',
          'lattice cubic', 'scattered nearest', 'scattered linear', 'scattered cubic')


def config(tmp_path, **kw):
    from ssrs_amd import Config
    args = dict(run_name='routes', out_dir=str(tmp_path), sim_seed=3, region_width_km=(4., 3.), resolution=RES,
                sim_mode='seasonal', track_count=4, thermals_realization_count=0)
    args.update(kw)
    return Config(**args)


def saved(sim, name):
    return [np.load(os.path.join(sim.mode_data_dir, f'{case}_{name}.npy')) for case in sim.case_ids]


def assert_files_equal(got, want):
    assert len(got) == len(want) == NCASE
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 == w.dtype and g.shape == GRID == w.shape
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), f'case {k}: {int((g != w).sum())} cells differ'
        assert float(g.max()) > 0.


@pytest.fixture(scope='module')
def dem(gpu):
    from ssrs_amd.synthetic import synthetic_dem
    return np.asarray(synthetic_dem(GRID, RES), dtype=np.float64)


@pytest.mark.parametrize('route', ROUTES)
def test_orograph_files_equal_the_routes_library_call(gpu, tmp_path, dem, route):
    from ssrs_amd import Simulator, layers
    from ssrs_amd.wind import interpolate_wind_lattice, interpolate_wind_scattered
    method = route.split()[-1] if route.split()[-1] in ('nearest', 'cubic') else 'linear'
    axes = [(XK + 0.5, YK) if route.endswith('shifted axes') and k == NCASE - 1 else (XK, YK) for k in range(NCASE)]
    if route.startswith('scattered'):
        wind = [dict(datetime=DATES[k], x_km=SX, y_km=SY, wspeed=WS[k].ravel(), wdirn=WD[k].ravel()) for k in range(NCASE)]
    else:
        wind = [dict(datetime=DATES[k], x_km=axes[k][0], y_km=axes[k][1], wspeed=WS[k], wdirn=WD[k]) for k in range(NCASE)]
    terrain = dem
    if 'injected' in route:
        slope, aspect = layers.slope_aspect(dem, RES)
        terrain = dict(Elevation=dem, Slope=slope + 0.25, Aspect=(aspect + 3.) % 360.)     # not what the fallback computes
    sim = Simulator(config(tmp_path, wtk_interp_type=method), terrain=terrain, wind=wind)
    assert sim.gridsize == GRID and len(sim.case_ids) == NCASE
    slope, aspect = sim.get_terrain_slope(), sim.get_terrain_aspect()
    want = []
    for b0 in range(0, NCASE, CHUNK):
        ks = range(b0, min(b0 + CHUNK, NCASE))
        if route == 'fused lattice':
            oro, _ = layers.updraft_from_dem_lattice(dem, RES, XK, YK, WS[b0:b0 + CHUNK], WD[b0:b0 + CHUNK])
        else:
            if route.startswith('scattered'):
                rasters = [interpolate_wind_scattered(SX, SY, WS[k].ravel(), WD[k].ravel(), GRID, RES, method=method) for k in ks]
            elif method == 'linear':
                rasters = [interpolate_wind_lattice(*axes[k], WS[k], WD[k], GRID, RES) for k in ks]
            else:
                rasters = [interpolate_wind_scattered(GX, GY, WS[k].ravel(), WD[k].ravel(), GRID, RES, method=method) for k in ks]
            assert not any(bool(torch.isnan(r).any()) for pair in rasters for r in pair)
            ws, wd = (torch.stack(r) for r in zip(*rasters))
            oro, _ = layers.orographic_updraft(ws, wd, torch.from_numpy(slope).cuda(), torch.from_numpy(aspect).cuda())
        want.extend(oro.cpu().numpy())
    assert_files_equal(saved(sim, 'orograph'), want)


def test_wtk_thermal_files_equal_the_fused_call_on_the_meshgrid_points(gpu, tmp_path, dem):
    from ssrs_amd import Simulator
    from ssrs_amd.thermals import compute_wtk_thermals
    rng = np.random.default_rng(23)
    layers4 = dict(pressure=rng.uniform(8.5e4, 9.5e4, (NCASE, 3, 4)), temperature=rng.uniform(10., 25., (NCASE, 3, 4)),
                   blheight=rng.uniform(600., 1500., (NCASE, 3, 4)), surfheatflux=rng.uniform(50., 400., (NCASE, 3, 4)))
    wind = [dict(datetime=DATES[k], x_km=XK, y_km=YK, wspeed=WS[k], wdirn=WD[k], **{n: a[k] for n, a in layers4.items()})
            for k in range(NCASE)]
    sim = Simulator(config(tmp_path, thermal_model='wtk', thermals_realization_count=1), terrain=dem, wind=wind)
    want = []
    for b0 in range(0, NCASE, CHUNK):
        chunk = [layers4[n][b0:b0 + CHUNK].reshape(-1, 12) for n in Simulator.THERMAL_LAYERS]
        want.extend(compute_wtk_thermals(GX, GY, *chunk, GRID, RES, float(sim.wtk_thermal_height), method='linear',
                                         dtype=torch.float32))
    assert_files_equal(saved(sim, 'r0_thermals'), want)
