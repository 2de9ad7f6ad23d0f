"""K10 through `Simulator`: origin='southwest_lonlat' places the grid by the projection, and terrain, turbines and
wind samples may then come in degrees.  A 60 x 50 grid at 100 m on the default southwest_lonlat and CRS, under a smooth
analytic longitude / latitude DEM with 1 / 1024 degree pixels (about 80 m x 110 m)."""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from warp_ref import analytic_dem

pytestmark = pytest.mark.gpu
STEP = 1. / 1024.


def _config(tmp_path, **kw):
    from ssrs_amd import Config
    base = Config(run_name='geo', out_dir=str(tmp_path), sim_seed=30, region_width_km=(5., 6.), resolution=100.,
                  track_count=50)
    return replace(base, **kw)


def _corners(cfg):
    """(projection, lon, lat) of the four corners of the grid the default origin would give."""
    from ssrs_amd import Projection
    proj = Projection.from_crs(cfg.projected_crs)
    west, south = proj.forward(*cfg.southwest_lonlat)
    east, north = west + 49 * 100., south + 59 * 100.
    lon, lat = proj.inverse([west, west, east, east], [south, north, south, north])
    return proj, lon, lat


def _dem(cfg, margin_px=4, north_up=True, cols=None):
    from ssrs_amd import LonLatRaster
    _, lon, lat = _corners(cfg)
    lon0 = (np.floor(lon.min() / STEP) - margin_px) * STEP
    lat0 = (np.floor(lat.min() / STEP) - margin_px) * STEP
    nx = int(np.ceil((lon.max() - lon0) / STEP)) + margin_px + 1
    ny = int(np.ceil((lat.max() - lat0) / STEP)) + margin_px + 1
    nx = nx if cols is None else cols
    data = analytic_dem(*np.meshgrid(lon0 + np.arange(nx) * STEP, lat0 + np.arange(ny) * STEP))
    if north_up:                       # the order a GeoTIFF comes in
        return LonLatRaster(np.ascontiguousarray(data[::-1]).astype(np.float32), lon0, lat0 + (ny - 1) * STEP, STEP, -STEP)
    return LonLatRaster(data, lon0, lat0, STEP, STEP)


def test_georeferenced_origin_and_warped_terrain(gpu, tmp_path):
    from ssrs_amd import Simulator, layers, warp_to_grid
    cfg = _config(tmp_path)
    proj, lon, lat = _corners(cfg)
    raster = _dem(cfg)
    sim = Simulator(cfg, terrain=raster, origin='southwest_lonlat')
    assert sim.gridsize == (60, 50) and sim.projection == proj
    assert sim.bounds[:2] == tuple(float(v) for v in proj.forward(*cfg.southwest_lonlat))
    assert sim.bounds[2:] == (sim.bounds[0] + 49 * 100., sim.bounds[1] + 59 * 100.)
    w, s, e, n = sim.lonlat_bounds
    assert np.all((lon >= w) & (lon <= e) & (lat >= s) & (lat <= n))
    assert (w, s, e, n) == (lon.min(), lat.min(), lon.max(), lat.max())
    dem, uncovered = warp_to_grid(raster, cfg.projected_crs, sim.bounds[0], sim.bounds[1], sim.gridsize, cfg.resolution)
    assert uncovered == 0
    elevation = sim.get_terrain_elevation()
    assert elevation.dtype == np.float64 and np.array_equal(elevation, dem.cpu().numpy())
    # the terrain is the analytic surface: bilinear interpolation of a smooth field on 100 m pixels, well within 1 m
    x, y = np.meshgrid(*sim.get_terrain_grid())
    assert np.abs(elevation - analytic_dem(*proj.inverse(x, y))).max() < 1.
    # from here on the run is an ordinary uniform one: the orograph of the fused DEM kernel
    want, _ = layers.updraft_from_dem(elevation, cfg.resolution, float(cfg.uniform_windspeed), float(cfg.uniform_winddirn))
    got = np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy'))
    assert got.dtype == np.float32 and np.array_equal(got, np.asarray(want, dtype=np.float32))
    assert np.array_equal(sim.get_terrain_slope(), layers.compute_slope_degrees(elevation, cfg.resolution))

    # a south-up f64 source gives the same terrain to f32 rounding of the pixels
    again = Simulator(replace(cfg, run_name='s'), terrain=_dem(cfg, north_up=False), origin='southwest_lonlat')
    assert np.abs(again.get_terrain_elevation() - elevation).max() < 1e-3


def test_a_source_that_is_too_small_raises_with_the_count(gpu, tmp_path):
    from ssrs_amd import Simulator, warp_to_grid
    cfg = _config(tmp_path)
    proj, _, _ = _corners(cfg)
    small = _dem(cfg, cols=40)
    west, south = proj.forward(*cfg.southwest_lonlat)
    _, count = warp_to_grid(small, proj, west, south, (60, 50), 100.)
    assert 0 < count < 3000
    with pytest.raises(ValueError, match=rf'{count} of the 3000 cells are not covered.*lonlat_bounds = \['):
        Simulator(cfg, terrain=small, origin='southwest_lonlat')


def test_turbines_in_degrees_land_in_the_same_cells(gpu, tmp_path):
    from ssrs_amd import Simulator
    cfg = _config(tmp_path)
    proj, lon, lat = _corners(cfg)
    rng = np.random.default_rng(8)
    xlong = rng.uniform(lon.min() - 0.01, lon.max() + 0.01, 40)
    ylat = rng.uniform(lat.min() - 0.01, lat.max() + 0.01, 40)
    table = dict(p_name=np.array(['A', 'B'] * 20), t_hh=rng.uniform(40., 120., 40), xlong=xlong, ylat=ylat)
    x, y = proj.forward(xlong, ylat)
    a = Simulator(cfg, terrain='synthetic', origin='southwest_lonlat', turbines=table)
    b = Simulator(replace(cfg, run_name='b'), terrain='synthetic', origin='southwest_lonlat',
                  turbines=dict(p_name=table['p_name'], t_hh=table['t_hh'], x=x, y=y))
    assert 0 < len(a.turbines) < 40                              # the filter to the bounds and the hub height ran
    cells = a.turbines.cell_coordinates(a.bounds, a.resolution)
    assert np.array_equal(cells, b.turbines.cell_coordinates(b.bounds, b.resolution))
    assert cells.min() >= 0. and cells[:, 0].max() <= 49. and cells[:, 1].max() <= 59.
    # the degrees are carried along, filtered with the rest
    assert np.array_equal(np.stack(proj.forward(a.turbines.columns['xlong'], a.turbines.columns['ylat'])),
                          np.stack(a.turbines.get_locations()))


def _wind_entry(cfg, **where):
    rng = np.random.default_rng(9)
    n = 25
    return dict(datetime=cfg.snapshot_datetime, wspeed=rng.uniform(4., 12., n), wdirn=rng.uniform(200., 320., n), **where)


def test_wind_samples_in_degrees_give_the_same_rasters(gpu, tmp_path):
    from ssrs_amd import Simulator
    cfg = _config(tmp_path, sim_mode='snapshot')
    proj, lon, lat = _corners(cfg)
    glon, glat = np.meshgrid(np.linspace(lon.min() - 0.02, lon.max() + 0.02, 5), np.linspace(lat.min() - 0.02, lat.max() + 0.02, 5))
    glon, glat = glon.ravel(), glat.ravel()
    west, south = proj.forward(*cfg.southwest_lonlat)
    x, y = proj.forward(glon, glat)
    a = Simulator(cfg, terrain='synthetic', origin='southwest_lonlat', wind=[_wind_entry(cfg, lon=glon, lat=glat)])
    b = Simulator(replace(cfg, run_name='b'), terrain='synthetic', origin='southwest_lonlat',
                  wind=[_wind_entry(cfg, x_km=(x - west) / 1000., y_km=(y - south) / 1000.)])
    for got, want in zip(a._wind_rasters(a._wind[0]), b._wind_rasters(b._wind[0])):
        assert not bool(torch.isnan(want).any()) and torch.equal(got, want)
    files = [np.load(s._get_orograph_fname(s.case_ids[0], s.mode_data_dir) + '.npy') for s in (a, b)]
    assert np.array_equal(files[0], files[1]) and files[0].max() > 0.
    # a lattice in degrees (axes and (ny, nx) arrays) is its meshgrid points
    ws, wd = (np.asarray(v).reshape(5, 5) for v in a._wind[0].wind.values)
    c = Simulator(replace(cfg, run_name='c'), terrain='synthetic', origin='southwest_lonlat',
                  wind=[dict(datetime=cfg.snapshot_datetime, wspeed=ws, wdirn=wd, lon=glon[:5], lat=glat[::5])])
    assert np.array_equal(np.load(c._get_orograph_fname(c.case_ids[0], c.mode_data_dir) + '.npy'), files[0])
    with pytest.raises(ValueError, match="both 'lon' / 'lat' and 'x_km' / 'y_km'"):
        Simulator(replace(cfg, run_name='d'), terrain='synthetic', origin='southwest_lonlat',
                  wind=[_wind_entry(cfg, lon=glon, lat=glat, x_km=x / 1000., y_km=y / 1000.)])


def test_inputs_in_degrees_need_the_georeferenced_origin(gpu, tmp_path):
    from ssrs_amd import Simulator
    cfg = _config(tmp_path)
    _, lon, lat = _corners(cfg)
    for origin in ((0., 0.), (-783797.7, 370554.4)):
        with pytest.raises(ValueError, match="terrain=LonLatRaster.*origin='southwest_lonlat'"):
            Simulator(cfg, terrain=_dem(cfg), origin=origin)
        with pytest.raises(ValueError, match="turbines=.*origin='southwest_lonlat'"):
            Simulator(cfg, terrain='synthetic', origin=origin, turbines=dict(xlong=lon, ylat=lat))
        with pytest.raises(ValueError, match="wind samples at 'lon', 'lat'.*origin='southwest_lonlat'"):
            Simulator(replace(cfg, sim_mode='snapshot'), terrain='synthetic', origin=origin,
                      wind=[_wind_entry(cfg, lon=np.resize(lon, 25), lat=np.resize(lat, 25))])
    with pytest.raises(ValueError, match='southwest_lonlat'):
        Simulator(cfg, terrain='synthetic', origin='northeast')
    with pytest.raises(ValueError, match='ESRI:102008'):
        Simulator(replace(cfg, projected_crs='EPSG:32613'), terrain='synthetic', origin='southwest_lonlat')


def test_defaults_are_unchanged(gpu, tmp_path):
    """A numeric origin and array terrain: no projection, lonlat_bounds stays None, the projected CRS is not even read."""
    from ssrs_amd import Simulator
    sim = Simulator(_config(tmp_path, projected_crs='EPSG:32613'), terrain='synthetic')
    assert sim.projection is None and sim.lonlat_bounds is None and sim.bounds[:2] == (0., 0.)
    with pytest.raises(NotImplementedError):
        Simulator(_config(tmp_path, run_name='n'), terrain=None)
