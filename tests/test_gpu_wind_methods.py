"""`wtk_interp_type` 'nearest' and 'cubic' on the device against scipy itself (the reference hands the field to
scipy.interpolate.griddata, ssrs/simulator.py:774-775): the kernels behind `interpolate_wind_scattered(method=...)`
on three random clouds, a jittered 2 km lattice with three snapshots and the exact lattice (whose midlines are ties
of the nearest rule), batching, the prebuilt index, 'linear' left as it was, and `Simulator` in snapshot and seasonal
mode."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CLOUDS = [(180, 230, 0.1, 60, 1), (400, 300, 0.01, 400, 2), (97, 1031, 0.05, 12, 3)]


def _geometries():
    """(name, rows, cols, cell, x, y, wspeed (B, npts), wdirn (B, npts))"""
    out = []
    for rows, cols, cell, npts, seed in CLOUDS:
        rng = np.random.default_rng(seed)
        w, h = (cols - 1) * cell, (rows - 1) * cell
        x = rng.uniform(-0.1 * w, 1.1 * w, npts)
        y = rng.uniform(-0.1 * h, 1.1 * h, npts)
        ws = rng.uniform(0., 15., npts)
        wd = rng.uniform(0., 360., npts)
        out.append((f'cloud{seed}', rows, cols, cell, x, y, ws[None], wd[None]))
    for name, jitter in (('jittered', 1.), ('lattice', 0.)):
        rng = np.random.default_rng(9)
        gx, gy = np.meshgrid(np.arange(-2., 33., 2.), np.arange(-2., 23., 2.))
        x = (gx + jitter * rng.uniform(-0.3, 0.3, gx.shape)).ravel()
        y = (gy + jitter * rng.uniform(-0.3, 0.3, gy.shape)).ravel()
        ws = rng.uniform(2., 14., (3, x.size))
        wd = (270. + rng.normal(0., 40., (3, x.size))) % 360.
        out.append((name, 200, 300, 0.1, x, y, ws, wd))
    return out


GEOMETRIES = _geometries()


def _reference(x, y, ws, wd, rows, cols, cell, method):
    """(speed, direction, east, north) as the reference computes them (simulator.py:778-792)."""
    from scipy.interpolate import griddata
    east = ws * np.sin(wd * np.pi / 180.)
    north = ws * np.cos(wd * np.pi / 180.)
    xm, ym = np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)
    pts = np.array([x, y]).T
    ie = griddata(pts, east, (xm, ym), method=method)
    inn = griddata(pts, north, (xm, ym), method=method)
    spd = np.sqrt(np.square(ie) + np.square(inn))
    ang = np.mod(np.arctan2(ie, inn) + 2. * np.pi, 2. * np.pi) * 180. / np.pi
    return spd, ang, ie, inn


def _direction_gap(a, b):
    dd = np.abs(a - b)
    return np.minimum(dd, 360. - dd)


@pytest.mark.parametrize('geometry', GEOMETRIES, ids=lambda g: g[0])
def test_cubic_vs_scipy_griddata(gpu, geometry):
    from ssrs_amd.wind import interpolate_wind_scattered
    name, rows, cols, cell, x, y, ws, wd = geometry
    s, d = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method='cubic')
    assert tuple(s.shape) == (ws.shape[0], rows, cols) and s.dtype == torch.float64
    s, d = s.cpu().numpy(), d.cpu().numpy()
    for b in range(ws.shape[0]):
        ref_s, ref_d, ref_e, ref_n = _reference(x, y, ws[b], wd[b], rows, cols, cell, 'cubic')
        got_s, got_d = s[b], d[b]
        nan_g, nan_r = np.isnan(got_s), np.isnan(ref_s)
        mismatch = float(np.mean(nan_g != nan_r))
        ok = ~nan_g & ~nan_r
        assert ok.sum() > 0
        top = float(np.max(np.abs(ref_s[ok])))
        bound = 1e-10 * max(1., top)
        rad = got_d[ok] * np.pi / 180.
        err_s = float(np.max(np.abs(got_s[ok] - ref_s[ok])))
        err_e = float(np.max(np.abs(got_s[ok] * np.sin(rad) - ref_e[ok])))
        err_n = float(np.max(np.abs(got_s[ok] * np.cos(rad) - ref_n[ok])))
        strong = ref_s[ok] > 1e-3 * top
        err_d = float(np.max(_direction_gap(got_d[ok], ref_d[ok])[strong]))
        print(f'cubic {name}[{b}]: NaN mismatch {mismatch:.3g}, |speed| {err_s:.3g}, |east| {err_e:.3g}, |north| {err_n:.3g} '
              f'(bound {bound:.3g}), direction {err_d:.3g} deg (bound 1e-7), max ref speed {top:.4g}')
        assert mismatch < 1e-4
        assert err_s <= bound and err_e <= bound and err_n <= bound
        assert err_d <= 1e-7
        assert np.array_equal(np.isnan(got_d), nan_g)


@pytest.mark.parametrize('geometry', GEOMETRIES, ids=lambda g: g[0])
def test_nearest_vs_ckdtree(gpu, geometry):
    from scipy.spatial import cKDTree
    from ssrs_amd.wind import interpolate_wind_scattered, nearest_sample_index
    name, rows, cols, cell, x, y, ws, wd = geometry
    index = nearest_sample_index(x, y, (rows, cols), cell * 1000.)
    assert index.dtype == torch.int32 and tuple(index.shape) == (rows, cols)
    got = index.cpu().numpy().ravel().astype(np.int64)
    assert got.min() >= 0 and got.max() < x.size
    pts = np.array([x, y]).T
    xm, ym = np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)
    cells = np.stack([xm.ravel(), ym.ravel()], 1)
    dist, near = cKDTree(pts).query(cells, k=2)
    tie = dist[:, 1]**2 <= dist[:, 0]**2 * (1. + 1e-12)
    print(f'nearest {name}: {int(tie.sum())} tie cells of {tie.size}')
    assert np.array_equal(got[~tie], near[~tie, 0])
    if tie.any():
        tc = cells[tie]
        d_all = np.sqrt((tc[:, None, 0] - pts[None, :, 0])**2 + (tc[:, None, 1] - pts[None, :, 1])**2)    # (ties, npts)
        as_near = d_all <= dist[tie, 0][:, None] * (1. + 1e-12)
        assert np.all(as_near[np.arange(tc.shape[0]), got[tie]])
        assert np.array_equal(got[tie], np.argmax(as_near, axis=1))          # the lowest index among those
    if name == 'lattice':
        assert tie.sum() > 0.05 * tie.size           # 100 m cells on the midlines of a 2 km lattice: the tie rule is exercised
    s, d = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method='nearest')
    assert tuple(s.shape) == (ws.shape[0], rows, cols) and s.dtype == torch.float64
    s, d = s.cpu().numpy(), d.cpu().numpy()
    assert not np.isnan(s).any() and not np.isnan(d).any()
    for b in range(ws.shape[0]):
        east, north = ws[b] * np.sin(wd[b] * np.pi / 180.), ws[b] * np.cos(wd[b] * np.pi / 180.)
        spd = np.sqrt(np.square(east) + np.square(north))
        ang = np.mod(np.arctan2(east, north) + 2. * np.pi, 2. * np.pi) * 180. / np.pi
        want_s, want_d = spd[got], ang[got]
        top = float(np.max(want_s))
        err_s = float(np.max(np.abs(s[b].ravel() - want_s)))
        strong = want_s > 1e-3 * top
        err_d = float(np.max(_direction_gap(d[b].ravel(), want_d)[strong]))
        print(f'nearest {name}[{b}]: |speed| {err_s:.3g} (bound {1e-10 * max(1., top):.3g}), direction {err_d:.3g} deg')
        assert err_s <= 1e-10 * max(1., top)
        assert err_d <= 1e-7


def test_nearest_tie_rule_is_lowest_index(gpu):
    """Lowest index among ALL equally near samples on the exact lattice, by brute force in the kernel's arithmetic
    (d^2 = dx * dx + dy * dy in f64, unfused)."""
    from ssrs_amd.wind import nearest_sample_index
    _, rows, cols, cell, x, y, _, _ = GEOMETRIES[4]
    got = nearest_sample_index(x, y, (rows, cols), cell * 1000.).cpu().numpy()
    xm, ym = np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)
    dx, dy = xm[..., None] - x, ym[..., None] - y
    d2 = dx * dx + dy * dy
    assert np.array_equal(got, np.argmin(d2, axis=2))            # (argmin returns the first minimum)


@pytest.mark.parametrize('method', ['nearest', 'cubic'])
def test_batch_equals_single_calls(gpu, method):
    from ssrs_amd.wind import interpolate_wind_scattered
    _, rows, cols, cell, x, y, ws, wd = GEOMETRIES[3]
    s, d = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method=method)
    for b in range(3):
        s1, d1 = interpolate_wind_scattered(x, y, ws[b], wd[b], (rows, cols), cell * 1000., method=method)
        assert tuple(s1.shape) == (rows, cols)
        assert torch.equal(s1, s[b]) and torch.equal(d1, d[b])


def test_prebuilt_index_equals_none(gpu):
    from ssrs_amd.wind import interpolate_wind_scattered, nearest_sample_index
    _, rows, cols, cell, x, y, ws, wd = GEOMETRIES[3]
    index = nearest_sample_index(x, y, (rows, cols), cell * 1000.)
    s0, d0 = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method='nearest')
    s1, d1 = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method='nearest', index=index)
    assert torch.equal(s0, s1) and torch.equal(d0, d1)
    with pytest.raises(ValueError):
        interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method='nearest', index=index[:10])


def test_many_samples_take_the_same_values(gpu):
    """More samples than the per-block table of ssrs_wind_from_nearest holds, and more candidates per tile than the
    cull keeps (a dense cloud under coarse cells): the general paths give what the fast ones give."""
    from scipy.spatial import cKDTree
    from ssrs_amd.wind import interpolate_wind_scattered, nearest_sample_index
    rng = np.random.default_rng(21)
    rows, cols, cell, npts = 70, 90, 0.1, 5000
    x, y = rng.uniform(-1., 10., npts), rng.uniform(-1., 8., npts)
    ws, wd = rng.uniform(1., 15., npts), rng.uniform(0., 360., npts)
    got = nearest_sample_index(x, y, (rows, cols), cell * 1000.).cpu().numpy().ravel()
    xm, ym = np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)
    dist, near = cKDTree(np.array([x, y]).T).query(np.stack([xm.ravel(), ym.ravel()], 1), k=2)
    tie = dist[:, 1]**2 <= dist[:, 0]**2 * (1. + 1e-12)
    assert np.array_equal(got[~tie], near[~tie, 0]) and tie.mean() < 1e-3
    s, d = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method='nearest')
    east, north = ws * np.sin(wd * np.pi / 180.), ws * np.cos(wd * np.pi / 180.)
    spd = np.sqrt(np.square(east) + np.square(north))
    ang = np.mod(np.arctan2(east, north) + 2. * np.pi, 2. * np.pi) * 180. / np.pi
    assert np.max(np.abs(s.cpu().numpy().ravel() - spd[got])) <= 1e-10 * max(1., float(spd.max()))
    assert np.max(_direction_gap(d.cpu().numpy().ravel(), ang[got])) <= 1e-7


def test_nearest_cull_engages_and_is_not_needed(gpu):
    """The per-tile cull serves every tile of the 2 km lattice and none of a dense cloud (the first int32 of the
    workspace counts the tiles that scanned all samples); both index rasters were checked above."""
    import ctypes as C
    from ssrs_amd import _native as nat
    from ssrs_amd._device import stream_ptr, to_dev
    L = nat.lib()
    rng = np.random.default_rng(21)
    dense = (70, 90, 0.1, rng.uniform(-1., 10., 5000), rng.uniform(-1., 8., 5000))
    for (rows, cols, cell, x, y), want in ((GEOMETRIES[3][1:6], 'none'), (dense, 'all')):
        pts = to_dev(np.ascontiguousarray(np.stack([x, y], 1)), torch.float64)
        index = torch.empty((rows, cols), dtype=torch.int32, device=pts.device)
        nbytes = int(L.ssrs_wind_nearest_workspace_bytes(int(x.size), rows, cols))
        scratch = torch.full((nbytes,), 0xff, dtype=torch.uint8, device=pts.device)
        nat.check(L.ssrs_wind_nearest_index(nat.ptr(pts), int(x.size), C.c_double(cell), nat.ptr(index), rows, cols,
                                            nat.ptr(scratch), C.c_size_t(nbytes), stream_ptr()))
        full = int(scratch[:4].view(torch.int32).item())
        tiles = -(-rows // 32) * -(-cols // 64)
        assert full == (0 if want == 'none' else tiles), (full, tiles)


def test_linear_is_the_default_and_unchanged(gpu):
    from ssrs_amd.wind import interpolate_wind_scattered
    _, rows, cols, cell, x, y, ws, wd = GEOMETRIES[3]
    s0, d0 = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000.)
    for method in ('linear', 'Linear'):
        s1, d1 = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method=method)
        assert torch.equal(s0, s1) and torch.equal(d0, d1)
    with pytest.raises(ValueError):
        interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method='spline')


def _scattered_case(rng):
    from ssrs_amd.synthetic import synthetic_dem
    rows, cols, res = 120, 160, 100.
    dem = synthetic_dem((rows, cols), res)
    gx, gy = np.meshgrid(np.arange(-2., 19., 2.), np.arange(-2., 15., 2.))
    x = (gx + rng.uniform(-0.3, 0.3, gx.shape)).ravel()
    y = (gy + rng.uniform(-0.3, 0.3, gy.shape)).ravel()
    ws = rng.uniform(4., 12., x.size)
    wd = (250. + rng.normal(0., 30., x.size)) % 360.
    return rows, cols, res, dem, x, y, ws, wd


def _config(tmp_path, name, rows, cols, res, **kw):
    from ssrs_amd import Config
    return Config(run_name=name, out_dir=str(tmp_path), region_width_km=(cols * res / 1000., rows * res / 1000.), resolution=res,
                  track_count=10, sim_seed=3, **kw)


def _orograph(sim, case_id):
    return np.load(sim._get_orograph_fname(case_id, sim.mode_data_dir) + '.npy')


@pytest.mark.parametrize('interp', ['nearest', 'cubic', 'CUBIC'])
def test_snapshot_mode_with_scattered_wind(gpu, tmp_path, interp):
    """The orograph file is the three-kernel chain on the rasters scipy's griddata gives with that method (what the
    reference computes, simulator.py:200-215)."""
    from ssrs_amd import Simulator, layers
    rows, cols, res, dem, x, y, ws, wd = _scattered_case(np.random.default_rng(4))
    cfg = _config(tmp_path, 'scat_' + interp, rows, cols, res, sim_mode='snapshot', snapshot_datetime=(2010, 6, 17, 13),
                  wtk_interp_type=interp)
    sim = Simulator(cfg, terrain=dem, wind=[dict(datetime=(2010, 6, 17, 13), wspeed=ws, wdirn=wd, x_km=x, y_km=y)])
    oro = _orograph(sim, sim.case_ids[0])
    ref_s, ref_d, _, _ = _reference(x, y, ws, wd, rows, cols, res / 1000., interp.lower())
    slope, aspect = layers.slope_aspect(torch.from_numpy(dem).cuda(), res)
    want, _ = layers.orographic_updraft(torch.from_numpy(ref_s).cuda(), torch.from_numpy(ref_d).cuda(), slope, aspect)
    want = want.cpu().numpy()
    assert oro.shape == want.shape and oro.dtype == want.dtype
    err = float(np.max(np.abs(oro.astype(np.float64) - want.astype(np.float64))))
    print(f'{interp}: max |orograph - chain on griddata| = {err:.3g} (bound {1e-5 * max(1., float(np.abs(want).max())):.3g})')
    assert err <= 1e-5 * max(1., float(np.abs(want).max()))


def test_snapshot_mode_lattice_wind_cubic_goes_through_the_scattered_path(gpu, tmp_path):
    """Wind on a regular lattice (ny, nx) with 'cubic' is the scattered call on the meshgrid points: the reference
    triangulates whatever points it gets."""
    from ssrs_amd import Simulator
    from ssrs_amd.synthetic import synthetic_dem
    rng = np.random.default_rng(5)
    rows, cols, res = 120, 160, 100.
    dem = synthetic_dem((rows, cols), res)
    xk, yk = np.arange(-2., 19., 2.), np.arange(-2., 15., 2.)
    ws = rng.uniform(4., 12., (yk.size, xk.size))
    wd = (250. + rng.normal(0., 30., ws.shape)) % 360.
    gx, gy = np.meshgrid(xk, yk)
    oro = []
    for name, item in (('lat', dict(wspeed=ws, wdirn=wd, x_km=xk, y_km=yk)),
                       ('pts', dict(wspeed=ws.ravel(), wdirn=wd.ravel(), x_km=gx.ravel(), y_km=gy.ravel()))):
        cfg = _config(tmp_path, name, rows, cols, res, sim_mode='snapshot', snapshot_datetime=(2010, 6, 17, 13),
                      wtk_interp_type='cubic')
        sim = Simulator(cfg, terrain=dem, wind=[dict(datetime=(2010, 6, 17, 13), **item)])
        oro.append(_orograph(sim, sim.case_ids[0]))
    assert np.array_equal(oro[0], oro[1])
    # and it is not what the fused lattice kernel ('linear') writes
    cfg = _config(tmp_path, 'lin', rows, cols, res, sim_mode='snapshot', snapshot_datetime=(2010, 6, 17, 13))
    sim = Simulator(cfg, terrain=dem, wind=[dict(datetime=(2010, 6, 17, 13), wspeed=ws, wdirn=wd, x_km=xk, y_km=yk)])
    assert not np.array_equal(oro[0], _orograph(sim, sim.case_ids[0]))


def test_seasonal_mode_lattice_wind_nearest(gpu, tmp_path):
    """Three lattice snapshots in seasonal mode with 'nearest': three orograph files, each the file its own
    single-case run writes."""
    from ssrs_amd import Simulator
    from ssrs_amd.synthetic import synthetic_dem
    rng = np.random.default_rng(6)
    rows, cols, res = 120, 160, 100.
    dem = synthetic_dem((rows, cols), res)
    xk, yk = np.arange(-2., 19., 2.), np.arange(-2., 15., 2.)
    items = []
    for k in range(3):
        ws = rng.uniform(4., 12., (yk.size, xk.size))
        wd = (250. + rng.normal(0., 30., ws.shape)) % 360.
        items.append(dict(datetime=(2010, 3 + k, 10 + k, 12), wspeed=ws, wdirn=wd, x_km=xk, y_km=yk))
    cfg = _config(tmp_path, 'season', rows, cols, res, sim_mode='seasonal', wtk_interp_type='nearest')
    sim = Simulator(cfg, terrain=dem, wind=items)
    assert len(sim.case_ids) == 3
    for k, case_id in enumerate(sim.case_ids):
        one = Simulator(_config(tmp_path, f'one{k}', rows, cols, res, sim_mode='snapshot',
                                snapshot_datetime=items[k]['datetime'], wtk_interp_type='nearest'),
                        terrain=dem, wind=[items[k]])
        a, b = _orograph(sim, case_id), _orograph(one, one.case_ids[0])
        assert a.shape == (rows, cols) and np.array_equal(a, b)
        assert not np.isnan(a).any() and float(np.abs(a).max()) > 0.
    assert not np.array_equal(_orograph(sim, sim.case_ids[0]), _orograph(sim, sim.case_ids[1]))
