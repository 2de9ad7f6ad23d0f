"""K1 on the DEMs that smooth synthetic terrain never produces: plateaus (interior cells with
dz_dx == 0, where the reference substitutes 1e-10, layers.py:124, and three kernels carry a
second hand-written formula), ridges, nodata (NaN) cells and rasters ragged against the
32 x 64 tile -- through every entry point and template variant of raster.hip.

References: fixture G14 (tests/golden/g14_raster_edges.npz, written by the reference; the
oracle is pinned to it by test_oracle_golden.py::test_g14_raster_edges) and the oracle on
other shapes.  f32 DEMs / rasters are exact numbers computed in f64 (ssrs_amd/layers.py), so
they are compared with the oracle on the widened values.  Criteria and their reasons:
tests/raster_checks.py.

Winds: the 1e-10 changes a value by about 1e-10 / dz_dy * tan(angle to the ridge) relatively,
so only winds close to a ridge's direction (270, and 85 / 95 / 265 / 275) tell the second
formula from the first; they are in every wind list here for that reason.
"""
import numpy as np
import pytest
import torch

from raster_checks import (SLOPE_TOL, ASPECT_TOL, USABLE_TOL, branch_share, check_orograph_cells,
                           check_usable, lattice_reference, nan_stencil_cells)

pytestmark = pytest.mark.gpu

G14_DEMS = ('integer', 'terraced', 'ridge_cols', 'ridge_rows', 'nodata')
SHAPES = [(3, 3), (4, 5), (31, 63), (32, 64), (33, 65), (97, 161), (130, 67)]
RAGGED = {(97, 161), (130, 67)}
WINDS = (0., 90., 180., 270., 45., 123.4, -30., 725., 85., 95., 265., 275.)
SPEEDS = (7.5, 3.0, 20.0)
THRESHOLDS = (0.3, 0.75, 2.0)


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def oracle_chain(z, res, wspeed, wdirn, min_val=0.):
    from oracle import ssrs_oracle as orc
    z = np.asarray(z, dtype=np.float64)
    return orc.compute_orographic_updraft(wspeed, wdirn, orc.compute_slope_degrees(z, res),
                                          orc.compute_aspect_degrees(z, res), min_val)


def assert_branch_reached(z, res, least=0.01):
    from oracle import ssrs_oracle as orc
    share = branch_share(z, res, orc)
    assert share >= least, f'only {share:.4f} of the cells have dz_dx == 0 != dz_dy'


# ----------------------------------------------------------------------------------------------
# 1. G14 through every entry point
@pytest.mark.parametrize('name', G14_DEMS)
def test_g14_every_entry_point(gpu, golden, name):
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    g = golden('g14_raster_edges.npz')
    res, thr = float(g['res']), float(g['threshold'])
    dem = g[f'{name}_dem']
    z = dem.astype(np.float64)
    g_slope, g_aspect = g[f'{name}_slope'], g[f'{name}_aspect']
    if name in ('integer', 'terraced', 'ridge_cols', 'nodata'):
        assert_branch_reached(z, res)
    hit = nan_stencil_cells(z)
    assert hit.any() == (name == 'nodata')
    assert (g_slope[hit] == 0).all() and (g_aspect[hit] == 0).all()      # what nan_to_num left

    slope, aspect = layers.slope_aspect(z, res)
    assert slope.dtype == np.float64 and aspect.dtype == np.float64
    assert not np.isnan(slope).any() and not np.isnan(aspect).any()
    np.testing.assert_allclose(slope, g_slope, **SLOPE_TOL)
    np.testing.assert_allclose(aspect, g_aspect, **ASPECT_TOL)
    assert (slope[hit] == 0).all() and (aspect[hit] == 0).all()
    np.testing.assert_array_equal(layers.compute_slope_degrees(z, res), slope)
    np.testing.assert_array_equal(layers.compute_aspect_degrees(z, res), aspect)

    most_signal = 0
    for j, (ws, wd, mn) in enumerate(g['cases']):
        ws, wd, mn = float(ws), float(wd), float(mn)
        ref = orc.compute_orographic_updraft(ws, wd, g_slope, g_aspect, mn)
        ref32, ref_use = g[f'{name}_oro{j}'], g[f'{name}_use{j}']
        assert np.array_equal(ref.astype(np.float32), ref32)
        assert (ref32[hit] == np.float32(mn)).all()

        oro = layers.compute_orographic_updraft(ws, wd, g_slope, g_aspect, mn)
        st = check_orograph_cells(oro, ref, ws, f'k_orographic g14/{name} wind {wd:g}')
        most_signal = max(most_signal, st['signal'])
        assert (oro[hit] == np.float32(mn)).all()

        use = layers.get_above_threshold_speed(ref32, thr)
        assert use.dtype == np.float64
        np.testing.assert_allclose(use, ref_use, **USABLE_TOL)

        # the DEM as stored (int16, or f32 with NaN: promoted / the f32 instantiation) and as f64
        for d in (dem, z):
            oro, use = layers.updraft_from_dem(d, res, ws, wd, threshold=thr, min_updraft_val=mn)
            st = check_orograph_cells(oro, ref, ws, f'k_updraft_from_dem g14/{name} wind {wd:g}')
            most_signal = max(most_signal, st['signal'])
            check_usable(use, oro, thr, ref32, ref_use, orc)
            assert not np.isnan(oro).any()
            # nodata: the reference's slope = aspect = 0 there, so orograph = max(min_updraft_val, 0)
            # and its usable updraft is 0 for min_updraft_val = 0 (0.05 is above the function's
            # 0.01 cut-off, so there it is the reference's small positive value)
            assert (oro[hit] == np.float32(mn)).all()
            np.testing.assert_allclose(use[hit], ref_use[hit], **USABLE_TOL)
            if mn == 0.:
                assert (use[hit] == 0).all()
    assert most_signal >= 1000, most_signal


# ----------------------------------------------------------------------------------------------
# 2. fused kernel: variant and shape matrix against the oracle
def matrix_dem(shape, kind, dtype, index):
    from ssrs_amd.synthetic import synthetic_dem
    z = synthetic_dem(shape, 30., seed=20 + index)
    if kind == 'integer':
        z = np.rint(z)
    return z.astype(dtype)          # int16 truncates a smooth DEM: integer metres either way


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('kind', ('smooth', 'integer'))
@pytest.mark.parametrize('dtype', (np.float64, np.float32, np.int16), ids=lambda d: np.dtype(d).name)
def test_fused_matrix_vs_oracle(gpu, shape, kind, dtype):
    """Every shape meets both DEM kinds and the three DEM dtypes; in each of these cases every wind
    is run with a threshold that rotates with it, with both min_updraft_val on the ragged shapes
    and alternating ones elsewhere: every wind, min_updraft_val and threshold meets all seven
    shapes and both DEM kinds."""
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    res = 30.
    dem = matrix_dem(shape, kind, dtype, SHAPES.index(shape))
    z = dem.astype(np.float64)
    if shape[0] >= 31 and (kind == 'integer' or dtype == np.int16):
        assert_branch_reached(z, res)
    slope, aspect = orc.compute_slope_degrees(z, res), orc.compute_aspect_degrees(z, res)
    label = f'k_updraft_from_dem {kind}/{np.dtype(dtype).name}/{shape[0]}x{shape[1]}'
    most_signal = 0
    for i, wd in enumerate(WINDS):
        ws = SPEEDS[i % 3]
        for k, mn in enumerate((0., 0.05) if shape in RAGGED else ((0., 0.05)[i % 2],)):
            thr = THRESHOLDS[(i + k) % 3]
            ref = orc.compute_orographic_updraft(ws, wd, slope, aspect, mn)
            ref32 = ref.astype(np.float32)
            ref_use = orc.get_above_threshold_speed(ref32, thr)
            oro, use = layers.updraft_from_dem(dem, res, ws, wd, threshold=thr, min_updraft_val=mn)
            assert oro.dtype == np.float32 and oro.shape == shape
            st = check_orograph_cells(oro, ref, ws, f'{label} wind {wd:g}')
            most_signal = max(most_signal, st['signal'])
            check_usable(use, oro, thr, ref32, ref_use, orc)
            assert (oro[0] == np.float32(mn)).all() and (oro[:, -1] == np.float32(mn)).all()
            if k == 0 and i % 4 == 3:
                # the other ways to call it give the same bits
                only_use = layers.updraft_from_dem(dem, res, ws, wd, threshold=thr, min_updraft_val=mn,
                                                   want_orograph=False)
                assert only_use[0] is None and np.array_equal(only_use[1], use)
                only_oro = layers.updraft_from_dem(dem, res, ws, wd, min_updraft_val=mn)
                assert only_oro[1] is None and np.array_equal(only_oro[0], oro)
                o = torch.full(shape, -1., dtype=torch.float32, device='cuda')
                u = torch.full(shape, -1., dtype=torch.float64, device='cuda')
                layers.updraft_from_dem(dem, res, ws, wd, threshold=thr, min_updraft_val=mn, out=(o, u))
                assert np.array_equal(host(o), oro) and np.array_equal(host(u), use)
                u.fill_(-1.)
                layers.updraft_from_dem(dem, res, ws, wd, threshold=thr, min_updraft_val=mn, out=(None, u),
                                        want_orograph=False)
                assert np.array_equal(host(u), use)
    if shape[0] >= 31:
        assert most_signal >= 1000 * shape[0] * shape[1] // (97 * 161), most_signal


# ----------------------------------------------------------------------------------------------
# 3. k_slope_aspect: the four (DEM type, output type) instantiations and the optional outputs
@pytest.mark.parametrize('name', ('integer', 'nodata'))
def test_slope_aspect_variants(gpu, golden, name):
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    g = golden('g14_raster_edges.npz')
    res = float(g['res'])
    z = g[f'{name}_dem'].astype(np.float64)
    assert_branch_reached(z, res)
    hit = nan_stencil_cells(z)
    z32 = z.astype(np.float32)
    assert np.array_equal(z32.astype(np.float64), z, equal_nan=True)       # integer metres: exact in f32
    rough = z + np.random.default_rng(3).normal(0., 0.3, z.shape)          # an f32 DEM that is not exact in f64
    for dem, dem64 in ((z, z), (z32, z), (rough.astype(np.float32), rough.astype(np.float32).astype(np.float64))):
        s, a = layers.slope_aspect(dem, res)
        assert s.dtype == np.float64 and a.dtype == np.float64
        np.testing.assert_allclose(s, orc.compute_slope_degrees(dem64, res), **SLOPE_TOL)
        np.testing.assert_allclose(a, orc.compute_aspect_degrees(dem64, res), **ASPECT_TOL)
        assert (s[hit] == 0).all() and (a[hit] == 0).all()
        s32, a32 = layers.slope_aspect(dem, res, out_dtype=torch.float32)
        assert s32.dtype == np.float32 and a32.dtype == np.float32
        # the same arithmetic, rounded once at the store
        np.testing.assert_array_equal(s32, s.astype(np.float32))
        np.testing.assert_array_equal(a32, a.astype(np.float32))
        for dt, (sp, ap) in ((torch.float64, (s, a)), (torch.float32, (s32, a32))):
            s1, none = layers.slope_aspect(dem, res, want_aspect=False, out_dtype=dt)
            assert none is None
            np.testing.assert_array_equal(s1, sp)
            none, a1 = layers.slope_aspect(dem, res, want_slope=False, out_dtype=dt)
            assert none is None
            np.testing.assert_array_equal(a1, ap)


# ----------------------------------------------------------------------------------------------
# 4. k_orographic: (terrain type, wind type) pairs, the scalar path, uniform batches
def g14_terrain(golden, crop=None):
    g = golden('g14_raster_edges.npz')
    assert_branch_reached(g['integer_dem'], float(g['res']))
    s, a = g['integer_slope'], g['integer_aspect']
    if crop:
        s, a = np.ascontiguousarray(s[:crop[0], :crop[1]]), np.ascontiguousarray(a[:crop[0], :crop[1]])
    return s, a


def wind_rasters(shape):
    r = np.arange(shape[0], dtype=np.float64)[:, None]
    c = np.arange(shape[1], dtype=np.float64)[None, :]
    return 8. + 3. * np.sin(c / 17.) * np.cos(r / 13.), 268. + 40. * np.sin(c / 23. + r / 31.)


@pytest.mark.parametrize('crop', (None, (96, 160)), ids=('scalar_path', 'vector_path'))
@pytest.mark.parametrize('tdt', (np.float64, np.float32), ids=('terrain_f64', 'terrain_f32'))
@pytest.mark.parametrize('wdt', (np.float64, np.float32), ids=('wind_f64', 'wind_f32'))
def test_orographic_type_pairs_with_wind_rasters(gpu, golden, crop, tdt, wdt):
    """97 x 161 = 15617 cells is odd (one cell per thread); 96 x 160 takes four per thread."""
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    s, a = (x.astype(tdt) for x in g14_terrain(golden, crop))
    ws, wd = (x.astype(wdt) for x in wind_rasters(s.shape))
    wide = [x.astype(np.float64) for x in (ws, wd, s, a)]
    for mn in (0., 0.05):
        ref = orc.compute_orographic_updraft(*wide, mn)
        ref32 = ref.astype(np.float32)
        oro, use = layers.orographic_updraft(ws, wd, s, a, mn, threshold=0.75)
        oro, use = host(oro), host(use)
        st = check_orograph_cells(oro, ref, wide[0].max(),
                                  f'k_orographic rasters {np.dtype(tdt).name}/{np.dtype(wdt).name}')
        assert st['signal'] >= 1000
        check_usable(use, oro, 0.75, ref32, orc.get_above_threshold_speed(ref32, 0.75), orc)
        np.testing.assert_array_equal(layers.compute_orographic_updraft(ws, wd, s, a, mn), oro)


@pytest.mark.parametrize('uniform', (True, False), ids=('uniform', 'rasters'))
def test_orographic_scalar_path_gives_the_vector_path_bits(gpu, golden, uniform):
    """One cell per thread is taken when the cell count is not a multiple of 4 or a pointer is not
    32-byte aligned; both must give what four cells per thread give."""
    from ssrs_amd import layers
    s, a = g14_terrain(golden, (96, 160))
    n = s.size
    assert n % 4 == 0
    ws, wd = wind_rasters((1, n))
    s, a = s.reshape(1, n), a.reshape(1, n)

    def run(s, a, ws, wd):
        if uniform:
            return layers.orographic_updraft([7.5, 9.0], [270., 95.], s, a, 0.01, threshold=0.75)
        return layers.orographic_updraft(ws, wd, s, a, 0.01, threshold=0.75)
    dev = [torch.from_numpy(x).cuda() for x in (s, a, ws, wd)]
    assert all(t.data_ptr() % 32 == 0 for t in dev)
    oro, use = run(*dev)
    # (a) one cell fewer: 15359 is odd
    o1, u1 = run(*[t[:, :n - 1].contiguous() for t in dev])
    assert torch.equal(o1, oro[..., :n - 1]) and torch.equal(u1, use[..., :n - 1])
    # (b) the same cells at an address 8 bytes past a 32-byte boundary, one array at a time and all
    def shifted(t):
        buf = torch.empty(n + 1, dtype=t.dtype, device='cuda')
        view = buf[1:].view(1, n)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 32 == 8
        return view
    for which in ((0,), (1,), (2, 3), (0, 1, 2, 3)):
        if uniform and which == (2, 3):
            continue
        args = [shifted(t) if k in which else t for k, t in enumerate(dev)]
        o2, u2 = run(*args)
        assert torch.equal(o2, oro) and torch.equal(u2, use), which


@pytest.mark.parametrize('tdt', (np.float64, np.float32), ids=('terrain_f64', 'terrain_f32'))
def test_orographic_uniform_batch_beyond_one_chunk(gpu, golden, tdt):
    """19 uniform winds = one kernel-argument chunk of 16 and one of 3: orograph AND usable updraft of
    the first and last case of each chunk."""
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    s, a = (x.astype(tdt) for x in g14_terrain(golden))
    s64, a64 = s.astype(np.float64), a.astype(np.float64)
    speeds = np.linspace(4., 14., 19)
    dirns = np.array([0., 90., 180., 270., 45., 123.4, -30., 725., 85., 95., 265., 275.,
                      10., 200., 300., 265., 270., 33., 275.])
    for mn, thr in ((0., 0.75), (0.05, 2.0)):
        oro, use = layers.orographic_updraft(speeds, dirns, s, a, mn, threshold=thr)
        assert tuple(oro.shape) == (19,) + s.shape and tuple(use.shape) == (19,) + s.shape
        oro, use = host(oro), host(use)
        for b in (0, 15, 16, 18):
            ref = orc.compute_orographic_updraft(speeds[b], dirns[b], s64, a64, mn)
            ref32 = ref.astype(np.float32)
            st = check_orograph_cells(oro[b], ref, speeds[b],
                                      f'k_orographic uniform batch case {b} {np.dtype(tdt).name}')
            assert st['signal'] >= 1000
            check_usable(use[b], oro[b], thr, ref32, orc.get_above_threshold_speed(ref32, thr), orc)
            o1, u1 = layers.orographic_updraft(float(speeds[b]), float(dirns[b]), s, a, mn, threshold=thr)
            assert np.array_equal(host(o1), oro[b]) and np.array_equal(host(u1), use[b])


# ----------------------------------------------------------------------------------------------
# 5. / 6. the lattice kernel against an independent reference
def g14_dem(golden, name):
    g = golden('g14_raster_edges.npz')
    return g[f'{name}_dem'].astype(np.float64), float(g['res'])


def lattices(name, rows, cols, res):
    """name -> (x_km, y_km, wspeed (B, ny, nx), wdirn (B, ny, nx))"""
    from ssrs_amd.synthetic import wind_lattice
    width = (cols * res / 1000., rows * res / 1000.)          # 4.83 x 2.91 km
    if name in ('cover', 'calm', 'ridge265', 'batch9'):
        phases = [0.3 + 0.7 * k for k in range(9)] if name == 'batch9' else [0.3]
        lat = [wind_lattice(width, 0.6, phase=p) for p in phases]
        x, y = lat[0][0], lat[0][1]
        ws, wd = np.stack([l[2] for l in lat]), np.stack([l[3] for l in lat])
        if name == 'calm':
            ws[0, 2, 3] = 0.
        if name == 'ridge265':                                # uniform, 5 degrees off the ridges
            ws[:], wd[:] = 7.5, 265.
        return x, y, ws, wd
    if name == 'middle':                                      # hull strictly inside: clamp on all four sides
        x, y = 1.0 + 0.5 * np.arange(5), 0.8 + 0.4 * np.arange(4)
    elif name == 'nx1':
        x, y = np.array([2.0]), 0.7 * np.arange(5)
    elif name == 'ny1':
        x, y = 0.9 * np.arange(6), np.array([1.1])
    elif name in ('one', 'one_calm'):
        x, y = np.array([2.0]), np.array([1.1])
    xx, yy = np.meshgrid(x, y)
    ws = 8. + 3. * np.sin(xx / 1.7 + 0.3) * np.cos(yy / 1.3)
    wd = 268. + 40. * np.sin(xx / 2.3 + yy / 3.1)
    if name == 'one_calm':
        ws[:] = 0.
    return x, y, ws[None], wd[None]


@pytest.mark.parametrize('lattice', ('cover', 'middle', 'nx1', 'ny1', 'one', 'one_calm', 'calm', 'ridge265', 'batch9'))
@pytest.mark.parametrize('dem_name', ('smooth', 'integer', 'terraced'))
def test_lattice_kernel_vs_independent_reference(gpu, golden, dem_name, lattice):
    from ssrs_amd import layers
    from ssrs_amd.synthetic import synthetic_dem
    from oracle import ssrs_oracle as orc
    if dem_name == 'smooth':
        z, res = synthetic_dem((97, 161), 30., seed=14), 30.
    else:
        z, res = g14_dem(golden, dem_name)
        assert_branch_reached(z, res)
    rows, cols = z.shape
    x, y, ws, wd = lattices(lattice, rows, cols, res)
    B = ws.shape[0]
    most_signal = 0
    for dem, mn, thr in ((z, 0., 0.75), (z.astype(np.float32), 0.05, 0.3)):
        oro, use = layers.updraft_from_dem_lattice(dem, res, x, y, ws, wd, threshold=thr, min_updraft_val=mn)
        assert tuple(oro.shape) == (B, rows, cols) and oro.dtype == torch.float32 and use.dtype == torch.float64
        for b in range(B):
            ref, ref_use, wmax = lattice_reference(dem, res, x, y, ws[b], wd[b], orc, mn, thr)
            o, u = host(oro[b]), host(use[b])
            st = check_orograph_cells(o, ref, wmax, f'k_updraft_from_dem_lattice {dem_name}/{lattice}'
                                                    f'/{dem.dtype.name} snapshot {b}')
            most_signal = max(most_signal, st['signal'])
            check_usable(u, o, thr, ref.astype(np.float32), ref_use, orc)
            if lattice == 'one_calm':
                assert (o == np.float32(mn)).all()
            # a single call equals its slice of the batch
            if b in (0, B - 1):
                o1, u1 = layers.updraft_from_dem_lattice(dem, res, x, y, ws[b], wd[b], threshold=thr,
                                                         min_updraft_val=mn)
                assert tuple(o1.shape) == (rows, cols)
                assert torch.equal(o1, oro[b]) and torch.equal(u1, use[b])
        only_oro = layers.updraft_from_dem_lattice(dem, res, x, y, ws, wd, min_updraft_val=mn)
        assert only_oro[1] is None and torch.equal(only_oro[0], oro)
        only_use = layers.updraft_from_dem_lattice(dem, res, x, y, ws, wd, threshold=thr, min_updraft_val=mn,
                                                   want_orograph=False)
        assert only_use[0] is None and torch.equal(only_use[1], use)
    assert most_signal >= 1000, most_signal
