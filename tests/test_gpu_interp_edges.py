"""The K6 interpolation family on tiny rasters and degenerate samples: ssrs_wind_from_lattice,
ssrs_updraft_from_dem_lattice, ssrs_wind_from_triangles, ssrs_wind_nearest_index, ssrs_wind_from_nearest,
ssrs_wind_from_triangles_cubic, ssrs_scalar_from_samples and ssrs_wtk_thermal_fields against interp_ref.py (the
header's contract in numpy f64, pinned to scipy by test_interp_ref_host.py) and against scipy's griddata itself.

What the geometries of interp_ref.CASES reach: triangles wholly outside the raster, overhanging it on every side, a
hull strictly inside it, cells exactly on hull edges and on shared edges, a NaN-transform triangle, the 1024 / 1025
candidate limit of the nearest-sample cull, partial cull tiles, one sample, duplicate samples, the 3072 / 3073 sample
limit of the LDS table, indices outside [0, npts), rows shorter than a lane's four cells, an unaligned output, lattices
of one point along an axis, rasters that overhang their lattice, calm wind and the 0 / 360 degree wrap.

Bounds.  Against griddata: NaN class exactly equal, values within 1e-10 * max(1, max |reference|), direction within
1e-7 degrees on cells faster than 1e-3 * max speed (test_gpu_wind_methods.py).  Scalar 'linear' against owner_linear and
the polynomial fields: 1e-12 * max(1, max |field|), the project's bound for f64 rasters.  Lattice wind: rtol = atol =
1e-12, direction 1e-10 degrees on the circle (test_gpu_raster.py).  Fused calls: the bits of their chains."""
import ctypes as C

import numpy as np
import pytest
import torch

import interp_ref as ir

pytestmark = pytest.mark.gpu

METHODS = ('nearest', 'linear', 'cubic')
NAMES = tuple(ir.CASES)


def _res(cell):
    """The resolution in metres whose cell size in km is exactly `cell`."""
    res = cell * 1000.
    assert res / 1000. == cell
    return res


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _ulps_f64(a, b):
    """Distance in f64 ulps of finite arrays of like sign pattern (0 for equal bits)."""
    ia, ib = (np.ascontiguousarray(v, dtype=np.float64).view(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, np.int64(-2**63) - i, i) for i in (ia, ib))
    return np.abs(ia - ib)


def _scalar(pts, vals, rows, cols, cell, method, index=None):
    from ssrs_amd.wind import interpolate_scalar_scattered
    return interpolate_scalar_scattered(pts[:, 0], pts[:, 1], vals, (rows, cols), _res(cell), method=method, index=index)


def _wind(pts, ws, wd, rows, cols, cell, method, index=None):
    from ssrs_amd.wind import interpolate_wind_scattered
    return interpolate_wind_scattered(pts[:, 0], pts[:, 1], ws, wd, (rows, cols), _res(cell), method=method, index=index)


def _index(pts, rows, cols, cell):
    from ssrs_amd.wind import nearest_sample_index
    return nearest_sample_index(pts[:, 0], pts[:, 1], (rows, cols), _res(cell))


def _check_wind(label, got_s, got_d, ref_e, ref_n, dir_bound=1e-7):
    """Speed / direction rasters against reference components: NaN class exact, speed and the components within
    1e-10 * max(1, max speed), direction within dir_bound degrees on the strong cells."""
    ref_s, ref_d = ir.uv_recipe(ref_e, ref_n)
    nan = np.isnan(ref_s)
    assert np.array_equal(np.isnan(got_s), nan), f'{label}: NaN class of the speed differs'
    assert np.array_equal(np.isnan(got_d), nan), f'{label}: NaN class of the direction differs'
    ok = ~nan
    if not ok.any():
        print(f'{label}: every cell NaN')
        return 0., 0.
    top = float(np.max(ref_s[ok]))
    bound = 1e-10 * max(1., top)
    rad = got_d[ok] * np.pi / 180.
    err_s = float(np.max(np.abs(got_s[ok] - ref_s[ok])))
    err_e = float(np.max(np.abs(got_s[ok] * np.sin(rad) - ref_e[ok])))
    err_n = float(np.max(np.abs(got_s[ok] * np.cos(rad) - ref_n[ok])))
    strong = ref_s[ok] > 1e-3 * top
    err_d = float(np.max(ir.direction_gap(got_d[ok], ref_d[ok])[strong])) if strong.any() else 0.
    print(f'{label}: |speed| {err_s:.3g}, |east| {err_e:.3g}, |north| {err_n:.3g} (bound {bound:.3g}), '
          f'direction {err_d:.3g} deg (bound {dir_bound:.3g})')
    assert err_s <= bound and err_e <= bound and err_n <= bound
    assert err_d <= dir_bound
    return err_s, err_d


# ------------------------------------------------------------------------------------------- every geometry, scalar
@pytest.mark.parametrize('name', NAMES)
def test_scalar_methods_on_tiny_geometries(gpu, name):
    pts, rows, cols, cell = ir.CASES[name]
    vals = np.stack([ir.case_values(name, k) for k in range(3)])
    for method in METHODS:
        got3 = _scalar(pts, vals, rows, cols, cell, method)
        assert tuple(got3.shape) == (3, rows, cols) and got3.dtype == torch.float64
        for k in range(3):
            one = _scalar(pts, vals[k], rows, cols, cell, method)
            assert tuple(one.shape) == (rows, cols)
            assert _same_bits(one, got3[k]), f'{name} {method}: field {k} of the batch differs from its single call'
        got3 = got3.cpu().numpy()
        if method == 'nearest':
            want_i = ir.nearest_index(pts, rows, cols, cell)
            got_i = _index(pts, rows, cols, cell)
            assert got_i.dtype == torch.int32 and np.array_equal(got_i.cpu().numpy(), want_i), f'{name}: index raster'
            if name == 'duplicates':
                assert int(got_i[2, 2]) == 4
            for k in range(3):
                assert np.array_equal(got3[k].view(np.int64), vals[k][want_i].view(np.int64)), f'{name}: gather'
            continue
        for k in range(3):
            ref = ir.griddata(pts, vals[k], rows, cols, cell, method)
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(got3[k]), nan), f'{name} {method}: NaN class differs from griddata'
            if name == 'outside':
                assert nan.all()
            if (~nan).any():
                bound = 1e-10 * max(1., float(np.max(np.abs(ref[~nan]))))
                err = float(np.max(np.abs(got3[k][~nan] - ref[~nan])))
                print(f'{name} {method} field {k}: max |device - griddata| {err:.3g} (bound {bound:.3g})')
                assert err <= bound
        if method == 'linear':
            want, owner, multi = ir.owner_linear(pts, rows, cols, cell, vals)
            nan = owner < 0
            assert np.array_equal(np.isnan(got3), np.isnan(want))
            if (~nan).any():
                bound = 1e-12 * max(1., float(np.max(np.abs(want[:, ~nan]))))
                err = float(np.max(np.abs(got3[:, ~nan] - want[:, ~nan])))
                ulps = int(np.max(_ulps_f64(got3[:, ~nan], want[:, ~nan])))
                print(f"{name} 'linear' vs owner_linear: max |d| {err:.3g} (bound {bound:.3g}), {ulps} ulp, "
                      f'{int(multi.sum())} cells in more than one triangle')
                assert err <= bound


# --------------------------------------------------------------------------------------------- every geometry, wind
@pytest.mark.parametrize('name', NAMES)
def test_wind_methods_on_tiny_geometries(gpu, name):
    pts, rows, cols, cell = ir.CASES[name]
    ws, wd = (np.stack(v) for v in zip(*(ir.sample_wind(pts, k) for k in range(3))))
    for method in METHODS:
        s3, d3 = _wind(pts, ws, wd, rows, cols, cell, method)
        assert tuple(s3.shape) == (3, rows, cols) and s3.dtype == torch.float64 and d3.shape == s3.shape
        for k in range(3):
            s1, d1 = _wind(pts, ws[k], wd[k], rows, cols, cell, method)
            assert tuple(s1.shape) == (rows, cols)
            assert _same_bits(s1, s3[k]) and _same_bits(d1, d3[k]), f'{name} {method}: snapshot {k} differs from its single call'
        s3, d3 = s3.cpu().numpy(), d3.cpu().numpy()
        for k in range(3):
            east, north = ir.components(ws[k], wd[k])
            if method == 'nearest':
                idx = ir.nearest_index(pts, rows, cols, cell)
                ref_e, ref_n = east[idx], north[idx]
            else:
                ref_e = ir.griddata(pts, east, rows, cols, cell, method)
                ref_n = ir.griddata(pts, north, rows, cols, cell, method)
            _check_wind(f'{name} {method}[{k}]', s3[k], d3[k], ref_e, ref_n)
        if method == 'nearest':
            assert not np.isnan(s3).any() and not np.isnan(d3).any()


# ------------------------------------------------------------------------------- the owner rule decides the result
def test_owner_rule_where_it_decides(gpu):
    """One NaN and one +inf sample on the exact lattice: a cell on an edge between a triangle with such a vertex and
    one without is NaN (0 * NaN, 0 * inf) or finite depending on which of them owns it."""
    pts, rows, cols, cell = ir.CASES['lattice']
    vals = ir.case_values('lattice').copy()
    vals[8], vals[21] = np.nan, np.inf                                # the vertices (4, 2) and (6, 6)
    want, owner, multi = ir.owner_linear(pts, rows, cols, cell, vals)
    got = _scalar(pts, vals, rows, cols, cell, 'linear').cpu().numpy()
    decided = multi & (np.isnan(want) | np.isinf(want))
    print(f'owner rule: {int(np.isnan(want).sum())} NaN, {int(np.isinf(want).sum())} inf cells, '
          f'{int(decided.sum())} of them in more than one triangle')
    assert decided.sum() >= 8 and (owner >= 0).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.max(np.abs(got[fin] - want[fin])) <= 1e-12 * max(1., float(np.max(np.abs(want[fin]))))
    near = _scalar(pts, vals, rows, cols, cell, 'nearest').cpu().numpy()
    idx = ir.nearest_index(pts, rows, cols, cell)
    assert np.isnan(near).sum() == (idx == 8).sum() > 0 and np.isposinf(near).sum() == (idx == 21).sum() > 0
    assert np.array_equal(near.view(np.int64), vals[idx].view(np.int64))


# --------------------------------------------------------------------------------------------------- through the C ABI
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _triangulation(pts):
    """(tri (ntri, 3) int32, nbr (ntri, 3) int32, transform (ntri, 3, 2) f64) of scipy.spatial.Delaunay, numpy."""
    from scipy.spatial import Delaunay
    d = Delaunay(pts)
    return d.simplices.astype(np.int32), d.neighbors.astype(np.int32), d.transform.astype(np.float64)


def _abi_scalar(method, pts, tri, nbr, tr, values, grad, rows, cols, cell):
    """ssrs_scalar_from_samples on a caller-built triangulation: values (F, npts), grad (F, npts, 2) or None."""
    from ssrs_amd import _native as nat
    from ssrs_amd._device import stream_ptr
    L = nat.lib()
    F, npts = values.shape
    keep = [_dev(pts, torch.float64), _dev(tri, torch.int32), _dev(nbr, torch.int32), _dev(tr, torch.float64),
            _dev(values, torch.float64), None if grad is None else _dev(grad, torch.float64)]
    code = nat.SSRS_INTERP[method]
    nbytes = int(L.ssrs_scalar_interp_workspace_bytes(code, int(tri.shape[0]), rows, cols, F))
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    out = torch.empty((F, rows, cols), dtype=torch.float64, device='cuda')
    nat.check(L.ssrs_scalar_from_samples(code, nat.ptr(keep[0]), nat.ptr(keep[1]), nat.ptr(keep[2]), nat.ptr(keep[3]),
                                         nat.ptr(None), nat.ptr(keep[4]), nat.ptr(keep[5]), npts, int(tri.shape[0]),
                                         C.c_double(cell), nat.ptr(out), rows, cols, F, nat.ptr(scratch),
                                         C.c_size_t(nbytes), stream_ptr()))
    torch.cuda.synchronize()
    return out


def _abi_wind(method, pts, tri, nbr, tr, ws, wd, grad_e, grad_n, rows, cols, cell):
    """ssrs_wind_from_triangles ('linear': ws, wd are speed / direction) or ssrs_wind_from_triangles_cubic ('cubic':
    ws, wd are the east / north components, grad_e / grad_n their vertex gradients), each (B, npts)."""
    from ssrs_amd import _native as nat
    from ssrs_amd._device import stream_ptr
    L = nat.lib()
    B, npts = ws.shape
    ntri = int(tri.shape[0])
    keep = [_dev(pts, torch.float64), _dev(tri, torch.int32), _dev(nbr, torch.int32), _dev(tr, torch.float64),
            _dev(ws, torch.float64), _dev(wd, torch.float64)]
    out_s = torch.empty((B, rows, cols), dtype=torch.float64, device='cuda')
    out_d = torch.empty_like(out_s)
    if method == 'linear':
        nbytes = int(L.ssrs_wind_triangles_workspace_bytes(npts, rows, cols, B))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        nat.check(L.ssrs_wind_from_triangles(nat.ptr(keep[0]), nat.ptr(keep[1]), nat.ptr(keep[3]), nat.ptr(keep[4]),
                                             nat.ptr(keep[5]), npts, ntri, C.c_double(cell), nat.ptr(out_s), nat.ptr(out_d),
                                             rows, cols, B, nat.ptr(scratch), C.c_size_t(nbytes), stream_ptr()))
    else:
        keep += [_dev(grad_e, torch.float64), _dev(grad_n, torch.float64)]
        nbytes = int(L.ssrs_wind_cubic_workspace_bytes(npts, ntri, rows, cols, B))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        nat.check(L.ssrs_wind_from_triangles_cubic(nat.ptr(keep[0]), nat.ptr(keep[1]), nat.ptr(keep[2]), nat.ptr(keep[3]),
                                                   nat.ptr(keep[4]), nat.ptr(keep[5]), nat.ptr(keep[6]), nat.ptr(keep[7]),
                                                   npts, ntri, C.c_double(cell), nat.ptr(out_s), nat.ptr(out_d), rows, cols,
                                                   B, nat.ptr(scratch), C.c_size_t(nbytes), stream_ptr()))
    assert nbytes > 0
    torch.cuda.synchronize()
    return out_s, out_d


def test_nan_transform_triangle_is_skipped(gpu):
    """The `hull_inside` triangulation with a degenerate triangle in front: index 0, collinear vertices (0, 1, 1), an
    all-NaN transform (what scipy stores for a degenerate simplex), no neighbours, nobody's neighbour.  Its bounding
    box lies in the raster, so only the transform test keeps it from owning cells; every real triangle moves up by
    one index and nothing else changes."""
    pts, rows, cols, cell = ir.CASES['hull_inside']
    tri, nbr, tr = _triangulation(pts)
    tri2 = np.concatenate([np.array([[0, 1, 1]], dtype=np.int32), tri])
    nbr2 = np.concatenate([np.full((1, 3), -1, dtype=np.int32), np.where(nbr >= 0, nbr + 1, -1).astype(np.int32)])
    tr2 = np.concatenate([np.full((1, 3, 2), np.nan), tr])
    vals = np.stack([ir.case_values('hull_inside', k) for k in range(2)])
    grad = np.stack([ir.quadratic_grad(pts[:, 0], pts[:, 1]), ir.affine_grad(pts[:, 0], pts[:, 1])])
    ws, wd = (np.stack(v) for v in zip(*(ir.sample_wind(pts, k) for k in range(2))))
    east, north = ir.components(ws, wd)
    inside = ir.owner_linear(pts, rows, cols, cell, vals[0])[1] >= 0
    for method in ('linear', 'cubic'):
        g = grad if method == 'cubic' else None
        a = _abi_scalar(method, pts, tri, nbr, tr, vals, g, rows, cols, cell)
        b = _abi_scalar(method, pts, tri2, nbr2, tr2, vals, g, rows, cols, cell)
        assert np.array_equal(torch.isnan(a[0]).cpu().numpy(), ~inside)
        assert _same_bits(a, b), f'scalar {method}: the NaN-transform triangle changed the result'
        wa = (ws, wd, None, None) if method == 'linear' else (east, north, grad, grad[::-1].copy())
        sa, da = _abi_wind(method, pts, tri, nbr, tr, *wa, rows, cols, cell)
        sb, db = _abi_wind(method, pts, tri2, nbr2, tr2, *wa, rows, cols, cell)
        assert np.array_equal(torch.isnan(sa[0]).cpu().numpy(), ~inside)
        assert _same_bits(sa, sb) and _same_bits(da, db), f'wind {method}: the NaN-transform triangle changed the result'
    # the entry points of wind.py are these calls: 'linear' through the ABI is interpolate_scalar_scattered
    assert _same_bits(_abi_scalar('linear', pts, tri, nbr, tr, vals, None, rows, cols, cell),
                      _scalar(pts, vals, rows, cols, cell, 'linear'))


@pytest.mark.parametrize('name', ir.POLYNOMIAL_CASES)
def test_polynomial_exactness(gpu, name):
    """Independent of scipy's gradient estimate: 'linear' reproduces an affine field, the Clough-Tocher patch with the
    exact vertex gradients an affine and a quadratic one (test_interp_ref_host.py shows scipy's own evaluation does)."""
    pts, rows, cols, cell = ir.CASES[name]
    x, y = pts[:, 0], pts[:, 1]
    xm, ym = ir.mesh(rows, cols, cell)
    inside = ir.owner_linear(pts, rows, cols, cell, np.zeros(x.size))[1] >= 0
    assert inside.any()
    fields = np.stack([ir.affine(x, y), ir.quadratic(x, y)])
    grads = np.stack([ir.affine_grad(x, y), ir.quadratic_grad(x, y)])
    want = np.stack([ir.affine(xm, ym), ir.quadratic(xm, ym)])
    lin = _scalar(pts, fields[0], rows, cols, cell, 'linear').cpu().numpy()
    tri, nbr, tr = _triangulation(pts)
    cub = _abi_scalar('cubic', pts, tri, nbr, tr, fields, grads, rows, cols, cell).cpu().numpy()
    for label, got, ref in (("'linear' affine", lin, want[0]), ("'cubic' affine", cub[0], want[0]),
                            ("'cubic' quadratic", cub[1], want[1])):
        assert np.array_equal(np.isnan(got), ~inside), f'{name} {label}: NaN class'
        bound = 1e-12 * max(1., float(np.max(np.abs(ref[inside]))))
        err = float(np.max(np.abs(got[inside] - ref[inside])))
        print(f'{name} {label}: max |device - field| {err:.3g} (bound {bound:.3g})')
        assert err <= bound
    # the same patch as scipy evaluates it with these gradients
    for f in range(2):
        ref = ir.ct_exact(pts, fields[f], grads[f])(xm, ym)
        assert np.max(np.abs(cub[f][inside] - ref[inside])) <= 1e-12 * max(1., float(np.max(np.abs(ref[inside]))))


# ------------------------------------------------------------------------------------------------ nearest: the cull
def _index_and_full_scans(pts, rows, cols, cell):
    """ssrs_wind_nearest_index through the C ABI: (index raster, the workspace's count of tiles that scanned all
    samples)."""
    from ssrs_amd import _native as nat
    from ssrs_amd._device import stream_ptr
    L = nat.lib()
    d_pts = _dev(pts, torch.float64)
    index = torch.empty((rows, cols), dtype=torch.int32, device='cuda')
    nbytes = int(L.ssrs_wind_nearest_workspace_bytes(int(pts.shape[0]), rows, cols))
    scratch = torch.full((nbytes,), 0xff, dtype=torch.uint8, device='cuda')
    nat.check(L.ssrs_wind_nearest_index(nat.ptr(d_pts), int(pts.shape[0]), C.c_double(cell), nat.ptr(index), rows, cols,
                                        nat.ptr(scratch), C.c_size_t(nbytes), stream_ptr()))
    return index.cpu().numpy(), int(scratch[:4].view(torch.int32).item())


def test_nearest_cull_at_its_capacity(gpu):
    """One 32 x 64 tile and samples that all lie within its reach: 1024 candidates fit the list, 1025 do not."""
    rng = np.random.default_rng(1024)
    pts = np.stack([rng.uniform(0., 6.3, 1025), rng.uniform(0., 3.1, 1025)], 1)
    for npts, want_full in ((1024, 0), (1025, 1)):
        got, full = _index_and_full_scans(pts[:npts], 32, 64, 0.1)
        print(f'nearest cull, {npts} samples: {full} tile(s) scanned all samples')
        assert full == want_full
        assert np.array_equal(got, ir.nearest_index(pts[:npts], 32, 64, 0.1))


@pytest.mark.parametrize('shape', [(33, 65), (5, 7)])
@pytest.mark.parametrize('npts', [1, 2, 40])
def test_nearest_partial_tiles(gpu, shape, npts):
    """Tiles one cell wide and one row high, and fewer samples than a wave has lanes."""
    rows, cols = shape
    cell = 0.1
    rng = np.random.default_rng(100 * rows + npts)
    pts = np.stack([rng.uniform(-0.2, 1.2, npts) * (cols - 1) * cell, rng.uniform(-0.2, 1.2, npts) * (rows - 1) * cell], 1)
    got, full = _index_and_full_scans(pts, rows, cols, cell)
    assert full == 0
    assert np.array_equal(got, ir.nearest_index(pts, rows, cols, cell))
    assert np.array_equal(_index(pts, rows, cols, cell).cpu().numpy(), got)


def _big_cloud():
    """3072 samples in and around a 16 x 16 raster of 100 m cells, one more far away (nearest to no cell), and two
    snapshots of wind on them."""
    rng = np.random.default_rng(3072)
    pts = np.concatenate([rng.uniform(-0.5, 2.0, (3072, 2)), np.array([[1000., 1000.]])])
    ws, wd = rng.uniform(0.5, 15., (2, 3073)), rng.uniform(0., 360., (2, 3073))
    return pts, ws, wd


def test_nearest_table_at_its_capacity(gpu):
    """3072 samples fill the 48 KB LDS table of ssrs_wind_from_nearest, 3073 take the per-cell recipe: same bits."""
    pts, ws, wd = _big_cloud()
    rows = cols = 16
    cell = 0.1
    out = []
    for npts in (3072, 3073):
        idx = _index(pts[:npts], rows, cols, cell)
        assert np.array_equal(idx.cpu().numpy(), ir.nearest_index(pts[:npts], rows, cols, cell))
        assert int(idx.max()) < 3072
        out.append(_wind(pts[:npts], ws[:, :npts], wd[:, :npts], rows, cols, cell, 'nearest', index=idx))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    idx = ir.nearest_index(pts, rows, cols, cell)
    for npts, (s, d) in zip((3072, 3073), out):
        assert tuple(s.shape) == (2, rows, cols)
        for b in range(2):
            east, north = ir.components(ws[b], wd[b])
            _check_wind(f'nearest table, {npts} samples [{b}]', s[b].cpu().numpy(), d[b].cpu().numpy(), east[idx], north[idx])


def _thermal_layers(npts, batch, seed=7):
    """(4, batch, npts): pressure, temperature, blheight, surfheatflux in their physical ranges."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(8e4, 9.5e4, (batch, npts)), rng.uniform(-5., 30., (batch, npts)),
                     rng.uniform(20., 2500., (batch, npts)), rng.uniform(20., 500., (batch, npts))])


def _wtk(pts, snaps, rows, cols, cell, method, dtype, index=None, height=120.):
    from ssrs_amd.thermals import compute_wtk_thermals
    args = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in snaps]
    return compute_wtk_thermals(pts[:, 0], pts[:, 1], *args, (rows, cols), _res(cell), height, method=method, dtype=dtype,
                                index=index)


def test_index_out_of_range_is_nan(gpu):
    """The header: an index outside [0, npts) gives NaN.  -1 and npts in two cells of a prebuilt index raster."""
    cases = [('hull_inside',) + ir.CASES['hull_inside']]
    big, big_ws, big_wd = _big_cloud()
    cases.append(('3073 samples', big, 16, 16, 0.1))                  # past the LDS table: the per-cell recipe
    for name, pts, rows, cols, cell in cases:
        npts = pts.shape[0]
        good = _index(pts, rows, cols, cell)
        bad = good.clone()
        bad[1, 2], bad[rows - 1, cols - 1] = -1, npts
        hit = np.zeros((rows, cols), dtype=bool)
        hit[1, 2] = hit[rows - 1, cols - 1] = True
        if npts == 3073:
            ws, wd = big_ws, big_wd
        else:
            ws, wd = (np.stack(v) for v in zip(*(ir.sample_wind(pts, k) for k in range(2))))
        calls = [('ssrs_wind_from_nearest speed', lambda i: _wind(pts, ws, wd, rows, cols, cell, 'nearest', index=i)[0]),
                 ('ssrs_wind_from_nearest direction', lambda i: _wind(pts, ws, wd, rows, cols, cell, 'nearest', index=i)[1]),
                 ('ssrs_scalar_from_samples', lambda i: _scalar(pts, ws, rows, cols, cell, 'nearest', index=i))]
        snaps = _thermal_layers(npts, 2)
        for dtype in (torch.float32, torch.float64):
            calls.append((f'ssrs_wtk_thermal_fields {dtype}',
                          lambda i, dtype=dtype: _wtk(pts, snaps, rows, cols, cell, 'nearest', dtype, index=i)))
        for label, call in calls:
            a, b = call(good), call(bad)
            assert tuple(a.shape) == (2, rows, cols) and not torch.isnan(a).any(), f'{name} {label}'
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.isnan(b[:, hit]).all(), f'{name} {label}: an index out of range is not NaN'
            assert np.array_equal(a[:, ~hit], b[:, ~hit]), f'{name} {label}: other cells changed'


# ------------------------------------------------------------------------------------------------- the fused WTK tail
def _scaled_overhang(rows, cols):
    """The `overhang` points scaled about cell (0, 0) so that they cover a rows x cols raster of 1 km cells."""
    pts = ir.CASES['overhang'][0]
    assert rows <= 9 and cols <= 13
    return pts * np.array([cols / 13., rows / 9.])


def _chain(pts, snaps, rows, cols, cell, method, height):
    from ssrs_amd import layers as L
    batch, npts = snaps.shape[1:]
    v = _scalar(pts, snaps.reshape(4 * batch, npts), rows, cols, cell, method).reshape(4, batch, rows, cols)
    wstar = L.deardoff_velocity_function(L.compute_potential_temperature(v[0], v[1]), v[2], v[3])
    return L.compute_thermal_updraft(height, wstar, v[2])


WTK_SHAPES = [(1, 1), (1, 3), (3, 2), (3, 5), (2, 8)]


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('shape', WTK_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_wtk_tail_equals_the_chain(gpu, shape, method):
    """Rows shorter than, equal to and one past a lane's four cells; one row; one cell."""
    rows, cols = shape
    pts = _scaled_overhang(rows, cols)
    all_snaps = _thermal_layers(pts.shape[0], 3)
    for batch in (1, 3):
        snaps = all_snaps[:, :batch]
        want = _chain(pts, snaps, rows, cols, 1.0, method, 120.)
        assert tuple(want.shape) == (batch, rows, cols) and not torch.isnan(want).any()
        assert float(want.min()) > 1e-3                                 # (no cell sits on the 1e-5 floor)
        got64 = _wtk(pts, snaps, rows, cols, 1.0, method, torch.float64)
        got32 = _wtk(pts, snaps, rows, cols, 1.0, method, torch.float32)
        assert _same_bits(got64, want), f'{shape} {method} batch {batch}: f64 differs from the chain'
        assert _same_bits(got32, want.to(torch.float32)), f'{shape} {method} batch {batch}: f32 differs from the chain'
        # a height raster instead of the scalar
        height = np.random.default_rng(3).uniform(-20., 3000., (rows, cols))
        want = _chain(pts, snaps, rows, cols, 1.0, method, torch.from_numpy(height).cuda()[None].expand(batch, rows, cols))
        got = _wtk(pts, snaps, rows, cols, 1.0, method, torch.float64, height=height)
        assert _same_bits(got, want), f'{shape} {method} batch {batch}: height raster'


@pytest.mark.parametrize('method', METHODS)
def test_wtk_unaligned_output(gpu, method):
    """cols % 4 == 0 but `out` one element past an aligned address: the per-cell stores give the bits of the packed
    ones, and write nothing outside their rows x cols x batch elements."""
    from ssrs_amd import _native as nat
    from ssrs_amd.wind import _scalar_geometry
    rows, cols, batch = 2, 8, 3
    pts = _scaled_overhang(rows, cols)
    snaps = _thermal_layers(pts.shape[0], batch)
    n = batch * rows * cols
    for dtype in (torch.float32, torch.float64):
        head, tail, keep = _scalar_geometry(pts[:, 0], pts[:, 1], snaps.reshape(4 * batch, -1), (rows, cols), 1000., method,
                                            None, 'test')
        item = torch.empty((), dtype=dtype).element_size()
        outs = []
        for shift in (0, 1):
            buf = torch.full((n + 8,), -7., dtype=dtype, device='cuda')
            out = buf[shift:shift + n]
            assert (out.data_ptr() % (4 * item) == 0) == (shift == 0)
            nat.check(nat.lib().ssrs_wtk_thermal_fields(*head, nat.ptr(None), C.c_double(120.), C.c_double(1e-5), nat.ptr(out),
                                                        int(dtype == torch.float32), rows, cols, batch, *tail))
            torch.cuda.synchronize()
            assert bool((buf[:shift] == -7.).all()) and bool((buf[shift + n:] == -7.).all()), 'a store outside `out`'
            outs.append(out.clone())
        assert not torch.isnan(outs[0]).any()
        assert _same_bits(outs[0], outs[1]), f'{method} {dtype}: the unaligned call differs from the aligned one'
        want = _wtk(pts, snaps, rows, cols, 1.0, method, dtype)
        assert _same_bits(outs[0].reshape(batch, rows, cols), want)


# ---------------------------------------------------------------------------------------------------- the lattice path
LATTICES = [(1, 1), (1, 4), (5, 1), (2, 2), (4, 3)]


def _lattice(nx, ny, k=0):
    """Lattice origin (1.0, 0.5) km, spacing (1.5, 1.0) km; the components are e = 1 + 0.5 x - 0.25 y + 0.125 x y and
    n = -2 + 0.25 x + 0.5 y at the lattice points (snapshot k: scaled and turned), as speed / direction (ny, nx)."""
    x, y = 1.0 + 1.5 * np.arange(nx), 0.5 + 1.0 * np.arange(ny)
    gx, gy = np.meshgrid(x, y)
    ws, wd = ir.uv_recipe(1. + 0.5 * gx - 0.25 * gy + 0.125 * gx * gy, -2. + 0.25 * gx + 0.5 * gy)
    return x, y, ws * (1. + 0.5 * k), np.mod(wd + 40. * k, 360.)


@pytest.mark.parametrize('lattice', LATTICES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_wind_lattice_edges(gpu, lattice):
    from ssrs_amd.wind import interpolate_wind_lattice
    nx, ny = lattice
    rows, cols, cell = 9, 13, 0.5
    x, y, _, _ = _lattice(nx, ny)
    ws, wd = (np.stack(v) for v in zip(*(_lattice(nx, ny, k)[2:] for k in range(3))))
    s3, d3 = interpolate_wind_lattice(x, y, ws, wd, (rows, cols), _res(cell))
    assert tuple(s3.shape) == (3, rows, cols) and s3.dtype == torch.float64
    xm, ym = ir.mesh(rows, cols, cell)
    inside = (xm >= x[0]) & (xm <= x[-1]) & (ym >= y[0]) & (ym <= y[-1])
    if (nx, ny) == (4, 3):          # the raster overhangs the lattice on all four sides
        assert not inside[0].any() and not inside[-1].any() and not inside[:, 0].any() and not inside[:, -1].any()
    for k in range(3):
        s1, d1 = interpolate_wind_lattice(x, y, ws[k], wd[k], (rows, cols), _res(cell))
        assert tuple(s1.shape) == (rows, cols) and torch.equal(s1, s3[k]) and torch.equal(d1, d3[k])
        ref_s, ref_d = ir.uv_recipe(*ir.lattice_uv(x, y, ws[k], wd[k], rows, cols, cell))
        got_s, got_d = s3[k].cpu().numpy(), d3[k].cpu().numpy()
        err_s = float(np.max(np.abs(got_s - ref_s) / (1e-12 + 1e-12 * np.abs(ref_s))))
        err_d = float(np.max(ir.direction_gap(got_d, ref_d)))
        print(f'lattice {nx}x{ny}[{k}]: speed error {err_s:.3g} of its rtol = atol = 1e-12 bound, direction {err_d:.3g} deg '
              f'(bound 1e-10)')
        assert not np.isnan(got_s).any() and not np.isnan(got_d).any()
        assert err_s <= 1. and err_d <= 1e-10
    if nx > 1 and ny > 1:           # bilinear interpolation reproduces the two polynomials inside the hull
        pol_s, pol_d = ir.uv_recipe(1. + 0.5 * xm - 0.25 * ym + 0.125 * xm * ym, -2. + 0.25 * xm + 0.5 * ym)
        got_s, got_d = s3[0].cpu().numpy(), d3[0].cpu().numpy()
        assert inside.any()
        assert np.allclose(got_s[inside], pol_s[inside], rtol=1e-12, atol=1e-12)
        assert np.max(ir.direction_gap(got_d[inside], pol_d[inside])) <= 1e-10
    if ny > 1:
        with pytest.raises(ValueError):
            interpolate_wind_lattice(x, y[::-1], ws, wd, (rows, cols), _res(cell))
    if nx > 1:
        with pytest.raises(ValueError):
            interpolate_wind_lattice(x[::-1], y, ws, wd, (rows, cols), _res(cell))


@pytest.mark.parametrize('lattice', [(1, 1), (1, 4), (4, 3)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_fused_lattice_updraft_edges(gpu, lattice):
    """ssrs_updraft_from_dem_lattice against wind interpolation -> slope / aspect -> orographic updraft + threshold on
    four ragged tiles, by the criteria of test_fused_dem_lattice_updraft_equals_the_three_kernel_chain."""
    from raster_checks import ulp_diff_f32
    from ssrs_amd import layers
    from ssrs_amd.synthetic import synthetic_dem
    from ssrs_amd.wind import interpolate_wind_lattice
    nx, ny = lattice
    rows, cols, res = 35, 67, 100.
    z = synthetic_dem((rows, cols), res, seed=9)
    slope, aspect = layers.slope_aspect(z, res)
    x, y, _, _ = _lattice(nx, ny)
    ws, wd = (np.stack(v) for v in zip(*(_lattice(nx, ny, k)[2:] for k in range(3))))
    s_r, d_r = interpolate_wind_lattice(x, y, ws, wd, (rows, cols), res)
    oro_ref, use_ref = layers.orographic_updraft(s_r, d_r, slope, aspect, threshold=0.75)
    oro, use = layers.updraft_from_dem_lattice(z, res, x, y, ws, wd, threshold=0.75)
    assert tuple(oro.shape) == (3, rows, cols) and oro.dtype == torch.float32 and use.dtype == torch.float64
    a, b = oro.cpu().numpy(), oro_ref.cpu().numpy()
    d = ulp_diff_f32(a, b)
    noise = np.abs(a.astype(np.float64) - b.astype(np.float64)) < 1e-11
    print(f'fused lattice updraft {nx}x{ny}: max {int(d[~noise].max()) if (~noise).any() else 0} f32 ulp off the noise cells, '
          f'{float((d == 0).mean()):.4f} of the cells bit-equal, max orograph {float(a.max()):.3g}')
    assert float(a.max()) > 0.1
    assert (d[~noise] <= 1).all()
    np.testing.assert_allclose(use.cpu().numpy(), use_ref.cpu().numpy(), rtol=2e-5, atol=1e-7)
    same = a == b
    np.testing.assert_allclose(use.cpu().numpy()[same], use_ref.cpu().numpy()[same], rtol=1e-12, atol=1e-15)
    o1, u1 = layers.updraft_from_dem_lattice(z, res, x, y, ws[1], wd[1], threshold=0.75)
    assert tuple(o1.shape) == (rows, cols) and torch.equal(o1, oro[1]) and torch.equal(u1, use[1])


# ------------------------------------------------------------------------------------------------------ calm and wrap
def _four_wind_paths(ws, wd):
    """The four wind paths on the `lattice` geometry, samples (ny, nx): label -> (speed, direction) numpy rasters."""
    from ssrs_amd.wind import interpolate_wind_lattice
    pts, rows, cols, cell = ir.CASES['lattice']
    out = {m: _wind(pts, ws.ravel(), wd.ravel(), rows, cols, cell, m) for m in METHODS}
    out['lattice'] = interpolate_wind_lattice(np.arange(0., 11., 2.), np.arange(0., 9., 2.), ws, wd, (rows, cols), _res(cell))
    return {k: (s.cpu().numpy(), d.cpu().numpy()) for k, (s, d) in out.items()}


def test_calm_wind(gpu):
    """Speed 0 at every sample (directions in the first quadrant, so both components are +0): speed 0 and direction 0
    everywhere, on all four paths."""
    wd = np.linspace(0., 89., 30).reshape(5, 6)
    for label, (s, d) in _four_wind_paths(np.zeros((5, 6)), wd).items():
        assert s.shape == (17, 21)
        assert np.all(s == 0.), f'{label}: calm samples, speed not 0'
        assert np.all(d == 0.), f'{label}: calm samples, direction not 0'


def test_direction_wrap(gpu):
    """Samples that alternate between 359.999999 and 0.000001 degrees at speed 5, compared as a gap on the circle."""
    pts, rows, cols, cell = ir.CASES['lattice']
    wd = np.where(np.arange(30) % 2 == 0, 359.999999, 0.000001).reshape(5, 6)
    ws = np.full((5, 6), 5.)
    east, north = ir.components(ws.ravel(), wd.ravel())
    idx = ir.nearest_index(pts, rows, cols, cell)
    refs = {'nearest': (east[idx], north[idx]),
            'linear': tuple(ir.owner_linear(pts, rows, cols, cell, v)[0] for v in (east, north)),
            'cubic': tuple(ir.griddata(pts, v, rows, cols, cell, 'cubic') for v in (east, north)),
            'lattice': ir.lattice_uv(np.arange(0., 11., 2.), np.arange(0., 9., 2.), ws, wd, rows, cols, cell)}
    for label, (s, d) in _four_wind_paths(ws, wd).items():
        _check_wind(f'wrap {label}', s, d, *refs[label], dir_bound=1e-10 if label == 'lattice' else 1e-7)
        assert np.all((d >= 0.) & (d <= 360.))
        assert np.max(ir.direction_gap(d, 0.)) < 1e-5
