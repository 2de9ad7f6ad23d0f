"""Pins tests/interp_ref.py -- the numpy f64 statement of the K6 interpolation contract -- to scipy (the function the
reference calls) on every geometry of interp_ref.CASES, before test_gpu_interp_edges.py judges the device by it.  No GPU.

Bounds: 'linear' NaN class exactly griddata's; values within 1e-12 on the cells one triangle owns (the same three
products and two sums in f64, in whichever triangle: a few ulp of values of order 10); Clough-Tocher with exact
gradients reproduces affine and quadratic fields within 1e-12 * max(1, max |field|) (19 products and sums)."""
import numpy as np
import pytest

import interp_ref as ir

NAMES = tuple(ir.CASES)


@pytest.mark.parametrize('name', NAMES)
def test_owner_linear_is_griddata(name):
    from scipy.spatial import Delaunay
    pts, rows, cols, cell = ir.CASES[name]
    vals = np.stack([ir.case_values(name, k) for k in range(2)])
    got, owner, multi = ir.owner_linear(pts, rows, cols, cell, vals)
    assert got.shape == (2, rows, cols) and owner.shape == (rows, cols) and multi.dtype == bool
    ntri = Delaunay(pts).simplices.shape[0]
    nan = np.isnan(got[0])
    print(f'{name}: {ntri} triangles, {int(nan.sum())} NaN cells of {nan.size}, {int(multi.sum())} cells in more than one triangle')
    assert np.array_equal(nan, owner < 0) and not (multi & nan).any()
    if name in ir.EXPECTED_COUNTS:
        assert (ntri, int(nan.sum()), int(multi.sum())) == ir.EXPECTED_COUNTS[name]
    if name == 'outside':
        assert nan.all()
    worst = 0.
    for f in range(2):
        ref = ir.griddata(pts, vals[f], rows, cols, cell, 'linear')
        assert np.array_equal(np.isnan(got[f]), np.isnan(ref)), f'{name}: NaN class differs from griddata'
        single = ~multi & ~nan
        if single.any():
            worst = max(worst, float(np.max(np.abs(got[f][single] - ref[single]))))
        both = ~nan
        if both.any():          # the interpolant is continuous: shared cells agree to rounding too
            assert np.max(np.abs(got[f][both] - ref[both])) <= 1e-10 * max(1., float(np.max(np.abs(ref[both]))))
    print(f'{name}: max |owner_linear - griddata| on singly owned cells {worst:.3g} (bound 1e-12)')
    assert worst <= 1e-12
    one, owner1, _ = ir.owner_linear(pts, rows, cols, cell, vals[1])
    assert np.array_equal(one, got[1], equal_nan=True) and np.array_equal(owner1, owner)


@pytest.mark.parametrize('name', NAMES)
def test_nearest_index_is_ckdtree(name):
    from scipy.spatial import cKDTree
    pts, rows, cols, cell = ir.CASES[name]
    got = ir.nearest_index(pts, rows, cols, cell)
    assert got.shape == (rows, cols) and got.min() >= 0 and got.max() < pts.shape[0]
    xm, ym = ir.mesh(rows, cols, cell)
    cells = np.stack([xm.ravel(), ym.ravel()], 1)
    dist, near = cKDTree(pts).query(cells, k=2)
    unique = dist[:, 1]**2 > dist[:, 0]**2 * (1. + 1e-12)
    print(f'{name}: {int((~unique).sum())} tie cells of {unique.size}')
    assert np.array_equal(got.ravel()[unique], near[unique, 0])
    # a tie takes the lowest index of the equally near samples
    d_all = np.hypot(cells[:, None, 0] - pts[None, :, 0], cells[:, None, 1] - pts[None, :, 1])
    as_near = d_all <= dist[:, :1] * (1. + 1e-12)
    assert np.array_equal(got.ravel()[~unique], np.argmax(as_near, axis=1)[~unique])
    if name == 'duplicates':
        assert got[2, 2] == 4
    vals = ir.case_values(name)
    ref = ir.griddata(pts, vals, rows, cols, cell, 'nearest')
    assert np.array_equal(vals[got].ravel()[unique], ref.ravel()[unique])


def test_lattice_uv_and_recipe():
    """lattice_uv against scipy's RegularGridInterpolator at the clamped centres; collapsed axes; the recipe."""
    from scipy.interpolate import RegularGridInterpolator
    rows, cols, cell = 9, 13, 0.5
    x, y = 1.0 + 1.5 * np.arange(4), 0.5 + 1.0 * np.arange(3)
    gx, gy = np.meshgrid(x, y)
    e, n = 1. + 0.5 * gx - 0.25 * gy + 0.125 * gx * gy, -2. + 0.25 * gx + 0.5 * gy
    ws, wd = ir.uv_recipe(e, n)
    got_e, got_n = ir.lattice_uv(x, y, ws, wd, rows, cols, cell)
    xs, ys = np.arange(cols) * cell, np.arange(rows) * cell
    at = np.stack(np.meshgrid(np.clip(ys, y[0], y[-1]), np.clip(xs, x[0], x[-1]), indexing='ij'), -1)
    pe, pn = ir.components(ws, wd)
    assert np.allclose(got_e, RegularGridInterpolator((y, x), pe)(at), rtol=1e-13, atol=1e-13)
    assert np.allclose(got_n, RegularGridInterpolator((y, x), pn)(at), rtol=1e-13, atol=1e-13)
    # one lattice point along an axis: that axis does not matter
    e1, n1 = ir.lattice_uv(x[:1], y, ws[:, :1], wd[:, :1], rows, cols, cell)
    assert np.array_equal(e1, np.repeat(e1[:, :1], cols, 1)) and np.array_equal(n1, np.repeat(n1[:, :1], cols, 1))
    e2, n2 = ir.lattice_uv(x[:1], y[:1], ws[:1, :1], wd[:1, :1], rows, cols, cell)
    assert np.all(e2 == pe[0, 0]) and np.all(n2 == pn[0, 0])
    spd, ang = ir.uv_recipe(np.array([0., 1., 0., -1.]), np.array([1., 0., -1., 0.]))
    assert np.array_equal(spd, np.ones(4)) and np.allclose(ang, [0., 90., 180., 270.], rtol=0, atol=1e-13)
    assert np.allclose(ir.direction_gap([359.5, 0.25, 10.], [0.5, 359.75, 350.]), [1., 0.5, 20.])


@pytest.mark.parametrize('name', ir.POLYNOMIAL_CASES)
def test_ct_exact_reproduces_polynomials(name):
    pts, rows, cols, cell = ir.CASES[name]
    xm, ym = ir.mesh(rows, cols, cell)
    inside = ir.owner_linear(pts, rows, cols, cell, np.zeros(pts.shape[0]))[1] >= 0
    for label, field, grad in (('affine', ir.affine, ir.affine_grad), ('quadratic', ir.quadratic, ir.quadratic_grad)):
        ct = ir.ct_exact(pts, field(pts[:, 0], pts[:, 1]), grad(pts[:, 0], pts[:, 1]))
        got = ct(xm, ym)
        want = field(xm, ym)
        assert np.array_equal(np.isnan(got), ~inside)
        top = float(np.max(np.abs(want[inside])))
        err = float(np.max(np.abs(got[inside] - want[inside])))
        print(f'{name} {label}: max |Clough-Tocher(exact gradients) - field| = {err:.3g} (bound {1e-12 * max(1., top):.3g})')
        assert err <= 1e-12 * max(1., top)
    # and scipy's own estimate of the gradients is what the override replaces: not exact on the quadratic
    from scipy.interpolate import CloughTocher2DInterpolator
    est = CloughTocher2DInterpolator(pts, ir.quadratic(pts[:, 0], pts[:, 1]), tol=1e-6, maxiter=400)
    assert np.max(np.abs(est.grad[:, 0, :] - ir.quadratic_grad(pts[:, 0], pts[:, 1]))) > 1e-9
    lin, _, _ = ir.owner_linear(pts, rows, cols, cell, ir.affine(pts[:, 0], pts[:, 1]))
    assert np.max(np.abs(lin[inside] - ir.affine(xm, ym)[inside])) <= 1e-12 * max(1., float(np.max(np.abs(ir.affine(xm, ym)[inside]))))
