"""K1 parity on the MI355X: HIP raster kernels (through the C ABI) vs the
golden vectors captured from the reference and vs the oracle.

Tolerances (stated per north_star "within stated FP tolerance"):
  * f64 layers (slope, aspect, usable updraft): rtol 1e-12 (+ atol 1e-15 for
    the threshold function, whose exp(x)-1 cancels for x ~ 1e-10 in the
    reference too) -- ocml vs glibc transcendental differences are a few ulp;
  * f32 orograph: at most 1 f32 ulp from the reference's f32-rounded value, and
    bit-identical in >= 99.9 % of cells.  (Cells where cos(aspect - wdirn) cancels to
    rounding noise, |w| ~ 1e-15 m/s, carry no information in their low bits in the
    reference either; tests/dev/soak_raster.py compares those absolutely, < 1e-12 * wspeed:
    7311 random cases, 1.1e9 cells, none beyond that.  On plateau, ridge and nodata DEMs such cells
    are many: test_gpu_raster_edges.py, criterion in raster_checks.py.)
"""
import numpy as np
import pytest
import torch

from raster_checks import check_orograph, ulp_diff_f32

pytestmark = pytest.mark.gpu


def test_slope_aspect_vs_golden(gpu, golden):
    from ssrs_amd import layers
    g = golden('g2_raster.npz')
    slope = layers.compute_slope_degrees(g['dem'], float(g['res']))
    aspect = layers.compute_aspect_degrees(g['dem'], float(g['res']))
    assert slope.dtype == np.float64 and slope.shape == g['slope'].shape
    np.testing.assert_allclose(slope, g['slope'], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(aspect, g['aspect'], rtol=1e-12, atol=1e-11)
    assert (slope[0] == 0).all() and (slope[:, -1] == 0).all() and (aspect[-1] == 0).all()


def test_slope_aspect_f32_dem_and_ragged_shapes(gpu):
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    rng = np.random.default_rng(5)
    for shape in [(3, 3), (5, 7), (33, 65), (64, 64), (67, 130), (129, 63)]:
        z = rng.normal(1000., 30., size=shape)
        s, a = layers.slope_aspect(z, 30.)
        np.testing.assert_allclose(s, orc.compute_slope_degrees(z, 30.), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(a, orc.compute_aspect_degrees(z, 30.), rtol=1e-12, atol=1e-11)
        z32 = z.astype(np.float32)
        s32, _ = layers.slope_aspect(z32, 30.)
        np.testing.assert_allclose(s32, orc.compute_slope_degrees(z32.astype(np.float64), 30.),
                                   rtol=1e-12, atol=1e-13)


def test_flat_dem_has_zero_gradient_quirk(gpu):
    """dz_dx == 0 -> 1e-10 substitution (layers.py:124): aspect = 270 on flat ground."""
    from ssrs_amd import layers
    from oracle import ssrs_oracle as orc
    z = np.full((9, 11), 123.0)
    s, a = layers.slope_aspect(z, 10.)
    assert np.array_equal(s, orc.compute_slope_degrees(z, 10.))
    assert np.array_equal(a, orc.compute_aspect_degrees(z, 10.))
    oro, use = layers.updraft_from_dem(z, 10., 10., 270., threshold=0.75)
    assert (oro == 0).all() and (use == 0).all()


def test_orographic_uniform_vs_golden(gpu, golden):
    from ssrs_amd import layers
    g = golden('g2_raster.npz')
    for dt in (np.float64, np.float32):
        oro = layers.compute_orographic_updraft(10., 270., g['slope'].astype(dt),
                                                g['aspect'].astype(dt))
        assert oro.dtype == np.float32
        if dt == np.float64:
            check_orograph(oro, g['orograph_f32'])
        else:   # f32 terrain inputs: 12 B/cell path, looser (input rounding)
            np.testing.assert_allclose(oro, g['orograph_f32'], rtol=2e-5, atol=2e-5)
    # reference call shape: constant-filled wind rasters (simulator.py:194-195)
    ones = np.ones_like(g['slope'])
    oro = layers.compute_orographic_updraft(10. * ones, 270. * ones, g['slope'], g['aspect'])
    check_orograph(oro, g['orograph_f32'])
    oro = layers.compute_orographic_updraft(10., 45., g['slope'], g['aspect'], 0.05)
    check_orograph(oro, g['orograph_min'].astype(np.float32))


def test_orographic_varying_wind_and_batch(gpu, golden):
    from ssrs_amd import layers
    g = golden('g2_raster.npz')
    oro = layers.compute_orographic_updraft(g['wspeed_var'], g['wdirn_var'], g['slope'],
                                            g['aspect'])
    check_orograph(oro, g['orograph_var'].astype(np.float32))
    # batched: [uniform-as-raster, varying] in one launch + fused threshold
    ws = np.stack([10. * np.ones_like(g['slope']), g['wspeed_var']])
    wd = np.stack([270. * np.ones_like(g['slope']), g['wdirn_var']])
    o, u = layers.orographic_updraft(ws, wd, g['slope'], g['aspect'], threshold=0.75)
    o, u = o.cpu().numpy(), u.cpu().numpy()
    check_orograph(o[0], g['orograph_f32'])
    check_orograph(o[1], g['orograph_var'].astype(np.float32))
    same = o[0] == g['orograph_f32']
    np.testing.assert_allclose(u[0][same], g['updraft'][same], rtol=1e-12, atol=1e-15)
    same = o[1] == g['orograph_var'].astype(np.float32)
    np.testing.assert_allclose(u[1][same], g['updraft_var'][same], rtol=1e-12, atol=1e-15)
    # uniform batch of scalars, more than one kernel-arg chunk (16)
    speeds = np.linspace(4., 14., 19)
    dirns = np.linspace(0., 350., 19)
    o, _ = layers.orographic_updraft(speeds, dirns, g['slope'], g['aspect'])
    from oracle import ssrs_oracle as orc
    for b in (0, 7, 16, 18):
        ref = orc.compute_orographic_updraft(speeds[b], dirns[b], g['slope'], g['aspect'])
        check_orograph(o[b].cpu().numpy(), ref.astype(np.float32))


def test_threshold_vs_golden(gpu, golden):
    from ssrs_amd import layers
    g = golden('g3_threshold.npz')
    for thr in (0.75, 0.5, 1.2):
        out = layers.get_above_threshold_speed(g['v'], thr)
        assert out.dtype == np.float64
        np.testing.assert_allclose(out, g[f'out_t{int(thr * 100)}'], rtol=1e-12, atol=1e-15)
    g2 = golden('g2_raster.npz')
    out = layers.get_above_threshold_speed(g2['orograph_f32'], 0.75)
    np.testing.assert_allclose(out, g2['updraft'], rtol=1e-12, atol=1e-15)
    # odd length -> scalar (non-vector) kernel
    out = layers.get_above_threshold_speed(g['v'][:1201], 0.75)
    np.testing.assert_allclose(out, g['out_t75'][:1201], rtol=1e-12, atol=1e-15)


def test_fused_dem_updraft_vs_golden(gpu, golden):
    """Trig-free fused kernel == reference slope/aspect/orographic/threshold chain."""
    from ssrs_amd import layers
    g = golden('g2_raster.npz')
    oro, use = layers.updraft_from_dem(g['dem'], float(g['res']), 10., 270., threshold=0.75)
    check_orograph(oro, g['orograph_f32'])
    same = oro == g['orograph_f32']
    np.testing.assert_allclose(use[same], g['updraft'][same], rtol=1e-12, atol=1e-15)
    # cells one f32 ulp off still give a usable updraft within f32 resolution
    np.testing.assert_allclose(use, g['updraft'], rtol=1e-5, atol=1e-7)
    from oracle import ssrs_oracle as orc
    for wd in (0., 45., 123.4, 270., 359.):
        oro, _ = layers.updraft_from_dem(g['dem'], float(g['res']), 7.5, wd)
        ref = orc.compute_orographic_updraft(7.5, wd, g['slope'], g['aspect'])
        check_orograph(oro, ref.astype(np.float32))


def test_raster_c2_size_properties(gpu):
    """BASELINE config-2 grid (5000 x 6000 @10 m): fused kernel vs elementwise
    kernels on the same device + linearity in wind speed (size-independent)."""
    from ssrs_amd import layers
    from ssrs_amd.synthetic import synthetic_dem
    dem = torch.from_numpy(synthetic_dem((5000, 6000), 10.)).cuda()
    oro, use = layers.updraft_from_dem(dem, 10., 10., 270., threshold=0.75)
    slope, aspect = layers.slope_aspect(dem, 10.)
    oro2, use2 = layers.orographic_updraft(10., 270., slope, aspect, threshold=0.75)
    d = (oro.view(torch.int32).long() - oro2.view(torch.int32).long()).abs()
    assert int(d.max()) <= 1 and float((d == 0).float().mean()) >= 0.999
    same = d == 0
    assert torch.allclose(use[same], use2[same], rtol=1e-12, atol=1e-15)
    oro_half, _ = layers.updraft_from_dem(dem, 10., 5., 270.)
    assert torch.allclose(oro_half * 2, oro, rtol=3e-7, atol=0)   # linear in wspeed
    assert float(oro.min()) >= 0.0 and bool((oro[0] == 0).all()) and bool((oro[:, 0] == 0).all())


def test_wind_lattice_interpolation_vs_oracle(gpu):
    """K6: u/v bilinear interpolation of a WTK-shaped lattice (simulator.py:778-792)."""
    from ssrs_amd.wind import interpolate_wind_lattice
    from ssrs_amd.synthetic import wind_lattice
    from oracle import ssrs_oracle as orc
    from scipy.interpolate import RegularGridInterpolator
    rows, cols, res = 120, 150, 100.
    x, y, ws, wd = wind_lattice((cols * res / 1000., rows * res / 1000.), 2.0, phase=0.3)
    xs = np.arange(cols) * res / 1000.
    ys = np.arange(rows) * res / 1000.
    pts = np.stack(np.meshgrid(np.clip(ys, y[0], y[-1]), np.clip(xs, x[0], x[-1]), indexing='ij'), -1)

    def interp(vals):
        return RegularGridInterpolator((y, x), vals.reshape(y.size, x.size))(pts)
    ref_s, ref_d = orc.interpolate_wind_uv(ws, wd, interp)
    got_s, got_d = interpolate_wind_lattice(x, y, ws, wd, (rows, cols), res)
    np.testing.assert_allclose(got_s.cpu().numpy(), ref_s, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got_d.cpu().numpy(), ref_d, rtol=1e-12, atol=1e-10)
    assert float(got_d.min()) >= 0.0 and float(got_d.max()) < 360.0
    # batched (seasonal) call == per-snapshot calls
    phases = [0.0, 1.0, 2.0]
    lat = [wind_lattice((cols * res / 1000., rows * res / 1000.), 2.0, phase=p) for p in phases]
    bs, bd = interpolate_wind_lattice(x, y, np.stack([l[2] for l in lat]),
                                      np.stack([l[3] for l in lat]), (rows, cols), res)
    for i, l in enumerate(lat):
        s1, d1 = interpolate_wind_lattice(x, y, l[2], l[3], (rows, cols), res)
        assert torch.equal(bs[i], s1) and torch.equal(bd[i], d1)


def test_thermals_blur_exact_and_seeding_statistics(gpu):
    """a5 (layers.py:188-214): the Gaussian blur equals scipy's on the same seed
    field; the seeding is checked statistically (the reference replays a serial
    global RNG: only statistical parity exists)."""
    from scipy import ndimage
    from ssrs_amd import thermals
    rng = np.random.default_rng(4)
    field = (rng.random((90, 130)) < 0.01) * rng.lognormal(5., 0.5, size=(90, 130))
    got = thermals.gaussian_blur(field, 4.0)
    np.testing.assert_allclose(got, ndimage.gaussian_filter(field, sigma=4, mode='constant'),
                               rtol=1e-12, atol=1e-12)
    rows, cols = 1000, 1200
    aspect = rng.uniform(0., 360., (rows, cols))
    seeds = thermals.thermal_seeds(aspect, 2.0, seed=11)
    by, bx = int(0.1 * rows), int(0.1 * cols)
    assert (seeds[:by] == 0).all() and (seeds[-by:] == 0).all()
    assert (seeds[:, :bx] == 0).all() and (seeds[:, -bx:] == 0).all()
    inner = seeds[by:rows - by, bx:cols - bx]
    wt = 1000. + np.abs(aspect[by:rows - by, bx:cols - bx] - 180.) / 180. * 2000.
    expect = (1. / (wt.astype(int) - 1)).sum()             # expected number of seeded cells
    n = int((inner > 0).sum())
    assert abs(n - expect) < 5 * np.sqrt(expect), (n, expect)
    logs = np.log(inner[inner > 0])
    assert abs(logs.mean() - 5.0) < 5 * 0.5 / np.sqrt(n) and abs(logs.std() - 0.5) < 0.1
    # reproducible per seed, different across seeds
    assert np.array_equal(seeds, thermals.thermal_seeds(aspect, 2.0, seed=11))
    assert not np.array_equal(seeds, thermals.thermal_seeds(aspect, 2.0, seed=12))
    th = thermals.compute_thermals(aspect, 2.0, seed=11)
    np.testing.assert_allclose(th, ndimage.gaussian_filter(seeds, sigma=4, mode='constant'),
                               rtol=1e-12, atol=1e-12)


def test_fused_dem_lattice_updraft_equals_the_three_kernel_chain(gpu):
    """Snapshot / seasonal raster in one pass (ssrs_updraft_from_dem_lattice) against
    wind interpolation -> slope/aspect -> orographic + threshold: the same numbers up to
    the orograph's f32 rounding (<= 1 ulp; cells whose value is cancellation noise are
    compared absolutely), for one snapshot and for a batch; ragged shape."""
    from ssrs_amd import layers
    from ssrs_amd.wind import interpolate_wind_lattice
    from ssrs_amd.synthetic import synthetic_dem, wind_lattice
    rows, cols, res = 300, 517, 100.
    z = synthetic_dem((rows, cols), res, seed=9)
    slope, aspect = layers.slope_aspect(z, res)
    B = 3
    lat = [wind_lattice((cols * res / 1000., rows * res / 1000.), phase=0.7 * s) for s in range(B)]
    x, y = lat[0][0], lat[0][1]
    ws = np.stack([l[2] for l in lat]); wd = np.stack([l[3] for l in lat])
    s_r, d_r = interpolate_wind_lattice(x, y, ws, wd, (rows, cols), res)
    oro_ref, use_ref = layers.orographic_updraft(s_r, d_r, slope, aspect, threshold=0.75)
    oro, use = layers.updraft_from_dem_lattice(z, res, x, y, ws, wd, threshold=0.75)
    assert tuple(oro.shape) == (B, rows, cols) and oro.dtype == torch.float32 and use.dtype == torch.float64
    a, b = oro.cpu().numpy(), oro_ref.cpu().numpy()
    d = ulp_diff_f32(a, b)
    noise = np.abs(a.astype(np.float64) - b.astype(np.float64)) < 1e-11
    assert (d[~noise] <= 1).all(), int(d[~noise].max())
    assert (d == 0).mean() > 0.99
    np.testing.assert_allclose(use.cpu().numpy(), use_ref.cpu().numpy(), rtol=2e-5, atol=1e-7)
    same = a == b
    np.testing.assert_allclose(use.cpu().numpy()[same], use_ref.cpu().numpy()[same], rtol=1e-12, atol=1e-15)
    o1, u1 = layers.updraft_from_dem_lattice(z, res, x, y, ws[1], wd[1], threshold=0.75)
    assert tuple(o1.shape) == (rows, cols)
    assert torch.equal(o1, oro[1]) and torch.equal(u1, use[1])
