"""Checks shared by the raster (K1) tests: test_gpu_raster.py, test_gpu_raster_edges.py and
tests/dev/soak_raster.py.  Plain numpy; nothing here touches the device.

The criterion for an f32 orograph (check_orograph_cells), against the reference's f64 value:
  * every cell is within 1 f32 ulp of f32(ref), OR |got - ref| <= 1e-12 * wspeed.  No cell is
    left out.  The second clause is an absolute bound far tighter than one ulp of any value that
    matters; it exists because the reference's own value is rounding noise of the degree ->
    radian conversion where cos(aspect - wdirn) cancels (1e-17 m/s against an exact 0), which on
    plateau and ridge DEMs is a large share of the raster (a wind along a ridge: most of it);
  * of the cells with ref > 1e-9 * wspeed ("signal" cells), at least 99.9 % are bit-identical.
    A wind along a ridge leaves no such cell, so the count is returned and the caller asserts
    that at least one of its winds had enough of them.
f64 layers: slope rtol 1e-12 / atol 1e-13, aspect rtol 1e-12 / atol 1e-11, usable updraft
rtol 1e-12 / atol 1e-15 (ocml against glibc transcendentals: a few ulp; exp(x) - 1 cancels for
x ~ 1e-10 in the reference too).
"""
import numpy as np

SLOPE_TOL = dict(rtol=1e-12, atol=1e-13)
ASPECT_TOL = dict(rtol=1e-12, atol=1e-11)
USABLE_TOL = dict(rtol=1e-12, atol=1e-15)
NOISE_ABS = 1e-12        # x wspeed: absolute bound on cancellation-noise cells
SIGNAL_MIN = 1e-9        # x wspeed: cells above this carry a value, not noise
IDENTICAL_SHARE = 0.999


def ulp_diff_f32(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def check_orograph(got, ref32):
    """The strict form for smooth DEMs: every cell within 1 f32 ulp, >= 99.9 % bit-identical."""
    d = ulp_diff_f32(got, ref32)
    assert d.max() <= 1, f'max f32 ulp diff {d.max()}'
    assert (d == 0).mean() >= IDENTICAL_SHARE, f'only {(d == 0).mean():.5f} bit-identical'


def check_orograph_cells(got, ref_f64, wspeed, label=''):
    """The criterion of the module docstring.  Returns the figures it judged by:
    signal (cells with ref > 1e-9 wspeed), worst_ulp and identical (share) over them,
    noise_cells (cells that pass by the absolute clause only) and noise_abs (the largest
    absolute difference on those).  Prints them, so that a run with -s records them."""
    got = np.asarray(got)
    ref = np.asarray(ref_f64, dtype=np.float64)
    assert got.dtype == np.float32 and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    wspeed = float(wspeed)
    d = ulp_diff_f32(got, ref.astype(np.float32))
    with np.errstate(invalid='ignore'):
        absd = np.abs(got.astype(np.float64) - ref)
        near = absd <= NOISE_ABS * wspeed          # False for a NaN
    bad = (d > 1) & ~near
    assert not bad.any(), (f'{label}: {int(bad.sum())} cells beyond 1 f32 ulp and {NOISE_ABS:g} * wspeed; '
                           f'first at {tuple(np.argwhere(bad)[0])}: got {got[bad][0]!r} ref {ref[bad][0]!r}')
    signal = ref > SIGNAL_MIN * wspeed
    n = int(signal.sum())
    noise = d > 1
    stats = dict(signal=n, worst_ulp=int(d[signal].max()) if n else 0,
                 identical=float((d[signal] == 0).mean()) if n else 1.0,
                 noise_cells=int(noise.sum()), noise_abs=float(absd[noise].max()) if noise.any() else 0.0)
    print(f'orograph {label}: signal {n} worst_ulp {stats["worst_ulp"]} identical {stats["identical"]:.5f} '
          f'noise_cells {stats["noise_cells"]} noise_abs {stats["noise_abs"]:.2e}')
    assert stats['identical'] >= IDENTICAL_SHARE, \
        f'{label}: only {stats["identical"]:.5f} of {n} signal cells bit-identical'
    return stats


def check_usable(use, oro, threshold, ref_oro32, ref_use, orc):
    """Usable updraft (f64): against the reference's on the cells whose orograph is bit-equal,
    and on EVERY cell against the oracle's threshold function of the f32 orograph it came with."""
    use, oro = np.asarray(use), np.asarray(oro)
    assert use.dtype == np.float64 and use.shape == oro.shape and not np.isnan(use).any()
    same = oro == np.asarray(ref_oro32, dtype=np.float32)
    np.testing.assert_allclose(use[same], np.asarray(ref_use)[same], **USABLE_TOL)
    np.testing.assert_allclose(use, orc.get_above_threshold_speed(oro, threshold), **USABLE_TOL)


def branch_share(z, res, orc):
    """Share of the interior cells that take the dz_dx == 0 -> 1e-10 substitution with a value
    that shows (dz_dy != 0), from the oracle's gradients."""
    gx, gy = orc._horn_gradients(np.asarray(z, dtype=np.float64), res)
    with np.errstate(invalid='ignore'):
        return float(((gx == 0) & (gy != 0)).mean())


def nan_stencil_cells(z):
    """Interior cells whose 3 x 3 Horn stencil (the centre is not part of it) touches a NaN."""
    nan = np.isnan(np.asarray(z, dtype=np.float64))
    p = np.pad(nan, 1)
    rows, cols = nan.shape
    hit = np.zeros_like(nan)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if (dr, dc) != (1, 1):
                hit |= p[dr:dr + rows, dc:dc + cols]
    hit[0] = hit[-1] = False
    hit[:, 0] = hit[:, -1] = False
    return hit


def lattice_reference(z, res, x_km, y_km, wspeed, wdirn, orc, min_updraft_val=0., threshold=None):
    """Independent reference of the DEM + wind-lattice raster for ONE snapshot: east / north
    components through scipy's RegularGridInterpolator at the cell centres clamped to the lattice
    hull (simulator.py:778-792 as oracle.interpolate_wind_uv restates it), then the oracle's
    slope / aspect / orographic / threshold.  An axis with a single sample is constant along it.
    Returns (orograph f64, usable f64 | None, largest interpolated speed)."""
    from scipy.interpolate import RegularGridInterpolator
    z = np.asarray(z, dtype=np.float64)
    rows, cols = z.shape
    x, y = np.asarray(x_km, dtype=np.float64), np.asarray(y_km, dtype=np.float64)
    ws = np.asarray(wspeed, dtype=np.float64).reshape(y.size, x.size)
    wd = np.asarray(wdirn, dtype=np.float64).reshape(y.size, x.size)
    if x.size == 1:
        x, ws, wd = np.array([x[0], x[0] + 1.]), np.repeat(ws, 2, axis=1), np.repeat(wd, 2, axis=1)
    if y.size == 1:
        y, ws, wd = np.array([y[0], y[0] + 1.]), np.repeat(ws, 2, axis=0), np.repeat(wd, 2, axis=0)
    xs = np.arange(cols) * res / 1000.
    ys = np.arange(rows) * res / 1000.
    pts = np.stack(np.meshgrid(np.clip(ys, y[0], y[-1]), np.clip(xs, x[0], x[-1]), indexing='ij'), -1)

    def interp(vals):
        return RegularGridInterpolator((y, x), vals)(pts)
    s, d = orc.interpolate_wind_uv(ws, wd, interp)
    oro = orc.compute_orographic_updraft(s, d, orc.compute_slope_degrees(z, res),
                                         orc.compute_aspect_degrees(z, res), min_updraft_val)
    use = None if threshold is None else orc.get_above_threshold_speed(oro.astype(np.float32), threshold)
    return oro, use, float(s.max())
