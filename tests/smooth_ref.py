"""References for K11, the reflected Gaussian smoothing of the improved orographic updraft (include/ssrs_hip.h):
scipy's gaussian_filter, a plain-numpy statement of the index rule in ascending order of the taps, the same statement in
the kernel's own order (k = R .. 1, pairs first), the bound the tests hold the device to, and the cases that the emulation
and the GPU tests share."""
import math

import numpy as np

MIN_VAL, THRESHOLD = 0., 0.75


def sanitised(x):
    """The raster as the kernel loads it: f64, a non-finite value enters as 0."""
    x = np.asarray(x)
    return np.where(np.isfinite(x), x, 0.).astype(np.float64)


def scipy_smooth(x, sigma):
    """THE reference: gaussian_filter of the sanitised raster, mode='reflect' (scipy's default), truncate = 4."""
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(sanitised(x), sigma, mode='reflect')


def radius(sigma):
    return int(4. * sigma + 0.5)


def weights(sigma):
    """(R, w[0 .. R]) as csrc/gauss.h forms them: libm's exp, the sum in ascending k = -R .. R, one division each."""
    R = radius(sigma)
    e = [math.exp(-0.5 / (sigma * sigma) * k * k) for k in range(-R, R + 1)]
    total = 0.
    for v in e:
        total += v
    return R, np.array([v / total for v in e[R:]])


def reflect_index(i, n):
    """Source index of position i of the 'reflect' extension d c b a | a b c d | d c b a of [0, n), to any depth."""
    m = np.mod(np.asarray(i, dtype=np.int64), 2 * n)          # (non-negative)
    return np.where(m < n, m, 2 * n - 1 - m)


def numpy_smooth(x, sigma):
    """The index rule in plain numpy, summed in ASCENDING tap order k = -R .. R from 0.0 (not the kernel's order)."""
    R, w = weights(sigma)
    out = sanitised(x)
    for axis in (0, 1):
        n = out.shape[axis]
        acc = np.zeros_like(out)
        for k in range(-R, R + 1):
            acc += w[abs(k)] * np.take(out, reflect_index(np.arange(n) + k, n), axis=axis)
        out = acc
    return out


def kernel_order_smooth(x, sigma):
    """The sum as the header states it: acc = x[p] w[0], then k = R .. 1: acc = acc + (x[p - k] + x[p + k]) w[k], every
    operation rounded.  IEEE f64 elementwise, so the kernel's bits."""
    R, w = weights(sigma)
    out = sanitised(x)
    for axis in (0, 1):
        n = out.shape[axis]
        p = np.arange(n)
        acc = out * w[0]
        for k in range(R, 0, -1):
            acc = acc + (np.take(out, reflect_index(p - k, n), axis=axis) + np.take(out, reflect_index(p + k, n), axis=axis)) * w[k]
        out = acc
    return out


def bound(sigma, x):
    """4 (2 R + 3) 2^-53 max|x|, absolute: two passes of R + 1 rounded terms plus the normalisation of the weights."""
    return 4. * (2 * radius(sigma) + 3) * 2. ** -53 * float(np.abs(sanitised(x)).max())


def clamp_f32(smooth, min_val=MIN_VAL):
    """orograph = (float)(smooth > min ? smooth : min)."""
    return np.where(smooth > min_val, smooth, min_val).astype(np.float32)


def field(shape, seed=0):
    """An unclamped updraft-like f32 raster: both signs, a few m/s, structure at several scales."""
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    x = 1.9 * np.sin(r / 3.3 + seed) * np.cos(c / 4.1) + 0.8 * np.sin((r + 2. * c) / 2.7) - 0.3 + 0.01 * r - 0.02 * c
    return x.astype(np.float32)


def holed(x):
    """A NaN block, one -inf (what the sheltered kernel gives a nodata cell with the clamp lifted) and one +inf."""
    x = x.copy()
    rows, cols = x.shape
    x[rows // 2 - 1:rows // 2 + 2, cols // 3:cols // 3 + 3] = np.nan
    x[1, cols - 2] = -np.inf
    x[rows - 1, 0] = np.inf
    return x


# (name, shape, sigma, holes): R = 32 is two rounds of the unrolled loop, 5 / 3 / 8 its leading steps alone, 18 and 120 both;
# (150, 140) has two tiles along either blur axis, the others several along the lines; (3, 5) with R = 8 > 2 n, (1, 7),
# (7, 1) and (2, 2) reflect repeatedly; R = 120 takes the large LDS tile, R = 160 global memory; sigma 0.1 is the identity
CASES = [
    ('70x45-s8', (70, 45), 8., False), ('70x45-s1.3', (70, 45), 1.3, False),
    ('33x65-s8', (33, 65), 8., False), ('33x65-s1.3', (33, 65), 1.3, False),
    ('3x5-s2', (3, 5), 2., False), ('1x7-s1.3', (1, 7), 1.3, False), ('7x1-s1.3', (7, 1), 1.3, False),
    ('2x2-s0.8', (2, 2), 0.8, False),
    ('40x50-s40', (40, 50), 40., False),
    ('33x65-s0.1', (33, 65), 0.1, False),
    ('70x45-s8-holes', (70, 45), 8., True), ('33x65-s1.3-holes', (33, 65), 1.3, True),
    ('150x140-s8', (150, 140), 8., False), ('150x140-s4.5-holes', (150, 140), 4.5, True),
    ('33x65-s30', (33, 65), 30., False),
]
CASE_IDS = [c[0] for c in CASES]
LDS_MAX_RADIUS = 128


def case_input(shape, holes):
    x = field(shape)
    return holed(x) if holes and min(shape) >= 3 else x


def check_outputs(x, sigma, smooth, orograph, usable, label, min_val=MIN_VAL, threshold=THRESHOLD):
    """The three properties every case is held to; prints the largest deviation from scipy."""
    from oracle import ssrs_oracle as orc
    want = scipy_smooth(x, sigma)
    dev, lim = float(np.abs(smooth - want).max()), bound(sigma, x)
    exact = np.array_equal(smooth.view(np.int64), want.view(np.int64))
    print(f'{label}: R = {radius(sigma)}, largest |smooth - scipy| = {dev:.3e} (bound {lim:.3e}), bit for bit: {exact}')
    assert not np.isnan(smooth).any()
    assert dev <= lim, label
    if orograph is not None:
        assert orograph.dtype == np.float32
        assert np.array_equal(orograph.view(np.int32), clamp_f32(smooth, min_val).view(np.int32)), label
    if usable is not None:
        np.testing.assert_allclose(usable, orc.get_above_threshold_speed(clamp_f32(smooth, min_val), threshold),
                                   rtol=1e-12, atol=1e-15, err_msg=label)
    return dev
