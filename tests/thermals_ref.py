"""References for a5, the random thermal fields (ssrs_amd/csrc/thermals.hip): the device's own seeding rule restated in
numpy cell by cell (the Philox draw is stateless and keyed by (seed, flat cell index), so the seed field is a pure
function), the zero-padded blur in the kernel's order of the taps, scipy's gaussian_filter, the bound the tests hold the
device to, and the cases that the host and the GPU tests share.  Which cells are seeded is an integer decision and exact;
only the amplitude goes through libm.  Parity with the REFERENCE's random stream stays statistical (tests/g13_stats.py)."""
import math

import numpy as np

import smooth_ref
from oracle.philox import philox4x32_10
from smooth_ref import radius, weights                    # (R, w[0 .. R]) as csrc/gauss.h forms them  # noqa: F401

SCALE = 2.0                                                # thermal_intensity_scale of every case (what Simulator passes)
TWO32 = 1 << 32


def words(seed, cell):
    """The four Philox4x32-10 words of rocrand_init(seed, cell, 0) + rocrand4: counter (0, 0, cell lo, cell hi), key
    (seed lo, seed hi), the seed masked to 64 bits.  uint64 arrays holding 32-bit values, shaped like `cell`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    i = np.asarray(cell, dtype=np.uint64)
    return philox4x32_10(0, 0, i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)


def interior(shape):
    """The cells inside the 10 % border: by <= r < rows - by, bx <= c < cols - bx, by = int(0.1 rows), bx = int(0.1 cols)."""
    rows, cols = shape
    by, bx = int(0.1 * rows), int(0.1 * cols)
    inside = np.zeros(shape, dtype=bool)
    inside[by:rows - by, bx:cols - bx] = True
    return inside


def ring(shape):
    """The interior cells that touch the border (or the raster's edge where the border is empty)."""
    inside = interior(shape)
    core = np.zeros(shape, dtype=bool)
    core[1:-1, 1:-1] = inside[:-2, 1:-1] & inside[2:, 1:-1] & inside[1:-1, :-2] & inside[1:-1, 2:]
    return inside & ~core


def nvals_of(aspect):
    """int(wt) - 1 with wt = 1000 + |aspect - 180| / 180 * 2000, truncated; int64.  -1 where the aspect is NaN: that is
    what the DEVICE's conversion of a NaN gives today (so the draw always passes); the reference raises there."""
    a = np.asarray(aspect, dtype=np.float64)
    wt = 1000.0 + (np.abs(a - 180.0) / 180.0) * 2000.0
    nan = np.isnan(wt)
    return np.where(nan, -1, np.trunc(np.where(nan, 0., wt)).astype(np.int64) - 1)


def amplitude(w1, w2, scale):
    """exp((scale + 3) + 0.5 z), z the Box-Muller normal of words 1 and 2; Python f64 and libm, one cell."""
    u1 = (float(w1) + 1.0) * 2.0 ** -32                    # (0, 1]
    u2 = float(w2) * 2.0 ** -32
    z = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * 3.141592653589793 * u2)
    return math.exp((scale + 3.0) + 0.5 * z)


def seed_field(aspect, scale, seed):
    """(values f64, hit bool) of k_thermal_seeds: a cell is seeded iff it is interior and w0 nvals < 2^32 -- in integers;
    the kernel's u0 * nvals < 1.0 is the same decision, both products being exact in f64 below 2^44 -- and then holds
    `amplitude`; every other cell is +0.0.  A NaN aspect counts as always seeded (see nvals_of)."""
    a = np.asarray(aspect, dtype=np.float64)
    rows, cols = a.shape
    cell = np.arange(rows * cols, dtype=np.uint64).reshape(rows, cols)
    w = words(seed, cell)
    hit = interior(a.shape) & (w[0].astype(np.int64) * nvals_of(a) < TWO32)
    values = np.zeros(a.shape)
    for r, c in zip(*np.nonzero(hit)):
        values[r, c] = amplitude(w[1][r, c], w[2][r, c], scale)
    return values, hit


def full_weights(sigma):
    """(R, w[-R .. R]): the 2 R + 1 weights of csrc/gauss.h from smooth_ref.weights' half (w[-k] has w[k]'s bits)."""
    R, w = weights(sigma)
    return R, np.concatenate((w[:0:-1], w))


def blur_kernel_order(x, sigma):
    """k_blur_pass, axis 0 then axis 1: acc = 0.0, then k = -R .. R ascending acc = acc + w[k] x[p + k], every operation
    rounded, an out-of-raster tap skipped.  IEEE f64 elementwise, so the kernel's bits."""
    R, w = full_weights(sigma)
    out = np.array(x, dtype=np.float64)
    for axis in (0, 1):
        n = out.shape[axis]
        src, acc = np.moveaxis(out, axis, 0), np.zeros_like(out)
        dst = np.moveaxis(acc, axis, 0)
        for k in range(-R, R + 1):
            lo, hi = max(0, -k), min(n, n - k)            # p with 0 <= p + k < n
            if lo < hi:
                dst[lo:hi] = dst[lo:hi] + w[k + R] * src[lo + k:hi + k]
        out = acc
    return out


def scipy_blur(x, sigma):
    """THE reference for the blur: gaussian_filter(x, sigma, mode='constant'), truncate = 4 (layers.py of the reference)."""
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(np.asarray(x, dtype=np.float64), sigma, mode='constant')


def bound(sigma, x):
    """4 (2 R + 3) 2^-53 max|x|, absolute: smooth_ref.bound's derivation (two passes of at most 2 R + 1 rounded terms
    plus the normalisation of the weights)."""
    return smooth_ref.bound(sigma, x)


def field(aspect, scale, seed, sigma):
    return blur_kernel_order(seed_field(aspect, scale, seed)[0], sigma)


# ---------------------------------------------------------------------------------------------------- the shared cases
SIGMA = 4.0                                                # every case; R = 16, the widest the fused kernel serves
# R = 0, 1, 5; 4.1: R = 16 with other weights; 4.2: R = 17, the first radius that takes the chain inside
# ssrs_thermal_fields; 5.0: R = 20
EXTRA_SIGMAS = (0.1, 0.3, 1.3, 4.1, 4.2, 5.0)
EXTRA_SIGMA_SHAPES = ((1, 64), (64, 1), (9, 9), (33, 65), (20, 200))
# tiny rasters, aspect 180 everywhere: below one 32 x 64 tile, narrower than the radius, and (1, 1) .. (9, 9) with
# int(0.1 rows) == 0, where every cell is interior.  Each listed seed puts exactly ONE thermal on the raster.
TINY = (((1, 1), (856, 1801, 1831)), ((2, 2), (409, 856, 870)), ((1, 64), (18, 20, 28)), ((64, 1), (18, 20, 28)),
        ((9, 9), (18, 20, 28)), ((10, 10), (18, 20, 28)), ((3, 5), (35, 128, 250)), ((16, 16), (12, 18, 20)))
# one tile exactly, one cell less and more, two tiles along either axis, thin rasters, ragged ones
MID_SHAPES = ((7, 300), (300, 7), (31, 63), (32, 64), (33, 65), (64, 128), (65, 129), (20, 200), (96, 70))
MID_SEEDS = tuple(range(1000, 1040)) + (2 ** 63 + 5, 2 ** 64 - 1)          # 42: more than one launch of 32
# (64, 128), aspect 180: the first four lose a seeded cell under nvals + 1, the last four gain one under nvals - 1
CRITICAL_SHAPE = (64, 128)
CRITICAL_LOSE, CRITICAL_GAIN = (83, 195, 262, 624), (43, 366, 375, 720)
# the same raster at aspect 180.0675: wt = 1000.75, so nvals is still 999 and the first four seeds hold the same cells, but a
# ROUNDED wt gives 1000 and loses one each (the random aspects of the mid-size cases cannot tell: a 0.05 % change of rate)
FRACTION_ASPECT = 180.0675
DENSE_SHAPE, DENSE_SEED = (90, 140), 7                     # aspect NaN: every interior cell seeded


def flat_aspect(shape):
    return np.full(shape, 180.0)


def fraction_aspect(shape):
    return np.full(shape, FRACTION_ASPECT)


def mid_aspect(shape):
    rows, cols = shape
    a = np.random.default_rng(rows * 1000 + cols).uniform(0, 360, shape)
    a[::3, ::2] = 180.0
    return a


def sigmas_of(shape):
    return (SIGMA,) + (EXTRA_SIGMAS if shape in EXTRA_SIGMA_SHAPES else ())


# (name, shape, aspect function, seeds)
CASES = ([('%dx%d-flat' % shape, shape, flat_aspect, seeds) for shape, seeds in TINY]
         + [('%dx%d' % shape, shape, mid_aspect, MID_SEEDS) for shape in MID_SHAPES]
         + [('%dx%d-critical' % CRITICAL_SHAPE, CRITICAL_SHAPE, flat_aspect, CRITICAL_LOSE + CRITICAL_GAIN),
            ('%dx%d-fraction' % CRITICAL_SHAPE, CRITICAL_SHAPE, fraction_aspect, CRITICAL_LOSE)])
CASE_IDS = [c[0] for c in CASES]
BLUR_CASES = [(shape, sigma) for shape in [s for s, _ in TINY] + list(MID_SHAPES) for sigma in sigmas_of(shape)]
