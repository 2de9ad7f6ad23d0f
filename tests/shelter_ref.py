"""Plain-numpy statement of the sheltered orographic updraft (K9): the terrain-shelter angle Sx and the adjustment
by it and by the flight height.  Written from the model's text (DESIGN.md K9 / include/ssrs_hip.h), looping over the
K samples and vectorised over the cells, every expression in the operation order the text gives.  Nothing here touches
the device; test_shelter_host.py pins it analytically, test_gpu_shelter.py judges the kernels by it."""
import numpy as np

DEFAULT_COEFFS = (4e-5, 2.8e-3, 0.8, 0.35, 0.095, -0.09, 1.0)
NEUTRAL_COEFFS = (0., 0., 1., 1., 0., 0., 0.)
SNAP = 1e-9


def ray_step(wdirn, ray_axes):
    """Upwind unit step (ur, uc) in (row, col) for a wind from `wdirn` degrees clockwise from north."""
    rad = np.asarray(wdirn, dtype=np.float64) * np.pi / 180.
    if ray_axes == 'row_north':
        return np.cos(rad), np.sin(rad)
    if ray_axes == 'row_east':
        return np.sin(rad), np.cos(rad)
    raise ValueError(ray_axes)


def sample_offset(k, u):
    """o = (double)k * u -> (io, fo) with the snap: fo < 1e-9 -> 0; fo > 1 - 1e-9 -> io + 1, 0."""
    o = float(k) * np.asarray(u, dtype=np.float64)
    fl = np.floor(o)
    fo = o - fl
    io = fl.astype(np.int64)
    low = fo < SNAP
    high = ~low & (fo > 1. - SNAP)
    io = np.where(high, io + 1, io)
    fo = np.where(low | high, 0., fo)
    return io, fo


def tan_sx(z, res, wdirn=None, dmax=500., ray_axes='row_east', step=None, return_count=False):
    """T = max_k (zs_k - z0) / (k res) per cell; 0 where no sample is valid, z0 is NaN or the direction is NaN.
    wdirn: a scalar or a (rows, cols) raster of degrees; or `step` = (ur, uc) directly.  return_count: also the
    number of valid (in-raster) samples of every cell."""
    z = np.asarray(z, dtype=np.float64)
    rows, cols = z.shape
    K = int(np.floor(dmax / res))
    if K < 1:
        raise ValueError('K = floor(dmax / res) < 1')
    ur, uc = ray_step(wdirn, ray_axes) if step is None else step
    ur = np.broadcast_to(np.asarray(ur, dtype=np.float64), z.shape)
    uc = np.broadcast_to(np.asarray(uc, dtype=np.float64), z.shape)
    dir_ok = ~(np.isnan(ur) | np.isnan(uc))
    ur = np.where(dir_ok, ur, 0.)
    uc = np.where(dir_ok, uc, 0.)
    r0, c0 = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    T = np.full(z.shape, -np.inf)
    count = np.zeros(z.shape, dtype=np.int64)

    def gather(i, j, mask):
        out = np.zeros(z.shape)                  # a neighbour of weight 0 is not read and enters as 0.0
        out[mask] = z[i[mask], j[mask]]
        return out

    with np.errstate(invalid='ignore'):
        for k in range(1, K + 1):
            io_r, fo_r = sample_offset(k, ur)
            io_c, fo_c = sample_offset(k, uc)
            i, j = r0 + io_r, c0 + io_c
            ok = dir_ok & (i >= 0) & ((i + 1 <= rows - 1) | ((fo_r == 0.) & (i <= rows - 1))) \
                & (j >= 0) & ((j + 1 <= cols - 1) | ((fo_c == 0.) & (j <= cols - 1)))
            z00 = gather(i, j, ok)
            z01 = gather(i, j + 1, ok & (fo_c != 0.))
            z10 = gather(i + 1, j, ok & (fo_r != 0.))
            z11 = gather(i + 1, j + 1, ok & (fo_r != 0.) & (fo_c != 0.))
            zs = (z00 * (1. - fo_c) + z01 * fo_c) * (1. - fo_r) + (z10 * (1. - fo_c) + z11 * fo_c) * fo_r
            inv_d = 1.0 / (float(k) * res)
            tk = (zs - z) * inv_d
            take = ok & (tk > T)                 # a NaN tk compares false: skipped
            T = np.where(take, tk, T)
            count += ok
    T = np.where(np.isneginf(T) | np.isnan(z), 0., T)
    return (T, count) if return_count else T


def sx_degrees(T):
    return np.degrees(np.arctan(T))


def height_factor(slope_deg, height, coeffs):
    a, b, c, d, e, f, _ = coeffs
    return (a * height ** 2 + b * height + c) * d ** (e - np.cos(np.radians(slope_deg))) + f


def adjust(w0, T, slope_deg, height=80., coeffs=DEFAULT_COEFFS, min_updraft_val=0.):
    """w = max(min_updraft_val, w0 F_sx / F_h): w0 the unclamped original updraft (f64), T = tan Sx."""
    f_sx = np.maximum(0., 1. + coeffs[6] * T)
    return np.maximum(min_updraft_val, w0 * f_sx / height_factor(slope_deg, height, coeffs))
