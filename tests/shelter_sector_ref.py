"""Plain-numpy statement of the sector-averaged shelter angle (K9, include/ssrs_hip.h): Winstral's Sx averaged over
M = 2 H + 1 azimuths around the direction the wind comes from.  Every ray is shelter_ref.tan_sx; only the azimuth list,
the mean of the angles and its tangent are stated here.  Nothing touches the device."""
import numpy as np

import shelter_ref as ref

MAX_RAYS = 61


def ray_count(half_width, step):
    """(H, M): H = floor(W / S + 1e-9), M = 2 H + 1."""
    if not (np.isfinite(half_width) and 0. <= half_width <= 90.):
        raise ValueError(f'sector half-width {half_width!r}')
    if not (np.isfinite(step) and step > 0.):
        raise ValueError(f'sector step {step!r}')
    h = np.floor(float(half_width) / float(step) + 1e-9)
    if not 2. * h + 1. <= MAX_RAYS:
        raise ValueError(f'M = {2. * h + 1.:.0f} > {MAX_RAYS}')
    return int(h), 2 * int(h) + 1


def azimuths(wdirn, half_width, step):
    """[A_m] = [A + (double)(m - H) S for m = 0 .. 2 H]; A a scalar or a raster of degrees."""
    half, count = ray_count(half_width, step)
    wdirn = np.asarray(wdirn, dtype=np.float64)
    return [wdirn + float(m - half) * float(step) for m in range(count)]


def sector_sx(z, res, wdirn, half_width, step, dmax=500., ray_axes='row_east'):
    """(T-bar, Sx-bar in degrees).  Sx-bar = (sum_m atan(T_m) (180 / pi)) / M in ascending m, T-bar = tan(Sx-bar
    (pi / 180)); one ray (M = 1) keeps T_0 and atan(T_0) (180 / pi) without the round trip."""
    rays = [ref.tan_sx(z, res, a, dmax=dmax, ray_axes=ray_axes) for a in azimuths(wdirn, half_width, step)]
    if len(rays) == 1:
        return rays[0], np.arctan(rays[0]) * (180. / np.pi)
    acc = np.zeros(np.shape(z))
    for t_m in rays:
        acc = acc + np.arctan(t_m) * (180. / np.pi)
    sx = acc / float(len(rays))
    return np.tan(sx * (np.pi / 180.)), sx
