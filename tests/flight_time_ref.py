"""K16 as its serial definition (include/ssrs_hip.h "flight time") in Python ints and numpy -- the only oracle of the flight
time -- and the named cases that tests/test_flight_time_emulation.py (the kernel's own code on the CPU) and
tests/test_gpu_flight_time.py (the device) share.  The cases are the smallest shapes at which the kernel can go wrong;
every comparison is integer equality."""
import math

import numpy as np

from altitude_ref import flat, walks

SHAPE = (37, 301)
TILE = 4096                     # SSRS_FLIGHT_TIME_TILE
CAP = 2 ** 31 - 1               # microseconds
CLIP = 2 ** 20                  # |wr|, |wc|, va in mm/s
SQRT2_16, HALF_SQRT2_16 = 92682, 46341
DEFAULT = (15_000, 1_000, 10_000)                # (va, gmin, res_mm): 15 m/s, 1 m/s, 10 m


def ray_step(wdirn, ray_axes):
    rad = np.asarray(wdirn, dtype=np.float64) * np.pi / 180.
    with np.errstate(invalid='ignore'):                   # (an infinite direction: NaN, still air)
        return (np.cos(rad), np.sin(rad)) if ray_axes == 'row_north' else (np.sin(rad), np.cos(rad))


def windinfo_unrounded(wspeed, wdirn, ray_axes='row_east'):
    """(-1000 wspeed) ur and (-1000 wspeed) uc in f64, before rint and the clip."""
    ws = np.asarray(wspeed).astype(np.float64)
    ur, uc = ray_step(np.asarray(wdirn).astype(np.float64), ray_axes)
    with np.errstate(invalid='ignore'):
        return (-1000. * ws) * ur, (-1000. * ws) * uc


def windinfo(wspeed, wdirn, ray_axes='row_east'):
    """(wr, wc) int32 rasters of ssrs_flight_windinfo."""
    out = []
    for v in windinfo_unrounded(wspeed, wdirn, ray_axes):
        with np.errstate(invalid='ignore'):
            v = np.clip(np.rint(v), -float(CLIP), float(CLIP))
        out.append(np.where(np.isnan(v), 0., v).astype(np.int64).astype(np.int32))
    return tuple(out)


def windinfo_inputs(dtype):
    """Random per-cell wind speed and direction of SHAPE for the windinfo tests, with NaN cells, winds that clip and
    directions on the axes."""
    rng = np.random.default_rng(7)
    ws = rng.uniform(0., 40., SHAPE)
    wd = rng.uniform(-360., 720., SHAPE)
    ws[0, :5] = (np.nan, 5., np.nan, 2000., np.inf)
    wd[0, :5] = (10., np.nan, np.nan, 45., 45.)
    wd[1, :5] = (0., 90., 180., 270., 360.)
    ws[-1, -1] = np.nan
    return np.ascontiguousarray(ws.astype(dtype)), np.ascontiguousarray(wd.astype(dtype))


def windinfo_exempt(wspeed, wdirn, ray_axes):
    """Cells where a component, before rounding, lies within 1e-6 of a half-integer: there a last-bit difference of the
    device's sin or cos from numpy's may round the other way (the results are then within 1 of each other)."""
    out = np.zeros(np.shape(wspeed), dtype=bool)
    for v in windinfo_unrounded(wspeed, wdirn, ray_axes):
        with np.errstate(invalid='ignore'):
            out |= np.abs(np.abs(v - np.floor(v)) - 0.5) <= 1e-6
    return out


def sign(x):
    return (x > 0) - (x < 0)


def move_dt(params, sr, sc, wr, wc):
    """dt in microseconds of a move of signs (sr, sc) out of a cell with wind (wr, wc); Python ints throughout."""
    va, gmin, res_mm = (int(v) for v in params)
    wr, wc = int(wr), int(wc)
    num_orth = res_mm * 10 ** 6
    num_diag = ((res_mm * SQRT2_16 + 32768) >> 16) * 10 ** 6
    if sr == 0 and sc == 0:
        return min((num_orth + va // 2) // va, CAP)
    if sr != 0 and sc != 0:
        a = ((sr * wr + sc * wc) * HALF_SQRT2_16 + 32768) >> 16
        b = sr * wc - sc * wr
        cross2, num = (b * b) >> 1, num_diag
    else:
        a, b = (sr * wr, wc) if sr != 0 else (sc * wc, wr)
        cross2, num = b * b, num_orth
    s = va * va - cross2
    g = gmin if s <= 0 else max(a + math.isqrt(s), gmin)
    return min((num + (g >> 1)) // g, CAP)


def flight_times(tracks, wr, wc, shape, params, masked=None):
    """The serial loop.  masked: int16 (points, 2) in the order of the concatenated tracks, or None.  Returns
    dict(time_hist, band_time_hist uint64 (rows, cols), times int64 (ntracks, 2), dt int32 (points))."""
    rows, cols = shape
    hist, band = np.zeros(shape, dtype=np.uint64), np.zeros(shape, dtype=np.uint64)
    times, dts, base = [], [], 0
    for track in tracks:
        pts = [(int(r), int(c)) for r, c in np.asarray(track).reshape(-1, 2)]
        total = zone = 0
        for k, (r0, c0) in enumerate(pts):
            dt = 0
            if k + 1 < len(pts):
                r1, c1 = pts[k + 1]
                if 0 <= r0 < rows and 0 <= c0 < cols and 0 <= r1 < rows and 0 <= c1 < cols:
                    dt = move_dt(params, sign(r1 - r0), sign(c1 - c0), wr[r0, c0], wc[r0, c0])
                    hist[r0, c0] += np.uint64(dt)
                    total += dt
                    if masked is not None and int(masked[base + k, 0]) >= 0:
                        band[r0, c0] += np.uint64(dt)
                        zone += dt
            dts.append(dt)
        base += len(pts)
        times.append((total, zone))
    return dict(time_hist=hist, band_time_hist=band, times=np.array(times, dtype=np.int64).reshape(-1, 2),
                dt=np.array(dts, dtype=np.int64).astype(np.int32))


def _wind_raster(seed):
    """A random wind through windinfo(): NaN cells, cross winds above va = 15 m/s (stall), headwinds that push the ground
    speed below gmin, and one cell whose wind no airspeed of a case holds against (the CAP at res_mm = 10^6)."""
    rng = np.random.default_rng(seed)
    ws = rng.uniform(0., 26., SHAPE)
    wd = rng.uniform(0., 360., SHAPE)
    ws[rng.random(SHAPE) < 0.05] = np.nan
    wd[rng.random(SHAPE) < 0.05] = np.nan
    ws[5, 5], wd[5, 5] = 1000., 90.            # 'row_east': 10^6 mm/s along -row, nothing along +col
    ws[6, 6], wd[6, 6] = 14.5, 180.            # +col is downwind at 14.5 m/s: flying -col leaves 0.5 m/s, below gmin
    return windinfo(ws, wd)


def masked_of(traj):
    """The points with every other one knocked out, as ssrs_track_altitude's traj_band would."""
    out = np.array(traj, dtype=np.int16, copy=True)
    out[1::2] = -1
    return out


def trap(cells, n):
    """n points going round `cells` again and again."""
    return np.array([cells[k % len(cells)] for k in range(n)], dtype=np.int16)


def _cases():
    out = []
    wr, wc = _wind_raster(1)

    def add(name, tracks, wr=wr, wc=wc, params=DEFAULT, lead=0, shift=0, uniform=None):
        # lead, shift: as in altitude_ref.  uniform: the (wr, wc) pair the call may get with a NULL raster instead
        out.append(dict(name=name, shape=SHAPE, tracks=[np.asarray(t, dtype=np.int16).reshape(-1, 2) for t in tracks],
                        wr=np.ascontiguousarray(wr, dtype=np.int32), wc=np.ascontiguousarray(wc, dtype=np.int32),
                        params=tuple(int(v) for v in params), lead=lead, shift=shift, uniform=uniform))

    T = TILE
    add('lengths', walks(10, SHAPE, [0, 1, 2, T - 1, T, T + 1, 3 * T + 5]))                 # one track longer than three tiles
    add('short_300', walks(11, SHAPE, np.random.default_rng(11).integers(1, 8, 300)))       # more tracks in a tile than slots
    add('empties', walks(12, SHAPE, [0, 0, 5, T - 5, 0, 0, 0, 7, 1, 0, T - 8, 0, 3, 0, 0]))
    add('all_empty', walks(13, SHAPE, [0] * 9))
    add('short_then_long', walks(14, SHAPE, [3] * 280 + [2 * T]))                           # a long track past the slots
    # the register cache: two cells for more than a tile, three cells, four (one more than it holds), and a walk between
    add('traps', [trap([(7, 7), (7, 8)], T + 700), trap([(6, 6), (6, 5), (5, 5)], 1500),
                  trap([(20, 100), (21, 101), (20, 102), (19, 101)], 900), walks(15, SHAPE, [600])[0],
                  trap([(30, 200), (30, 201)], 800)])
    add('stay_put', [trap([(9, 9)], 70), np.repeat(walks(16, SHAPE, [300])[0], 3, axis=0), trap([(5, 5)], 3)])
    # burn-in jumps of several cells: along a row, along a column, diagonal and skew ones
    add('jumps', [[(2, 2), (2, 9), (12, 9), (20, 17), (30, 19), (30, 20), (5, 5), (36, 300), (0, 0)], [(20, 3), (17, 0)],
                  [(6, 6), (6, 1)], [(5, 5), (9, 5), (5, 5), (5, 9), (5, 5), (1, 1)]])
    # points outside the raster: (-1, -1) in the middle of a track, as its first and last point, and a track wholly outside
    outside = walks(40, SHAPE, np.random.default_rng(40).integers(4, 12, 36))
    for k, t in enumerate(outside):
        t[k % len(t)] = [(-1, -1), (-1, 5), (5, -1), (SHAPE[0], 5), (5, SHAPE[1]), (-32768, 32767)][k % 6]
    outside[7][:] = (-1, -1)
    add('outside', outside)
    for lead, shift in ((1, 0), (2, 1), (7, 2), (0, 3), (4099, 1)):
        add(f'lead_{lead}_shift_{shift}', walks(20 + lead, SHAPE, [9, 0, T + 3, 40, 1, 0, 5]), lead=lead, shift=shift)
    # one wind everywhere: the NULL-raster path against a constant raster
    for k, pair in enumerate([(0, 0), (-7071, 7071), (16000, 300), (-CLIP, CLIP)]):
        add(f'uniform_{k}', walks(50 + k, SHAPE, [700, 30, 0, 900]), wr=np.full(SHAPE, pair[0]), wc=np.full(SHAPE, pair[1]),
            uniform=pair)
    # the scalars' corners: the CAP at res_mm = 10^6 (cell (5, 5) stalls every move but the one along its wind); gmin == va;
    # the fastest bird in the finest raster (dt rounds to 0 and 1); an odd cell size
    add('cap', [[(5, 5), (5, 6), (5, 5), (4, 5), (5, 5), (6, 5), (5, 5), (6, 6), (5, 5), (5, 5)]] + walks(60, SHAPE, [400]),
        params=(15_000, 1, 10 ** 6))
    add('gmin_is_va', walks(61, SHAPE, [500]), params=(15_000, 15_000, 10_000))
    add('fast_fine', walks(62, SHAPE, [500]), params=(CLIP, 1, 1))
    add('odd_scalars', walks(63, SHAPE, [900, 17]), params=(12_345, 77, 33_333))
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
KEYS = ('time_hist', 'band_time_hist', 'times', 'dt')
_expected = {}


def case(name):
    return CASES[CASE_IDS.index(name)]


def points(c):
    """(traj with the lead points, offsets with the lead's, masked with the lead points kept) of a case."""
    traj, offsets = flat(c)
    masked = traj.copy()
    masked[c['lead']:] = masked_of(traj[c['lead']:])
    return traj, offsets, masked


def expected(name):
    """The oracle's outputs of a case with its masked copy, computed once and shared (read-only)."""
    if name not in _expected:
        c = case(name)
        traj, _, masked = points(c)
        res = flight_times(c['tracks'], c['wr'], c['wc'], c['shape'], c['params'], masked[c['lead']:])
        for a in res.values():
            a.setflags(write=False)
        _expected[name] = res
    return _expected[name]


def packed(c):
    """The {wr, wc} raster the library reads: int32 (rows, cols, 2)."""
    return np.ascontiguousarray(np.stack([c['wr'], c['wc']], -1), dtype=np.int32)


def check(name, got, before=None, times=1):
    """`got`: dict of the outputs of one call on a case (any subset of KEYS; dt WITHOUT the lead points).  before: what
    the rasters held on entry (they are added to), a dict by key; times: how often the case was added."""
    want = expected(name)
    for key, value in got.items():
        value = np.asarray(value)
        if key in ('time_hist', 'band_time_hist'):
            value = value.view(np.uint64).reshape(SHAPE)
            if before is not None:
                value = value - np.asarray(before[key]).view(np.uint64).reshape(SHAPE)
            ref = want[key] * np.uint64(times)
        else:
            ref = want[key]
        assert value.shape == ref.shape, (name, key, value.shape, ref.shape)
        assert value.dtype.itemsize == ref.dtype.itemsize, (name, key, value.dtype)
        assert np.array_equal(value, ref), (name, key, np.flatnonzero((value != ref).reshape(-1))[:8])
    # the checksums Simulator raises on
    if times == 1:
        assert int(want['time_hist'].sum(dtype=np.uint64)) == int(want['times'][:, 0].sum()) % 2 ** 64
        assert int(want['band_time_hist'].sum(dtype=np.uint64)) == int(want['times'][:, 1].sum()) % 2 ** 64
