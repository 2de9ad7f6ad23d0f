"""K15 as its definition (include/ssrs_hip.h, ssrs_rotor_encounters) in plain numpy: a brute force over ALL (point, turbine)
pairs -- the only oracle of the rotor encounters -- and the named cases that tests/test_rotor_host.py (the cull lists) and
tests/test_gpu_rotor_encounters.py (the device) share.  Every comparison is integer equality."""
import numpy as np

ROWS, COLS = 70, 90                         # 3 x 3 bins of 32 x 32 cells, neither side a multiple of 32
SHAPE = (ROWS, COLS)
LENGTHS = [1, 1, 0, 2, 63, 64, 65, 255, 256, 257, 1000, 4097] + [3] * 300
NTURB = 70                                  # three bitmap words
SENTINEL = -2 ** 31                         # the elev of a nodata cell
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
WIDE = (I32_MIN, I32_MAX)


def inside_matrix(traj, alt, elev, xy, reach, zband, shape):
    """bool (points, nturb): point k inside turbine t, by the four conditions of the header, every pair on its own."""
    rows, cols = shape
    traj = np.asarray(traj).reshape(-1, 2)
    r, c = traj[:, 0].astype(np.int64), traj[:, 1].astype(np.int64)
    in_raster = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
    e = np.where(in_raster, np.asarray(elev)[np.where(in_raster, r, 0), np.where(in_raster, c, 0)], SENTINEL).astype(np.int64)
    valid = in_raster & (e != SENTINEL)
    xy, reach, zband = np.asarray(xy, dtype=np.float64), np.asarray(reach, dtype=np.float64), np.asarray(zband)
    with np.errstate(invalid='ignore'):
        d2 = (c[:, None] - xy[None, :, 0]) ** 2 + (r[:, None] - xy[None, :, 1]) ** 2
        flat = (d2 <= (reach * reach)[None, :]) & (reach >= 0.)[None, :]
    z = e + np.asarray(alt).astype(np.int64)
    tall = (zband[None, :, 0].astype(np.int64) <= z[:, None]) & (z[:, None] <= zband[None, :, 1].astype(np.int64))
    return valid[:, None] & flat & tall


def brute_force(traj, alt, off, elev, xy, reach, zband, shape):
    """dict(bitmap uint32 (ntracks, words), tracks_per_turbine int64, turbines_per_track int32, first_step int32, points int64
    (nturb)) of the points [off[0], off[-1]); `off` indexes traj and alt."""
    inside = inside_matrix(traj, alt, elev, xy, reach, zband, shape)
    n, nturb = len(off) - 1, inside.shape[1]
    words = (nturb + 31) // 32
    enc = np.zeros((n, words * 32), dtype=bool)
    first = np.full(n, -1, dtype=np.int32)
    for k in range(n):
        seg = inside[off[k]:off[k + 1]]
        enc[k, :nturb] = seg.any(0)
        where = np.nonzero(seg.any(1))[0]
        if where.size:
            first[k] = where[0]
    weights = 1 << np.arange(32, dtype=np.uint64)
    bitmap = (enc.reshape(n, words, 32) * weights).sum(2).astype(np.uint32)
    return dict(bitmap=bitmap, tracks_per_turbine=enc[:, :nturb].sum(0).astype(np.int64),
                turbines_per_track=enc[:, :nturb].sum(1).astype(np.int32), first_step=first,
                points=inside[off[0]:off[-1]].sum(0).astype(np.int64))


def walk(rng, n, shape=SHAPE, start=None):
    """A random walk of n cells (king's moves and rests), reflected at the raster's edges: int16 (n, 2) [row, col]."""
    rows, cols = shape
    pos = np.array([rng.integers(0, rows), rng.integers(0, cols)]) if start is None else np.array(start)
    steps = rng.integers(-1, 2, (n, 2))
    steps[:1] = 0
    out = pos + np.cumsum(steps, 0)
    for ax, hi in ((0, rows - 1), (1, cols - 1)):
        v = np.abs(out[:, ax]) % (2 * hi)
        out[:, ax] = np.where(v > hi, 2 * hi - v, v)
    return out.astype(np.int16)


def random_turbines(rng, shape, n, z_lo, z_hi):
    """n cylinders all over (and a little beyond) a raster: positions partly on cell centres, edges and corners, a reach of
    0.5 .. 6 cells, bands of 20 .. 200 m that start in [z_lo, z_hi) mm."""
    rows, cols = shape
    xy = np.stack([rng.uniform(-3., cols + 2., n), rng.uniform(-3., rows + 2., n)], 1)
    xy[:n // 2] = np.round(xy[:n // 2] * 2.) / 2.
    reach = rng.uniform(0.5, 6., n)
    lo = rng.integers(z_lo, z_hi, n)
    zband = np.stack([lo, lo + rng.integers(20_000, 200_000, n)], 1).astype(np.int32)
    return xy, reach, zband


def _base():
    rng = np.random.default_rng(15)
    tracks = [walk(rng, n) for n in LENGTHS]
    elev = rng.integers(0, 400_000, SHAPE).astype(np.int32)
    elev[rng.random(SHAPE) < 0.05] = SENTINEL                       # nodata cells under the tracks
    alts = [rng.integers(10_000, 300_000, len(t)).astype(np.int32) for t in tracks]
    xy, reach, zband = random_turbines(rng, SHAPE, NTURB, 0, 600_000)

    def put(t, at, point, alt):
        tracks[t][at], alts[t][at] = point, alt

    # 0, 1: the centre of cell (row 20, col 30), every height: offsets (3, 4) and (4, -3) are exactly on the circle of reach 5,
    # the axis neighbours exactly on that of reach 1
    xy[0], reach[0], zband[0] = (30., 20.), 5., WIDE
    xy[1], reach[1], zband[1] = (30., 20.), 1., WIDE
    for k, p in enumerate([(20, 31), (20, 29), (21, 30), (19, 30), (23, 34), (24, 27), (21, 31), (26, 30), (20, 36)]):
        elev[p] = 1000 * k
        put(10, 100 + k, p, 50_000)
    # 2, 3: one position, disjoint bands that touch: 200 000 mm belongs to the lower, 200 001 to the upper
    xy[2], reach[2], zband[2] = (60., 10.), 3., (0, 200_000)
    xy[3], reach[3], zband[3] = (60., 10.), 3., (200_001, 500_000)
    elev[10, 60], elev[11, 61] = 150_000, 150_000
    for k, a in enumerate([49_999, 50_000, 50_001, 350_000, 350_001, -150_000, -150_001]):
        put(10, 200 + k, (10 + (k & 1), 60 + (k & 1)), a)
    # 4: reach 0 on a cell centre: that cell alone
    xy[4], reach[4], zband[4] = (45., 50.), 0., WIDE
    elev[50, 45] = 7
    put(10, 300, (50, 45), 0)
    put(10, 301, (50, 46), 0)
    # 5 .. 8 are hit by nothing: an empty band, a NaN reach, a NaN coordinate, a negative reach -- all of them on turbine 0
    for t, (x, rch, band) in zip((5, 6, 7, 8), ((30., 5., (1, 0)), (30., np.nan, WIDE), (np.nan, 5., WIDE), (30., -1., WIDE))):
        xy[t], reach[t], zband[t] = (x, 20.), rch, band
    # 9: outside the raster, reaching in
    xy[9], reach[9], zband[9] = (-2., 30.), 4., WIDE
    elev[30, 0:3] = 100
    put(10, 400, (30, 0), 1)
    put(10, 401, (30, 2), 1)                                           # distance exactly 4
    put(10, 402, (30, 3), 1)
    # 10: the ends of the band, and one millimetre beyond each
    xy[10], reach[10], zband[10] = (70., 40.), 2., (500_000, 600_000)
    elev[40, 70] = 300_000
    for k, a in enumerate([199_999, 200_000, 300_000, 300_001]):
        put(10, 500 + k, (40, 70), a)
    # 11, 12: sums past int32.  2^30 + INT32_MAX wraps to a negative int32 inside band 11, -2^30 + INT32_MIN to a positive one
    # inside band 12: neither is a hit; 2^30 + INT32_MIN = -2^30 (band 11) and -2^30 + INT32_MAX (band 12) are
    xy[11], reach[11], zband[11] = (80.5, 60.), 1., (I32_MIN, 0)
    xy[12], reach[12], zband[12] = (80.5, 60.), 1., (0, I32_MAX)
    elev[60, 80], elev[60, 81] = 2 ** 30, -2 ** 30
    for k, (p, a) in enumerate([((60, 80), I32_MAX), ((60, 81), I32_MIN), ((60, 80), I32_MIN), ((60, 81), I32_MAX)]):
        put(10, 600 + 2 * k, p, a)
    # bits 31 / 32 and 63 / 64: cylinders of every height where the long tracks wander
    for t, (x, y) in zip((31, 32, 63, 64), ((20., 15.), (45.5, 35.), (66., 52.5), (33., 60.))):
        xy[t], reach[t], zband[t] = (x, y), 6., WIDE
    # points outside the raster inside tracks, and nodata under a point that is inside turbine 0 in the plane
    for at in (150, 151, 700):
        put(10, at, (-1, -1), 50_000)
    elev[22, 30] = SENTINEL
    put(10, 110, (22, 30), 50_000)
    # short tracks that begin inside turbine 0 (a first step of 0, several tracks per span)
    for k in range(4):
        tracks[40 + 5 * k] = walk(rng, 3, start=(20, 30))
    return tracks, alts, elev, xy, reach, zband


def _cases():
    tracks, alts, elev, xy, reach, zband = _base()
    out = []

    def add(name, tracks=tracks, alts=alts, lead=0, shift=0):
        # lead: points of another owner in front of the first track (inside turbine 0: a kernel that read them would count
        # them); shift: the buffers start this many points (4 bytes each) past a 16-byte boundary
        out.append(dict(name=name, shape=SHAPE, tracks=tracks, alts=alts, elev=elev, xy=xy, reach=reach, zband=zband,
                        lead=lead, shift=shift))

    add('planted')
    for lead, shift in ((5, 1), (2, 2), (7, 3), (256, 0)):
        add(f'lead_{lead}_shift_{shift}', lead=lead, shift=shift)
    # the 4097-point track loiters between two cells inside turbines 0 and 1 (and turbine 5 .. 8's, which nothing hits), the
    # short ones around it stay: thousands of points for one counter
    loiter, heights = [t.copy() for t in tracks], [a.copy() for a in alts]
    loiter[11][0::2], loiter[11][1::2] = (20, 30), (20, 31)
    heights[11][:] = 80_000
    add('loiter', loiter, heights)
    add('loiter_shift_3', loiter, heights, lead=1, shift=3)
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
_expected = {}


def case(name):
    return CASES[CASE_IDS.index(name)]


def flat(c):
    """(traj int16 (lead + points, 2), alt int32 (lead + points), offsets int64 (2 + ntracks)): offsets[1:] is what the call
    gets.  The lead points lie on turbine 0 at a height every wide band holds."""
    lead = np.tile(np.array([[20, 30]], dtype=np.int16), (c['lead'], 1))
    traj = np.ascontiguousarray(np.concatenate([lead] + list(c['tracks'])))
    alt = np.concatenate([np.full(c['lead'], 50_000, dtype=np.int32)] + list(c['alts'])).astype(np.int32)
    lengths = np.array([c['lead']] + [len(t) for t in c['tracks']], dtype=np.int64)
    return traj, alt, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def packed(elev):
    """The {climb, elev} raster the library reads: int32 (rows, cols, 2); the climbs are not K15's to read."""
    elev = np.asarray(elev, dtype=np.int32)
    return np.ascontiguousarray(np.stack([np.full_like(elev, 123_456_789), elev], -1))


def expected(name):
    """The brute force of a case, computed once and shared (read-only)."""
    if name not in _expected:
        c = case(name)
        traj, alt, off = flat(c)
        res = brute_force(traj, alt, off[1:], c['elev'], c['xy'], c['reach'], c['zband'], c['shape'])
        for a in res.values():
            a.setflags(write=False)
        _expected[name] = res
    return _expected[name]
