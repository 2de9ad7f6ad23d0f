"""K14 as its serial definition (include/ssrs_hip.h "altitude") in plain numpy and Python ints -- the only oracle of the
flight-height scan -- and the named cases that tests/test_altitude_emulation.py (the kernel's own code on the CPU) and
tests/test_gpu_altitude.py (the device) share.  The cases are the smallest shapes at which the scan can go wrong; every
comparison is integer equality."""
import numpy as np

SHAPE = (24, 20)
TILE = 4096                     # SSRS_ALTITUDE_TILE
SENTINEL = -2 ** 31             # the elev of a nodata cell
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SQRT2_16 = 92682                # round(sqrt(2) * 2^16)
# (start, floor, ceil, band_lo, band_hi) in mm: the Config defaults
DEFAULT = (100_000, 10_000, 1_000_000, 30_000, 150_000)


def cellinfo(updraft, dem, resolution, airspeed, sink):
    """(climb, elev) int32 rasters of ssrs_altitude_cellinfo."""
    scale = 1000. * float(resolution) / float(airspeed)
    w = np.asarray(updraft).astype(np.float64)
    w = np.where(np.isnan(w), 0., w)
    climb = np.clip(np.rint((w - float(sink)) * scale), -2. ** 26, 2. ** 26).astype(np.int32)
    z = np.asarray(dem).astype(np.float64)
    with np.errstate(invalid='ignore'):
        elev = np.clip(np.rint(1000. * z), -2. ** 30, 2. ** 30)
    elev = np.where(np.isnan(z), float(SENTINEL), elev).astype(np.int64).astype(np.int32)
    return climb, elev


def diagonal_step(climb):
    """The millimetres of a diagonal move out of a cell of `climb` (a Python int; >> is arithmetic)."""
    return (int(climb) * SQRT2_16 + 32768) >> 16


def moves(track, climb, elev, shape):
    """a_k of the moves k -> k + 1 of one track, as a list of Python ints."""
    rows, cols = shape
    out = []
    pts = [(int(r), int(c)) for r, c in np.asarray(track).reshape(-1, 2)]
    for (r0, c0), (r1, c1) in zip(pts[:-1], pts[1:]):
        if not (0 <= r0 < rows and 0 <= c0 < cols and 0 <= r1 < rows and 0 <= c1 < cols):
            out.append(0)
            continue
        step = diagonal_step(climb[r0, c0]) if r1 != r0 and c1 != c0 else int(climb[r0, c0])
        e0, e1 = int(elev[r0, c0]), int(elev[r1, c1])
        out.append(step - (0 if e0 == SENTINEL or e1 == SENTINEL else e1 - e0))
    return out


def altitude(tracks, climb, elev, shape, params):
    """The serial loop.  Returns dict(alt int32 (points), traj_band int16 (points, 2), band_hist uint32 (rows, cols),
    in_band / h_min / h_max int32 (ntracks))."""
    rows, cols = shape
    start, floor, ceil, band_lo, band_hi = (int(v) for v in params)
    clamp = lambda x: min(max(x, floor), ceil)
    alt, masked = [], []
    hist = np.zeros(shape, dtype=np.int64)
    in_band, h_min, h_max = [], [], []
    for track in tracks:
        track = np.asarray(track).reshape(-1, 2)
        cnt, lo, hi = 0, I32_MAX, I32_MIN
        h = clamp(start)
        for k, a in enumerate([None] + moves(track, climb, elev, shape) if len(track) else []):
            if a is not None:
                h = clamp(h + a)
            r, c = int(track[k, 0]), int(track[k, 1])
            zone = 0 <= r < rows and 0 <= c < cols and band_lo <= h <= band_hi
            alt.append(h)
            masked.append((r, c) if zone else (-1, -1))
            lo, hi = min(lo, h), max(hi, h)
            if zone:
                cnt += 1
                hist[r, c] += 1
        in_band.append(cnt), h_min.append(lo), h_max.append(hi)
    return dict(alt=np.array(alt, dtype=np.int64).astype(np.int32),
                traj_band=np.array(masked, dtype=np.int16).reshape(-1, 2), band_hist=hist.astype(np.uint32),
                in_band=np.array(in_band, dtype=np.int64).astype(np.int32),
                h_min=np.array(h_min, dtype=np.int64).astype(np.int32), h_max=np.array(h_max, dtype=np.int64).astype(np.int32))


def walk(rng, shape, n):
    """A track of n points: king's moves (rests included) from a random cell, clipped to the raster."""
    rows, cols = shape
    if n == 0:
        return np.zeros((0, 2), dtype=np.int16)
    steps = rng.integers(-1, 2, size=(n, 2))
    steps[0] = (rng.integers(0, rows), rng.integers(0, cols))
    pts = np.cumsum(steps, 0)
    return np.stack([pts[:, 0].clip(0, rows - 1), pts[:, 1].clip(0, cols - 1)], 1).astype(np.int16)


def walks(seed, shape, lengths):
    rng = np.random.default_rng(seed)
    return [walk(rng, shape, int(n)) for n in lengths]


def zigzag(rows, n, c0=0, c1=SHAPE[1] - 1):
    """n points of orthogonal moves only: east and west along the rows `rows`, one step down the list at every turn."""
    pts, k, c, d = [], 0, c0, 1
    while len(pts) < n:
        pts.append((rows[k % len(rows)], c))
        if (c == c1 and d == 1) or (c == c0 and d == -1):
            k, d = k + 1, -d
        else:
            c += d
    return np.array(pts, dtype=np.int16)


def _rasters(seed):
    rng = np.random.default_rng(seed)
    climb = (rng.integers(-1500, 1500, SHAPE) * 2 + 1).astype(np.int32)            # odd millimetres, both signs
    elev = rng.integers(0, 400_000, SHAPE).astype(np.int32)
    return climb, elev


def _cases():
    out = []
    climb, elev = _rasters(1)

    def add(name, tracks, climb=climb, elev=elev, params=DEFAULT, lead=0, shift=0):
        # lead: points of another owner in front of the first track (the offsets are then a slice of a longer vector and
        # start at `lead`); shift: the buffers start this many points (4 bytes each) past a 16-byte boundary
        out.append(dict(name=name, shape=SHAPE, tracks=[np.asarray(t, dtype=np.int16).reshape(-1, 2) for t in tracks],
                        climb=np.ascontiguousarray(climb, dtype=np.int32), elev=np.ascontiguousarray(elev, dtype=np.int32),
                        params=tuple(int(v) for v in params), lead=lead, shift=shift))

    T = TILE
    # track borders against tile borders and lane runs
    add('lengths', walks(10, SHAPE, [0, 1, 2, T - 1, T, T + 1, 3 * T + 5]))
    add('short_300', walks(11, SHAPE, np.random.default_rng(11).integers(1, 8, 300)))      # more tracks in a tile than slots
    add('empties', walks(12, SHAPE, [0, 0, 5, T - 5, 0, 0, 0, 7, 1, 0, T - 8, 0, 3, 0, 0]))  # start, end, at the tile borders
    add('all_empty', walks(13, SHAPE, [0] * 9))
    # many tracks, nearly all of them empty: the searches over 20 001 offsets and long runs of empty tracks inside a lane's run
    sparse = np.zeros(20_000, dtype=int)
    sparse[::97] = np.random.default_rng(15).integers(1, 6, sparse[::97].size)
    sparse[[0, -1]] = 0
    add('sparse_20000', walks(15, SHAPE, sparse))
    add('short_then_long', walks(14, SHAPE, [3] * 280 + [2 * T]))                          # a long track past the slots
    for lead, shift in ((1, 0), (2, 1), (7, 2), (0, 3), (4099, 1)):
        add(f'lead_{lead}_shift_{shift}', walks(20 + lead, SHAPE, [9, 0, T + 3, 40, 1, 0, 5]), lead=lead, shift=shift)
    # pinned to the ceiling, then to the floor, over more than a tile
    high, low = np.full(SHAPE, 40_001, dtype=np.int32), np.full(SHAPE, -40_001, dtype=np.int32)
    flat_elev = np.zeros(SHAPE, dtype=np.int32)
    add('pinned_ceiling', walks(30, SHAPE, [T + 100, 50]), climb=high, elev=flat_elev)
    add('pinned_floor', walks(31, SHAPE, [T + 100, 50]), climb=low, elev=flat_elev)
    split = np.where(np.arange(SHAPE[0])[:, None] < 12, high, low) + np.zeros(SHAPE, dtype=np.int32)
    add('ceiling_then_floor', [np.concatenate([zigzag(list(range(0, 12)), 2500), zigzag(list(range(12, 24)), 2500)])],
        climb=split, elev=flat_elev)
    # sums past int32 with the clamps out of reach: 60 orthogonal moves of 2^26 mm up from INT32_MIN, and down again
    big = np.where(np.arange(SHAPE[0])[:, None] < 12, 2 ** 26, -2 ** 26) + np.zeros(SHAPE, dtype=np.int32)
    updown = np.concatenate([zigzag([0, 1, 2, 3], 60), zigzag([12, 13, 14, 15], 61)])
    add('beyond_int32', [updown, updown[:40], updown], climb=big, elev=flat_elev,
        params=(I32_MIN, I32_MIN, I32_MAX, -1_000_000_000, 1_000_000_000))
    # terrain steps of 2^31 between the clips of elev, on the widest clamps
    steep = np.where((np.arange(SHAPE[0])[:, None] + np.arange(SHAPE[1])[None, :]) % 2 == 0, 2 ** 30, -2 ** 30).astype(np.int32)
    add('steep', walks(32, SHAPE, [200, 300]), elev=steep, params=(0, I32_MIN, I32_MAX, -5, 5))
    # diagonal against orthogonal moves on odd and negative climbs: the same cells left both ways
    pairs = []
    for r in range(1, 22, 3):
        for c in range(1, 18, 3):
            pairs += [[(r, c), (r, c + 1)], [(r, c), (r + 1, c + 1)], [(r, c), (r - 1, c)], [(r, c), (r - 1, c - 1)]]
    add('diagonals', pairs, elev=flat_elev, params=(100_000, 0, 1_000_000, 99_000, 101_000))
    # burn-in jumps of 3 cells: along a row, along a column, and two diagonal ones
    add('jumps', [[(2, 2), (2, 5), (5, 5), (8, 8), (11, 9), (11, 10)], [(20, 3), (17, 0)]])
    # points outside the raster: in the middle of a track, as its first point, and a track wholly outside
    outside = walks(40, SHAPE, np.random.default_rng(40).integers(4, 12, 36))
    for k, t in enumerate(outside):
        t[k % len(t)] = [(-1, 5), (5, -1), (SHAPE[0], 5), (5, SHAPE[1]), (-32768, 32767), (SHAPE[0], SHAPE[1])][k % 6]
    outside[7][:] = (-3, 4)
    outside[9][0] = (0, SHAPE[1])
    add('outside', outside)
    # nodata elevations on either end of a move
    holes = elev.copy()
    holes[np.random.default_rng(41).random(SHAPE) < 0.3] = SENTINEL
    add('nodata', walks(42, SHAPE, [300, 0, 200, 5000]), elev=holes)
    # bands: everything, nothing (below the floor), and one millimetre on a height that occurs
    tracks = walks(50, SHAPE, [700, 30, 0, 900])
    add('band_all', tracks, params=DEFAULT[:3] + (I32_MIN, I32_MAX))
    add('band_none', tracks, params=DEFAULT[:3] + (DEFAULT[1] - 9, DEFAULT[1] - 1))
    seen = altitude(tracks, climb, elev, SHAPE, DEFAULT)['alt']
    values, counts = np.unique(seen[(seen > DEFAULT[1]) & (seen < DEFAULT[2])], return_counts=True)
    add('band_1mm', tracks, params=DEFAULT[:3] + (int(values[counts.argmax()]),) * 2)
    # a start outside [floor, ceil] is clamped; floor == ceil
    add('start_clamped', tracks, params=(5, 10_000, 1_000_000, 10_000, 10_000))
    add('floor_is_ceil', tracks, params=(0, 77_000, 77_000, 77_000, 77_000))
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
_expected = {}


def case(name):
    return CASES[CASE_IDS.index(name)]


def expected(name):
    """The oracle's outputs of a case, computed once and shared (read-only)."""
    if name not in _expected:
        c = case(name)
        res = altitude(c['tracks'], c['climb'], c['elev'], c['shape'], c['params'])
        for a in res.values():
            a.setflags(write=False)
        _expected[name] = res
    return _expected[name]


def packed(c):
    """The {climb, elev} raster the library reads: int32 (rows, cols, 2)."""
    return np.ascontiguousarray(np.stack([c['climb'], c['elev']], -1), dtype=np.int32)


def flat(c):
    """(traj int16 (lead + points, 2), offsets int64 (2 + ntracks)): offsets[1:] is what the call gets.  The `lead`
    points in front are in-raster, so a kernel that read them would count them."""
    lead = np.tile(np.array([[3, 3]], dtype=np.int16), (c['lead'], 1))
    traj = np.concatenate([lead] + c['tracks'] + [np.zeros((0, 2), dtype=np.int16)])
    lengths = np.array([c['lead']] + [len(t) for t in c['tracks']], dtype=np.int64)
    return np.ascontiguousarray(traj), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def check(name, got, before=None):
    """`got`: dict of the outputs of one call on a case (any subset; the per-point ones WITHOUT the lead points).
    before: what band_hist held on entry (it is added to)."""
    want = expected(name)
    for key, value in got.items():
        value = np.asarray(value)
        if key == 'band_hist':
            value = value.view(np.uint32).reshape(SHAPE)
            if before is not None:
                value = value - np.asarray(before).view(np.uint32).reshape(SHAPE)
        assert value.shape == want[key].shape, (name, key, value.shape, want[key].shape)
        assert np.array_equal(value, want[key]), (name, key, np.flatnonzero((value != want[key]).reshape(-1))[:8])
    if 'band_hist' in got and 'in_band' in got:
        assert int(want['band_hist'].sum(dtype=np.int64)) == int(np.asarray(got['in_band']).sum(dtype=np.int64))
