"""K13 in numpy (include/ssrs_hip.h "occupancy"): per track the set of in-raster cells it touched, then how many tracks
touched each cell -- and the named cases of tests/test_occupancy_emulation.py (the kernel's own code on the CPU) and
tests/test_gpu_occupancy.py (the device).  The cases are the smallest shapes at which the kernel can go wrong; every
comparison is integer equality."""
import numpy as np

SHAPE = (97, 131)
PLANES = (1, 3, 8)


def occupancy(tracks, shape):
    """(counts uint32 (rows, cols), cells_per_track uint32 (ntracks)) of a list of int (n_i, 2) [row, col] arrays."""
    rows, cols = shape
    counts = np.zeros(rows * cols, dtype=np.int64)
    per_track = np.zeros(len(tracks), dtype=np.uint32)
    for k, t in enumerate(tracks):
        t = np.asarray(t, dtype=np.int64).reshape(-1, 2)
        inside = (t[:, 0] >= 0) & (t[:, 0] < rows) & (t[:, 1] >= 0) & (t[:, 1] < cols)
        cells = np.unique(t[inside, 0] * cols + t[inside, 1])
        per_track[k] = cells.size
        counts += np.bincount(cells, minlength=rows * cols)
    return counts.astype(np.uint32).reshape(rows, cols), per_track


def visits(tracks, shape):
    """The plain histogram of all in-raster points (what compute_presence_counts gives)."""
    rows, cols = shape
    t = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1, 2) for t in tracks] + [np.zeros((0, 2), dtype=np.int64)])
    inside = (t[:, 0] >= 0) & (t[:, 0] < rows) & (t[:, 1] >= 0) & (t[:, 1] < cols)
    return np.bincount(t[inside, 0] * cols + t[inside, 1], minlength=rows * cols).reshape(rows, cols)


def walk(rng, shape, n):
    """A track of n points: unit steps (rests included) from a random cell, clipped to the raster, so that it revisits
    cells."""
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


def pingpong(a, b, n):
    t = np.empty((n, 2), dtype=np.int16)
    t[0::2], t[1::2] = a, b
    return t


def _cases():
    out = []

    def add(name, shape, tracks, lead=0, shift=0):
        # lead: points of another owner in front of the first track (traj_offsets is then a slice of a longer vector and
        # starts at `lead`); shift: the buffer starts this many points (4 bytes each) past a 16-byte boundary
        out.append(dict(name=name, shape=shape, tracks=[np.asarray(t, dtype=np.int16).reshape(-1, 2) for t in tracks],
                        lead=lead, shift=shift))

    # round borders: 32 * planes and 32 * planes + 1 tracks for planes 1, 3 and 8, and the small counts.  About six
    # points a track: ~200 a round of 32, far fewer bytes than a plane -> the unset path
    for n in (0, 1, 31, 32, 33, 96, 97, 256, 257):
        rng = np.random.default_rng(100 + n)
        add(f'borders_{n}', SHAPE, walks(200 + n, SHAPE, rng.integers(1, 12, n)))
    # empty tracks: at the start, at the end, on both sides of every round border (planes 1, 3, 8), several in a row
    # inside one lane's four points; tracks of 1, 2 and 3 points, which end inside a lane's load
    lengths = np.random.default_rng(7).integers(1, 10, 260)
    lengths[[0, 1, 31, 32, 63, 64, 95, 96, 255, 256, 258, 259]] = 0
    lengths[10:16] = (1, 0, 0, 0, 1, 1)
    lengths[20:29] = (1, 2, 3, 3, 2, 1, 1, 1, 2)
    add('empty_tracks', SHAPE, walks(8, SHAPE, lengths))
    add('all_empty', SHAPE, walks(9, SHAPE, np.zeros(40, dtype=int)))
    # the race: every lane of every wave wants the same two words
    pp = pingpong((40, 50), (40, 51), 5000)
    add('pingpong_alone', SHAPE, [pp])
    add('pingpong_41', SHAPE, [pp] * 41)                  # the copies sit on other bits and other planes
    # shared paths
    same = walks(11, SHAPE, [50])[0]
    add('identical_two', SHAPE, [same, same])
    through = walks(12, SHAPE, np.random.default_rng(12).integers(3, 9, 33))
    for t in through:
        t[len(t) // 2] = (48, 65)
    add('common_cell_33', SHAPE, through)
    # offsets that are a slice of a longer vector, first entry 1, 2 and 3 mod 4
    for lead in (1, 2, 7):
        add(f'lead_{lead}', SHAPE, walks(20 + lead, SHAPE, np.random.default_rng(20 + lead).integers(0, 9, 40)), lead=lead)
    # a traj pointer that is 4- but not 16-byte aligned (alone, and with a first offset that is not 0 either)
    add('misaligned', SHAPE, walks(30, SHAPE, np.random.default_rng(30).integers(0, 40, 70)), shift=1)
    add('misaligned_lead', SHAPE, walks(31, SHAPE, np.random.default_rng(31).integers(0, 40, 70)), lead=2, shift=3)
    # points outside the raster: negative, == rows, == cols; one track wholly outside
    rng = np.random.default_rng(40)
    outside = walks(41, SHAPE, rng.integers(4, 12, 36))
    for k, t in enumerate(outside):
        t[k % len(t)] = [(-1, 5), (5, -1), (SHAPE[0], 5), (5, SHAPE[1]), (-32768, 32767), (SHAPE[0], SHAPE[1])][k % 6]
    outside[7][:] = (-3, 4)
    add('outside', SHAPE, outside)
    # the memset path: an 8 x 8 raster with about 5000 points a round of 32 tracks
    add('memset_path', (8, 8), walks(50, (8, 8), np.full(40, 157)))
    # degenerate shapes (walks clipped to them, and points outside)
    for shape in ((1, 1), (1, 40), (40, 1)):
        ts = walks(60 + shape[1], shape, np.random.default_rng(60).integers(1, 30, 35))
        ts[3][0] = (shape[0], 0)
        ts[4][-1] = (0, shape[1])
        add(f'shape_{shape[0]}x{shape[1]}', shape, ts)
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
_expected = {}


def case(name):
    return CASES[CASE_IDS.index(name)]


def expected(name):
    """(counts, cells_per_track, visits) of a case, computed once and shared (read-only)."""
    if name not in _expected:
        c = case(name)
        res = occupancy(c['tracks'], c['shape']) + (visits(c['tracks'], c['shape']),)
        for a in res:
            a.setflags(write=False)
        _expected[name] = res
    return _expected[name]


def flat(c):
    """(traj int16 (lead + points, 2), offsets int64 (2 + ntracks)): offsets[1:] is what the call gets.  The `lead`
    points in front are in-raster, so a kernel that read them would count them."""
    lead = np.tile(np.array([[3, 3]], dtype=np.int16), (c['lead'], 1))
    traj = np.concatenate([lead] + c['tracks'] + [np.zeros((0, 2), dtype=np.int16)])
    lengths = np.array([c['lead']] + [len(t) for t in c['tracks']], dtype=np.int64)
    return np.ascontiguousarray(traj), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def clearing_paths(c, planes):
    """The clearing step of every round with points, by the header's rule: 'unset' when the round's points are fewer
    bytes than its planes."""
    rows, cols = c['shape']
    lengths = [len(t) for t in c['tracks']]
    out = []
    for t0 in range(0, len(lengths), 32 * planes):
        part = lengths[t0:t0 + 32 * planes]
        if sum(part):
            out.append('unset' if sum(part) * 4 < -(-len(part) // 32) * rows * cols * 4 else 'memset')
    return out


def check(name, counts, per_track, before=None):
    """counts / per_track (uint32 views) of one call on a case against the reference, plus the invariants.  before: what
    counts held on entry (it is added to)."""
    c = case(name)
    ref_counts, ref_per_track, hist = expected(name)
    counts = np.asarray(counts).view(np.uint32).reshape(c['shape'])
    per_track = np.asarray(per_track).view(np.uint32)
    if before is not None:
        counts = counts - np.asarray(before).view(np.uint32).reshape(c['shape'])
    assert np.array_equal(counts, ref_counts), name
    assert np.array_equal(per_track, ref_per_track), name
    assert int(counts.sum(dtype=np.int64)) == int(per_track.sum(dtype=np.int64))
    assert (counts <= hist).all() and np.array_equal(counts > 0, hist > 0)
    assert int(counts.max()) <= len(c['tracks'])
