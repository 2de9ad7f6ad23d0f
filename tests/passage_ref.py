"""K17 in numpy (include/ssrs_hip_passage.h): per track the boolean raster of its in-raster cells, ORed over shifted copies
for every offset of the explicit list D = {(dr, dc) : dr*dr + dc*dc <= r2}, then summed over the tracks -- and the named
cases of tests/test_passage_emulation.py (the kernel's own code on the CPU) and tests/test_gpu_passage.py (the device).
There is no crescent logic here: this is what checks the crescents.  Every comparison is integer equality."""
import numpy as np

RASTERS = ((1, 1), (1, 9), (9, 1), (5, 3), (37, 53), (70, 130))
R2S = (0, 1, 2, 4, 5, 8, 9, 25, 26)             # 26: the first disk whose diagonal reach exceeds that of 25
PLANES = (1, 3, 8)
MOVES = tuple((mr, mc) for mr in (-1, 0, 1) for mc in (-1, 0, 1) if (mr, mc) != (0, 0))


def disk(r2):
    """The offsets (dr, dc) with dr*dr + dc*dc <= r2, by trying every pair of a square that holds them all."""
    reach = int(np.sqrt(r2)) + 1
    return [(dr, dc) for dr in range(-reach, reach + 1) for dc in range(-reach, reach + 1) if dr * dr + dc * dc <= r2]


def crescent_sizes(r2):
    """|D \\ (D - m)| for each of the eight unit moves m, by set difference on the offset list."""
    d = set(disk(r2))
    return [len(d - {(dr - mr, dc - mc) for dr, dc in d}) for mr, mc in MOVES]


def dilate(hit, r2):
    """The boolean raster `hit` ORed over its copies shifted by every offset of D, clipped to the raster."""
    rows, cols = hit.shape
    out = np.zeros_like(hit)
    for dr, dc in disk(r2):
        if abs(dr) >= rows or abs(dc) >= cols:
            continue
        out[max(dr, 0):rows + min(dr, 0), max(dc, 0):cols + min(dc, 0)] |= \
            hit[max(-dr, 0):rows + min(-dr, 0), max(-dc, 0):cols + min(-dc, 0)]
    return out


def passage(tracks, shape, r2):
    """(counts uint32 (rows, cols), cells_per_track uint32 (ntracks)) of a list of int (n_i, 2) [row, col] arrays."""
    rows, cols = shape
    counts = np.zeros(shape, dtype=np.int64)
    per_track = np.zeros(len(tracks), dtype=np.uint32)
    for k, t in enumerate(tracks):
        t = np.asarray(t, dtype=np.int64).reshape(-1, 2)
        inside = (t[:, 0] >= 0) & (t[:, 0] < rows) & (t[:, 1] >= 0) & (t[:, 1] < cols)
        cells = np.unique(t[inside, 0] * cols + t[inside, 1])
        hit = np.zeros(rows * cols, dtype=bool)
        hit[cells] = True
        near = dilate(hit.reshape(shape), r2)
        per_track[k] = near.sum()
        counts += near
    return counts.astype(np.uint32), per_track


def brute(tracks, shape, r2):
    """The definition itself: every cell measured against every point (the smallest cases only)."""
    rows, cols = shape
    counts = np.zeros(shape, dtype=np.uint32)
    per_track = np.zeros(len(tracks), dtype=np.uint32)
    for k, t in enumerate(tracks):
        for r in range(rows):
            for c in range(cols):
                if any(0 <= pr < rows and 0 <= pc < cols and (r - pr) ** 2 + (c - pc) ** 2 <= r2
                       for pr, pc in np.asarray(t, dtype=np.int64).reshape(-1, 2).tolist()):
                    counts[r, c] += 1
                    per_track[k] += 1
    return counts, per_track


def walk(rng, shape, n):
    """A track of n points: unit steps (rests included) from a random cell, clipped to the raster."""
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


def basic_tracks(shape):
    """The small shapes of the table of cases, fitted to a raster: empty, one point, a rest, a ping-pong, one unit move in
    each of the 8 directions from a cell whose disk a corner clips (on the thin rasters some of them leave the raster, and
    come back), a jump of 3 cells, an out-of-raster point in the middle, and a track along each edge."""
    rows, cols = shape
    top, right = rows - 1, cols - 1
    inner = (min(1, top), min(1, right))                 # next to the corner (0, 0): every disk here is clipped
    far = (max(top - 1, 0), max(right - 1, 0))
    out = [np.zeros((0, 2)), [inner], [inner, inner, inner], pingpong(inner, (inner[0], min(inner[1] + 1, right)), 7),
           pingpong(far, (max(far[0] - 1, 0), far[1]), 6)]
    for corner in (inner, far):
        for mr, mc in MOVES:
            out.append([corner, (corner[0] + mr, corner[1] + mc)])
            out.append([corner, (corner[0] + mr, corner[1] + mc), corner])      # there and back
    out.append([(0, 0), (min(3, top), 0), (min(3, top), min(3, right)), (0, 0)])               # jumps of 3 cells
    out.append([inner, (-1, inner[1]), inner, (inner[0], cols), (inner[0], min(inner[1] + 1, right))])
    out.append([far, (rows, cols), far, far, (-32768, 32767)])
    out.append([(0, c) for c in range(cols)])
    out.append([(top, c) for c in range(right, -1, -1)])
    out.append([(r, 0) for r in range(top, -1, -1)])
    out.append([(r, right) for r in range(rows)])
    return out


def _cases():
    out = []

    def add(name, shape, r2, tracks, lead=0):
        # lead: points of another owner in front of the first track (traj_offsets is then a slice of a longer vector and
        # starts at `lead`)
        out.append(dict(name=name, shape=shape, r2=int(r2), lead=lead,
                        tracks=[np.asarray(t, dtype=np.int16).reshape(-1, 2) for t in tracks]))

    # every raster at every radius, and on the small ones a disk that covers the raster from any cell
    for shape in RASTERS:
        small = shape[0] * shape[1] <= 15
        for r2 in R2S + ((shape[0] ** 2 + shape[1] ** 2 + 1,) if small else ()):
            add(f'basic_{shape[0]}x{shape[1]}_r{r2}', shape, r2, basic_tracks(shape))
    # lengths that cross the lane (4 points) and span (256 points) cuts; walks with rests and revisits
    lengths = (1, 3, 4, 5, 255, 256, 257, 1025)
    for r2 in (1, 8, 26):
        add(f'lengths_r{r2}', (37, 53), r2, walks(300 + r2, (37, 53), lengths))
    # round borders at planes 1 and 8 (and the counts around them), about six points a track: the unset path
    for n in (31, 32, 33, 257):
        rng = np.random.default_rng(100 + n)
        add(f'borders_{n}', (70, 130), 5, walks(200 + n, (70, 130), rng.integers(0, 12, n)))
    add('borders_257_r26', (70, 130), 26, walks(457, (70, 130), np.random.default_rng(357).integers(0, 12, 257)))
    # the memset path: a tiny raster and many points a round
    add('memset_path', (5, 3), 2, walks(50, (5, 3), np.full(40, 157)))
    # a first offset that is not 0: 1, 2 and 3 mod 4
    for lead in (1, 2, 7):
        add(f'lead_{lead}', (37, 53), 4, walks(20 + lead, (37, 53), np.random.default_rng(20 + lead).integers(0, 9, 40)),
            lead=lead)
    # the two tracks of the work bounds (tests/test_passage_emulation.py): 1024 unit moves in a line, and a ping-pong
    add('straight_1024', (11, 1030), 25, [[(5, 2 + k) for k in range(1025)]])
    add('pingpong_4096', (37, 53), 25, [pingpong((18, 26), (18, 27), 4096)])
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
_expected = {}


def case(name):
    return CASES[CASE_IDS.index(name)]


def expected(name):
    """(counts, cells_per_track) of a case, computed once and shared (read-only)."""
    if name not in _expected:
        c = case(name)
        res = passage(c['tracks'], c['shape'], c['r2'])
        for a in res:
            a.setflags(write=False)
        _expected[name] = res
    return _expected[name]


def flat(c):
    """(traj int16 (lead + points, 2), offsets int64 (2 + ntracks)): offsets[1:] is what the call gets.  The `lead`
    points in front are in-raster, so a kernel that read them would count them."""
    lead = np.zeros((c['lead'], 2), dtype=np.int16)
    traj = np.concatenate([lead] + c['tracks'] + [np.zeros((0, 2), dtype=np.int16)])
    lengths = np.array([c['lead']] + [len(t) for t in c['tracks']], dtype=np.int64)
    return np.ascontiguousarray(traj), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def clearing_paths(c, planes):
    """How every round with points gets its planes cleared, by the rule of passage.hip: the first by a memset; a later
    one by the unset walk of the round before when that walk's bound -- 4 bytes read a point, 4 bytes stored to a whole
    disk a track and to the largest crescent for every point -- is below the bytes of this round's planes."""
    rows, cols = c['shape']
    lengths = [len(t) for t in c['tracks']]
    ndisk, ncres = len(disk(c['r2'])), max(crescent_sizes(c['r2']))
    out, prev = [], None
    for t0 in range(0, len(lengths), 32 * planes):
        part = lengths[t0:t0 + 32 * planes]
        if not sum(part):
            continue
        used = -(-len(part) // 32) * rows * cols * 4
        if prev is None:
            out.append('memset')
        else:
            out.append('unset' if sum(prev) * 4 * (1 + ncres) + len(prev) * 4 * ndisk < used else 'memset')
        prev = part
    return out


def check(name, counts, per_track, before=None):
    """counts / per_track (uint32 views) of one call on a case against the restatement, plus the checksum.  before: what
    counts held on entry (it is added to)."""
    c = case(name)
    ref_counts, ref_per_track = expected(name)
    counts = np.asarray(counts).view(np.uint32).reshape(c['shape'])
    per_track = np.asarray(per_track).view(np.uint32)
    if before is not None:
        counts = counts - np.asarray(before).view(np.uint32).reshape(c['shape'])
    assert np.array_equal(counts, ref_counts), name
    assert np.array_equal(per_track, ref_per_track), name
    assert int(counts.sum(dtype=np.int64)) == int(per_track.sum(dtype=np.int64))
    assert int(counts.max()) <= len(c['tracks'])
