"""K18 as its definition (include/ssrs_hip_transits.h, ssrs_rotor_transits) in plain numpy: a brute force over ALL (move,
turbine) pairs with the header's operation order (numpy does not contract) -- the only oracle of the rotor transits -- and
the named cases that tests/test_transit_host.py (hand-made numbers, the cull lists), tests/test_transit_emulation.py (the
kernel's own code on the CPU) and tests/test_gpu_rotor_transits.py (the device) share.  Every comparison is integer
equality."""
import numpy as np

import rotor_ref

ROWS, COLS = rotor_ref.ROWS, rotor_ref.COLS         # 70 x 90: 3 x 3 bins of 32 x 32 cells, neither side a multiple of 32
SHAPE = rotor_ref.SHAPE
LENGTHS = rotor_ref.LENGTHS                         # [1, 1, 0, 2, 63, 64, 65, 255, 256, 257, 1000, 4097] + [3] * 300
NTURB = rotor_ref.NTURB                             # 70: three bitmap words
SENTINEL = rotor_ref.SENTINEL
I32_MIN, I32_MAX = rotor_ref.I32_MIN, rotor_ref.I32_MAX
RESOLUTION = 100.                                   # metres a cell
MM = 1000. * RESOLUTION                             # mm_per_cell
CULL_MARGIN = 1.5                                   # the caller's lists are built from reach + 1.5
GROUND, LEVEL = 100_000, 50_000                     # the planted cells' elev and the planted points' alt: z = HUB
HUB = GROUND + LEVEL


def move_matrix(traj, alt, off, elev, xy, reach, hub, axis, shape, mm_per_cell=MM):
    """(first, track, dirn): the index of every move's first point (off[0] <= k, k + 1 in the same track), its track, and
    int8 (moves, nturb): -1 where the move is no transit of the turbine, else its direction, every pair on its own."""
    rows, cols = shape
    traj = np.asarray(traj).reshape(-1, 2)
    off = np.asarray(off, dtype=np.int64)
    lengths = np.diff(off)
    track_of = np.repeat(np.arange(lengths.size), lengths)              # of the points off[0] ..
    k = np.arange(off[0], off[-1] - 1, dtype=np.int64)
    same = track_of[k - off[0]] == track_of[k + 1 - off[0]] if k.size else np.zeros(0, dtype=bool)
    k = k[same]
    r0, c0 = traj[k, 0].astype(np.int64), traj[k, 1].astype(np.int64)
    r1, c1 = traj[k + 1, 0].astype(np.int64), traj[k + 1, 1].astype(np.int64)
    inside = (r0 >= 0) & (r0 < rows) & (c0 >= 0) & (c0 < cols) & (r1 >= 0) & (r1 < rows) & (c1 >= 0) & (c1 < cols)
    k, r0, c0, r1, c1 = (v[inside] for v in (k, r0, c0, r1, c1))
    elev = np.asarray(elev)
    e0, e1 = elev[r0, c0].astype(np.int64), elev[r1, c1].astype(np.int64)
    ok = (e0 != SENTINEL) & (e1 != SENTINEL) & (np.maximum(np.abs(r1 - r0), np.abs(c1 - c0)) <= 1)
    k, r0, c0, r1, c1, e0, e1 = (v[ok] for v in (k, r0, c0, r1, c1, e0, e1))
    alt = np.asarray(alt).astype(np.int64)
    z0, z1 = e0 + alt[k], e1 + alt[k + 1]
    xy, reach = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(reach, dtype=np.float64)
    axis, hub = np.asarray(axis, dtype=np.float64).reshape(-1, 2), np.asarray(hub).astype(np.int64)
    xt, yt, ax, ay = xy[None, :, 0], xy[None, :, 1], axis[None, :, 0], axis[None, :, 1]
    mm = np.float64(mm_per_cell)
    with np.errstate(invalid='ignore', over='ignore'):
        dx0, dy0 = c0.astype(np.float64)[:, None] - xt, r0.astype(np.float64)[:, None] - yt
        dx1, dy1 = c1.astype(np.float64)[:, None] - xt, r1.astype(np.float64)[:, None] - yt
        s0, s1 = ax * dx0 + ay * dy0, ax * dx1 + ay * dy1
        u0, u1 = ax * dy0 - ay * dx0, ax * dy1 - ay * dx1
        h0 = (z0[:, None] - hub[None, :]).astype(np.float64) / mm
        h1 = (z1[:, None] - hub[None, :]).astype(np.float64) / mm
        crossing = (s0 < 0.) != (s1 < 0.)
        d = s0 - s1
        U = s0 * u1 - s1 * u0
        H = s0 * h1 - s1 * h0
        transit = crossing & (reach >= 0.)[None, :] & (U * U + H * H <= (reach * reach)[None, :] * (d * d))
        dirn = np.where(transit, np.where(s0 < 0., 1, 0), -1).astype(np.int8)
    return k, track_of[k - off[0]], dirn


def brute_force(traj, alt, off, elev, xy, reach, hub, axis, shape, mm_per_cell=MM):
    """dict(bitmap uint32 (ntracks, words), tracks_per_turbine int64, turbines_per_track int32, transits int64 (nturb, 2)) of
    the moves inside [off[0], off[-1]); `off` indexes traj and alt."""
    _, track, dirn = move_matrix(traj, alt, off, elev, xy, reach, hub, axis, shape, mm_per_cell)
    n, nturb = len(off) - 1, dirn.shape[1]
    words = (nturb + 31) // 32
    enc = np.zeros((n, words * 32), dtype=bool)
    np.logical_or.at(enc[:, :nturb], track, dirn >= 0)
    weights = 1 << np.arange(32, dtype=np.uint64)
    bitmap = (enc.reshape(n, words, 32) * weights).sum(2).astype(np.uint32)
    transits = np.stack([(dirn == 0).sum(0), (dirn == 1).sum(0)], 1).astype(np.int64)
    return dict(bitmap=bitmap, tracks_per_turbine=enc[:, :nturb].sum(0).astype(np.int64),
                turbines_per_track=enc[:, :nturb].sum(1).astype(np.int32), transits=transits)


# the planted turbines' slots among the NTURB
A, B, C2, NAN_REACH, NEG_REACH, NAN_XY, NAN_AXIS, DIAG, OUTSIDE, BIG_HI, BIG_LO = range(11)
PLANE = (0., 1.)                                    # axis along +row: the plane is a row (or lies between two)


def planted_turbines(xy, reach, hub, axis):
    """Overwrites the first eleven turbines and those on bits 31 / 32 and 63 / 64 (in place)."""
    def put(t, pos, rch, h, a=PLANE):
        xy[t], reach[t], hub[t], axis[t] = pos, rch, h, a
    put(A, (30., 20.5), 3., HUB)                    # between two rows
    put(B, (30., 20.), 3., HUB)                     # on a row
    put(C2, (31., 20.5), 5., HUB)                   # overlaps A
    # nothing transits these four, all of them on A
    put(NAN_REACH, (30., 20.5), np.nan, HUB)
    put(NEG_REACH, (30., 20.5), -1., HUB)
    put(NAN_XY, (np.nan, 20.5), 3., HUB)
    put(NAN_AXIS, (30., 20.5), 3., HUB, (np.nan, 1.))
    put(DIAG, (60.5, 40.5), 1., HUB, (1., 0.))      # the plane is between two columns
    put(OUTSIDE, (-2., 29.5), 4., 101)              # outside the raster, reaching in
    put(BIG_HI, (80.5, 60.5), 1., I32_MAX)          # z beyond int32: a hit only in 64 bits
    put(BIG_LO, (80.5, 60.5), 1., 2 ** 30)          # z below int32: a hit only if the sum wrapped
    for t, pos in zip((31, 32, 63, 64), ((20., 15.), (45.5, 35.), (66., 52.5), (33., 60.))):
        put(t, pos, 6., 350_000, axis[t])


def planted_tracks():
    """[(points, alts, name)]: the short tracks whose transits tests/test_transit_host.py counts by hand (`name` groups
    them).  They need planted_ground() under them."""
    out = []

    def add(name, points, alts=None):
        alts = [LEVEL] * len(points) if alts is None else alts
        out.append((np.array(points, dtype=np.int16).reshape(-1, 2), np.array(alts, dtype=np.int32), name))
    for c in range(26, 35):                          # A's edge is at c = 27 and 33
        add('between_rows', [(20, c), (21, c)])
        add('between_rows_back', [(21, c), (20, c)])
    add('on_a_row', [(19, 30), (20, 30), (21, 30)])  # one transit of B
    add('on_a_row', [(20, 30), (19, 30)])            # one, with the wind
    add('on_a_row', [(20, 30), (21, 30)])            # none of B
    add('on_a_row', [(20, 30), (20, 31)])            # along B's plane: none
    for a in (LEVEL + 300_000, LEVEL + 300_001, LEVEL - 300_000, LEVEL - 300_001):
        add('height_edge', [(20, 30), (21, 30)], [a, a])
    add('diagonal', [(40, 60), (41, 61)], [350_000, -100_000])      # h = 3 and -1.5: 0.75 at the plane
    add('diagonal', [(40, 60), (41, 61)], [350_000, 0])             # h = 3 and -0.5: 1.25 at the plane
    add('beyond_int32', [(60, 80), (61, 80)], [I32_MAX + 50_000 - 2 ** 30] * 2)
    add('beyond_int32', [(60, 81), (61, 81)], [I32_MIN] * 2)
    # a track ENDS on one side of A while the next BEGINS on the other, then the same with empty tracks between
    add('end_begin', [(20, 28)])
    add('end_begin', [(21, 28)])
    add('end_begin', [])
    add('end_begin', [])
    add('end_begin', [(20, 28)])
    add('jump', [(19, 32), (22, 32)])                # three cells straight through A
    add('outside_end', [(29, 0), (30, -1)])
    add('nodata_end', [(20, 35), (21, 35)])          # inside C2 but for the nodata cell
    add('reaching_in', [(29, 0), (30, 0)], [1, 1])
    add('reaching_in', [(29, 2), (30, 2)], [1, 1])   # lateral offset exactly 4
    add('reaching_in', [(29, 3), (30, 3)], [1, 1])
    add('last', [(21, 29), (21, 30), (20, 31)])      # the case's last point: the tail lies across A from it
    return out


def planted_ground(elev):
    elev[18:23, 24:37] = GROUND
    elev[21, 35] = SENTINEL
    elev[40:42, 60:62] = GROUND
    elev[60:62, 80] = 2 ** 30
    elev[60:62, 81] = -2 ** 30
    elev[29:31, 0:4] = 100


def _base():
    rng = np.random.default_rng(18)
    tracks = [rotor_ref.walk(rng, n) for n in LENGTHS]
    elev = rng.integers(0, 400_000, SHAPE).astype(np.int32)
    elev[rng.random(SHAPE) < 0.05] = SENTINEL
    alts = [rng.integers(10_000, 300_000, len(t)).astype(np.int32) for t in tracks]
    xy, reach, _ = rotor_ref.random_turbines(rng, SHAPE, NTURB, 0, 600_000)
    hub = rng.integers(0, 600_000, NTURB).astype(np.int32)
    angle = rng.uniform(0., 2. * np.pi, NTURB)
    angle[:8] = np.arange(8) * (np.pi / 4.)
    axis = np.stack([np.sin(angle), np.cos(angle)], 1)
    axis[:8:2] = np.round(axis[:8:2])                # the four compass points, exactly
    return tracks, alts, elev, xy, reach, hub, axis


def _mirror(point):
    """The cell across A's plane from a point of row 20 or 21 within A's reach."""
    r, c = int(point[0]), int(point[1])
    assert r in (20, 21) and 27 <= c <= 33, point
    return 41 - r, c


def _cases():
    tracks, alts, elev, xy, reach, hub, axis = _base()
    # the random part alone, for the count of transits the cull test asks for
    random_part = dict(name='random', shape=SHAPE, tracks=tracks, alts=alts, elev=elev.copy(), xy=xy.copy(),
                       reach=reach.copy(), hub=hub.copy(), axis=axis.copy(), lead=0, tail=0, shift=0)
    elev, xy, reach, hub, axis = elev.copy(), xy.copy(), reach.copy(), hub.copy(), axis.copy()
    planted_turbines(xy, reach, hub, axis)
    planted_ground(elev)
    planted = planted_tracks()
    # the first track is one point at A's plane: lead points lie across it
    first = [(np.array([[21, 30]], dtype=np.int16), np.array([LEVEL], dtype=np.int32))]
    body = first + list(zip(tracks[1:], alts[1:])) + [(p, a) for p, a, _ in planted]
    out = [random_part]

    def add(name, body=body, lead=0, tail=0, shift=0, **kw):
        # lead / tail: points of another owner in front of off[0] and behind off[ntracks], across A's plane from the case's
        # first and last point (a kernel that read them as a move's end would count a transit); shift: the buffers start
        # this many points (4 bytes each) past a 16-byte boundary
        c = dict(name=name, shape=SHAPE, tracks=[p for p, _ in body], alts=[a for _, a in body], elev=elev, xy=xy,
                 reach=reach, hub=hub, axis=axis, lead=lead, tail=tail, shift=shift)
        c.update(kw)
        out.append(c)

    add('planted')
    for lead, shift in ((5, 1), (2, 2), (7, 3), (256, 0)):
        add(f'lead_{lead}_shift_{shift}', lead=lead, tail=5, shift=shift)
    # the 4097-point track ping-pongs across the plane inside A and C2 (and the four that nothing transits)
    pingpong = list(body)
    p = np.empty((4097, 2), dtype=np.int16)
    p[0::2], p[1::2] = (20, 30), (21, 30)
    pingpong[11] = (p, np.full(4097, LEVEL, dtype=np.int32))
    add('pingpong', pingpong)
    add('pingpong_shift_3', pingpong, lead=1, tail=3, shift=3)
    # a track that ends at point 255 on one side of A while the next begins at 256 on the other, then 64 tracks of four
    # points, a lane's load each, on alternating sides: every lane cut is such a pair (all of them rest: no transit)
    def rest(row, n):
        return np.tile(np.array([[row, 29]], dtype=np.int16), (n, 1)), np.full(n, LEVEL, dtype=np.int32)
    cuts = [rest(20, 256)] + [rest(21 - (k & 1), 4) for k in range(64)]
    add('cuts', cuts + body[1:])
    for shift in (1, 2, 3):
        add(f'cuts_shift_{shift}', cuts + body[1:], lead=4 + shift, tail=2, shift=shift)
    # the short tracks alone (the brute force of thousands of turbines stays small)
    short = first + [(t, a) for t, a in zip(tracks[12:], alts[12:])] + [(p, a) for p, a, _ in planted]
    add('short', short)
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
DEVICE_CASES = [c for c in CASES if c['name'] != 'random']           # ('random' has no planted ground for lead and tail)
DEVICE_IDS = [c['name'] for c in DEVICE_CASES]
_expected = {}


def case(name):
    return CASES[CASE_IDS.index(name)]


def many_turbines(nturb):
    """The 'short' case with `nturb` turbines: the planted and random ones first, random ones after them, and copies of A
    in the last slot and at 7679 / 7680 where there are that many (either side of the LDS rule's limit)."""
    c = dict(case('short'))
    rng = np.random.default_rng(nturb)
    extra = nturb - NTURB
    xy, reach, _ = rotor_ref.random_turbines(rng, SHAPE, extra, 0, 600_000)
    hub = rng.integers(0, 600_000, extra).astype(np.int32)
    angle = rng.uniform(0., 2. * np.pi, extra)
    c['xy'], c['reach'] = np.concatenate([c['xy'], xy]), np.concatenate([c['reach'], reach])
    c['hub'], c['axis'] = np.concatenate([c['hub'], hub]), np.concatenate([c['axis'], np.stack([np.sin(angle), np.cos(angle)], 1)])
    for t in (7679, 7680, nturb - 1):
        if NTURB <= t < nturb:
            for key in ('xy', 'reach', 'hub', 'axis'):
                c[key][t] = c[key][A]
    c['name'] = f'short_{nturb}'
    return c


def flat(c):
    """(traj int16 (lead + points + tail, 2), alt int32, offsets int64 (2 + ntracks)): offsets[1:] is what the call gets."""
    tracks = [np.asarray(t, dtype=np.int16).reshape(-1, 2) for t in c['tracks']]
    pieces, heights = list(tracks), list(c['alts'])
    lengths = [len(t) for t in tracks]
    nonempty = [t for t in tracks if len(t)]
    if c['lead']:
        pieces.insert(0, np.tile(np.array([_mirror(nonempty[0][0])], dtype=np.int16), (c['lead'], 1)))
        heights.insert(0, np.full(c['lead'], LEVEL, dtype=np.int32))
    if c['tail']:
        pieces.append(np.tile(np.array([_mirror(nonempty[-1][-1])], dtype=np.int16), (c['tail'], 1)))
        heights.append(np.full(c['tail'], LEVEL, dtype=np.int32))
    traj = np.ascontiguousarray(np.concatenate(pieces))
    alt = np.concatenate(heights).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([c['lead']] + lengths)]).astype(np.int64)
    assert traj.shape[0] == alt.size == off[-1] + c['tail']
    return traj, alt, off


def packed(elev):
    return rotor_ref.packed(elev)


def bins(c, margin=CULL_MARGIN):
    from ssrs_amd import turbines
    return turbines.build_bins(c['xy'], np.asarray(c['reach']) + margin, c['shape'])


def edit_bins(bins, turbine, times):
    """The cull lists with `turbine` named `times` times (0: omitted) wherever it was named once."""
    start, items = bins
    out, new_start = [], [0]
    for b in range(start.size - 1):
        seg = items[start[b]:start[b + 1]]
        seg = np.repeat(seg, np.where(seg == turbine, times, 1))
        out.append(seg)
        new_start.append(new_start[-1] + seg.size)
    return np.array(new_start, dtype=np.int32), np.ascontiguousarray(np.concatenate(out), dtype=np.int32)


def compute(c, off=None):
    """The brute force of a case over the tracks of `off` (default: all)."""
    traj, alt, offsets = flat(c)
    off = offsets[1:] if off is None else off
    return brute_force(traj, alt, off, c['elev'], c['xy'], c['reach'], c['hub'], c['axis'], c['shape'])


def expected(name):
    """The brute force of a named case, computed once and shared (read-only)."""
    if name not in _expected:
        res = compute(case(name))
        for a in res.values():
            a.setflags(write=False)
        _expected[name] = res
    return _expected[name]


def groups(name='planted'):
    """{group name: [track numbers]} of the planted tracks within a case built on `body`."""
    c = case(name)
    planted = planted_tracks()
    base = len(c['tracks']) - len(planted)
    out = {}
    for k, (_, _, group) in enumerate(planted):
        out.setdefault(group, []).append(base + k)
    return out
