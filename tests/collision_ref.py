"""K19 as its definition (include/ssrs_hip_collision.h, ssrs_rotor_collision_risk) in plain numpy and plain Python: Band's
probability evaluated one radius at a time (the independent statement of turbines.band_probability), the table of a class,
and a brute force over ALL (move, turbine) pairs that takes K18's transits from tests/transit_ref.py, restates the two
numbers its test compares in the header's operation order, turns them into the ring and sums the table's entries -- the
only oracle of the collision risk.  The cases are transit_ref's (each with classes and a table of its own) plus planted
crossings where the ring index can go wrong.  tests/test_collision_host.py (hand-made numbers), tests/
test_collision_emulation.py (the kernel's own code on the CPU) and tests/test_gpu_collision_risk.py (the device) share
them.  Every comparison of kernel outputs is integer equality."""
import math

import numpy as np

import transit_ref as tref

RINGS = 256
MM = tref.MM
SHAPE = tref.SHAPE
GROUND, LEVEL, HUB = tref.GROUND, tref.LEVEL, tref.HUB
PROFILE = (0.73, 0.79, 0.88, 0.96, 1.00, 0.98, 0.92, 0.85, 0.80, 0.75, 0.70, 0.64, 0.58, 0.52, 0.47, 0.41, 0.37, 0.30, 0.24,
           0.00)


# ------------------------------------------------------------------------------------------------ the model
def chord_at(x, profile=PROFILE):
    """The profile at x = r / R: its 20 values stand at 0.05, 0.10, ..., 1.00; linear between them, constant below 0.05."""
    if x <= 0.05:
        return profile[0]
    if x >= 1.:
        return profile[19]
    j = min(18, int(math.floor(x / 0.05 + 1e-12)) - 1)                  # the node at or below x
    x0 = 0.05 * (j + 1)
    return profile[j] + (profile[j + 1] - profile[j]) * (x - x0) / 0.05


def band_p(r, R, rpm, max_chord, pitch, blades, v, L, W, flapping, model_3d, upwind, profile=PROFILE):
    """Band's single-transit collision probability at ONE radius r, in plain Python."""
    omega = 2. * math.pi * rpm / 60.
    if not (blades > 0 and omega > 0. and v > 0. and R > 0. and 0. < r <= R):
        return 0.
    c = max_chord * chord_at(r / R, profile)
    gamma = math.radians(pitch)
    alpha = v / (r * omega)
    swept = abs((1. if upwind else -1.) * c * math.sin(gamma) + alpha * c * math.cos(gamma)) if model_3d else 0.
    body = L if alpha < L / W else W * alpha * (1. if flapping else 2. / math.pi)
    return min(1., max(0., blades * omega / (2. * math.pi * v) * (swept + body)))


def ring_midpoints(reach):
    return [reach * math.sqrt((k + 0.5) / RINGS) for k in range(RINGS)]


def band_rows(R, reach, rpm, max_chord, pitch, blades, v, L, W, flapping, model_3d, profile=PROFILE):
    """uint32 (2, 256): the table's two rows of one class, [with the wind (the bird flies downwind), against the wind]."""
    out = np.zeros((2, RINGS), dtype=np.uint32)
    for dirn in (0, 1):
        for k, r in enumerate(ring_midpoints(reach)):
            p = band_p(r, R, rpm, max_chord, pitch, blades, v, L, W, flapping, model_3d, dirn == 1, profile)
            out[dirn, k] = min(2 ** 32 - 1, int(np.rint(p * 2. ** 32)))
    return out


# ------------------------------------------------------------------------------------------------ the walk
def ring_matrix(traj, alt, off, elev, xy, reach, hub, axis, shape, mm_per_cell=MM):
    """(track, dirn, ring): transit_ref.move_matrix's track and direction of every testable move against every turbine, and
    int16 (moves, nturb) the ring of the crossing (meaningless where dirn < 0), from the header's definition."""
    k, track, dirn = tref.move_matrix(traj, alt, off, elev, xy, reach, hub, axis, shape, mm_per_cell)
    traj = np.asarray(traj).reshape(-1, 2)
    r0, c0 = traj[k, 0].astype(np.float64), traj[k, 1].astype(np.float64)
    r1, c1 = traj[k + 1, 0].astype(np.float64), traj[k + 1, 1].astype(np.float64)
    e = np.asarray(elev).astype(np.int64)
    alt = np.asarray(alt).astype(np.int64)
    z0 = e[traj[k, 0], traj[k, 1]] + alt[k]
    z1 = e[traj[k + 1, 0], traj[k + 1, 1]] + alt[k + 1]
    xy, reach = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(reach, dtype=np.float64)
    axis, hub = np.asarray(axis, dtype=np.float64).reshape(-1, 2), np.asarray(hub).astype(np.int64)
    xt, yt, ax, ay = xy[None, :, 0], xy[None, :, 1], axis[None, :, 0], axis[None, :, 1]
    mm = np.float64(mm_per_cell)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        dx0, dy0 = c0[:, None] - xt, r0[:, None] - yt
        dx1, dy1 = c1[:, None] - xt, r1[:, None] - yt
        s0, s1 = ax * dx0 + ay * dy0, ax * dx1 + ay * dy1
        u0, u1 = ax * dy0 - ay * dx0, ax * dy1 - ay * dx1
        h0 = (z0[:, None] - hub[None, :]).astype(np.float64) / mm
        h1 = (z1[:, None] - hub[None, :]).astype(np.float64) / mm
        d = s0 - s1
        U = s0 * u1 - s1 * u0
        H = s0 * h1 - s1 * h0
        lhs = U * U + H * H
        rhs = (reach * reach)[None, :] * (d * d)
        quotient = np.where(dirn >= 0, (lhs / rhs) * 256., 0.)
        quotient = np.where(np.isfinite(quotient), quotient, 0.)
        ring = np.minimum(255, np.trunc(quotient).astype(np.int64))
        ring = np.where(rhs == 0., 0, np.where(~(lhs < rhs), 255, ring)).astype(np.int16)
    return track, dirn, ring


def brute_force(traj, alt, off, elev, xy, reach, hub, axis, shape, cls, table, mm_per_cell=MM):
    """transit_ref.brute_force's dict plus risk int64 (nturb, 2) and track_risk int64 (ntracks,), the exact sums in units of
    2^-32, and rings: the (track, turbine, direction, ring) of every transit in move order (for hand checks)."""
    out = tref.brute_force(traj, alt, off, elev, xy, reach, hub, axis, shape, mm_per_cell)
    track, dirn, ring = ring_matrix(traj, alt, off, elev, xy, reach, hub, axis, shape, mm_per_cell)
    cls, table = np.asarray(cls).astype(np.int64), np.asarray(table)
    nclass, nturb, ntracks = table.shape[0], dirn.shape[1], len(off) - 1
    assert table.shape == (nclass, 2, RINGS) and table.dtype == np.uint32 and cls.shape == (nturb,)
    risk = np.zeros((nturb, 2), dtype=np.int64)
    track_risk = np.zeros(ntracks, dtype=np.int64)
    move, turbine = np.nonzero(dirn >= 0)
    rings = []
    for m, t in zip(move, turbine):
        dr, k = int(dirn[m, t]), int(ring[m, t])
        rings.append((int(track[m]), int(t), dr, k))
        if 0 <= cls[t] < nclass:
            q32 = int(table[cls[t], dr, k])
            risk[t, dr] += q32
            track_risk[track[m]] += q32
    out.update(risk=risk, track_risk=track_risk, rings=rings)
    return out


# ------------------------------------------------------------------------------------------------ the cases
BAND_CLASSES = ((50., 60., 12., 4., 15., 3.), (40., 40., 15.5, 3.2, 10., 3.), (63., 65., 9., 4.5, 20., 2.))   # R, reach, rpm ..
BIRD = dict(v=15., L=0.85, W=2.1)


def classes_of(nturb, seed):
    """(cls int32 (nturb,), table uint32 (nclass, 2, 256)) of a case: seven classes -- three of Band's model, four of random
    bits with the extremes 0 and 2^32 - 1 among them, so that a wrong ring, direction or class shows -- dealt at random, with
    -1, nclass, a far index and INT32_MIN among the turbines (they add nothing)."""
    rng = np.random.default_rng(seed)
    table = np.zeros((7, 2, RINGS), dtype=np.uint32)
    for c, row in enumerate(BAND_CLASSES):
        table[c] = band_rows(*row, BIRD['v'], BIRD['L'], BIRD['W'], c == 1, c != 2)
    table[3:] = rng.integers(0, 2 ** 32, (4, 2, RINGS), dtype=np.uint64).astype(np.uint32)
    table[3, :, ::7] = 0
    table[4, :, ::5] = 2 ** 32 - 1
    cls = rng.integers(0, 7, nturb).astype(np.int32)
    cls[rng.random(nturb) < 0.1] = -1
    if nturb > 12:
        cls[tref.A], cls[tref.B], cls[tref.C2] = 4, 0, 5              # (the ping-pong's turbines: large entries, two classes)
        cls[tref.DIAG], cls[tref.OUTSIDE], cls[tref.BIG_HI] = 7, 3, -2 ** 31
        cls[12] = 1 << 20
    return cls, table


# the planted rings: an axis along +row and integer coordinates, so that every product of the test is exact
T_MAIN, T_OTHER, T_NOCLASS, T_PASTCLASS, T_ZERO, T_FAR = range(6)
RING_XY = ((30., 20.), (30., 20.), (30., 20.), (30., 20.), (50., 20.), (70., 50.))
RING_REACH = (4., 4., 4., 4., 0., 4.)
RING_CLS = (0, 1, -1, 2, 0, 1)


def _ring_tracks():
    """[(points, alts, name, rings of T_MAIN in move order as (direction, ring))]: a move (19, c) -> (20, c) goes against the
    wind through the plane of the turbines of row 20 at lateral offset c - 30 and, with its second point h cells above the
    hub, at height h: lhs = (c - 30)^2 + h^2 against rhs = 16."""
    out = []

    def add(name, points, want, alts=None):
        alts = [LEVEL] * len(points) if alts is None else alts
        out.append((np.array(points, dtype=np.int16).reshape(-1, 2), np.array(alts, dtype=np.int32), name, want))
    add('hub', [(19, 30), (20, 30)], [(1, 0)])                                      # lhs = 0
    add('rim', [(19, 34), (20, 34)], [(1, 255)])                                    # lhs == rhs = 16
    add('rim', [(19, 26), (20, 26)], [(1, 255)])
    add('beyond', [(19, 35), (20, 35)], [])
    for c, k in ((31, 16), (29, 16), (32, 64), (33, 144)):                          # 1 / 16, 4 / 16, 9 / 16: exact multiples
        add('multiple', [(19, c), (20, c)], [(1, k)])
    add('multiple_height', [(19, 30), (20, 30)], [(1, 4)], [LEVEL, LEVEL + 50_000])           # h = 0.5: 1 / 64
    add('multiple_height', [(19, 31), (20, 31)], [(1, 32)], [LEVEL, LEVEL - 100_000])         # 1 + 1: 2 / 16
    add('multiple_height', [(19, 30), (20, 30)], [(1, 16)], [LEVEL, LEVEL + 100_000])         # h = 1: 1 / 16
    add('millimetre', [(19, 30), (20, 30)], [(1, 15)], [LEVEL, LEVEL + 99_999])
    add('millimetre', [(19, 30), (20, 30)], [(1, 16)], [LEVEL, LEVEL + 100_001])
    add('millimetre', [(19, 30), (20, 30)], [(1, 15)], [LEVEL, LEVEL - 99_999])
    add('millimetre', [(19, 30), (20, 30)], [(1, 16)], [LEVEL, LEVEL - 100_001])
    add('millimetre', [(19, 30), (20, 30)], [(1, 255)], [LEVEL, LEVEL + 400_000])             # the rim in height
    add('millimetre', [(19, 30), (20, 30)], [(1, 255)], [LEVEL, LEVEL + 399_999])             # 255.99 of 256
    add('millimetre', [(19, 30), (20, 30)], [], [LEVEL, LEVEL + 400_001])
    add('both_ways', [(19, 31), (20, 31), (19, 31), (19, 32), (20, 32)], [(1, 16), (0, 16), (1, 64)])
    add('zero_reach', [(19, 50), (20, 50)], [])                                     # through T_ZERO's hub: its ring 0
    add('zero_reach', [(19, 51), (20, 51)], [])                                     # beside it: nothing
    # transits on every move, across the lane, span and chunk cuts: 1200 points to and fro at lateral offset 2, then 3
    p = np.empty((1200, 2), dtype=np.int16)
    p[0::2], p[1::2] = (19, 32), (20, 32)
    add('to_and_fro', p, [(1, 64), (0, 64)] * 599 + [(1, 64)])
    p = p.copy()
    p[:, 1] = 33
    add('to_and_fro', p, [(1, 144), (0, 144)] * 599 + [(1, 144)])
    return out


def _ring_case(name, shift=0):
    planted = _ring_tracks()
    nturb = len(RING_XY)
    rng = np.random.default_rng(19)
    table = rng.integers(0, 2 ** 32, (2, 2, RINGS), dtype=np.uint64).astype(np.uint32)
    return dict(name=name, shape=SHAPE, tracks=[p for p, _, _, _ in planted], alts=[a for _, a, _, _ in planted],
                elev=np.full(SHAPE, GROUND, dtype=np.int32), xy=np.array(RING_XY), reach=np.array(RING_REACH),
                hub=np.full(nturb, HUB, dtype=np.int32), axis=np.tile(np.array([tref.PLANE]), (nturb, 1)), lead=0, tail=0,
                shift=shift, cls=np.array(RING_CLS, dtype=np.int32), table=table)


def _cases():
    out = []
    for c in tref.DEVICE_CASES:
        cls, table = classes_of(len(c['reach']), 19)
        out.append(dict(c, cls=cls, table=table))
    out.append(_ring_case('rings'))
    out.append(_ring_case('rings_shift_3', shift=3))
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
_expected = {}


def case(name):
    return CASES[CASE_IDS.index(name)]


def many_turbines(nturb):
    """transit_ref.many_turbines with classes: copies of A (class and all) in the last slot and either side of both LDS
    limits, K18's 7680 and K19's 2560."""
    c = tref.many_turbines(nturb)
    for t in (2559, 2560):
        if t < nturb - 1:
            for key in ('xy', 'reach', 'hub', 'axis'):
                c[key] = c[key].copy()
                c[key][t] = c[key][tref.A]
    cls, table = classes_of(nturb, nturb)
    for t in (2559, 2560, 7679, 7680, nturb - 1):
        if tref.NTURB <= t < nturb:
            cls[t] = cls[tref.A]
    return dict(c, cls=cls, table=table)


def compute(c, off=None):
    """The brute force of a case over the tracks of `off` (default: all)."""
    traj, alt, offsets = tref.flat(c)
    off = offsets[1:] if off is None else off
    return brute_force(traj, alt, off, c['elev'], c['xy'], c['reach'], c['hub'], c['axis'], c['shape'], c['cls'], c['table'])


def expected(name):
    """The brute force of a named case, computed once and shared (read-only)."""
    if name not in _expected:
        res = compute(case(name))
        for a in res.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _expected[name] = res
    return _expected[name]
