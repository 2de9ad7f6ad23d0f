"""K20 as its definition (include/ssrs_hip_sites.h, ssrs_site_collision_risk): the oracle is collision_ref.brute_force ITSELF
-- K19's pinned brute force over all (move, turbine) pairs -- called with the sites as turbines: xy = the cell centres, hub
from `elev` by the header's rule, reach = NaN on nodata, cls = 0 and the one class's table.  It is evaluated in slabs of
sites, so that no temporary exceeds ~100 MB, piece by piece of the chunk (the sums are adds over moves), and only over the
sites within Chebyshev distance W + 1 of some testable move's first point: every other site is 0 by the header's window statement, which tests/test_site_host.py proves separately by a
brute force over ALL sites.  The cases are transit_ref's and collision_ref's on their 70 x 90 raster, the candidate
classes below, rasters smaller than the window, and per-cell axes.  tests/test_site_host.py, tests/test_site_emulation.py
(the kernel's own code on the CPU) and tests/test_gpu_site_risk.py (the device) share them.  Every comparison of kernel
outputs is integer equality."""
import hashlib
import math

import numpy as np

import collision_ref as cref
import transit_ref as tref

MM = tref.MM
SHAPE = tref.SHAPE
GROUND, LEVEL = tref.GROUND, tref.LEVEL
PLANE = tref.PLANE
I32_MIN, I32_MAX = tref.I32_MIN, tref.I32_MAX
SENTINEL = tref.SENTINEL
SLAB_BYTES = 100e6


def window(reach):
    """W of the header: (int)floor(reach + 1.5); 0 for a reach nothing transits."""
    return int(math.floor(reach + 1.5)) if reach >= 0. else 0


def site_turbines(elev, reach, hub_mm, axis, sites=None):
    """(xy f64 (n, 2), reach f64 (n,), hub int32 (n,), axis f64 (n, 2)) of the sites `sites` (flat cell indices; default:
    all) as K19's turbines."""
    elev = np.asarray(elev)
    rows, cols = elev.shape
    sites = np.arange(rows * cols) if sites is None else np.asarray(sites, dtype=np.int64)
    r, c = sites // cols, sites % cols
    e = elev[r, c].astype(np.int64)
    hub = np.clip(e + int(hub_mm), I32_MIN, I32_MAX).astype(np.int32)
    rch = np.where(e == SENTINEL, np.nan, float(reach))
    axis = np.asarray(axis, dtype=np.float64)
    ax = np.broadcast_to(axis, (sites.size, 2)) if axis.ndim == 1 else axis.reshape(-1, 2)[sites]
    return np.stack([c, r], 1).astype(np.float64), rch, hub, np.ascontiguousarray(ax)


def first_points(traj, alt, off, elev, shape):
    """(k, r0, c0): every testable move's first point, by transit_ref.move_matrix's own selection."""
    k, _, _ = tref.move_matrix(traj, alt, off, elev, np.zeros((1, 2)), np.zeros(1), np.zeros(1, dtype=np.int32),
                               np.zeros((1, 2)), shape)
    pts = np.asarray(traj).reshape(-1, 2)
    return k, pts[k, 0].astype(np.int64), pts[k, 1].astype(np.int64)


PIECE = 64                                          # points of a piece of the chunk


def pieces(off):
    """The chunk cut into pieces of at most PIECE points, [(offsets of the piece, its first track)]: runs of whole short
    tracks, and a long track in pieces that each start at the last point of the one before, so that every move of the chunk
    is in exactly one piece.  The sums are adds over moves, so the pieces' results add up to the chunk's."""
    off = np.asarray(off, dtype=np.int64)
    out, t, ntracks = [], 0, off.size - 1
    while t < ntracks:
        if off[t + 1] - off[t] > PIECE:
            for lo in range(int(off[t]), int(off[t + 1]) - 1, PIECE - 1):
                out.append((np.array([lo, min(lo + PIECE, int(off[t + 1]))], dtype=np.int64), t))
            t += 1
            continue
        t1 = t + 1
        while t1 < ntracks and off[t1 + 1] - off[t] <= PIECE:
            t1 += 1
        out.append((off[t:t1 + 1], t))
        t = t1
    return out


def brute_force(traj, alt, off, elev, reach, hub_mm, axis, table, shape, mm_per_cell=MM, every_site=False):
    """dict(transits int64 (rows, cols, 2), risk int64 (rows, cols, 2), rings: collision_ref's (track, SITE, direction,
    ring) of every transit).  collision_ref.brute_force over the pieces of the chunk, each against the sites within W + 1 of
    one of its testable moves' first points, in slabs of sites.  every_site: the whole chunk against ALL sites in one piece
    (the host test of the window statement)."""
    rows, cols = shape
    table = np.asarray(table)
    assert table.shape == (2, cref.RINGS) and table.dtype == np.uint32
    transits = np.zeros((rows * cols, 2), dtype=np.int64)
    risk = np.zeros((rows * cols, 2), dtype=np.int64)
    rings = []
    reachable = window(reach) + 1
    for piece, track0 in ([(np.asarray(off, dtype=np.int64), 0)] if every_site else pieces(off)):
        k, r0, c0 = first_points(traj, alt, piece, elev, shape)
        if k.size == 0:
            continue
        if every_site:
            sites = np.arange(rows * cols)
        else:
            near = np.zeros((rows, cols), dtype=bool)
            for r, c in set(zip(r0.tolist(), c0.tolist())):
                near[max(0, r - reachable):r + reachable + 1, max(0, c - reachable):c + reachable + 1] = True
            sites = np.flatnonzero(near.reshape(-1))
        slab = max(1, int(SLAB_BYTES // (8 * k.size)))
        for lo in range(0, sites.size, slab):
            s = sites[lo:lo + slab]
            xy, rch, hub, ax = site_turbines(elev, reach, hub_mm, axis, s)
            out = cref.brute_force(traj, alt, piece, elev, xy, rch, hub, ax, shape, np.zeros(s.size, dtype=np.int32),
                                   table[None], mm_per_cell)
            transits[s] += out['transits']
            risk[s] += out['risk']
            rings += [(trk + track0, int(s[t]), d, ring) for trk, t, d, ring in out['rings']]
    return dict(transits=transits.reshape(rows, cols, 2), risk=risk.reshape(rows, cols, 2), rings=rings)


# ------------------------------------------------------------------------------------------------ the candidate classes
def _unit(degrees):
    return (math.sin(math.radians(degrees)), math.cos(math.radians(degrees)))


def _table():
    """One class's rows: random bits with zeros (a transit that adds nothing to the sum) and 2^32 - 1 among them, so that
    a wrong ring or direction shows."""
    rng = np.random.default_rng(20)
    table = rng.integers(0, 2 ** 32, (2, cref.RINGS), dtype=np.uint64).astype(np.uint32)
    table[:, ::7] = 0
    table[:, 3::11] = 2 ** 32 - 1
    return table


TABLE = _table()
# reach in cells, hub_mm, the uniform axis.  r4: the planted numbers of transit_ref and collision_ref are exact (integer
# coordinates, the axis along +row, the hub at the planted points' height).  r0: only a move through a hub itself transits
CLASSES = {
    'r4': dict(reach=4.0, hub_mm=LEVEL, axis=PLANE),
    'r065': dict(reach=0.65, hub_mm=80_000, axis=_unit(200.)),
    'r65': dict(reach=6.5, hub_mm=120_000, axis=_unit(33.)),
    'r0': dict(reach=0., hub_mm=LEVEL, axis=PLANE),
}
CLASS_IDS = list(CLASSES)


def cell_axes(shape, seed=20):
    """A per-cell raster of axes (rows, cols, 2): random unit steps, with NaNs (either component), a zero axis and axes that
    are no unit vectors among them."""
    rng = np.random.default_rng(seed)
    angle = rng.uniform(0., 2. * np.pi, shape)
    axes = np.stack([np.sin(angle), np.cos(angle)], -1)
    pick = rng.random(shape)
    axes[pick < 0.03, 0] = np.nan
    axes[(pick >= 0.03) & (pick < 0.06), 1] = np.nan
    axes[(pick >= 0.06) & (pick < 0.09)] = 0.
    axes[(pick >= 0.09) & (pick < 0.12)] *= 1.5
    if shape == SHAPE:
        axes[20, 28:33] = PLANE                     # (some of the planted crossings stay)
    return np.ascontiguousarray(axes)


# ------------------------------------------------------------------------------------------------ the cases
def _tiny(name, shape, tracks, elev=None):
    """A raster smaller than every window, with tracks along its edges and corners (the heights wander around the hub)."""
    tracks = [np.array(t, dtype=np.int16).reshape(-1, 2) for t in tracks]
    rng = np.random.default_rng(len(name))
    alts = [(LEVEL + rng.integers(-150_000, 150_000, len(t))).astype(np.int32) for t in tracks]
    elev = np.full(shape, GROUND, dtype=np.int32) if elev is None else elev
    return dict(name=name, shape=shape, tracks=tracks, alts=alts, elev=elev, lead=0, tail=0, shift=0)


def _tiny_cases():
    e32 = np.full((3, 2), GROUND, dtype=np.int32)
    e32[1, 1] = GROUND + 40_000
    e17 = np.full((1, 7), GROUND, dtype=np.int32)
    e17[0, 5] = SENTINEL                            # a nodata site, and nodata under the moves that touch it
    return [
        _tiny('tiny_1x1', (1, 1), [[(0, 0), (0, 0), (0, 0)], [(0, 0)], []]),
        _tiny('tiny_1x7', (1, 7), [[(0, c) for c in range(7)], [(0, c) for c in range(6, -1, -1)],
                                   [(0, 0), (0, 1), (0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 3)], [(0, 6), (0, 7)]], e17),
        _tiny('tiny_3x2', (3, 2), [[(0, 0), (1, 1), (2, 0), (1, 0), (0, 1), (0, 0), (1, 0), (2, 1), (2, 0)],
                                   [(2, 1), (1, 1), (0, 1), (0, 0), (1, 1), (2, 1)], [(0, 0), (-1, 0)], [(2, 1), (3, 2)]], e32),
    ]


TINY_CASES = _tiny_cases()
TINY_CLASSES = {
    'r4_col': dict(reach=4.0, hub_mm=LEVEL, axis=(1., 0.)),
    'r65_row': dict(reach=6.5, hub_mm=LEVEL + 30_000, axis=PLANE),
    'r065_skew': dict(reach=0.65, hub_mm=LEVEL, axis=_unit(40.)),
}
BASE_CASES = [c for c in cref.CASES if c['name'] != 'random']        # transit_ref.DEVICE_CASES and the rings
BASE_IDS = [c['name'] for c in BASE_CASES]
# every (case, class) the emulation and the device run with the uniform axis
COMBOS = [(c, k) for c in BASE_CASES for k in CLASS_IDS] + [(c, k) for c in TINY_CASES for k in TINY_CLASSES]
COMBO_IDS = [f"{c['name']}-{k}" for c, k in COMBOS]
# and with per-cell axes
CELL_COMBOS = [(cref.case('planted'), 'r4'), (cref.case('rings'), 'r65'), (cref.case('cuts_shift_1'), 'r065')] + \
    [(c, 'r4_col') for c in TINY_CASES]
CELL_IDS = [f"{c['name']}-{k}-cells" for c, k in CELL_COMBOS]


def klass(name):
    return CLASSES[name] if name in CLASSES else TINY_CLASSES[name]


def case(name):
    for c in BASE_CASES + TINY_CASES:
        if c['name'] == name:
            return c
    raise KeyError(name)


_expected = {}


def compute(c, k, off=None, axis=None, every_site=False):
    """The brute force of case `c` and class `k` (a name) over the tracks of `off` (default: all), with the class's uniform
    axis or the raster `axis`."""
    traj, alt, offsets = tref.flat(c)
    off = offsets[1:] if off is None else off
    k = klass(k)
    return brute_force(traj, alt, off, c['elev'], k['reach'], k['hub_mm'], k['axis'] if axis is None else axis, TABLE,
                       c['shape'], every_site=every_site)


def expected(c, k, per_cell=False):
    """The brute force of a case and a class, computed once and shared (read-only).  Cases that differ only in what lies
    around their chunk (lead, tail, the buffers' placement) share one evaluation: the key is the chunk's own content."""
    traj, alt, offsets = tref.flat(c)
    off = offsets[1:]
    h = hashlib.sha1()
    for a in (traj[off[0]:off[-1]], alt[off[0]:off[-1]], off - off[0], np.asarray(c['elev'])):
        h.update(np.ascontiguousarray(a).tobytes())
    key = (h.hexdigest(), c['shape'], k, per_cell)
    if key not in _expected:
        res = compute(c, k, axis=cell_axes(c['shape']) if per_cell else None)
        for a in res.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _expected[key] = res
    return _expected[key]
