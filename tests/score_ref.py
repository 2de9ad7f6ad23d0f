"""K21's expected values: the definition of include/ssrs_score.h in Python, on the oracle's own functions
(oracle/ssrs_oracle.py: window_weights, get_track_restrictions, move_away_from_boundary, _move_probabilities), and the small
cases that tests/test_score_emulation.py runs on the CPU build of score.hip and tests/test_gpu_score.py on the device.

A plain helper module; importing it needs no GPU.  expected(case) is computed once per process and must not be changed by
its users."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import ssrs_oracle as orc  # noqa: E402

SCORED, ZERO, NOT_A_MOVE, OUT, UNDEFINED, LAST = range(6)
COLUMNS = ('S', 'scored', 'zero', 'not_a_move', 'out', 'undefined')
_COLUMN_OF = {SCORED: 1, ZERO: 2, NOT_A_MOVE: 3, OUT: 4, UNDEFINED: 5}
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'g7_tracks.npz')
G7_SHAPE = (96, 128)
G7_TAGS = ('ff_m1', 'ff_m3', 'ff_d135_m2', 'drw_m1', 'drw_d250_m3', 'ff_m1_nu05')


def unit(d):
    return -1 <= d[0] <= 1 and -1 <= d[1] <= 1


def surprisal(p):
    """s = rint(-log2(p) * 2^32) of a SCORED move, a Python int."""
    return int(np.rint(-np.log2(np.float64(p)) * 4294967296.0))


def prior_of(move_dirn):
    return [float(v) for v in orc.get_directional_probs(move_dirn * np.pi / 180.)]


def score_track(track, shape, prior, memory, nu, updraft=None, potential=None):
    """(p f64 (n,), status uint8 (n,), base int (n, 2)) of one track, int (n, 2): entry j is the move that leaves point j."""
    rows, cols = shape
    burnin = int(min(rows, cols) / 10)
    n = len(track)
    pts = [(int(r), int(c)) for r, c in track]
    base = [p if j > burnin else orc.move_away_from_boundary(p[0], p[1], rows, cols) for j, p in enumerate(pts)]
    delta = [(pts[j + 1][0] - base[j][0], pts[j + 1][1] - base[j][1]) for j in range(n - 1)]
    p_out = np.zeros(n, dtype=np.float64)
    status = np.full(n, LAST, dtype=np.uint8)
    for j in range(n - 1):
        br, bc = base[j]
        if not (0 < br < rows - 1 and 0 < bc < cols - 1):
            status[j] = OUT
            continue
        if not unit(delta[j]):
            status[j] = NOT_A_MOVE
            continue
        mask = orc.get_track_restrictions(0, 0)
        for k in range(1, memory + 1):
            if j - k < 0 or not unit(delta[j - k]):        # the start, or a gap in the observations: the memory ends here
                break
            mask = mask & orc.get_track_restrictions(*delta[j - k])
        w = orc.window_weights(br, bc, updraft, potential, prior)
        with np.errstate(all='ignore'):
            p = orc._move_probabilities(w, prior, float(nu), [int(m) for m in mask])
        pj = p[3 * (delta[j][0] + 1) + (delta[j][1] + 1)]
        p_out[j] = pj
        status[j] = ZERO if pj == 0. else (SCORED if (pj > 0. and pj < np.inf) else UNDEFINED)
    return p_out, status, np.array(base, dtype=np.int64).reshape(n, 2)


def score(tracks, shape, move_dirn, memory, nu, updraft=None, potential=None):
    """The whole result of one call: p and status parallel to the concatenated points, rows int64 (ntracks, 6), the maps
    int64 (rows, cols), and s, the surprisal of every point's move (0 where not SCORED)."""
    prior = prior_of(move_dirn)
    ps, sts, ss = [np.zeros(0)], [np.zeros(0, dtype=np.uint8)], [np.zeros(0, dtype=np.int64)]
    rows = np.zeros((len(tracks), 6), dtype=np.int64)
    smap = np.zeros(shape, dtype=np.int64)
    cmap = np.zeros(shape, dtype=np.int64)
    for t, track in enumerate(tracks):
        p, st, base = score_track(track, shape, prior, memory, nu, updraft, potential)
        s = np.zeros(len(track), dtype=np.int64)
        for j in range(len(track)):
            if st[j] == LAST:
                continue
            rows[t, _COLUMN_OF[int(st[j])]] += 1
            if st[j] == SCORED:
                s[j] = surprisal(p[j])
                rows[t, 0] += s[j]
                smap[base[j, 0], base[j, 1]] += s[j]
                cmap[base[j, 0], base[j, 1]] += 1
        ps.append(p), sts.append(st), ss.append(s)
    return dict(p=np.concatenate(ps), status=np.concatenate(sts), s=np.concatenate(ss), rows=rows, surprisal_map=smap,
                scored_map=cmap)


# ------------------------------------------------------------------------------------------------ the fixture of the reference
_g7 = None


def g7():
    global _g7
    if _g7 is None:
        _g7 = dict(np.load(GOLDEN, allow_pickle=False))
    return _g7


def g7_case(tag):
    """(tracks, move_dirn, memory, nu, updraft, potential) of one of the reference's own runs."""
    g = g7()
    dirn, mem, nu, has_u, has_p = g[tag + '_params']
    off = np.concatenate([[0], np.cumsum(g[tag + '_lengths'])])
    tracks = [g[tag + '_tracks'][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return tracks, float(dirn), int(mem), float(nu), g['updraft'] if has_u else None, g['potential'] if has_p else None


# ------------------------------------------------------------------------------------------------ the small cases
def walk(n, shape, rng, start=None, rim=True):
    """n points of a random walk of moves in {-1, 0, 1}^2 (rests and reversals included), clipped to the raster (rim=True:
    the rim is visited, its moves are OUT) or to its interior."""
    lo = 0 if rim else 1
    r, c = start if start is not None else (int(rng.integers(1, shape[0] - 1)), int(rng.integers(1, shape[1] - 1)))
    pts = [(r, c)]
    for _ in range(n - 1):
        r = min(shape[0] - 1 - lo, max(lo, r + int(rng.integers(-1, 2))))
        c = min(shape[1] - 1 - lo, max(lo, c + int(rng.integers(-1, 2))))
        pts.append((r, c))
    return np.array(pts, dtype=np.int16).reshape(n, 2)


def forward(n, shape, rng):
    """n points that mostly go on within 45 degrees of the last move, bouncing off the rim: long runs of SCORED moves under
    any memory."""
    r, c = int(rng.integers(2, shape[0] - 2)), int(rng.integers(2, shape[1] - 2))
    ring = [(-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1)]
    h = int(rng.integers(0, 8))
    pts = [(r, c)]
    while len(pts) < n:
        h = (h + int(rng.integers(-1, 2))) % 8
        nr, nc = r + ring[h][0], c + ring[h][1]
        if not (1 <= nr <= shape[0] - 2 and 1 <= nc <= shape[1] - 2):
            h = (h + 3) % 8
            continue
        r, c = nr, nc
        pts.append((r, c))
    return np.array(pts, dtype=np.int16)


def hand_made(shape):
    """The planted tracks of every case: empty, one and two points, a jump and the moves after it, a rest, a move the mask
    forbids (a reversal), a point outside the raster, points on the rim."""
    rows, cols = shape
    r, c = rows // 2, cols // 2
    a = lambda *pts: np.array(pts, dtype=np.int16).reshape(len(pts), 2)
    return [
        a(),
        a((r, c)),
        a((r, c), (r + 1, c + 1)),
        a((r, c), (r + 1, c)),
        a((2, 2), (2, 3), (2, 4), (r, c + 2), (r + 1, c + 2), (r + 2, c + 2), (r + 2, c + 3), (r + 1, c + 3)),       # a jump
        a((2, 2), (3, 3), (3, 3), (3, 3), (4, 4), (3, 3), (4, 4), (4, 5), (4, 4)),                                    # rests, reversals
        a((2, 3), (3, 3), (3, 4), (-1, -1), (2, 4), (3, 4), (4, 4), (-1, -1), (-1, 0), (0, 0)),                       # off the raster
        a((1, 1), (0, 1), (0, 0), (1, 0), (1, 1), (2, 2), (rows - 2, cols - 2), (rows - 1, cols - 1), (rows - 1, cols - 2),
          (rows - 2, cols - 2), (rows - 3, cols - 3), (rows - 2, cols - 2)),                                          # the rim
        a((32767, 32767), (-32768, -32768), (1, 1), (2, 2)),                                                           # int16's ends
    ]


def oracle_tracks(shape, move_dirn, memory, nu, updraft, potential, rng, starts=None):
    """The oracle's own tracks, started on row 0, row 1, column 0, the far edges (where the burn-in relocation really
    happens) and inside."""
    rows, cols = shape
    if starts is None:
        starts = [(0, cols // 2), (1, 2), (rows // 2, 0), (rows - 1, cols // 3), (rows // 3, cols - 1), (rows - 2, cols - 2),
                  (0, 0), (rows // 2, cols // 2)]
    return [orc.generate_simulated_tracks(move_dirn, s, shape, memory, nu, updraft, potential,
                                          uniform=lambda k: float(rng.random())) for s in starts]


def fields(shape, rng):
    """A positive updraft and a potential that falls towards +row (heading 0), both rough."""
    rows, cols = shape
    upd = rng.uniform(0.2, 3.0, shape)
    pot = ((rows - np.arange(rows))[:, None] * 1.0 + rng.uniform(-0.4, 0.4, shape)).astype(np.float32)
    return upd, pot


def _case(name, shape, move_dirn, memory, nu, updraft, potential, tracks, lead=0, shift=0):
    return dict(name=name, shape=shape, move_dirn=float(move_dirn), memory=int(memory), nu=float(nu), updraft=updraft,
                potential=potential, tracks=[np.asarray(t, dtype=np.int16).reshape(-1, 2) for t in tracks], lead=lead,
                shift=shift)


def _make_cases():
    rng = np.random.default_rng(2121)
    cases = []
    small, thin = (7, 9), (12, 40)
    # 7 x 9 (burnin 0: only move 0 relocates), both fields
    upd, pot = fields(small, rng)
    bag = lambda shape: hand_made(shape) + [walk(65, shape, rng), walk(300, shape, rng), forward(70, shape, rng),
                                            walk(3, shape, rng, rim=False), walk(5, shape, rng, rim=False)]
    for memory, nu, lead, shift in ((1, 1., 3, 1), (3, 1., 0, 0), (8, 1., 5, 2), (1, 0., 0, 3), (2, 0.5, 2, 0), (1, 2., 0, 0)):
        tracks = bag(small) + oracle_tracks(small, 0., memory, nu, upd, pot, rng)
        cases.append(_case(f'7x9_m{memory}_nu{nu:g}', small, 0., memory, nu, upd, pot, tracks, lead, shift))
    # 12 x 40 (burnin 1): an updraft alone and another heading; no fields at all
    upd2, _ = fields(thin, rng)
    cases.append(_case('12x40_upd_m3', thin, 135., 3, 1., upd2, None,
                       bag(thin) + oracle_tracks(thin, 135., 3, 1., upd2, None, rng), 1, 3))
    cases.append(_case('12x40_drw_m1', thin, 0., 1, 1., None, None, bag(thin) + oracle_tracks(thin, 0., 1, 1., None, None, rng)))
    cases.append(_case('12x40_drw_d250_m3', thin, 250., 3, 1., None, None,
                       bag(thin) + oracle_tracks(thin, 250., 3, 1., None, None, rng), 7, 1))
    cases.append(_case('12x40_drw_m8_nu0.5', thin, 250., 8, .5, None, None,
                       bag(thin) + oracle_tracks(thin, 250., 8, .5, None, None, rng)))
    # the fields' corners, on 7 x 9 with walks that cover the whole interior
    nan_upd = upd.copy()
    nan_upd[3, 4] = np.nan
    flat = np.full(small, 5., dtype=np.float32)
    tiny = np.full(small, 1e-9)
    tiny[2:5, 3:6] = rng.uniform(0., 2e-6, (3, 3))
    tiny[1, 1] = -4.
    huge = np.zeros(small, dtype=np.float32)
    huge[3, 4], huge[3, 5], huge[2, 2] = 3e38, -3e38, np.inf
    walks = lambda: [walk(300, small, rng, rim=False), forward(200, small, rng), walk(65, small, rng)] + hand_made(small)
    cases.append(_case('nan_updraft', small, 0., 1, 1., nan_upd, pot, walks()))
    cases.append(_case('nan_updraft_alone_m2', small, 90., 2, 1., nan_upd, None, walks()))
    cases.append(_case('flat_potential', small, 0., 1, 1., upd, flat, walks()))
    cases.append(_case('flat_potential_d180_m3', small, 180., 3, 1., upd, flat, walks()))
    cases.append(_case('tiny_updraft', small, 0., 1, 1., tiny, pot, walks()))
    cases.append(_case('huge_potential', small, 0., 1, 1., upd, huge, walks()))
    cases.append(_case('huge_potential_nu0', small, 0., 2, 0., upd, huge, walks()))
    # G7's raster with the reference's own fields: a track across a block, the reference's tracks under a longer memory
    g = g7()
    ref_tracks = g7_case('ff_m1')[0]
    big = [forward(300, G7_SHAPE, rng), forward(65, G7_SHAPE, rng), walk(700, G7_SHAPE, rng)] + hand_made(G7_SHAPE) + ref_tracks[:6]
    cases.append(_case('g7_m1', G7_SHAPE, 0., 1, 1., g['updraft'], g['potential'], big, 0, 0))
    cases.append(_case('g7_m8', G7_SHAPE, 0., 8, 1., g['updraft'], g['potential'], big, 9, 2))
    cases.append(_case('g7_m3_nu2', G7_SHAPE, 0., 3, 2., g['updraft'], g['potential'], big[:4] + ref_tracks[6:9], 0, 1))
    return cases


_cases = None
_expected = {}


def cases():
    global _cases
    if _cases is None:
        _cases = _make_cases()
    return _cases


def case(name):
    (c,) = [c for c in cases() if c['name'] == name]
    return c


def case_names():
    return [c['name'] for c in cases()]


def expected(c, tracks=None):
    """score() of case c (cached), or of another list of tracks on the case's fields and parameters (not cached)."""
    if tracks is not None:
        return score(tracks, c['shape'], c['move_dirn'], c['memory'], c['nu'], c['updraft'], c['potential'])
    if c['name'] not in _expected:
        _expected[c['name']] = score(c['tracks'], c['shape'], c['move_dirn'], c['memory'], c['nu'], c['updraft'], c['potential'])
    return _expected[c['name']]


def flat(tracks, lead=0, tail=5):
    """(traj int16 (lead + points + tail, 2), offsets int64 (ntracks + 1,)): the tracks one after another behind `lead`
    points that belong to no track (so the first offset is `lead`), followed by `tail` more."""
    junk = lambda n: np.full((n, 2), 3, dtype=np.int16)
    traj = np.concatenate([junk(lead)] + [np.asarray(t, dtype=np.int16).reshape(-1, 2) for t in tracks] + [junk(tail)])
    offsets = lead + np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    return np.ascontiguousarray(traj), offsets


def s_bound_ok(got_rows, want_rows):
    """S within `scored` units of the expected sum: two correct log2 differ by a few ulp of a value <= 1075 * 2^32, whose ulp
    is 2^-10, so the rounded integer differs by at most 1 per SCORED move."""
    return bool((np.abs(got_rows[:, 0] - want_rows[:, 0]) <= want_rows[:, 1]).all())
