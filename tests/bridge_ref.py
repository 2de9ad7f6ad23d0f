"""K23's expected values: the definition of include/ssrs_bridge.h in Python, on the oracle's own functions
(oracle/ssrs_oracle.py: window_weights, get_track_restrictions, _move_probabilities), and the cases that
tests/test_bridge_emulation.py runs on the CPU build of bridge.hip and tests/test_gpu_bridge.py on the device.

The propagation here is UNCONFINED: a dictionary of the occupied states over the whole raster, with no window and no test of
what can still reach B.  A plain helper module; importing it needs no GPU.  expected(case) is computed once per process and
must not be changed by its users."""
import numpy as np

import score_ref as sref
from score_ref import orc

SCORED, ZERO, TOO_LONG, OUT, UNDEFINED = range(5)
MAX_MOVES = 32
DELTAS = [(k // 3 - 1, k % 3 - 1) for k in range(9)]
# the device's pow against the host's: K21's own bound (tests/test_gpu_score.py RTOL_NU, DESIGN.md limit 20 (viii)); one
# product and at most eight additions of non-negative terms per step round 10 times, half an ulp each at the most
RTOL_POW = 3.35e-15
RTOL_STEP = RTOL_POW + 10 * 2. ** -53


def bound(n):
    """The relative bound on g, arrivals and P after n steps for nu outside {0, 1}."""
    return n * RTOL_STEP


def state_of(d):
    return 3 * (int(d[0]) + 1) + (int(d[1]) + 1)


def sum9(x):
    return (((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))) + x[8]


class Model:
    """One case's probabilities p(y, d)[9], cached per (cell, state), and its forward passes, cached per (A, s)."""

    def __init__(self, c):
        self.shape, self.nu = c['shape'], float(c['nu'])
        self.updraft, self.potential = c['updraft'], c['potential']
        self.prior = sref.prior_of(c['move_dirn'])
        self._masks = [[int(m) for m in orc.get_track_restrictions(0, 0) & orc.get_track_restrictions(*d)] for d in DELTAS]
        self._p, self._w, self._passes = {}, {}, {}

    def p(self, r, c, d):
        key = (r, c, d)
        if key not in self._p:
            with np.errstate(all='ignore'):
                if (r, c) not in self._w:
                    self._w[(r, c)] = orc.window_weights(r, c, self.updraft, self.potential, self.prior)
                self._p[key] = [float(v) for v in orc._move_probabilities(self._w[(r, c)], self.prior, self.nu, self._masks[d])]
        return self._p[key]

    def step(self, alpha):
        """alpha_t -> alpha_{t+1}; both {cell: [9 values by last move]}, cells with no non-zero value left out."""
        rows, cols = self.shape
        new = {}
        for (r, c), states in alpha.items():
            if not (0 < r < rows - 1 and 0 < c < cols - 1):
                continue                                   # a rim cell emits nothing
            acc = [0.0] * 9
            for d in range(9):                             # ascending, sequentially, from 0.0
                a = states[d]
                if a == 0.0:
                    continue
                q = self.p(r, c, d)
                for k in range(9):
                    acc[k] = acc[k] + a * q[k]
            for k in range(9):
                if acc[k] != 0.0:                          # (a NaN stays)
                    x = (r + DELTAS[k][0], c + DELTAS[k][1])
                    if x not in new:
                        new[x] = [0.0] * 9
                    new[x][k] = acc[k]                     # (x, k) has the one source cell x - delta_k
        return new

    def forward(self, a, s, n):
        """[alpha_0, ..., alpha_n] from state (a, s); a longer pass from the same state is extended, not repeated."""
        passes = self._passes.setdefault((a, s), [{a: [1.0 if k == s else 0.0 for k in range(9)]}])
        while len(passes) <= n:
            passes.append(self.step(passes[-1]))
        return passes

    def job(self, job):
        """(g [9], status, P, arrivals [32]) of one job (row_a, col_a, incoming, row_b, col_b, moves)."""
        ra, ca, s, rb, cb, n = (int(v) for v in job)
        rows, cols = self.shape
        zeros = ([0.0] * 9, 0.0, [0.0] * MAX_MOVES)
        if not 1 <= n <= MAX_MOVES:
            return zeros[0], TOO_LONG, zeros[1], zeros[2]
        if not (0 < ra < rows - 1 and 0 < ca < cols - 1) or not (0 <= rb < rows and 0 <= cb < cols) or not 0 <= s <= 8:
            return zeros[0], OUT, zeros[1], zeros[2]
        passes = self.forward((ra, ca), s, n)
        at_b = [passes[t].get((rb, cb), [0.0] * 9) for t in range(1, n + 1)]
        arrivals = [sum9(v) for v in at_b] + [0.0] * (MAX_MOVES - n)
        g, P = list(at_b[-1]), arrivals[n - 1]
        status = ZERO if P == 0. else (SCORED if (P > 0. and P < np.inf) else UNDEFINED)
        return g, status, P, arrivals


def score(c, jobs=None):
    """The whole result of one call on case c: g f64 (m, 9), status uint8, p f64, surprisal int64, arrivals f64 (m, 32)."""
    jobs = c['jobs'] if jobs is None else np.asarray(jobs).reshape(-1, 6)
    model = Model(c)
    m = len(jobs)
    out = dict(g=np.zeros((m, 9)), status=np.zeros(m, dtype=np.uint8), p=np.zeros(m), surprisal=np.zeros(m, dtype=np.int64),
               arrivals=np.zeros((m, MAX_MOVES)))
    for i, job in enumerate(jobs):
        g, status, P, arrivals = model.job(job)
        out['g'][i], out['status'][i], out['p'][i], out['arrivals'][i] = g, status, P, arrivals
        if status == SCORED:
            out['surprisal'][i] = max(sref.surprisal(P), 0)
    return out


# ------------------------------------------------------------------------------------------------ where the gaps come from
def thinned(track, every, skip, true_incoming):
    """The jobs of one 8-connected track from point `skip` on (past the burn-in relocation), every `every`-th point and the
    last kept as fixes, with the true number of moves between them: reachable by construction.  The incoming state is the
    move that really arrived at the fix (true_incoming) or 4, which allows more."""
    pts = [(int(r), int(c)) for r, c in track][skip:]
    idx = list(range(0, len(pts), every))
    if len(pts) and idx[-1] != len(pts) - 1:
        idx.append(len(pts) - 1)
    jobs = []
    for i0, i1 in zip(idx[:-1], idx[1:]):
        s = 4
        if true_incoming and i0 > 0:
            s = state_of((pts[i0][0] - pts[i0 - 1][0], pts[i0][1] - pts[i0 - 1][1]))
        jobs.append(pts[i0] + (s,) + pts[i1] + (i1 - i0,))
    return jobs


def thinned_tracks(tracks, everies, shape):
    skip = int(min(shape) / 10) + 1                        # the first point whose move is not relocated
    jobs = []
    for t, track in enumerate(tracks):
        for e, every in enumerate(everies):
            jobs += thinned(track, every, skip, (t + e) % 2 == 0)
    return jobs


def planted(shape):
    """The hand-made jobs of every case: the refusals in their order, unreachable pairs, B on the rim, every incoming
    state, windows that the rim clips."""
    rows, cols = shape
    r, c = rows // 2, cols // 2
    jobs = [
        # TOO_LONG whatever else the job holds: nothing else of it is read
        (r, c, 4, r, c + 1, 0), (r, c, 4, r, c + 1, 33), (-7, 10 ** 6, 99, -1, -1, -5), (r, c, 4, r, c, 100), (0, 0, 4, 0, 0, 2 ** 31 - 1),
        # OUT: A on the rim or outside, B outside the raster, incoming outside 0..8
        (0, c, 4, 1, c, 1), (r, 0, 4, r, 1, 2), (rows - 1, c, 4, rows - 2, c, 1), (r, cols - 1, 4, r, cols - 2, 3),
        (-1, c, 4, 1, c, 2), (r, cols, 4, r, cols - 2, 2),
        (r, c, 4, -1, c, 32), (r, c, 4, rows, c, 32), (r, c, 4, r, -1, 32), (r, c, 4, r, cols, 32), (r, c, -1, r, c + 1, 1), (r, c, 9, r, c + 1, 1),
        # ZERO: further apart than n moves reach; one move too few; a rest under a model that never rests (nu != 0)
        (1, 1, 4, rows - 2, cols - 2, 3), (r, c, 4, r + 2, c + 2, 1), (r, c, 4, r, c, 1), (1, 1, 4, 1, cols - 1, cols - 3),
        # B on the rim and in the corners
        (2, c, 4, 0, c, 2), (2, c, 4, 0, c + 1, 4), (r, 2, 4, r + 1, 0, 3), (rows - 3, cols - 3, 4, rows - 1, cols - 1, 2),
        (rows - 3, cols - 3, 4, rows - 1, cols - 1, 5), (2, 2, 4, 0, 0, 2), (2, 2, 4, 0, 0, 6),
    ]
    # every incoming state into windows that the rim of a 7 x 9 raster clips on every side (n >= 4 around its centre)
    jobs += [(r, c, s, r, c + 1, 4) for s in range(9)] + [(r, c, s, r + 1, c, 6) for s in range(9)]
    jobs += [(r, c, s, r + DELTAS[s][0], c + DELTAS[s][1], 1) for s in range(9)]
    jobs += [(r, c, 4, r + 1, c - 1, n) for n in (1, 2, 3, 5, 7, 8, 12, 31, 32)]
    return jobs


def _case(name, shape, move_dirn, nu, updraft, potential, jobs):
    jobs = np.array(jobs, dtype=np.int64).reshape(-1, 6)
    assert np.abs(jobs).max() < 2 ** 31
    return dict(name=name, shape=shape, move_dirn=float(move_dirn), nu=float(nu), updraft=updraft, potential=potential,
                jobs=np.ascontiguousarray(jobs, dtype=np.int32))


def _make_cases():
    rng = np.random.default_rng(2323)
    cases = []
    small, thin = (7, 9), (12, 40)
    upd, pot = sref.fields(small, rng)
    for nu in (1., 0., .5, 2.):
        tracks = sref.oracle_tracks(small, 0., 1, nu, upd, pot, rng)
        cases.append(_case(f'7x9_nu{nu:g}', small, 0., nu, upd, pot, planted(small) + thinned_tracks(tracks, (2, 5), small)))
    upd2, pot2 = sref.fields(thin, rng)
    for name, dirn, nu, u, p in (('12x40_upd', 135., 1., upd2, None), ('12x40_drw_d0', 0., 1., None, None),
                                 ('12x40_drw_d250_nu0.5', 250., .5, None, None), ('12x40_ff_nu2', 0., 2., upd2, pot2),
                                 ('12x40_ff_nu0', 0., 0., upd2, pot2)):
        tracks = sref.oracle_tracks(thin, dirn, 1, nu, u, p, rng)
        everies = (5, 16) if nu == 0. else (2, 5, 16, 32)
        cases.append(_case(name, thin, dirn, nu, u, p, planted(thin)[:40] + thinned_tracks(tracks, everies, thin)))
    # G7's raster with the reference's own fields and tracks: n = 32 in a 33 x 33 window that the rim does not clip
    g = sref.g7()
    ref_tracks = sref.g7_case('ff_m1')[0]
    # (rows 26..58 x columns 49..81 and 47..79; the third returns to its start, which this model does not do; the fourth's
    # window is 17 x 33)
    wide = [(30, 64, 4, 54, 66, 32), (30, 64, 7, 56, 62, 32), (48, 64, 4, 48, 64, 32), (40, 30, 4, 56, 30, 32)]
    cases.append(_case('g7_nu1', sref.G7_SHAPE, 0., 1., g['updraft'], g['potential'],
                       wide + planted(sref.G7_SHAPE)[:21] + thinned_tracks(ref_tracks[:6], (16, 32), sref.G7_SHAPE)))
    cases.append(_case('g7_nu0.5', sref.G7_SHAPE, 0., .5, g['updraft'], g['potential'],
                       wide[:2] + thinned_tracks(ref_tracks[6:9], (16, 32), sref.G7_SHAPE)))
    # nu = 0 occupies the whole window: two gaps of 32 moves from one state (one forward pass here), one short one
    cases.append(_case('g7_nu0', sref.G7_SHAPE, 0., 0., g['updraft'], g['potential'],
                       wide[:1] + [(30, 64, 4, 42, 50, 32), (30, 64, 4, 32, 66, 4)]))
    # score_ref's huge potential (inf and +-3e38 beside the raster's centre): NaN probabilities, UNDEFINED gaps
    huge = sref.case('huge_potential')
    around = [(r, c, 4, r + dr, c + dc, n) for r in (2, 3, 4) for c in (2, 3, 4, 5, 6)
              for dr, dc, n in ((0, 1, 1), (1, 0, 1), (1, 1, 2), (2, 1, 3), (0, 0, 3), (-1, 0, 4))]
    cases.append(_case('huge_potential', small, 0., 1., huge['updraft'], huge['potential'], around))
    cases.append(_case('huge_potential_nu0', small, 0., 0., huge['updraft'], huge['potential'], around[::3]))
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


def expected(c):
    """score(c), cached."""
    if c['name'] not in _expected:
        _expected[c['name']] = score(c)
    return _expected[c['name']]


# ------------------------------------------------------------------------------------------------ the comparison
def same_bits(got, want):
    """Equal bit for bit; a NaN equals a NaN, whatever its sign and payload."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def check(c, got, want, jobs=None, say=None):
    """got against want, both dicts like score()'s (arrivals may be None in got): statuses equal; g, arrivals and P bit-equal
    at nu in {0, 1} and within bound(n) elsewhere; the surprisal equal, or within 1 + bound * 2^32 / ln 2."""
    jobs = c['jobs'] if jobs is None else jobs
    assert np.array_equal(got['status'], want['status'])
    n = jobs[:, 5].astype(np.float64)
    exact = c['nu'] in (0., 1.)
    evaluated = np.isin(want['status'], (SCORED, ZERO, UNDEFINED))
    tol = np.where(evaluated, bound(np.clip(n, 1, MAX_MOVES)), 0.)
    fields = [('g', got['g'], want['g'])]
    if got.get('arrivals') is not None:
        fields.append(('arrivals', got['arrivals'], want['arrivals']))
        last = got['arrivals'][np.arange(len(jobs)), np.clip(jobs[:, 5], 1, MAX_MOVES) - 1]
        assert same_bits(last[evaluated], sum9(got['g'].T)[evaluated]), 'arrivals[n - 1] is P bit for bit'
    for name, a, b in fields:
        if exact:
            assert same_bits(a, b), f'{name} is bit-equal for nu in {{0, 1}}'
            continue
        # (a gap that ends ZERO may have passed B earlier: its arrivals carry the same differences as a SCORED one's)
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        with np.errstate(invalid='ignore', divide='ignore'):
            rel = np.where(same, 0., np.where(b != 0., np.abs(a - b) / np.abs(b), np.inf))
        if say is not None and evaluated.any():
            say(f"{c['name']}: {name}: largest relative difference / bound {np.max(rel[evaluated] / tol[evaluated][:, None]):.3f}")
        assert (rel <= tol[:, None]).all(), name
    ds = np.abs(got['surprisal'] - want['surprisal'])
    if exact:
        assert (ds <= 1).all()                             # (two correct log2 of one P: score_ref.s_bound_ok's argument)
    else:
        assert (ds <= 1 + tol * 2. ** 32 / np.log(2.)).all()
    assert not got['surprisal'][want['status'] != SCORED].any()
