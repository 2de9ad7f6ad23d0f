"""K22's expected values: rows[t, a, b, :] of include/ssrs_score_profile.h is score_ref.score's row for memories[a] and
nus[b], so the expected profile is that function looped over the grid.  A plain helper module of the tests of K22 (host,
emulation and device); importing it needs no GPU.  What it returns is cached per process and must not be changed."""
import numpy as np

import score_ref as ref

# the grids of the CPU build's tests: a walk that stops at 1, 2, 3 and goes on to 8; the deepest memory alone; repeated and
# unordered nus with 0 (every cell 1 / 9), 1 (no pow) and both sides of 1
GRIDS = (((1, 2, 3, 8), (0., 1., .5, 2., 1.)), ((8,), (1.,)), ((2, 5), (3.7, .5, 1.)), ((1,), (0., 1.)))
# the grid of the device's tests
DEVICE_GRID = ((1, 2, 3, 5, 8), (0., .5, 1., 2., 1., 3.7))

_rows = {}


def one(c, memory, nu, tracks=None):
    """score_ref.score's rows (ntracks, 6) of case c's fields and heading under (memory, nu); cached for its own tracks."""
    if tracks is not None:
        return ref.score(tracks, c['shape'], c['move_dirn'], memory, nu, c['updraft'], c['potential'])['rows']
    key = (c['name'], int(memory), float(nu))
    if key not in _rows:
        _rows[key] = ref.score(c['tracks'], c['shape'], c['move_dirn'], memory, nu, c['updraft'], c['potential'])['rows']
    return _rows[key]


def expected(c, memories, nus, tracks=None):
    """int64 (ntracks, nmem, nnu, 6)."""
    with np.errstate(all='ignore'):
        return np.stack([np.stack([one(c, m, nu, tracks) for nu in nus], 1) for m in memories], 1)


def check(got, want):
    """The five counts exactly; S within one unit per SCORED move (score_ref.s_bound_ok, derived in K21)."""
    assert got.shape == want.shape and got.dtype == np.int64
    assert np.array_equal(got[..., 1:], want[..., 1:])
    assert ref.s_bound_ok(got.reshape(-1, 6), want.reshape(-1, 6))
