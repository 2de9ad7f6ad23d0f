"""tests/table_ref.py checks itself: its boundaries pick what the oracle's choose_index picks, and every field recipe of
the table tests has the states it is there for (so that tests/test_gpu_tables.py cannot pass on an empty class)."""
import numpy as np
import pytest

import table_ref as tr
from oracle import ssrs_oracle as orc

FLOOR_SHAPE = (40, 200)


@pytest.mark.parametrize('recipe,heading', [('two_phase', 0), ('half_way', 30)])
def test_boundaries_pick_what_choose_index_picks(recipe, heading):
    """Every state of a 17 x 65 field, six probes per state (each boundary and its two f64 neighbours): the interval B1, B2
    select is the cell choose_index selects from the probabilities the oracle computes for THAT state with the heading's
    own prior (FieldRef computes the ordinary states once per field with another heading's prior: this pins that too)."""
    h = tr.heading_ref(recipe, (17, 65), heading)
    f = h.field
    seen = {c: 0 for c in tr.CLASS_NAMES}
    for r in range(1, f.rows - 1):
        for c in range(1, f.cols - 1):
            w = [float(v) for v in f.w[r, c]]
            for rc in range(8):
                cls = int(h.cls[r, c, rc])
                seen[cls] += 1
                if cls == tr.NONFINITE:
                    continue
                p = orc._move_probabilities(w, h.prior, 1.0, tr.MASKS[rc])
                if cls == tr.REVERSAL:
                    bs = list(h.rev9)
                else:
                    bs = [float(v) for v in h.b12[r, c, rc]]
                    assert bs[0] <= bs[1]
                for b in bs:
                    for u in (np.nextafter(b, -1.), b, np.nextafter(b, 2.)):
                        if not 0. <= u < 1.:
                            continue
                        want = orc.choose_index(p, float(u))
                        if cls == tr.REVERSAL:
                            got = sum(1 for x in bs if x <= u)
                        else:
                            got = tr.ADMISSIBLE[rc][tr.pick(bs, u)]
                        assert got == want, (r, c, rc, cls, u, bs)
    assert seen[tr.ORDINARY] > 1000 and seen[tr.ZERO_ROW] > 100 and seen[tr.REVERSAL] > 0


def test_ring_geometry_is_the_oracles():
    for rc, k in enumerate(tr.RING_K):
        dr, dc = orc.NEIGHBOUR_DELTAS[k]
        # the three admissible cells are the ring neighbours of the move
        assert set(tr.ADMISSIBLE[rc]) == {tr.RING_K[(rc + 7) % 8], k, tr.RING_K[(rc + 1) % 8]}
        assert (dr, dc) != (0, 0) and tr.ADMISSIBLE[rc] == tuple(sorted(tr.ADMISSIBLE[rc]))


def test_axis_and_diagonal_headings_reverse_into_a_row():
    f = tr.field_ref('benign', (5, 5))
    for heading in tr.HEADINGS:
        h = tr.HeadingRef(f, heading)
        assert h.rev_ok == (0 if heading in (30, 200) else 1), heading
        # a lobe of n adjacent cells misses the 8 - n - 2 arcs of three that lie wholly outside it
        lobe = sum(1 for v in h.prior if v != 0.)
        assert lobe in (3, 4) and bin(h.reversal_mask).count('1') == 8 - lobe - 2


def _floor_refs(recipe, with_potential=True):
    return [tr.heading_ref(recipe, FLOOR_SHAPE, heading, with_potential) for heading in (0, 180, 30)]


def test_floor_benign():
    """Without a potential every weight is a positive harmonic mean: every state is ordinary.  With one, a last move
    against the gradient leaves three weights that the clip makes zero -- a quarter of all states even for pure noise
    (the centre below all three of its candidates) --, so >= 95 % ordinary is out of any potential's reach; there the
    floor is half of the states (the arcs on the downhill side of the ramp) and no poison."""
    for h in _floor_refs('benign', with_potential=False):
        n = h.counts()
        total = int(h.field.interior.sum()) * 8
        assert n['ordinary'] >= 0.95 * total and n['nonfinite'] == 0, n
    for h in _floor_refs('benign'):
        n = h.counts()
        total = int(h.field.interior.sum()) * 8
        assert n['ordinary'] >= 0.5 * total and n['nonfinite'] == 0, n


def test_floor_two_phase():
    for h in _floor_refs('two_phase'):
        n = h.counts()
        assert n['zero_row'] >= 200 and n['reversal'] >= 50, (h.heading, n)
        # exact zero weights next to positive ones (equal neighbours), not only whole zero rows
        cw = h.field.clipped()
        mixed = sum(int(((cw[:, :, list(tr.ADMISSIBLE[rc])] == 0.).any(axis=2) & (h.cls[:, :, rc] == tr.ORDINARY)).sum())
                    for rc in range(8))
        assert mixed >= 200


def test_floor_magnitudes():
    for h in _floor_refs('magnitudes'):
        wide = h.field.span_over(1e6) & (h.cls == tr.ORDINARY)
        assert int(wide.sum()) >= 500, int(wide.sum())
    f = tr.field_ref('magnitudes', FLOOR_SHAPE)
    d = np.abs(np.diff(f.potential.astype(np.float64), axis=1))
    assert ((d > 0) & (d < 1.1754944e-38)).sum() >= 20 and d.max() >= 1e3      # f32-denormal differences, and large ones
    assert f.updraft.min() < 1e-8 and 1e18 < f.updraft.max() <= 1e19


def test_floor_poison():
    for h in _floor_refs('poison'):
        n = h.counts()
        assert n['nonfinite'] >= 100, n
        clean = h.field.interior & ~h.field.nonfinite
        assert int(clean.sum()) >= 100
    f = tr.field_ref('poison', FLOOR_SHAPE)
    u, p = f.updraft, f.potential
    for present in (np.isnan(u).any(), np.isnan(p).any(), np.isposinf(u).any(), np.isneginf(p).any(), (u == 1e21).any(),
                    (u == 1e39).any(), (u < 0).any()):
        assert present
    # cells whose weights are finite in f64 although an updraft of their window is beyond the f32 builder's range
    assert int((f.interior & ~f.nonfinite & (f.window_updraft_max > 1e20)).sum()) >= 20


def test_floor_half_way():
    h = tr.heading_ref('half_way', FLOOR_SHAPE, 0)
    x = h.b12[:, :, 1, 0][h.cls[:, :, 1] == tr.ORDINARY] * 65536.        # after a move north-east; exact in f64
    halves = {int(v) for v in x if v - np.floor(v) == 0.5}
    assert halves >= set(tr.HALF_WAY_M), sorted(set(tr.HALF_WAY_M) - halves)
    b1 = set(h.b12[:, :, 1, 0][h.cls[:, :, 1] == tr.ORDINARY].tolist())
    for want in (0., 1. / 3., 2. / 3., 1. - 2. ** -17):
        assert want in b1, want


def test_small_shapes_keep_some_of_each_class():
    """The 5 x 5 raster has nine interior cells: each recipe still has what it is about there."""
    assert tr.heading_ref('two_phase', (5, 5), 0).counts()['zero_row'] > 0
    n = tr.heading_ref('poison', (5, 5), 0).counts()
    assert n['nonfinite'] > 0 and n['ordinary'] > 0, n
    assert tr.heading_ref('half_way', (5, 5), 0).b12[1, 1, 1, 0] * 65536. == 0.5
