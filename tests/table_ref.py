"""Reference of the stepper's decision tables, state by state, from the oracle's own functions only
(oracle/ssrs_oracle.py: window_weights, get_track_restrictions, _move_probabilities, get_directional_probs and the cdf of
choose_index -- pinned by G6 / G7), the decoders of the tables' layouts, and the field recipes of the table tests.

A state is (interior cell, last move rc); rc is a ring position 0..7, the move itself k = RING_K[rc].  Per state:
  * the nine raw weights of the cell (window_weights);
  * its class: NONFINITE (some raw weight, the centre's included, is NaN or +-inf), else REVERSAL (the three admissible
    weights are all zero after the clip and so is the masked prior), else ZERO_ROW (... the masked prior is not), else
    ORDINARY; EDGE marks the cells of the raster's rim, which have no window;
  * the two boundaries B1 = cdf[ka] / cdf[8], B2 = cdf[kb] / cdf[8] (ka < kb < kc the admissible k) of the probabilities
    _move_probabilities returns for that state, for every class but NONFINITE; the nine boundaries of the unmasked prior
    for REVERSAL.

The stepper hands a lane to the exact sequence iff ufi - T in {-1, 0}, takes ufi - T >= 1 as "cdf <= u" and ufi - T <= -2
as "u < cdf", with ufi <= 2^N u < ufi + 1: every decision is the reference's iff T - 1 <= 2^N B <= T + 1 (`within_one`).
"""
import numpy as np

from oracle import ssrs_oracle as orc

RING_K = (7, 8, 5, 2, 1, 0, 3, 6)                       # ring position -> k
RING_OF_K = {k: c for c, k in enumerate(RING_K)}
MASKS = [[int(m) for m in orc.get_track_restrictions(*orc.NEIGHBOUR_DELTAS[k])] for k in RING_K]
ADMISSIBLE = [tuple(k for k in range(9) if MASKS[rc][k]) for rc in range(8)]       # (ka, kb, kc), ascending
EDGE, ORDINARY, ZERO_ROW, REVERSAL, NONFINITE = -1, 0, 1, 2, 3
CLASS_NAMES = {ORDINARY: 'ordinary', ZERO_ROW: 'zero_row', REVERSAL: 'reversal', NONFINITE: 'nonfinite'}
THR_POISON, THR_BOUNDARY, THR_REVERSAL = 0x0000FFFF, 0x0001FFFF, 0x0002FFFF

SHAPES = ((5, 5), (16, 64), (17, 65), (48, 129), (40, 200))
HEADINGS = (0, 90, 180, 270, 45, 225, 30, 200)
RECIPES = ('benign', 'two_phase', 'magnitudes', 'poison', 'half_way')


def prior_of(heading):
    return [float(v) for v in orc.get_directional_probs(heading * np.pi / 180.)]


def boundaries(p):
    """cdf[k] / cdf[8] of choose_index, k = 0..8."""
    cdf, acc = [], 0.0
    for v in p:
        acc = acc + v
        cdf.append(acc)
    return [c / cdf[-1] for c in cdf]


def pick(b3, u):
    """The interval of u among the boundaries of the three admissible cells: 0, 1 or 2 (searchsorted 'right')."""
    return (1 if b3[0] <= u else 0) + (1 if b3[1] <= u else 0)


class FieldRef:
    """What depends on the fields only: raw weights, NONFINITE cells, and the boundaries of the states whose three
    admissible weights are not all zero (the prior does not enter those: _move_probabilities reads it only where a
    weight is NaN or all masked weights are zero)."""

    def __init__(self, updraft, potential):
        self.updraft = np.ascontiguousarray(updraft, dtype=np.float64)
        self.potential = None if potential is None else np.ascontiguousarray(potential, dtype=np.float32)
        rows, cols = self.updraft.shape
        self.rows, self.cols = rows, cols
        self.interior = np.zeros((rows, cols), dtype=bool)
        self.interior[1:-1, 1:-1] = True
        self.w = np.full((rows, cols, 9), np.nan)
        self.b12 = np.full((rows, cols, 8, 2), np.nan)
        self.zero3 = np.zeros((rows, cols, 8), dtype=bool)          # finite cell, the three admissible weights all zero
        any_prior = prior_of(0.)
        with np.errstate(all='ignore'):
            for r in range(1, rows - 1):
                for c in range(1, cols - 1):
                    w = orc.window_weights(r, c, self.updraft, self.potential, None)
                    self.w[r, c] = w
                    if not all(v - v == 0. for v in w):
                        continue
                    for rc in range(8):
                        ka, kb, kc = ADMISSIBLE[rc]
                        if not (w[ka] > 0. or w[kb] > 0. or w[kc] > 0.):
                            self.zero3[r, c, rc] = True
                            continue
                        b = boundaries(orc._move_probabilities(w, any_prior, 1.0, MASKS[rc]))
                        self.b12[r, c, rc] = (b[ka], b[kb])
        self.nonfinite = self.interior & ~np.isfinite(self.w).all(axis=2)
        self.window_updraft_max = np.full((rows, cols), np.inf)
        u = self.updraft
        with np.errstate(all='ignore'):
            stack = [u[1 + dr:rows - 1 + dr, 1 + dc:cols - 1 + dc] for dr in (-1, 0, 1) for dc in (-1, 0, 1)]
            # NaN counts as "above every limit"
            self.window_updraft_max[1:-1, 1:-1] = np.where(np.isnan(stack).any(axis=0), np.inf, np.max(stack, axis=0))

    def clipped(self):
        """The nine weights clipped at 0 (the oracle's `v if v > 0. else 0.`; NaN stays out of it: see has_nan)."""
        return np.where(self.w > 0., self.w, 0.)

    def admissible_sum(self):
        """f64 sum of the three admissible clipped weights, np.cumsum's order: (rows, cols, 8)."""
        cw = self.clipped()
        out = np.zeros((self.rows, self.cols, 8))
        for rc in range(8):
            ka, kb, kc = ADMISSIBLE[rc]
            out[:, :, rc] = (cw[:, :, ka] + cw[:, :, kb]) + cw[:, :, kc]
        return out

    def span_over(self, ratio):
        """States whose positive admissible weights (two at least) span more than `ratio`: (rows, cols, 8) bool."""
        cw = self.clipped()
        out = np.zeros((self.rows, self.cols, 8), dtype=bool)
        for rc in range(8):
            w3 = cw[:, :, list(ADMISSIBLE[rc])]
            pos = w3 > 0.
            lo = np.where(pos, w3, np.inf).min(axis=2)
            hi = w3.max(axis=2)
            out[:, :, rc] = (pos.sum(axis=2) >= 2) & (hi > ratio * lo)
        return out & ~self.nonfinite[:, :, None] & self.interior[:, :, None]


class HeadingRef:
    """A field under one heading: classes and boundaries of every state, the priors' own boundaries."""

    def __init__(self, field, heading):
        self.field, self.heading = field, heading
        self.prior = prior_of(heading)
        f = field
        zeros = [0.] * 9
        self.reversal_mask = 0
        self.zero_b12 = np.full((8, 2), np.nan)
        for rc in range(8):
            ka, kb, kc = ADMISSIBLE[rc]
            if not any(self.prior[k] != 0. for k in (ka, kb, kc)):
                self.reversal_mask |= 1 << rc
                continue
            b = boundaries(orc._move_probabilities(zeros, self.prior, 1.0, MASKS[rc]))
            self.zero_b12[rc] = (b[ka], b[kb])
        # the unmasked prior (:239-240): what a state gets whose weights and masked prior are all zero
        self.rev9 = np.array(boundaries(orc._move_probabilities(zeros, self.prior, 1.0, [0] * 9)))
        support = {k for k in range(9) if k != 4 and self.prior[k] != 0.}
        cand = [rh for rh in range(8) if support and support <= set(ADMISSIBLE[rh])]
        self.rev_ok = 1 if cand else 0
        self.rev_rc = cand[0] if cand else 0
        self.rev_b12 = (self.rev9[ADMISSIBLE[self.rev_rc][0]], self.rev9[ADMISSIBLE[self.rev_rc][1]]) if cand else None

        rev_rc_mask = np.array([(self.reversal_mask >> rc) & 1 for rc in range(8)], dtype=bool)
        self.cls = np.full((f.rows, f.cols, 8), EDGE, dtype=np.int8)
        self.cls[f.interior] = ORDINARY
        self.cls[f.zero3 & ~rev_rc_mask] = ZERO_ROW
        self.cls[f.zero3 & rev_rc_mask] = REVERSAL
        self.cls[f.nonfinite] = NONFINITE
        self.b12 = f.b12.copy()
        zr = self.cls == ZERO_ROW
        for rc in range(8):
            self.b12[:, :, rc][zr[:, :, rc]] = self.zero_b12[rc]

    def counts(self):
        return {name: int((self.cls == c).sum()) for c, name in CLASS_NAMES.items()}


def within_one(t, b, nbits):
    """T - 1 <= 2^N B <= T + 1, exactly: 2^N B, T - 1 and T + 1 are all exact in f64 (N <= 32)."""
    x = np.asarray(b, dtype=np.float64) * float(1 << nbits)
    t = np.asarray(t).astype(np.float64)
    return (t - 1. <= x) & (x <= t + 1.)


def margin(t, b, nbits):
    """|T - 2^N B| over the entries below the clamp (the clamp satisfies the condition on its own); 0 if none."""
    t = np.asarray(t).astype(np.float64).ravel()
    x = (np.asarray(b, dtype=np.float64) * float(1 << nbits)).ravel()
    keep = t < float((1 << nbits) - 1)
    return float(np.abs(t[keep] - x[keep]).max()) if keep.any() else 0.


# ---------------------------------------------------------------------------------------------- decoders
def thr_layout(rows, cols):
    """(guard bytes, plane shift) of the threshold table."""
    guard = -(-(cols + 2) * 4 // 256) * 256
    shift = 8
    while (1 << shift) < rows * cols * 4:
        shift += 1
    return guard, shift


def thr_decode(table, rows, cols):
    """int32 / uint32 buffer of ssrs_transition_thr_build -> (header dict, planes uint32 (8, rows, cols))."""
    raw = np.ascontiguousarray(table).view(np.uint8)
    guard, shift = thr_layout(rows, cols)
    assert raw.size == (8 << shift) + 2 * guard
    planes = np.stack([raw[guard + (rc << shift):guard + (rc << shift) + rows * cols * 4].view(np.uint32).reshape(rows, cols)
                       for rc in range(8)])
    header = {'magic': raw[:8].tobytes(), 'rows': int(raw[8:12].view(np.int32)[0]), 'cols': int(raw[12:16].view(np.int32)[0]),
              'prior': raw[16:88].view(np.float64).copy()}
    return header, planes


def ring_decode(table, rows, cols):
    """float32 buffer of ssrs_transition_ring_build -> (records f32 (rows, cols, 10): ring 7, 0, 1, ..., 7, 0; mask bytes)."""
    raw = np.ascontiguousarray(table).view(np.uint8)
    n = rows * cols
    records = raw[:n * 40].view(np.float32).reshape(rows, cols, 10)
    mask = raw[n * 40 + 8:n * 40 + 8 + n].reshape(rows, cols)
    return records, mask


def pair_expected(planes, rev_ok, rev_rc, rev_e):
    """The pair table by its successor rule, from the threshold planes: uint32 (rows, cols, 8, 4) = e0, ea, eb, ec."""
    _, rows, cols = planes.shape
    out = np.full((rows, cols, 8, 4), THR_POISON, dtype=np.uint32)
    for rc in range(8):
        e0 = planes[rc]
        out[:, :, rc, 0] = e0
        rev = (e0 == THR_REVERSAL) if rev_ok else np.zeros_like(e0, dtype=bool)
        for sel, rcd in ((~rev, rc), (rev, rev_rc)):
            eu = np.where(rev, np.uint32(rev_e), e0)
            live = sel & ((eu & 0xFFFF) <= (eu >> 16))
            rr, cc = np.nonzero(live)
            assert ((rr > 0) & (rr < rows - 1) & (cc > 0) & (cc < cols - 1)).all(), 'a rim cell without a flag'
            for j, k in enumerate(ADMISSIBLE[rcd]):
                dr, dc = orc.NEIGHBOUR_DELTAS[k]
                out[rr, cc, rc, 1 + j] = planes[RING_OF_K[k], rr + dr, cc + dc]
    return out


def prior_words_decode(words):
    w = [int(v) for v in words]
    assert len(w) == 38
    return {'zero_e': w[0:8], 'reversal': w[8], 'thr9': w[9:18], 'rev_ok': w[18], 'rev_rc': w[19], 'rev_e': w[20],
            'zero_t1': w[21:29], 'zero_t2': w[29:37], 'fine_reversal': w[37]}


# ---------------------------------------------------------------------------------------------- field recipes
# half-way: 2^16 B1 = m + 0.5 exactly for these m (and the ends of the range), then B1 = 0, 1/3, 2/3, 1 - 2^-17
HALF_WAY_M = (0, 1, 2, 3, 100, 1000, 12345, 32767, 32768, 40001, 65534, 65535)
HALF_WAY_EAST_NORTH = tuple((2 * m + 1, 131072 - 2 * m - 1) for m in HALF_WAY_M) + ((0, 7), (1, 2), (2, 1), (131071, 1))


def make_field(recipe, shape, seed=0):
    """(updraft f64, potential f32) of a recipe on a shape; fixed seeds."""
    rows, cols = shape
    rng = np.random.default_rng(1000 * RECIPES.index(recipe) + 7 * rows + cols + seed)
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    if recipe == 'benign':
        upd = np.clip(rng.lognormal(0., 1., shape), 0.05, 8.)
        pot = (1000. - 3. * rr + 0.5 * cc + rng.normal(0., 2., shape)).astype(np.float32)
    elif recipe == 'two_phase':
        upd = np.where(rng.random(shape) < 0.5, 0., rng.uniform(0.5, 3., shape))
        # plateaus of 3 x 4 cells, their levels a ramp with noise, and a few single cells off their plateau
        level = 500. - 2. * (rr // 3) + 1. * (cc // 4) + rng.integers(0, 3, (rows // 3 + 1, cols // 4 + 1))[rr // 3, cc // 4]
        pot = (level + np.where(rng.random(shape) < 0.1, rng.normal(0., 1., shape), 0.)).astype(np.float32)
    elif recipe == 'magnitudes':
        upd = 10. ** rng.uniform(-9., 19., shape)
        # differences from f32-denormal to 1e3: each cell a sum of steps of very different sizes
        scale = 10. ** rng.choice([-42., -40., -30., -10., -3., 0., 1., 3.], shape)
        pot = (rng.integers(-1, 2, shape) * scale).astype(np.float32)
        pot[rng.random(shape) < 0.2] = 0.
    elif recipe == 'poison':
        upd = np.clip(rng.lognormal(0., 1., shape), 0.05, 8.)
        pot = (300. - 1.5 * rr + 0.7 * cc + rng.normal(0., 2., shape)).astype(np.float32)
        kinds = rng.integers(0, 140, shape)          # 1 cell in 20 is special, seven kinds
        upd[kinds == 0] = np.nan
        pot[kinds == 1] = np.nan
        upd[kinds == 2] = np.inf
        pot[kinds == 3] = -np.inf
        upd[kinds == 4] = 1e21
        upd[kinds == 5] = 1e39
        upd[kinds == 6] = -2.5
        # (the smallest raster too: two rim corners, each in the window of one interior cell)
        upd[0, 0] = np.nan
        pot[rows - 1, cols - 1] = -np.inf
    elif recipe == 'half_way':
        upd = np.ones(shape)
        pot = np.full(shape, 200000., dtype=np.float32)
        n = 0
        for r in range(1, rows - 1, 3):
            for c in range(1, cols - 1, 3):
                east, north = HALF_WAY_EAST_NORTH[n % len(HALF_WAY_EAST_NORTH)]
                n += 1
                # after a move north-east (rc 1) the candidates are east (ka = 5), north (kb = 7) and north-east (kc = 8,
                # weight 0: same level): B1 = east / (east + north)
                pot[r, c + 1] = 200000. - east
                pot[r + 1, c] = 200000. - north
    else:
        raise ValueError(recipe)
    return upd, pot


_cache = {}


def field_ref(recipe, shape, with_potential=True):
    key = (recipe, tuple(shape), bool(with_potential))
    if key not in _cache:
        upd, pot = make_field(recipe, shape)
        _cache[key] = FieldRef(upd, pot if with_potential else None)
    return _cache[key]


def heading_ref(recipe, shape, heading, with_potential=True):
    key = (recipe, tuple(shape), bool(with_potential), heading)
    if key not in _cache:
        _cache[key] = HeadingRef(field_ref(recipe, shape, with_potential), heading)
    return _cache[key]
