"""The case table of fixture G16 (tests/golden/g16_potential_shapes.npz), the recipes of its media and
the CPU-side assembly of the potential solver's linear system from the oracle's pieces and scipy.
Shared by tests/golden/generate_g16_potential_shapes.py, tests/test_potential_shapes_host.py and
tests/test_gpu_potential_shapes.py; nothing here touches the device or the reference.

Shapes: the ABI minimum is 3 x 3; one wave of the fused level-0 cycle handles 62 columns, one block
248; level 1 is built from (rows + 1) / 2 x (cols + 1) / 2 blocks, so odd rows and odd columns leave
half-empty blocks on the north and east edges."""
from collections import namedtuple
from math import sqrt

import numpy as np

SMALL_SHAPES = ((3, 3), (3, 7), (7, 3), (4, 5), (5, 5), (9, 61), (9, 62), (10, 63))
LARGER_SHAPES = ((7, 247), (8, 248), (11, 249), (33, 31), (31, 33), (65, 97), (3, 250), (251, 3))
SHAPES = SMALL_SHAPES + LARGER_SHAPES
HEADINGS = (0., 45., 90., 135., 180., 225., 270., 315., 30., 120., 200., 290., -45., 359.9)
# The larger shapes: one cardinal heading (0, the heading of Simulator and of the benchmark, on the widths
# around the block edge) and one oblique heading from every quadrant; the largest shape does without
# the cardinal one (the fixture's size).  On a raster three cells thin the east-edge quirk shows only
# where the field has a gradient at the east end, hence 180 and 359.9 on 3 x 250.
LARGER_HEADINGS = {
    (7, 247): (0., 45., 135., 225., 315.),
    (8, 248): (0., 30., 120., 200., 290.),
    (11, 249): (0., 45., 135., 225., -45.),
    (33, 31): (90., 30., 120., 200., 359.9),
    (31, 33): (180., 45., 135., 225., 315.),
    (65, 97): (30., 120., 200., 290.),
    (3, 250): (180., 45., 135., 225., 359.9),
    (251, 3): (270., 30., 120., 200., -45.),
}
MEDIA = ('uniform', 'alldead', 'live', 'speckle50', 'speckle70', 'block', 'barrier_row', 'barrier_col', 'island')
SMOOTH_MEDIA = ('uniform', 'alldead', 'live', 'barrier_row', 'barrier_col')
# slots that do not take the medium of the rotation: 3 x 250 would otherwise have no non-uniform medium
# at a heading that leaves a gradient at its east end (condition (a) of the fixture); a slot where the
# refinement behind the exact solution does not converge (condition (c)) would be listed here too
_MEDIUM_OVERRIDES = {((3, 250), 180.): 'live'}
# per shape the heading of the case that shows the reference's east-edge quirk (condition (a)); the
# per-shape tests run on these cases
QUIRK_HEADINGS = {(3, 3): 225., (3, 7): 0., (7, 3): 135., (4, 5): 45., (5, 5): 200., (9, 61): 120., (9, 62): 0.,
                  (10, 63): 120., (7, 247): 0., (8, 248): 120., (11, 249): 0., (33, 31): 120., (31, 33): 135.,
                  (65, 97): 200., (3, 250): 180., (251, 3): 200.}

# max |phi - exact| on the 0..1000 range: two f32 ulps of the range on media without floating clusters
# (as test_potential_vs_reference_spsolve and the G12 test), the soak's gate on those with them
GATE_SMOOTH, GATE_CLUSTERS = 1.3e-4, 5e-3
GATE_RESIDUAL = 1e-5
ULP_RANGE = float(np.spacing(np.float32(1000.)))

Case = namedtuple('Case', 'idx rows cols heading medium')


def _headings_of(shape):
    return HEADINGS if shape in SMALL_SHAPES else LARGER_HEADINGS[shape]


def _build_cases():
    out = []
    for shape in SHAPES:
        for heading in _headings_of(shape):
            k = len(out)
            medium = _MEDIUM_OVERRIDES.get((shape, heading), MEDIA[k % len(MEDIA)])
            out.append(Case(k, shape[0], shape[1], heading, medium))
    return tuple(out)


CASES = _build_cases()


QUIRK_CASES = tuple(c for c in CASES if QUIRK_HEADINGS[(c.rows, c.cols)] == c.heading)


def find(rows, cols, medium_name):
    """The first case of that shape and medium."""
    return next(c for c in CASES if (c.rows, c.cols, c.medium) == (rows, cols, medium_name))


def case_id(case):
    return f'{case.idx:03d}-{case.rows}x{case.cols}-h{case.heading:g}-{case.medium}'


def gate(case, ref_max_err=0.):
    """The bound on max |phi - exact| for a device field of this case."""
    if case.medium in SMOOTH_MEDIA:
        return max(GATE_SMOOTH, float(ref_max_err))
    return GATE_CLUSTERS


def medium(case):
    """The conductivity raster of a case, f64 holding f32 values (the fixture stores f32)."""
    rows, cols = case.rows, case.cols
    rng = np.random.default_rng([16, case.idx])
    live = np.abs(rng.normal(0.8, 0.6, (rows, cols)))
    name = case.medium
    if name == 'uniform':
        cond = np.ones((rows, cols))
    elif name == 'alldead':
        cond = np.zeros((rows, cols))
    elif name == 'live':
        cond = live
    elif name == 'speckle50':
        cond = np.where(rng.random((rows, cols)) < 0.5, 0., live)
    elif name == 'speckle70':
        cond = np.where(rng.random((rows, cols)) < 0.7, 0., live * 1e-3)
    elif name == 'block':
        cond = live * 10.
        br, bc = max(1, rows // 3), max(1, cols // 2)
        r0, c0 = int(rng.integers(0, rows - br + 1)), int(rng.integers(0, cols - bc + 1))
        cond[r0:r0 + br, c0:c0 + bc] = 0.
    elif name == 'barrier_row':
        cond = live
        cond[int(rng.integers(1, rows - 1))] = 0.
    elif name == 'barrier_col':
        cond = live
        cond[:, int(rng.integers(1, cols - 1))] = 0.
    elif name == 'island':
        cond = np.zeros((rows, cols))
        rs, cs = slice(rows // 3, rows - rows // 3), slice(cols // 3, cols - cols // 3)
        cond[rs, cs] = live[rs, cs]
    else:
        raise ValueError(name)
    return cond.astype(np.float32).astype(np.float64)


def east_free_rows(case, bnodes):
    """Interior rows of the east column that are not Dirichlet nodes: where the quirk acts."""
    east = (case.cols - 1) * case.rows + np.arange(1, case.rows - 1)
    return np.setdiff1d(east, np.asarray(bnodes, dtype=np.int64)) % case.rows


def shows_quirk(case, bnodes):
    """Condition (a) of the fixture: a non-uniform medium and free interior cells in the east column."""
    return case.medium not in ('uniform', 'alldead') and east_free_rows(case, bnodes).size > 0


def natural_facs(grid_shape):
    """The link weights geometry gives: sqrt(2) for a diagonal link, 1 otherwise.  The reference deals
    them out by position in a node's filtered neighbour list, which swaps the S and SW weights of the
    interior nodes of the east column (oracle.neighbour_lists)."""
    from oracle import ssrs_oracle as orc
    nrow = grid_shape[0]
    r, c, _ = orc.neighbour_lists(grid_shape)
    r, c = r.astype(np.int64), c.astype(np.int64)
    return np.where((r % nrow != c % nrow) & (r // nrow != c // nrow), sqrt(2.), 1.).astype(np.float32)


System = namedtuple('System', 'a b inodes bnodes benergy shape')


def assemble(conductivity, heading, facs=None):
    """The reference's system from the oracle's pieces, in f64 with f64 dead-pair entries: the system
    ssrs_potential_solve solves.  `facs` replaces the reference's link weights (natural_facs)."""
    import scipy.sparse as ss
    from oracle import ssrs_oracle as orc
    conductivity = np.asarray(conductivity, dtype=np.float64)
    nrow, ncol = conductivity.shape
    n = nrow * ncol
    bnodes, benergy = orc.get_boundary_nodes(heading, (nrow, ncol))
    r, c, ref_facs = orc.neighbour_lists((nrow, ncol))
    facs = ref_facs if facs is None else facs
    r, c = r.astype(np.int64), c.astype(np.int64)
    ca, cb = conductivity[r % nrow, r // nrow], conductivity[c % nrow, c // nrow]
    with np.errstate(divide='ignore'):
        hm = np.where((ca != 0) & (cb != 0), 2. / (1. / ca + 1. / cb), 1e-08)
    g = ss.coo_matrix((hm / facs, (r, c)), shape=(n, n)).tocsr()
    row_sums = np.add.reduceat(g.data, g.indptr[:-1])
    g.data = g.data / row_sums[np.repeat(np.arange(n), np.diff(g.indptr))]
    inodes = np.setdiff1d(np.arange(n), bnodes, assume_unique=True)
    gi = g[inodes, :].tocoo().tocsc()
    a_mat = (ss.eye(inodes.size).tocsc() - gi[:, inodes]).tocsc()
    return System(a_mat, gi[:, bnodes].dot(benergy), inodes, bnodes, benergy, (nrow, ncol))


def solve(system):
    """SuperLU on the system in f64 -> f64 field (rows, cols)."""
    import scipy.sparse.linalg as ssl
    nrow, ncol = system.shape
    energy = np.empty(nrow * ncol)
    energy[system.inodes] = ssl.spsolve(system.a, system.b)
    energy[system.bnodes] = system.benergy
    return energy.reshape(ncol, nrow).T


def relative_residual(system, field):
    """|A x - b| / |b| in f64 of a (rows, cols) field's free nodes; node id = col * nrow + row."""
    x = np.asarray(field, dtype=np.float64).T.reshape(-1)[system.inodes]
    return float(np.linalg.norm(system.a @ x - system.b) / np.linalg.norm(system.b))


def one_ulp_share(field, exact):
    """Share of the cells of an f32 field at most one f32 ulp from the correctly rounded exact value."""
    def ordinal(x):                                    # sign-magnitude bits -> a monotone integer
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return float(np.mean(np.abs(ordinal(field) - ordinal(np.asarray(exact).astype(np.float32))) <= 1))


def load_case(g, case):
    """A case's arrays from the loaded fixture (cond as f64 holding the stored f32 values)."""
    k = f'c{case.idx:03d}_'
    assert (int(g['rows'][case.idx]), int(g['cols'][case.idx]), float(g['headings'][case.idx]),
            str(g['media'][case.idx])) == (case.rows, case.cols, case.heading, case.medium), 'fixture and case table differ'
    ref = g[k + 'ref']
    return dict(cond=g[k + 'cond'].astype(np.float64), bnodes=g[k + 'bnodes'], benergy=g[k + 'benergy'],
                ref=ref, exact=ref.astype(np.float64) + g[k + 'exact_minus_ref'], ref_max_err=float(g['ref_max_err'][case.idx]),
                floor_residual=float(g['floor_residual'][case.idx]))
