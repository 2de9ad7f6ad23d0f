"""K12 in numpy: Allen's (2006) field of discrete updrafts as include/ssrs_hip.h states it (the model the reference carries
commented out at ssrs/layers.py:304-493), f64, the nearest updraft by brute-force argmin in row chunks -- and the cases
that tests/test_allen_emulation.py and tests/test_gpu_allen.py share.  The kernel and this file share every f64
operation except pow and sin, so the table and `nearest` must agree exactly and the field within FIELD_BOUND."""
import functools

import numpy as np

S = (0.14, 0.25, 0.36, 0.47, 0.58, 0.69, 0.80)
K = np.array([[1.5352, 2.5826, -0.0113, -0.1950],
              [1.5265, 3.6054, -0.0176, -0.1265],
              [1.4866, 4.8356, -0.0320, -0.0818],
              [1.2042, 7.7904, 0.0848, -0.0445],
              [0.8816, 13.9720, 0.3404, -0.0216],
              [0.7067, 23.9940, 0.5689, -0.0099],
              [0.6189, 42.7965, 0.7157, -0.0033]])
RGAINS = (0.1, 0.5, 1, 2.2, 4.3, 6.5, 8.7, 10.8, 12.5, 13.5, 16)

# max |field - field_ref| / max |wpeak| over CASES, measured: 2.6e-16 with the kernels compiled for the CPU and 3.4e-16 on
# an MI355X (ROCm's pow and sin against numpy's; profiles/allen_thermals.md) -- the last bits of pow, sin and the sums
# that follow them.  Asserted: 64 x the larger, to leave room for other libm versions; far below the 1e-12 above which a
# difference is a wrong neighbour or a wrong branch and not rounding.
FIELD_MEASURED_CPU, FIELD_MEASURED_GPU = 2.6e-16, 3.4e-16
FIELD_BOUND = 64 * max(FIELD_MEASURED_CPU, FIELD_MEASURED_GPU)
assert FIELD_BOUND <= 1e-12


def scalars(z, zi, wstar, shape, res, n, sink):
    """zzi, rbar, wtbar, we, below: the host scalars of a field of n updrafts."""
    zzi = z / zi
    rbar = 0.102 * zzi ** (1 / 3) * (1 - 0.25 * zzi) * zi
    wtbar = zzi ** (1 / 3) * (1 - 1.1 * zzi) * wstar
    X, Y = shape[1] * res, shape[0] * res
    we = 0.
    if sink:
        area = n * np.pi * rbar ** 2
        assert area < X * Y
        we = min(-(wtbar * area * (-2.5 * (zzi - 0.5))) / (X * Y - area), 0.)
    return zzi, rbar, wtbar, we, z < zi


def table(rbar, wtbar, wgain, rgain):
    """(n, 6) f64: r2, r1r2, r1, wbar, wpeak, row."""
    r2 = np.maximum(10., rbar * rgain)
    r1r2 = np.where(r2 < 600., 0.0011 * r2 + 0.14, 0.8)
    r1 = r1r2 * r2
    wbar = wtbar * wgain
    wpeak = 3 * wbar * (r2 * r2 * r2 - r2 * r2 * r1) / (r2 * r2 * r2 - r1 * r1 * r1)
    row = np.full(r2.shape, 6.)
    for j in range(5, -1, -1):
        row[r1r2 < 0.5 * (S[j] + S[j + 1])] = j
    return np.stack([r2, r1r2, r1, wbar, wpeak, row], 1)


def nearest(xt, yt, shape, res, chunk=16):
    """(nearest int32, d2 f64): per cell the smallest d2, the lowest index among equals (argmin returns the first)."""
    rows, cols = shape
    xc = np.arange(cols) * res
    near = np.empty(shape, dtype=np.int32)
    d2min = np.empty(shape)
    for r0 in range(0, rows, chunk):
        yc = np.arange(r0, min(rows, r0 + chunk)) * res
        dx = xc[None, :, None] - xt[None, None, :]
        dy = yc[:, None, None] - yt[None, None, :]
        d2 = dx * dx + dy * dy
        u = d2.argmin(axis=2)
        near[r0:r0 + len(yc)] = u
        d2min[r0:r0 + len(yc)] = np.take_along_axis(d2, u[..., None], 2)[..., 0]
    return near, d2min


def field(tab, near, d2, zzi, we, below):
    r2, r1, wbar, wpeak = (tab[:, c][near] for c in (0, 2, 3, 4))
    k1, k2, k3, k4 = (K[tab[:, 5].astype(int), c][near] for c in range(4))
    dist = np.sqrt(d2)
    rr2 = dist / r2
    ws = np.maximum(1 / (1 + np.power(k1 * np.abs(rr2 + k3), k2)) + k4 * rr2, 0) if below else np.zeros_like(rr2)
    wl = np.where((dist > r1) & (rr2 < 2), (np.pi / 6) * np.sin(np.pi * rr2), 0.)
    wd = np.minimum(2.5 * wl * (zzi - 0.5), 0) if 0.5 < zzi <= 0.9 else np.zeros_like(rr2)
    w = wpeak * ws + wd * wbar
    if we != 0:
        with np.errstate(divide='ignore', invalid='ignore'):
            stretched = np.where(wpeak != 0, w * (1 - we / wpeak) + we, we)
        w = np.where(dist > r1, stretched, w)
    return w


# ---------------------------------------------------------------------------------------------------------- cases
def _uniform(n, shape, res, seed, lo=(0., 0.), hi=None):
    rng = np.random.default_rng(seed)
    hi = hi or (shape[1] * res, shape[0] * res)
    return (rng.uniform(lo[0], hi[0], n), rng.uniform(lo[1], hi[1], n), rng.uniform(0.7, 1.3, n), rng.uniform(0.8, 1.2, n))


def _lattice(shape, res, seed):
    """Updrafts at the centres of cells (3 + 8 i, 3 + 8 j), the first five repeated at the end, the order shuffled."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(3, shape[0], 8), np.arange(3, shape[1], 8), indexing='ij')
    x, y = c.ravel() * res, r.ravel() * res
    x, y = np.concatenate([x, x[:5]]), np.concatenate([y, y[:5]])
    order = rng.permutation(x.size)
    n = x.size
    return x[order].astype(np.float64), y[order].astype(np.float64), rng.uniform(0.7, 1.3, n), rng.uniform(0.8, 1.2, n)


def _build_cases():
    cases = []

    def add(name, shape, res, ups, z=100., zi=1000., wstar=2., sink=False, overflow=False):
        cases.append(dict(name=name, shape=shape, res=res, z=z, zi=zi, wstar=wstar, sink=sink, overflow=overflow,
                          xt=ups[0], yt=ups[1], wgain=ups[2], rgain=ups[3]))
    ragged = ((97, 131), 30.)
    add('ragged', *ragged, _uniform(149, *ragged, 1))
    ties = _lattice(*ragged, 2)
    add('ties', *ragged, ties)
    add('clustered', (150, 200), 30., _uniform(40, (150, 200), 30., 3, hi=(75., 75.)))
    add('single', *ragged, _uniform(1, *ragged, 4))
    add('dense', (40, 50), 30., _uniform(5000, (40, 50), 30., 5), overflow=True)
    rng = np.random.default_rng(6)
    shaped = ties[:3] + (rng.choice(np.array(RGAINS, dtype=np.float64), ties[0].size),)
    add('shapes', *ragged, shaped)
    for z in (700., 950., 1000., 1200.):
        for sink in (False, True):
            add(f'z{int(z)}{"-sink" if sink else ""}', *ragged, shaped, z=z, sink=sink)
    calm = ties[:2] + (np.zeros(ties[0].size), ties[3])
    add('calm', *ragged, calm)
    add('calm-sink', *ragged, calm, sink=True)
    add('tiles', (512, 640), 10., _uniform(426, (512, 640), 10., 9))
    return cases


CASES = _build_cases()
CASE_IDS = [c['name'] for c in CASES]


@functools.lru_cache(maxsize=None)
def expected(name):
    """dict(table, nearest, field, we, scale = max |wpeak|) of a case, computed once and shared; read-only."""
    c = CASES[CASE_IDS.index(name)]
    zzi, rbar, wtbar, we, below = scalars(c['z'], c['zi'], c['wstar'], c['shape'], c['res'], c['xt'].size, c['sink'])
    tab = table(rbar, wtbar, c['wgain'], c['rgain'])
    near, d2 = nearest(c['xt'], c['yt'], c['shape'], c['res'])
    out = dict(table=tab, nearest=near, field=field(tab, near, d2, zzi, we, below), we=we, d2=d2,
               scale=float(np.abs(tab[:, 4]).max()), scalars=(zzi, rbar, wtbar, we, below))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def field_error(got, name):
    """max |got - field_ref| / max |wpeak| of a case; where every wpeak is 0 the field is 0 or `we` exactly, and any
    difference counts as infinite."""
    e = expected(name)
    diff = float(np.abs(np.asarray(got, dtype=np.float64) - e['field']).max())
    if e['scale'] == 0.:
        return 0. if diff == 0. else np.inf
    return diff / e['scale']


def check_case(name, near, tab, fld):
    """The assertions every case makes, on the CPU emulation and on the GPU alike."""
    e = expected(name)
    assert near.dtype == np.int32 and near.shape == e['nearest'].shape
    assert np.array_equal(near, e['nearest']), (name, int((near != e['nearest']).sum()))
    assert tab.shape == e['table'].shape and np.array_equal(tab.view(np.uint64), e['table'].view(np.uint64)), name
    assert np.isfinite(fld).all(), name
    err = field_error(fld, name)
    print(f'allen {name}: field error {err:.3g} of max |wpeak|')
    assert err <= FIELD_BOUND, (name, err)
    if name == 'shapes':
        assert set(e['table'][:, 5].astype(int)) == set(range(7))
        assert (e['table'][:, 0] == 10.).any() and (e['table'][:, 1] == 0.8).any()
    if name.startswith('calm'):
        inside = np.sqrt(e['d2']) <= e['table'][:, 2][e['nearest']]
        assert (fld[inside] == 0.).all() and (fld[~inside] == e['we']).all() and (~inside).any() and inside.any()
        assert (e['we'] < 0.) == name.endswith('sink')
