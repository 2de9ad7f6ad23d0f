"""The restatement of the random thermals (tests/thermals_ref.py) on the host: the Philox words against rocRAND's host
engine, the tiny rasters that really hold a thermal, the seeds that tell an off-by-one in the seeding rate, the blur in the
kernel's order against scipy and against the reference's own recorded field (fixture G13), the weights against
csrc/gauss.h bit for bit, and the condition that the shared cases are populated."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import thermals_ref as ref

DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'thermal_weights_driver.cpp')
WEIGHT_SIGMAS = ('0.1', '0.3', '1.3', '4.0', '4.1', '4.2', '5.0', '8.0')

# rocRAND's host engine, rocrand_init(seed, cell, 0) + rocrand4, recorded
KNOWN_WORDS = [(11, 0, (3848496742, 4117957564, 1519192786, 1437745381)),
               (11, 5394, (424935821, 753542670, 2268895696, 907014675)),
               (2 ** 63 + 5, 4000000123, (4143558960, 671735789, 404969430, 291607626)),
               (2 ** 64 - 1, 1, (2806134509, 2122658050, 1278364322, 1108527830))]

# shape -> {seed: the one seeded cell}, aspect 180, scale 2
ONE_THERMAL = {(1, 1): {856: (0, 0), 1801: (0, 0), 1831: (0, 0)},
               (2, 2): {409: (0, 1), 856: (0, 0), 870: (1, 0)},
               (1, 64): {18: (0, 22), 20: (0, 23), 28: (0, 41)},
               (64, 1): {18: (22, 0), 20: (23, 0), 28: (41, 0)},
               (9, 9): {18: (2, 4), 20: (2, 5), 28: (4, 5)},
               (10, 10): {18: (2, 2), 20: (2, 3), 28: (4, 1)},
               (3, 5): {35: (1, 0), 128: (1, 0), 250: (2, 3)},
               (16, 16): {12: (10, 5), 18: (1, 6), 20: (1, 7)}}


def test_philox_words_are_rocrands():
    """The counter layout (0, 0, cell lo, cell hi) and the key (seed lo, seed hi).  Cell 4 000 000 123 is the only check
    of the counter's HIGH word and of a flat index beyond 2^31: no device test reaches such an index at sizes a test can
    afford, so that part of the layout is covered on the CPU alone."""
    for seed, cell, want in KNOWN_WORDS:
        assert tuple(int(w) for w in ref.words(seed, cell)) == want, (seed, cell)
    assert tuple(int(w) for w in ref.words(11 + 2 ** 64, 5394)) == KNOWN_WORDS[1][2]          # the seed is masked to 64 bits
    cells = np.array([[0, 5394], [1, 2]])
    w = ref.words(11, cells)
    assert w[0].shape == (2, 2) and [int(x[0, 1]) for x in w] == list(KNOWN_WORDS[1][2])


def test_tiny_rasters_really_hold_a_thermal():
    assert {shape: tuple(seeds) for shape, seeds in ONE_THERMAL.items()} == dict(ref.TINY)
    for shape, cells in ONE_THERMAL.items():
        for seed, cell in cells.items():
            values, hit = ref.seed_field(ref.flat_aspect(shape), ref.SCALE, seed)
            assert [tuple(int(i) for i in rc) for rc in np.argwhere(hit)] == [cell], (shape, seed)
            assert values[cell] > 0. and np.count_nonzero(values) == 1 and not np.signbit(values).any()
    values, _ = ref.seed_field(ref.flat_aspect((9, 9)), ref.SCALE, 18)
    np.testing.assert_allclose(values[2, 4], 154.05589679961525, rtol=1e-12)       # (numpy's libm may differ in the last bits)
    # the flat index is r * cols + c: the seeds of (1, 64) give the transposed cells on (64, 1)
    for seed in (18, 20, 28):
        assert np.array_equal(ref.seed_field(ref.flat_aspect((64, 1)), 2., seed)[0],
                              ref.seed_field(ref.flat_aspect((1, 64)), 2., seed)[0].T)


def test_interior_and_nvals():
    assert ref.interior((9, 9)).all() and ref.interior((1, 1)).all()                  # int(0.1 * 9) == 0: no border
    inside = ref.interior((10, 25))
    assert inside[1:9, 2:23].all() and inside.sum() == 8 * 21
    assert ref.ring((10, 25)).sum() == 2 * 21 + 2 * 6
    # truncation, not rounding: 1000.9 -> 1000, 1011.1 -> 1011, 1999.9 -> 1999
    assert list(ref.nvals_of([180., 0., 360., 90., 270., 180.081, 179., 269.991])) == [999, 2999, 2999, 1999, 1999, 999, 1010, 1998]
    assert ref.nvals_of([float('nan')])[0] == -1                                      # the device's conversion, see nvals_of
    values, hit = ref.seed_field(np.full((20, 30), np.nan), 2., 7)
    assert np.array_equal(hit, ref.interior((20, 30))) and (values[hit] > 0.).all() and not values[~hit].any()


def _hits(shape, seed, nvals):
    """The seeded cells of aspect 180 under the rule w0 * nvals < 2^32 (ref.seed_field's, with nvals free)."""
    cell = np.arange(shape[0] * shape[1], dtype=np.uint64).reshape(shape)
    return ref.interior(shape) & (ref.words(seed, cell)[0].astype(np.int64) * nvals < ref.TWO32)


def test_the_cases_can_tell_an_off_by_one():
    """nvals = int(1000.0) - 1 = 999 at aspect 180.  Four of (64, 128)'s seeds hold a cell that 1000 drops, four a cell
    that 998 adds: with these among the GPU cases the exact mask comparison sees a 0.1 % error in the rate."""
    shape, nvals = ref.CRITICAL_SHAPE, int(ref.nvals_of([180.])[0])
    assert nvals == 999
    for seed in ref.CRITICAL_LOSE + ref.CRITICAL_GAIN:
        assert np.array_equal(_hits(shape, seed, nvals), ref.seed_field(ref.flat_aspect(shape), 2., seed)[1])
    for seed in ref.CRITICAL_LOSE:
        assert _hits(shape, seed, nvals + 1).sum() < _hits(shape, seed, nvals).sum(), seed
    for seed in ref.CRITICAL_GAIN:
        assert _hits(shape, seed, nvals - 1).sum() > _hits(shape, seed, nvals).sum(), seed
    assert set(ref.CRITICAL_LOSE + ref.CRITICAL_GAIN) == set(dict((c[0], c[3]) for c in ref.CASES)['64x128-critical'])


def test_the_cases_can_tell_rounding_from_truncation():
    """At aspect 180.0675 wt is 1000.75: int(wt) - 1 is still 999, so the seeded cells are those of aspect 180, while
    round(wt) - 1 = 1000 drops one for each of the case's four seeds."""
    shape, aspect = ref.CRITICAL_SHAPE, ref.fraction_aspect(ref.CRITICAL_SHAPE)
    wt = 1000.0 + (abs(ref.FRACTION_ASPECT - 180.0) / 180.0) * 2000.0
    assert abs(wt - 1000.75) < 1e-9 and int(wt) - 1 == 999 == int(ref.nvals_of(aspect)[0, 0]) and round(wt) - 1 == 1000
    assert dict((c[0], c[3]) for c in ref.CASES)['64x128-fraction'] == ref.CRITICAL_LOSE
    for seed in ref.CRITICAL_LOSE:
        hit = ref.seed_field(aspect, ref.SCALE, seed)[1]
        assert np.array_equal(hit, _hits(shape, seed, int(wt) - 1))
        assert _hits(shape, seed, round(wt) - 1).sum() < hit.sum(), seed


def _mutated_seed_field(aspect, scale, seed, mutation):
    """ref.seed_field with ONE of its rules changed (written out here, the restatement has no switches)."""
    a = np.asarray(aspect, dtype=np.float64)
    rows, cols = a.shape
    w = ref.words(seed, np.arange(rows * cols, dtype=np.uint64).reshape(rows, cols))
    wt = 1000.0 + (np.abs(a - 180.0) / 180.0) * 2000.0
    nan = np.isnan(wt)
    whole = np.round(np.where(nan, 0., wt)) if mutation == 'round' else np.trunc(np.where(nan, 0., wt))
    nvals = whole.astype(np.int64) - 1 + {'nvals + 1': 1, 'nvals - 1': -1}.get(mutation, 0)
    nvals = np.where(nan, -1, nvals)
    extra = 1 if mutation == 'border + 1' else 0
    by, bx = int(0.1 * rows) + extra, int(0.1 * cols) + extra
    inside = np.zeros(a.shape, dtype=bool)
    inside[by:rows - by, bx:cols - bx] = True
    decides = w[1] if mutation == 'decision on word 1' else w[0]
    hit = inside & (decides.astype(np.int64) * nvals < ref.TWO32)
    first, second = (w[2], w[1]) if mutation == 'words 1 and 2 swapped' else (w[1], w[2])
    values = np.zeros(a.shape)
    for r, c in zip(*np.nonzero(hit)):
        if mutation == 'u1 without + 1':
            u1 = float(first[r, c]) * 2.0 ** -32
            if u1 == 0.:
                values[r, c] = np.inf
                continue
            z = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * 3.141592653589793 * float(second[r, c]) * 2.0 ** -32)
            values[r, c] = math.exp((scale + 3.0) + 0.5 * z)
        else:
            values[r, c] = ref.amplitude(first[r, c], second[r, c], scale)
    return values, hit


def test_every_mutated_rule_differs_on_the_gpu_cases():
    """What the GPU tests can tell apart: each single change of the seeding rule moves a seeded cell, or an amplitude by
    more than 1e-13 (the cap of the GPU test's RTOL_AMP), in at least one (case, seed) the GPU tests run -- so a device
    that agrees with the restatement there cannot hold that change.  The unchanged rule written the same way differs
    nowhere."""
    cases = [(name, aspect_of(shape), seeds) for name, shape, aspect_of, seeds in ref.CASES]
    cases.append(('dense', np.full(ref.DENSE_SHAPE, np.nan), (ref.DENSE_SEED,)))
    want = {(name, seed): ref.seed_field(aspect, ref.SCALE, seed) for name, aspect, seeds in cases for seed in seeds}
    for mutation in (None, 'nvals + 1', 'nvals - 1', 'round', 'border + 1', 'decision on word 1', 'u1 without + 1',
                     'words 1 and 2 swapped'):
        moved, off = 0, 0
        for name, aspect, seeds in cases:
            for seed in seeds:
                (v0, h0), (v, h) = want[(name, seed)], _mutated_seed_field(aspect, ref.SCALE, seed, mutation)
                moved += not np.array_equal(h, h0)
                both = h & h0
                off += bool((np.abs(v[both] - v0[both]) > 1e-13 * v0[both]).any())
        print(f'{mutation}: seeded cells differ in {moved} (case, seed) pairs, amplitudes beyond 1e-13 in {off}')
        assert (moved + off > 0) == (mutation is not None), mutation


@pytest.mark.parametrize('shape, sigma', ref.BLUR_CASES, ids=['%dx%d-s%g' % (s + (g,)) for s, g in ref.BLUR_CASES])
def test_kernel_order_blur_against_scipy(shape, sigma):
    """The stated order against gaussian_filter(mode='constant') within 4 (2 R + 3) 2^-53 max|x|: on a dense signed input
    (no term is zero; a raster narrower than 2 R + 1 sums fewer taps than weights) and on a seed field."""
    dense = np.random.default_rng(1).normal(size=shape)
    sparse = np.zeros(shape)
    sparse.flat[::max(1, sparse.size // 7)] = 150.
    for name, x in (('dense', dense), ('sparse', sparse)):
        dev, lim = float(np.abs(ref.blur_kernel_order(x, sigma) - ref.scipy_blur(x, sigma)).max()), ref.bound(sigma, x)
        print(f'{shape} sigma {sigma:g} {name}: largest deviation {dev:.3e}, bound {lim:.3e}')
        assert dev <= lim
    if ref.radius(sigma) == 0:
        assert np.array_equal(ref.blur_kernel_order(dense, sigma), dense)


def test_kernel_order_blur_against_the_reference_field(golden):
    """The blur of the seed field the reference drew (G13) against the field the reference returned."""
    g = golden('g13_thermals.npz')
    seeds = np.zeros(g['aspect'].shape)
    seeds.flat[g['seed0_index']] = g['seed0_value']
    got = ref.blur_kernel_order(seeds, float(g['sigma']))
    print('largest deviation from the reference field', np.abs(got - g['field0']).max())
    np.testing.assert_allclose(got, g['field0'], rtol=1e-12, atol=1e-12)


def test_weights_are_gauss_h_bit_for_bit(tmp_path):
    """csrc/gauss.h compiled for the host: blur_radius and the bits of blur_weights equal smooth_ref's radius and weights
    (which thermals_ref shares), so both restatements rest on the header's own numbers."""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'thermal_weights_driver')
    subprocess.run(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-Wall', '-Werror', '-Wno-unused-function', DRIVER,
                    '-o', exe], check=True)
    out = subprocess.run([exe, *WEIGHT_SIGMAS], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split('\n')[:-1]
    assert len(lines) == len(WEIGHT_SIGMAS)
    for text, line in zip(WEIGHT_SIGMAS, lines):
        name, R, *bits = line.split()
        sigma = float(text)
        want_R, want = ref.full_weights(sigma)
        assert name == text and int(R) == want_R == ref.radius(sigma) and len(bits) == 2 * want_R + 1
        assert [int(b, 16) for b in bits] == [int(v) for v in want.view(np.uint64)], text
    assert [ref.radius(float(s)) for s in WEIGHT_SIGMAS] == [0, 1, 5, 16, 16, 17, 20, 32]


def test_the_mid_size_cases_are_populated():
    """A condition on the cases, from the restatement alone: every mid-size shape holds at least 30 seeded cells over its
    seeds, at least 3 of them on the ring of interior cells next to the border."""
    for name, shape, aspect_of, seeds in ref.CASES:
        if aspect_of is not ref.mid_aspect:
            continue
        aspect, ring = aspect_of(shape), ref.ring(shape)
        hits = [ref.seed_field(aspect, ref.SCALE, seed)[1] for seed in seeds]
        total, on_ring = sum(int(h.sum()) for h in hits), sum(int((h & ring).sum()) for h in hits)
        print(f'{name}: {total} seeded cells over {len(seeds)} seeds, {on_ring} on the ring')
        assert len(seeds) == 42 and total >= 30 and on_ring >= 3, name
