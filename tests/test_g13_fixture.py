"""G13 (tests/golden/g13_thermals.npz): what the reference's compute_thermals (layers.py:188-214)
drew and returned over 256 runs, written by tests/golden/generate_g13_thermals.py.  These tests
need no GPU: they show that the reference alone stays inside the bounds the device is held to in
test_gpu_thermal_fields.py, that its blur is scipy's gaussian_filter(sigma=4, mode='constant'),
and that the batched C entry point validates its arguments before any GPU work."""
import ctypes as C

import numpy as np

from g13_stats import Z_BOUND, aspect_band, fixture_sample, thermal_z


def test_reference_halves_stay_inside_the_device_bounds(golden):
    g = golden('g13_thermals.npz')
    runs = len(g['field_max'])
    assert runs == 256 and g['aspect'].shape == (200, 240) and float(g['thermal_intensity_scale']) == 2.0
    z = thermal_z(fixture_sample(g, 0, runs // 2), fixture_sample(g, runs // 2, runs))
    print({k: round(float(v), 3) for k, v in z.items()})
    assert len(z) == 9
    for name, value in z.items():
        assert abs(value) <= Z_BOUND, (name, value)


def test_reference_band_counts_match_the_seeding_probability(golden):
    """Seeded cells per aspect band over the ensemble against runs * sum 1 / (int(wt) - 1) over the
    band's interior cells, within 5 sqrt(expected)."""
    g = golden('g13_thermals.npz')
    aspect = g['aspect']
    rows, cols = aspect.shape
    by, bx = int(0.1 * rows), int(0.1 * cols)
    inner = aspect[by:rows - by, bx:cols - bx]
    p = 1. / ((1000. + np.abs(inner - 180.) / 180. * 2000.).astype(int) - 1)
    band = aspect_band(inner)
    got = g['band_counts'].sum(0)
    for b in range(4):
        expect = len(g['field_max']) * p[band == b].sum()
        assert abs(got[b] - expect) <= 5 * np.sqrt(expect), (b, got[b], expect)
    assert g['logamp_offsets'][-1] == len(g['logamp']) == got.sum()


def test_reference_blur_is_scipys_constant_mode_gaussian(golden):
    from scipy import ndimage
    g = golden('g13_thermals.npz')
    seeds = np.zeros(g['aspect'].shape)
    seeds.flat[g['seed0_index']] = g['seed0_value']
    assert np.array_equal(np.log(g['seed0_value']), g['logamp'][:g['logamp_offsets'][1]])
    assert np.array_equal(ndimage.gaussian_filter(seeds, 4, mode='constant'), g['field0'])
    assert g['field0'].max() == g['field_max'][0] and g['field0'].var() == g['field_var'][0]


def test_thermal_fields_argument_validation_needs_no_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    seeds = (C.c_uint64 * 2)(1, 2)
    buf = (C.c_char * 64)()

    def call(aspect=buf, sigma=4.0, seeds=seeds, count=2, out=buf, rows=10, cols=10):
        return lib.ssrs_thermal_fields(aspect, C.c_double(2.0), C.c_double(sigma), seeds, count, out, 1,
                                       rows, cols, None)
    for bad in (dict(aspect=None), dict(seeds=None), dict(out=None)):
        assert call(**bad) == _native.SSRS_ERR_INVALID and b'NULL' in lib.ssrs_last_error()
    for bad in (dict(count=0), dict(count=-1), dict(rows=0), dict(cols=-3), dict(sigma=0.0), dict(sigma=-1.0),
                dict(sigma=float('nan'))):
        assert call(**bad) == _native.SSRS_ERR_INVALID and b'ssrs_thermal_fields' in lib.ssrs_last_error(), bad
