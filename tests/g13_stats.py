"""The two-sample z statistics that hold thermal seeding to the reference ensemble G13
(tests/golden/g13_thermals.npz), shared by test_g13_fixture.py (the reference's halves against
each other) and test_gpu_thermal_fields.py (the device against the whole fixture).

A sample is a dict: band_counts (runs, 4) seeded cells per run and aspect band, logamp (N,) the
log-amplitudes of all seeded cells, field_max / field_var (runs,) per blurred field.

  counts per band (4) and in all   z = (n_a - n_b) / sqrt(n_a + n_b)   sums of rare Bernoullis:
                                                                       variance = mean
  log-amp mean      z = d / sqrt(s2_a / n_a + s2_b / n_b)
  log-amp sd        z = d / sqrt(s2_a / 2 n_a + s2_b / 2 n_b)
  field max, var    Welch's z over the runs
Bound |z| <= 5 for each of the nine: the seeds are fixed, so a test is deterministic; 5 sigma
makes a false alarm for a correct implementation a ~5e-6 event at the one time the seeds are
chosen, while dropping the aspect weighting moves the band counts by tens of sigma and mu off by
0.08 or sigma off by 0.06 is 5 sigma at the ~2200 seeded cells of an ensemble.
"""
import numpy as np

Z_BOUND = 5.0


def aspect_band(aspect):
    return np.minimum((np.abs(np.asarray(aspect) - 180.) / 45.).astype(np.int64), 3)


def fixture_sample(g, first=0, last=None):
    """Runs first .. last - 1 of the fixture (default: all) as a sample."""
    last = len(g['field_max']) if last is None else last
    off = g['logamp_offsets']
    return dict(band_counts=g['band_counts'][first:last], logamp=g['logamp'][off[first]:off[last]],
                field_max=g['field_max'][first:last], field_var=g['field_var'][first:last])


def welch_z(a, b):
    return (a.mean() - b.mean()) / np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))


def thermal_z(a, b):
    """name -> z of sample a against sample b (nine entries)."""
    z = {}
    na, nb = a['band_counts'].sum(0).astype(float), b['band_counts'].sum(0).astype(float)
    for band in range(4):
        z[f'count_band{band}'] = (na[band] - nb[band]) / np.sqrt(na[band] + nb[band])
    z['count_all'] = (na.sum() - nb.sum()) / np.sqrt(na.sum() + nb.sum())
    la, lb = a['logamp'], b['logamp']
    va, vb = la.var(ddof=1), lb.var(ddof=1)
    z['logamp_mean'] = (la.mean() - lb.mean()) / np.sqrt(va / len(la) + vb / len(lb))
    z['logamp_sd'] = (np.sqrt(va) - np.sqrt(vb)) / np.sqrt(va / (2 * len(la)) + vb / (2 * len(lb)))
    z['field_max'] = welch_z(a['field_max'], b['field_max'])
    z['field_var'] = welch_z(a['field_var'], b['field_var'])
    return z
