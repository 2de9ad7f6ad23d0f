"""a5 thermals through the fused, batched call (ssrs_thermal_fields / thermals.compute_thermals_batch)
on the MI355X: bit identity with the two-stage chain thermal_seeds -> gaussian_blur, the blur pinned to
the reference's own output (fixture G13), the seeding held to the reference ensemble of G13 by the
two-sample z statistics of g13_stats.py (|z| <= 5, derivation there), the Simulator's files, and
stream behaviour.  The reference replays a serial global RNG, so parity of the seeding is statistical;
everything else here is exact.  Rasters below one tile, thinner than the radius, other radii and the device's own
seeding rule cell by cell: thermals_ref.CASES, test_gpu_thermal_parity.py."""
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from g13_stats import Z_BOUND, aspect_band, fixture_sample, thermal_z

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 2 ** 63 + 5)


def chain(aspect, seed, sigma=4.0):
    from ssrs_amd import thermals
    return thermals.gaussian_blur(thermals.thermal_seeds(aspect, 2.0, seed), sigma)


@pytest.mark.parametrize('shape', [(61, 83), (200, 240), (1000, 1200), (25, 700)])
def test_batch_is_bit_identical_to_the_chain(gpu, shape):
    """f64: torch.equal with gaussian_blur(thermal_seeds(...), 4) per seed; f32: that field's .to(float32);
    a batch equals its members one by one.  (25, 700) has rows < 2 * radius; every shape is ragged
    against the 32 x 64 tile."""
    from ssrs_amd import thermals
    aspect = torch.from_numpy(np.random.default_rng(shape[0]).uniform(0., 360., shape)).to(gpu)
    f64 = thermals.compute_thermals_batch(aspect, 2.0, SEEDS)
    f32 = thermals.compute_thermals_batch(aspect, 2.0, SEEDS, dtype=torch.float32)
    assert f64.dtype == torch.float64 and f32.dtype == torch.float32 and tuple(f64.shape) == (3,) + shape
    for k, seed in enumerate(SEEDS):
        want = chain(aspect, seed)
        assert torch.equal(f64[k], want), (shape, seed, float((f64[k] - want).abs().max()))
        assert torch.equal(f32[k], want.to(torch.float32))
        assert torch.equal(thermals.compute_thermals_batch(aspect, 2.0, [seed])[0], f64[k])
        assert torch.equal(thermals.compute_thermals(aspect, 2.0, seed), f64[k])
    if shape[0] >= 200:
        assert f64.max() > 0 and not torch.equal(f64[0], f64[1])


def test_more_realisations_than_one_launch_holds(gpu):
    """40 seeds: two launches (32 + 8) write one (40, rows, cols) tensor."""
    from ssrs_amd import thermals
    aspect = torch.from_numpy(np.random.default_rng(2).uniform(0., 360., (150, 130))).to(gpu)
    seeds = list(range(100, 140))
    got = thermals.compute_thermals_batch(aspect, 2.0, seeds)
    for k in (0, 31, 32, 39):
        assert torch.equal(got[k], chain(aspect, seeds[k]))


def test_other_sigmas_and_the_wide_radius_path(gpu):
    """sigma stays a parameter: a narrower kernel runs in the fused kernel with a smaller halo, a radius
    beyond 16 (sigma 5 -> 20) takes the chain inside the same entry point; both equal the chain."""
    from ssrs_amd import thermals
    aspect = torch.from_numpy(np.random.default_rng(3).uniform(0., 360., (210, 190))).to(gpu)
    for sigma in (1.3, 5.0):
        for dtype in (torch.float64, torch.float32):
            got = thermals.compute_thermals_batch(aspect, 2.0, SEEDS[:2], dtype=dtype, sigma=sigma)
            for k in range(2):
                assert torch.equal(got[k], chain(aspect, SEEDS[k], sigma).to(dtype)), (sigma, dtype)


def test_dense_seed_field_is_still_bit_identical(gpu):
    """A NaN aspect seeds every interior cell (int(NaN) - 1 < 0 makes the draw always pass), so the
    column mask is full and nothing is skipped: the sums must still be the chain's."""
    from ssrs_amd import thermals
    aspect = torch.full((90, 140), float('nan'), dtype=torch.float64, device=gpu)
    seeds = thermals.thermal_seeds(aspect, 2.0, 7)
    assert int((seeds > 0).sum()) > (90 - 2 * 9) * (140 - 2 * 14) // 2
    assert torch.equal(thermals.compute_thermals_batch(aspect, 2.0, [7])[0], chain(aspect, 7))


def test_numpy_and_non_contiguous_aspect(gpu):
    from ssrs_amd import thermals
    big = np.random.default_rng(5).uniform(0., 360., (120, 2 * 150))
    view = big[:, ::2]                                   # non-contiguous host array
    got = thermals.compute_thermals_batch(view, 2.0, SEEDS[:2], dtype=torch.float32)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (2, 120, 150)
    dev = torch.from_numpy(big).to(gpu)[:, ::2]          # non-contiguous device tensor
    got_dev = thermals.compute_thermals_batch(dev, 2.0, SEEDS[:2], dtype=torch.float32)
    assert torch.is_tensor(got_dev) and np.array_equal(got_dev.cpu().numpy(), got)
    assert np.array_equal(got[1], chain(np.ascontiguousarray(view), SEEDS[1]).astype(np.float32))
    with pytest.raises(ValueError):
        thermals.compute_thermals_batch(view, 2.0, [])
    with pytest.raises(ValueError):
        thermals.compute_thermals_batch(view, 2.0, [1], dtype=torch.float16)


def test_blur_against_the_reference_field(gpu, golden):
    """Device gaussian_blur of the seed field the reference drew against the field the reference returned,
    rtol = atol = 1e-12 (scipy's correlate1d sums in another order, so not bit for bit)."""
    from ssrs_amd import thermals
    g = golden('g13_thermals.npz')
    seeds = np.zeros(g['aspect'].shape)
    seeds.flat[g['seed0_index']] = g['seed0_value']
    got = thermals.gaussian_blur(seeds, float(g['sigma']))
    err = np.abs(got - g['field0'])
    print('max abs error against the reference field', err.max())
    np.testing.assert_allclose(got, g['field0'], rtol=1e-12, atol=1e-12)


def test_statistics_against_the_reference_ensemble(gpu, golden):
    """One batched call, seeds 0 .. 255, on G13's aspect raster gives the fields (maximum, variance);
    the seeded cells and amplitudes come from thermal_seeds with the same seeds (the bit-identity test
    ties the two together).  |z| <= 5 for each of the nine statistics; every field is exactly zero
    farther than 16 cells from the seeded interior."""
    from ssrs_amd import thermals
    g = golden('g13_thermals.npz')
    aspect = torch.from_numpy(g['aspect']).to(gpu)
    rows, cols = aspect.shape
    runs = len(g['field_max'])
    fields = thermals.compute_thermals_batch(aspect, float(g['thermal_intensity_scale']), range(runs))
    band = torch.from_numpy(aspect_band(g['aspect'])).to(gpu)
    counts = np.zeros((runs, 4), dtype=np.int64)
    logamp = []
    for s in range(runs):
        seeds = thermals.thermal_seeds(aspect, float(g['thermal_intensity_scale']), s)
        hit = seeds > 0
        counts[s] = torch.bincount(band[hit], minlength=4).cpu().numpy()
        logamp.append(torch.log(seeds[hit]).cpu().numpy())
    dev = dict(band_counts=counts, logamp=np.concatenate(logamp),
               field_max=fields.amax(dim=(1, 2)).cpu().numpy(),
               field_var=fields.var(dim=(1, 2), unbiased=False).cpu().numpy())
    z = thermal_z(dev, fixture_sample(g))
    print({k: round(float(v), 3) for k, v in z.items()})
    assert len(z) == 9
    for name, value in z.items():
        assert abs(value) <= Z_BOUND, (name, value)
    by, bx, rad = int(0.1 * rows), int(0.1 * cols), 16
    assert by > rad and bx > rad
    assert not fields[:, :by - rad].any() and not fields[:, rows - by + rad:].any()
    assert not fields[:, :, :bx - rad].any() and not fields[:, :, cols - bx + rad:].any()
    assert (fields >= 0).all()


def test_simulator_writes_the_batched_fields(gpu, tmp_path):
    """sim_seed 3, three realisations, two injected cases: every <case>_r<k>_thermals.npy is f32 and equals
    compute_thermals(aspect, 2.0, seed = sim_seed + 7919 (k + 1) + 104729 case_no) rounded to f32; the six
    fields differ pairwise (240 x 300 cells: ~23 seeds per field, so no two fields are both empty)."""
    from ssrs_amd import Config, Simulator, thermals
    from ssrs_amd.synthetic import wind_lattice
    cfg = replace(Config(run_name='th', out_dir=str(tmp_path), sim_seed=3, region_width_km=(30., 24.),
                         resolution=100., track_count=10, track_start_region=(1, 7, 0.2, 0.6),
                         track_direction=0.),
                  sim_mode='seasonal', thermals_realization_count=3)
    wind = []
    for s in range(2):
        x, y, ws, wd = wind_lattice((30., 24.), 2.0, phase=2 * np.pi * s / 3)
        wind.append(dict(datetime=(2010, 4, 1 + s, 12), x_km=x, y_km=y, wspeed=ws, wdirn=wd))
    sim = Simulator(cfg, terrain='synthetic', wind=wind)
    assert len(sim.case_ids) == 2
    aspect = sim.get_terrain_aspect()
    seen = []
    for case_no, cid in enumerate(sim.case_ids):
        for k in range(3):
            th = np.load(os.path.join(sim.mode_data_dir, f'{cid}_r{k}_thermals.npy'))
            assert th.dtype == np.float32 and th.shape == (240, 300) and th.max() > 0
            want = thermals.compute_thermals(aspect, 2.0, seed=3 + 7919 * (k + 1) + 104729 * case_no)
            assert np.array_equal(th, np.asarray(want).astype(np.float32))
            assert np.array_equal(th, np.asarray(chain(aspect, 3 + 7919 * (k + 1) + 104729 * case_no),
                                                 dtype=np.float32))
            seen.append(th)
    for i in range(len(seen)):
        for j in range(i):
            assert not np.array_equal(seen[i], seen[j])
    assert len(sim.load_updrafts(sim.case_ids[1])) == 4


def test_call_is_ordered_on_the_current_stream(gpu):
    """Enqueued on a non-default stream behind a long-running producer of its input; correct after that
    stream alone is synchronised."""
    from ssrs_amd import thermals
    base = torch.from_numpy(np.random.default_rng(9).uniform(0., 360., (700, 900))).to(gpu)
    want = thermals.compute_thermals_batch(base, 2.0, SEEDS, dtype=torch.float32)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        aspect = torch.zeros_like(base)
        for _ in range(50):                       # the input is finished late, on this stream only
            aspect = aspect + base / 50.
        aspect = base + 0. * aspect
        got = thermals.compute_thermals_batch(aspect, 2.0, SEEDS, dtype=torch.float32)
    stream.synchronize()
    assert torch.equal(got, want)
