"""a5 thermals on the MI355X against tests/thermals_ref.py, cell by cell: the set of seeded cells of k_thermal_seeds
equals the restatement's EXACTLY and the amplitudes agree to RTOL_AMP; the zero-padded blur (k_blur_pass) is the stated
order bit for bit and within the bound of scipy; the fused, batched call (k_thermal_fields, and the chain it falls back
to beyond radius 16) is the chain bit for bit AND the restatement's field, so that an error in the seeding rule the two
share no longer cancels; the Simulator's files hold that field.  Shapes, seeds and sigmas: thermals_ref.CASES."""
import functools
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import thermals_ref as ref

pytestmark = pytest.mark.gpu

# The amplitude exp(mu + z / 2) goes through the device's log, sqrt, cos and exp and through the host's libm.  Largest
# relative deviation from the restatement over all seeded cells of all cases, the dense one included (8 064 of the 8 799
# cells), measured on an MI355X (gfx950, ROCm 7.2.0, host glibc libm; profiles/thermal_seeds_parity.md): 1.100e-15, in the
# dense case; 2.1e-16 at most among the sparse ones.  RTOL_AMP is 8 x that, the margin for another libm on the host and
# for other seeds; it may not exceed 1e-13 -- beyond that something other than rounding differs.
MEASURED_AMP = 1.100e-15
RTOL_AMP = 8 * MEASURED_AMP
assert RTOL_AMP <= 1e-13

CASE = {c[0]: c for c in ref.CASES}


@functools.lru_cache(maxsize=None)
def ref_seed_fields(name):
    """[(values, hit)] per seed of a case: the restatement, computed once and shared."""
    _, shape, aspect_of, seeds = CASE[name]
    aspect = aspect_of(shape)
    out = [ref.seed_field(aspect, ref.SCALE, seed) for seed in seeds]
    for values, hit in out:
        values.setflags(write=False), hit.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device_aspect(name):
    _, shape, aspect_of, _ = CASE[name]
    return torch.from_numpy(aspect_of(shape)).to(torch.device('cuda', 0))


@functools.lru_cache(maxsize=None)
def device_seed_fields(name):
    """thermals.thermal_seeds per seed of a case, as device tensors."""
    from ssrs_amd import thermals
    return [thermals.thermal_seeds(device_aspect(name), ref.SCALE, seed) for seed in CASE[name][3]]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def amplitude_deviation(got, want, hit):
    return float((np.abs(got[hit] - want[hit]) / want[hit]).max()) if hit.any() else 0.


def check_seed_field(got, want, hit, label):
    """The three properties of a seed field; returns the largest relative deviation of its amplitudes."""
    assert got.dtype == np.float64
    assert np.array_equal(got != 0., hit), (label, np.argwhere((got != 0.) != hit)[:8])
    assert not got.view(np.int64)[~hit].any(), label                  # +0.0, the border included
    assert not got[~ref.interior(got.shape)].any(), label
    dev = amplitude_deviation(got, want, hit)
    assert (np.abs(got[hit] - want[hit]) <= RTOL_AMP * want[hit]).all(), (label, dev)
    return dev


# ---------------------------------------------------------------------------------------------------- 1. the seeds
@pytest.mark.parametrize('name', ref.CASE_IDS)
def test_seed_field_cell_by_cell(gpu, name):
    seeds = CASE[name][3]
    worst, cells = 0., 0
    for seed, got, (want, hit) in zip(seeds, device_seed_fields(name), ref_seed_fields(name)):
        worst = max(worst, check_seed_field(got.cpu().numpy(), want, hit, (name, seed)))
        cells += int(hit.sum())
    print(f'{name}: {cells} seeded cells over {len(seeds)} seeds, largest amplitude deviation {worst:.3e}')
    assert cells >= (30 if CASE[name][2] is ref.mid_aspect else 1)


def test_dense_seed_field_cell_by_cell(gpu):
    """Aspect NaN everywhere: the device's conversion makes the draw always pass, so every interior cell is seeded and
    its ~8 800 amplitudes sample the Box-Muller tail (|z| up to ~4, u1 down to ~1e-4)."""
    from ssrs_amd import thermals
    aspect = np.full(ref.DENSE_SHAPE, np.nan)
    want, hit = ref.seed_field(aspect, ref.SCALE, ref.DENSE_SEED)
    assert np.array_equal(hit, ref.interior(ref.DENSE_SHAPE)) and hit.sum() == 72 * 112
    got = thermals.thermal_seeds(aspect, ref.SCALE, ref.DENSE_SEED)
    dev = check_seed_field(got, want, hit, 'dense')
    print(f'dense: {int(hit.sum())} seeded cells, largest amplitude deviation {dev:.3e}, amplitudes '
          f'{want[hit].min():.3g} .. {want[hit].max():.3g}')


# ---------------------------------------------------------------------------------------------------- 2. the blur
def check_blur(x, sigma, label):
    """gaussian_blur of the host raster x: the stated order bit for bit, and within the bound of scipy."""
    from ssrs_amd import thermals
    got = thermals.gaussian_blur(x, sigma)
    assert same_bits(got, ref.blur_kernel_order(x, sigma)), (label, sigma)
    dev, lim = float(np.abs(got - ref.scipy_blur(x, sigma)).max()), ref.bound(sigma, x)
    assert dev <= lim, (label, sigma, dev, lim)
    return dev / lim if lim > 0. else 0.


@pytest.mark.parametrize('name', ref.CASE_IDS)
def test_blur_of_the_device_seed_field(gpu, name):
    shape, seeds = CASE[name][1], CASE[name][3]
    for sigma in ref.sigmas_of(shape):
        worst = max(check_blur(x.cpu().numpy(), sigma, (name, seed)) for seed, x in zip(seeds, device_seed_fields(name)))
        print(f'{name} sigma {sigma:g} (R = {ref.radius(sigma)}): largest |blur - scipy| / bound = {worst:.3f}')


@pytest.mark.parametrize('shape', [s for s, _ in ref.TINY] + list(ref.MID_SHAPES), ids=lambda s: '%dx%d' % s)
def test_blur_of_a_dense_signed_raster(gpu, shape):
    """No term is zero, and a raster narrower than 2 R + 1 sums fewer taps than there are weights."""
    x = np.random.default_rng(1).normal(size=shape)
    for sigma in ref.sigmas_of(shape):
        frac = check_blur(x, sigma, shape)
        print(f'{shape} sigma {sigma:g}: largest |blur - scipy| / bound = {frac:.3f}')
        if ref.radius(sigma) == 0:
            from ssrs_amd import thermals
            assert same_bits(thermals.gaussian_blur(x, sigma), x)


# ---------------------------------------------------------------------------------------------------- 3. the fused call
@pytest.mark.parametrize('name', ref.CASE_IDS)
def test_batched_fields_are_the_chain_and_the_restatement(gpu, name):
    """All seeds of the case in one call (42: two launches), the first 3 and the first alone; f64 is the chain bit for
    bit, f32 that value rounded once; and |field - ref.field| <= RTOL_AMP ref.field + bound, the amplitudes' share
    being relative because the weights are non-negative."""
    from ssrs_amd import thermals
    _, shape, _, seeds = CASE[name]
    aspect = device_aspect(name)
    for sigma in ref.sigmas_of(shape):
        chain = [thermals.gaussian_blur(x, sigma) for x in device_seed_fields(name)]
        for count in sorted({1, 3, len(seeds)}):
            f64 = thermals.compute_thermals_batch(aspect, ref.SCALE, seeds[:count], sigma=sigma)
            f32 = thermals.compute_thermals_batch(aspect, ref.SCALE, seeds[:count], dtype=torch.float32, sigma=sigma)
            assert f64.dtype == torch.float64 and f32.dtype == torch.float32 and tuple(f64.shape) == (count,) + shape
            for k in range(count):
                assert torch.equal(f64[k], chain[k]), (name, sigma, count, seeds[k])
                assert torch.equal(f32[k], chain[k].to(torch.float32)), (name, sigma, count, seeds[k])
        got = f64.cpu().numpy()                                          # (the full count)
        worst = 0.
        for k, (values, _) in enumerate(ref_seed_fields(name)):
            want = ref.blur_kernel_order(values, sigma)
            err, tol = np.abs(got[k] - want), RTOL_AMP * want + ref.bound(sigma, values)
            assert (err <= tol).all(), (name, sigma, seeds[k], float(err.max()))
            worst = max(worst, float((err / tol).max()) if tol.max() > 0. else 0.)
        print(f'{name} sigma {sigma:g}: largest |field - ref.field| / tolerance = {worst:.3f}')


def test_dense_field_is_the_restatement(gpu):
    from ssrs_amd import thermals
    aspect = np.full(ref.DENSE_SHAPE, np.nan)
    values, _ = ref.seed_field(aspect, ref.SCALE, ref.DENSE_SEED)
    for sigma in (ref.SIGMA, 4.2):
        got = thermals.compute_thermals_batch(aspect, ref.SCALE, [ref.DENSE_SEED], sigma=sigma)[0]
        assert same_bits(got, thermals.gaussian_blur(thermals.thermal_seeds(aspect, ref.SCALE, ref.DENSE_SEED), sigma))
        want = ref.blur_kernel_order(values, sigma)
        assert (np.abs(got - want) <= RTOL_AMP * want + ref.bound(sigma, values)).all(), sigma


# ---------------------------------------------------------------------------------------------------- 5. the Simulator
def test_simulator_files_hold_the_restated_field(gpu, tmp_path):
    """sim_seed 3, two realisations of one case on a 100 x 120 raster: <case>_r<k>_thermals.npy is the f32 rounding of
    ref.field(aspect, 2.0, sim_seed + 7919 (k + 1), 4.0), to within the fused call's tolerance plus half an f32 ulp."""
    from ssrs_amd import Config, Simulator
    from ssrs_amd.synthetic import synthetic_dem, wind_lattice
    cfg = replace(Config(run_name='thp', out_dir=str(tmp_path), sim_seed=3, region_width_km=(12., 10.), resolution=100.,
                         track_count=4, track_start_region=(1, 7, 0.2, 0.6), track_direction=0.),
                  sim_mode='seasonal', thermals_realization_count=2)
    x, y, ws, wd = wind_lattice((12., 10.), 2.0)
    terrain = dict(Elevation=synthetic_dem((100, 120), 100.), Aspect=ref.mid_aspect((100, 120)))
    sim = Simulator(cfg, terrain=terrain, wind=[dict(datetime=(2010, 4, 1, 12), x_km=x, y_km=y, wspeed=ws, wdirn=wd)])
    assert len(sim.case_ids) == 1
    aspect = np.asarray(sim.get_terrain_aspect(), dtype=np.float64)
    assert same_bits(aspect, terrain['Aspect'])
    seeded = 0
    for k in range(2):
        th = np.load(os.path.join(sim.mode_data_dir, f'{sim.case_ids[0]}_r{k}_thermals.npy'))
        assert th.dtype == np.float32 and th.shape == aspect.shape
        values, hit = ref.seed_field(aspect, 2.0, 3 + 7919 * (k + 1))
        want = ref.blur_kernel_order(values, 4.0)
        tol = RTOL_AMP * want + ref.bound(4.0, values) + 0.5 * np.spacing(np.abs(th)).astype(np.float64)
        assert (np.abs(th.astype(np.float64) - want) <= tol).all(), k
        assert np.array_equal(th != 0., want.astype(np.float32) != 0.)
        seeded += int(hit.sum())
    assert seeded > 0
