"""K11 on the device: ssrs_smooth_reflect behind layers.smooth_orograph, layers.orographic_updraft_improved(...,
smooth_sigma=) and Config.orographic_smoothing through the Simulator.

The reference is scipy.ndimage.gaussian_filter(mode='reflect') of the raster with its non-finite cells set to 0
(tests/smooth_ref.py).  `smooth` is held to 4 (2 R + 3) 2^-53 max|x| absolute over ALL cells -- two passes of R + 1
rounded terms plus the normalisation of the weights, derived, not tuned; `orograph` is the f32 clamp of the device's own
`smooth` bit for bit; `usable` is within the rtol 1e-12 / atol 1e-15 that raster_math.h states for the threshold function.
Wherever the device is compared with itself -- LDS against global memory, a batch against single calls, NULL outputs,
the layers against each other -- bit for bit.  Every case prints its largest deviation from scipy and whether it
matches it bit for bit."""
import ctypes as C
import itertools
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import smooth_ref as ref

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def assert_same_bits(got, want, label=''):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), (f'{label}: {int(bad.sum())} of {bad.size} cells differ; first at {tuple(np.argwhere(bad)[0])}: '
                           f'got {got[bad][0]!r} want {want[bad][0]!r}')


def dev_smooth(x, sigma, path='auto', want=(True, True, True), min_val=ref.MIN_VAL, threshold=ref.THRESHOLD):
    """(smooth, orograph, usable) through the C ABI, None where not asked for: outputs pre-filled with NaN."""
    from ssrs_amd import _native as nat
    from ssrs_amd._device import stream_ptr
    lib = nat.lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    x3 = torch.from_numpy(x if x.ndim == 3 else x[None]).cuda()
    batch, rows, cols = x3.shape
    nbytes = lib.ssrs_smooth_workspace_bytes(rows, cols, batch, sigma)
    work = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    outs = [torch.full(x3.shape, float('nan'), dtype=dt, device='cuda') if w else None
            for w, dt in zip(want, (torch.float64, torch.float32, torch.float64))]
    nat.check(lib.ssrs_smooth_reflect(nat.ptr(x3), sigma, nat.SSRS_SMOOTH_PATH[path], min_val, threshold, nat.ptr(outs[0]),
                                      nat.ptr(outs[1]), nat.ptr(outs[2]), rows, cols, batch, nat.ptr(work), nbytes,
                                      stream_ptr()))
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy().reshape(x.shape) for o in outs)


# ------------------------------------------------------------------------------------------------ (a) the cases
@pytest.mark.parametrize('name, shape, sigma, holes', ref.CASES, ids=ref.CASE_IDS)
def test_smoothing(gpu, name, shape, sigma, holes):
    from ssrs_amd import layers
    x = ref.case_input(shape, holes)
    oro, use, smooth = layers.smooth_orograph(x, sigma, threshold=ref.THRESHOLD, want_smooth=True)
    ref.check_outputs(x, sigma, smooth, oro, use, name)
    for path in ('global',) + (('lds',) if ref.radius(sigma) <= ref.LDS_MAX_RADIUS else ()):
        other = layers.smooth_orograph(x, sigma, threshold=ref.THRESHOLD, want_smooth=True, path=path)
        for a, b in zip((oro, use, smooth), other):
            assert_same_bits(b, a, f'{name} {path}')
    if ref.radius(sigma) == 0:
        assert_same_bits(smooth, ref.sanitised(x), 'the identity')
        assert (oro >= 0.).all() and (oro == 0.).any()
    if ref.radius(sigma) > ref.LDS_MAX_RADIUS:
        with pytest.raises(ValueError, match='does not fit'):
            layers.smooth_orograph(x, sigma, path='lds')


def test_layers_interface(gpu):
    """numpy in, numpy out; a device tensor in, device tensors out; the tuple's shape; the clamp lifted and raised."""
    from ssrs_amd import layers
    x = ref.holed(ref.field((33, 65)))
    oro, use = layers.smooth_orograph(x, 1.3)
    assert isinstance(oro, np.ndarray) and oro.dtype == np.float32 and oro.shape == x.shape and use is None
    t_oro, t_use, t_smooth = layers.smooth_orograph(torch.from_numpy(x).cuda(), 1.3, threshold=0.75, want_smooth=True)
    assert all(t.is_cuda for t in (t_oro, t_use, t_smooth)) and t_use.dtype == t_smooth.dtype == torch.float64
    assert_same_bits(t_oro.cpu().numpy(), oro)
    for min_val in (-np.inf, -0.25, 1.5):
        o, u, s = layers.smooth_orograph(x, 1.3, min_updraft_val=min_val, threshold=0.75, want_smooth=True)
        ref.check_outputs(x, 1.3, s, o, u, f'min {min_val:g}', min_val=min_val)
    assert (layers.smooth_orograph(x, 1.3, min_updraft_val=-np.inf)[0] < 0.).any()
    stack = np.stack([x, ref.field((33, 65), 2)])
    o3, _ = layers.smooth_orograph(stack, 1.3)
    assert o3.shape == (2, 33, 65)
    assert_same_bits(o3[0], oro)


def test_batch_of_3_equals_single_calls(gpu):
    for shape, sigma in (((70, 45), 8.), ((33, 65), 1.3), ((40, 50), 40.)):
        x = np.stack([ref.holed(ref.field(shape, seed)) for seed in range(3)])
        batch = dev_smooth(x, sigma)
        for b in range(3):
            for g, s in zip(batch, dev_smooth(x[b], sigma)):
                assert_same_bits(g[b], s, f'{shape} case {b}')


def test_null_outputs(gpu):
    """Any of the three outputs may be NULL: the others keep their bits, on both paths."""
    x = ref.holed(ref.field((33, 65)))
    for path in ('lds', 'global'):
        full = dev_smooth(x, 8., path)
        for want in itertools.product((False, True), repeat=3):
            if not any(want):
                continue
            for w, g, f in zip(want, dev_smooth(x, 8., path, want=want), full):
                if w:
                    assert_same_bits(g, f, f'{path} {want}')
                else:
                    assert g is None


# ------------------------------------------------------------------------------------------------ (b) the improved updraft
def make_dem(shape):
    """The DEM of test_gpu_shelter_sector.py, with its hole."""
    r, c = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    z = 1500. + 180. * np.sin(r / 7.3) * np.cos(c / 9.1) + 90. * np.sin((r + 2. * c) / 5.7) + 2.5 * r - 1.5 * c
    z[shape[0] // 2 - 1:shape[0] // 2 + 2, shape[1] // 3:shape[1] // 3 + 3] = np.nan
    return z.astype(np.float32).astype(np.float64)


def test_improved_updraft_smoothed(gpu):
    """smooth_sigma = 80 m at 10 m (sigma 8 cells, R = 32) is smooth_orograph of the call's own unclamped f32 field, the
    non-finite cells entering as 0; Sx is unaffected; smooth_sigma = 0 is today's call."""
    from ssrs_amd import layers
    z, res = make_dem((70, 45)), 10.
    r, c = np.mgrid[0:70, 0:45].astype(np.float64)
    ws, wd = 8. + 3. * np.sin(c / 17.) * np.cos(r / 13.), 200. + 110. * np.sin(c / 7. + r / 9.)
    ws[5, 6] = np.nan
    for kwargs in (dict(), dict(sector=15.)):
        for wspeed, wdirn in ((10., 237.3), ([10., 7.], [270., 45.]), (ws, wd)):
            raw, _, sx_raw = layers.orographic_updraft_improved(z, res, wspeed, wdirn, min_updraft_val=-np.inf, want_sx=True,
                                                                **kwargs)
            got = layers.orographic_updraft_improved(z, res, wspeed, wdirn, threshold=0.75, want_sx=True, smooth_sigma=80.,
                                                     **kwargs)
            want = layers.smooth_orograph(raw, 8., threshold=0.75)
            assert_same_bits(got[0], want[0], 'orograph')
            assert_same_bits(got[1], want[1], 'usable')
            assert_same_bits(got[2], sx_raw, 'Sx')
            assert np.isfinite(got[0]).all() and (got[0] != np.where(np.isfinite(raw), raw, 0.)).mean() > 0.5
            plain = layers.orographic_updraft_improved(z, res, wspeed, wdirn, threshold=0.75, want_sx=True, **kwargs)
            off = layers.orographic_updraft_improved(z, res, wspeed, wdirn, threshold=0.75, want_sx=True, smooth_sigma=0.,
                                                     **kwargs)
            for a, b in zip(off, plain):
                assert_same_bits(a, b, 'smooth_sigma = 0')
    # no orograph asked for: the usable updraft alone, the same bits
    none, use = layers.orographic_updraft_improved(z, res, 10., 237.3, threshold=0.75, want_orograph=False, smooth_sigma=80.)
    full = layers.orographic_updraft_improved(z, res, 10., 237.3, threshold=0.75, smooth_sigma=80.)
    assert none is None
    assert_same_bits(use, full[1])


# ------------------------------------------------------------------------------------------------ (c) Simulator
def test_simulator_uniform_mode(gpu, tmp_path):
    from ssrs_amd import Config, Simulator, layers
    cfg = Config(run_name='smooth', out_dir=str(tmp_path), sim_seed=30, region_width_km=(6., 5.), resolution=100.,
                 track_count=8, track_start_region=(1, 5, 0.2, 0.6), track_direction=0., orographic_model='improved',
                 orographic_smoothing='gaussian')
    sim = Simulator(cfg, terrain='synthetic')
    assert sim.gridsize == (50, 60)
    dem = sim.get_terrain_elevation()
    oro, _, sx = layers.orographic_updraft_improved(dem, 100., 10., 270., want_sx=True, smooth_sigma=80.)
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, 's10d270_orograph.npy')), oro)
    assert_same_bits(np.load(os.path.join(sim.mode_data_dir, 's10d270_sx.npy')), sx.astype(np.float32))
    unsmoothed, _ = layers.orographic_updraft_improved(dem, 100., 10., 270.)
    lift = unsmoothed > 0.01                    # (sigma is 0.8 cells here: the flat lee side stays 0)
    assert (oro[lift] != unsmoothed[lift]).mean() > 0.5
    assert sim._get_id_string('s10d270', 0) == 's10d270_d0_t75_fluidflow-sx500h80g80_r0'
    sim.simulate_tracks()
    assert sorted(os.listdir(sim.mode_data_dir)) == [
        's10d270_d0_t75_fluidflow-sx500h80g80_r0_potential.npy', 's10d270_d0_t75_fluidflow-sx500h80g80_r0_tracks.pkl',
        's10d270_orograph.npy', 's10d270_sx.npy']
    # 'none' in the same out_dir / run_name: today's names and bytes, and the smoothed run's potential is not picked up
    sim0 = Simulator(replace(cfg, orographic_smoothing='none'), terrain='synthetic')
    assert sim0._get_id_string('s10d270', 0) == 's10d270_d0_t75_fluidflow-sx500h80_r0'
    assert_same_bits(np.load(os.path.join(sim0.mode_data_dir, 's10d270_orograph.npy')), unsmoothed)
    sim0.simulate_tracks()
    names = sorted(os.listdir(sim0.mode_data_dir))
    assert 's10d270_d0_t75_fluidflow-sx500h80_r0_potential.npy' in names and len(names) == 6
    assert not np.array_equal(np.load(os.path.join(sim0.mode_data_dir, 's10d270_d0_t75_fluidflow-sx500h80_r0_potential.npy')),
                              np.load(os.path.join(sim0.mode_data_dir, 's10d270_d0_t75_fluidflow-sx500h80g80_r0_potential.npy')))
