"""The Gaussian smoothing of the improved orographic updraft (K11) on the host: the numpy statements of the index rule
(tests/smooth_ref.py) against scipy, the Config fields, the model's width, the ValueErrors and SSRS_ERR_INVALID returns
that need no GPU, and the id string."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import smooth_ref as ref

BAD_SMOOTHING = [('gauss', 0., 'orographic_smoothing'), ('gaussian', -1., 'orographic_smooth_sigma'),
                 ('gaussian', float('nan'), 'orographic_smooth_sigma'), ('gaussian', float('inf'), 'orographic_smooth_sigma'),
                 ('none', -1., 'orographic_smooth_sigma'), ('gaussian', 12820., 'more than 512')]    # R = 513 at 100 m


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize('shape, sigma', [((3, 5), 2.), ((1, 7), 1.3), ((2, 2), 0.8), ((70, 45), 8.), ((33, 65), 30.)])
def test_numpy_statements_against_scipy(shape, sigma):
    """The index rule, summed in ascending tap order and in the kernel's order, against gaussian_filter(mode='reflect'):
    both within 4 (2 R + 3) 2^-53 max|x| on every cell, with and without non-finite cells."""
    for x in (ref.field(shape), ref.case_input(shape, True)):
        want = ref.scipy_smooth(x, sigma)
        for name, fn in (('ascending', ref.numpy_smooth), ('kernel order', ref.kernel_order_smooth)):
            dev = float(np.abs(fn(x, sigma) - want).max())
            print(f'{shape} sigma {sigma:g} {name}: largest deviation {dev:.3e}, bound {ref.bound(sigma, x):.3e}')
            assert dev <= ref.bound(sigma, x)


def test_reflect_index_and_weights():
    assert list(ref.reflect_index(np.arange(-8, 12), 4)) == [0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3]
    assert list(ref.reflect_index(np.arange(-3, 4), 1)) == [0] * 7
    assert [ref.radius(s) for s in (0.1, 0.124, 0.125, 0.8, 1.3, 2., 8., 30., 40.)] == [0, 0, 1, 3, 5, 8, 32, 120, 160]
    R, w = ref.weights(0.1)
    assert R == 0 and list(w) == [1.]
    R, w = ref.weights(8.)
    assert abs(w[0] + 2. * w[1:].sum() - 1.) < 1e-15 and (np.diff(w) < 0.).all()


# ------------------------------------------------------------------------------------------------ Config
def test_config_defaults_and_placement():
    from ssrs_amd.config import Config, _SECTIONS
    cfg = Config()
    assert cfg.orographic_smoothing == 'none' and cfg.orographic_smooth_sigma == 0.
    names = [f.name for f in dataclasses.fields(cfg)]
    at = names.index('orographic_sx_step')
    assert names[at + 1:at + 4] == ['orographic_smoothing', 'orographic_smooth_sigma', 'hist_safe_tracks']
    section = list(dict(_SECTIONS)['Updraft computation'])
    at = section.index('movement_model')
    assert section[at - 2:at] == ['orographic_smoothing', 'orographic_smooth_sigma']
    block = str(dataclasses.replace(cfg, orographic_smoothing='gaussian', orographic_smooth_sigma=25.))
    block = block.split(':::: Updraft computation')[1].split('::::')[0]
    assert 'orographic_smoothing = gaussian' in block and 'orographic_smooth_sigma = 25.0' in block


def test_smoothing_sigma_m():
    from ssrs_amd import layers
    assert layers.smoothing_sigma_m(80., 0.) == 80.
    assert layers.smoothing_sigma_m(400., 0.) == 300.
    assert layers.smoothing_sigma_m(80., 25.) == 25.
    assert layers.smoothing_sigma_m(0.) == 16.
    for bad in (-1., float('nan'), float('inf'), 'wide'):
        with pytest.raises(ValueError, match='orographic_smooth_sigma'):
            layers.smoothing_sigma_m(80., bad)


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda unavailable, and any attempt to reach the device fails the test."""
    import torch
    from ssrs_amd import _device, layers
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    for module in (_device, layers):
        for name in ('device', 'to_dev', 'float_dev'):
            monkeypatch.setattr(module, name, boom)


@pytest.mark.parametrize('mode, sigma, match', BAD_SMOOTHING)
def test_bad_smoothing_is_refused_before_device_work(tmp_path, no_gpu, mode, sigma, match):
    from ssrs_amd import Config, Simulator
    cfg = Config(run_name='bad', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100.,
                 orographic_model='improved', orographic_smoothing=mode, orographic_smooth_sigma=sigma)
    with pytest.raises(ValueError, match=match):
        Simulator(cfg, terrain=np.zeros((50, 60)))
    assert not (tmp_path / 'bad').exists()


def test_good_smoothing_reaches_the_device(tmp_path, no_gpu):
    """R = 512 exactly at this resolution passes the host checks: the constructor gets as far as the device."""
    from ssrs_amd import Config, Simulator
    cfg = Config(run_name='good', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100.,
                 orographic_model='improved', orographic_smoothing='gaussian', orographic_smooth_sigma=12810.)
    with pytest.raises(AssertionError, match='device work before'):
        Simulator(cfg, terrain=np.zeros((50, 60)))


def test_original_model_ignores_the_smoothing_fields(tmp_path, no_gpu):
    from ssrs_amd import Config, Simulator
    cfg = Config(run_name='orig', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100.,
                 orographic_smoothing='gauss', orographic_smooth_sigma=-1.)
    with pytest.raises(AssertionError, match='device work before'):
        Simulator(cfg, terrain=np.zeros((50, 60)))


@pytest.mark.parametrize('kwargs, match', [
    (dict(sigma_cells=0.), 'sigma_cells'), (dict(sigma_cells=-2.), 'sigma_cells'), (dict(sigma_cells=float('nan')), 'sigma_cells'),
    (dict(sigma_cells=float('inf')), 'sigma_cells'), (dict(sigma_cells=128.2), 'more than 512'),
    (dict(sigma_cells=2., path='fast'), 'path'), (dict(sigma_cells=2., threshold=0.), 'threshold'),
    (dict(sigma_cells=2., min_updraft_val=float('nan')), 'min_updraft_val')])
def test_layers_refuse_bad_arguments_before_device_work(no_gpu, kwargs, match):
    from ssrs_amd import layers
    with pytest.raises(ValueError, match=match):
        layers.smooth_orograph(np.zeros((8, 9), np.float32), **kwargs)


def test_layers_refuse_a_bad_smooth_sigma_before_device_work(no_gpu):
    from ssrs_amd import layers
    z = np.zeros((8, 9))
    for sigma, match in ((-80., 'smooth_sigma'), (float('nan'), 'smooth_sigma'), (1290., 'more than 512')):
        with pytest.raises(ValueError, match=match):
            layers.orographic_updraft_improved(z, 10., 10., 270., dmax=50., smooth_sigma=sigma)
    with pytest.raises(ValueError, match='raster'):
        layers.smooth_orograph(np.zeros(8, np.float32), 2.)


# ------------------------------------------------------------------------------------------------ C ABI
def test_library_refuses_bad_arguments_without_a_gpu():
    """Every check comes before any GPU work: the calls below run where there is no device."""
    from ssrs_amd import _native as nat
    lib = nat.lib()
    buf = (C.c_double * 4096)()
    p = C.cast(buf, C.c_void_p)

    def call(inp=p, sigma=2., path=0, min_val=0., thr=0.75, smooth=p, oro=None, use=None, rows=8, cols=8, batch=1,
             work=p, nbytes=C.sizeof(buf)):
        return lib.ssrs_smooth_reflect(inp, sigma, path, min_val, thr, smooth, oro, use, rows, cols, batch, work, nbytes, None)
    for kwargs, text in [(dict(rows=0), b'rows, cols, batch'), (dict(cols=0), b'rows, cols, batch'),
                         (dict(batch=0), b'rows, cols, batch'), (dict(sigma=0.), b'sigma'), (dict(sigma=-1.), b'sigma'),
                         (dict(sigma=float('nan')), b'sigma'), (dict(sigma=float('inf')), b'sigma'),
                         (dict(sigma=128.2), b'more than 512'), (dict(sigma=1e300), b'more than 512'), (dict(path=3), b'path'),
                         (dict(path=1, sigma=32.2), b'does not fit'), (dict(smooth=None), b'all NULL'),
                         (dict(use=p, thr=0.), b'positive threshold'), (dict(use=p, thr=-1.), b'positive threshold'),
                         (dict(min_val=float('nan')), b'min_updraft_val'), (dict(inp=None), b'in is NULL'),
                         (dict(work=None), b'workspace'), (dict(nbytes=8 * 64 + 255), b'workspace too small')]:
        assert call(**kwargs) == nat.SSRS_ERR_INVALID, kwargs
        assert b'ssrs_smooth_reflect' in lib.ssrs_last_error() and text in lib.ssrs_last_error(), (kwargs, lib.ssrs_last_error())
    with pytest.raises(ValueError):
        nat.check(call(sigma=0.))
    # sigma 128.1: R = int(512.9) = 512 is the last radius served
    assert lib.ssrs_smooth_workspace_bytes(8, 8, 1, 128.1) == (513 * 8 + 255) // 256 * 256 + 8 * 64
    assert lib.ssrs_smooth_workspace_bytes(8, 8, 1, 128.2) == 0
    assert lib.ssrs_smooth_workspace_bytes(70, 45, 1, 8.) == lib.ssrs_smooth_workspace_bytes(70, 45, 8, 8.) == 512 + 8 * 70 * 45
    for bad in ((0, 8, 1, 2.), (8, 0, 1, 2.), (8, 8, 0, 2.), (8, 8, 1, 0.), (8, 8, 1, float('nan'))):
        assert lib.ssrs_smooth_workspace_bytes(*bad) == 0


# ------------------------------------------------------------------------------------------------ the id string
def test_id_string_carries_the_width():
    from ssrs_amd import Config, Simulator

    def ident(**kwargs):
        sim = object.__new__(Simulator)
        Config.__init__(sim, **kwargs)
        return sim._get_id_string('s10d270')
    plain = ident(orographic_model='improved')
    assert plain == 's10d270_d0_t75_fluidflow-sx500h80'
    assert ident(orographic_model='improved', orographic_smoothing='gaussian') == plain + 'g80'
    assert ident(orographic_model='improved', orographic_smoothing='gaussian', orographic_smooth_sigma=25.5) == plain + 'g25.5'
    assert ident(orographic_model='improved', orographic_smoothing='gaussian', orographic_height=400.) == \
        's10d270_d0_t75_fluidflow-sx500h400g300'
    assert ident(orographic_model='improved', orographic_sx_sector=15., orographic_smoothing='gaussian') == \
        's10d270_d0_t75_fluidflow-sx500h80a15s5g80'
    assert ident(orographic_model='improved', orographic_smooth_sigma=25.) == plain            # 'none': no smoothing
    assert ident(orographic_smoothing='gaussian') == 's10d270_d0_t75_fluidflow'                 # the original model ignores it
