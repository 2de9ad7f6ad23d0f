"""tests/stream_order.py without a GPU: the header-derived list of streamed exports, and the proxy's handle check on a
stand-in library."""
import ctypes as C
import types

import pytest

import stream_order
import test_native_abi as abi


def _letter_codes():
    from ssrs_amd import _native as nat
    return {**nat.PROTOTYPES, **nat.PASSAGE_PROTOTYPES, **nat.TRANSIT_PROTOTYPES, **nat.COLLISION_PROTOTYPES,
            **nat.SITE_PROTOTYPES}


def test_streamed_exports_are_those_of_the_headers():
    """Every export whose prototype ends in a pointer and whose last header parameter is named `stream` is in the list, and
    nothing else is: no *_bytes query, no recorder helper, nothing without arguments."""
    params = stream_order.header_parameters()
    codes = _letter_codes()
    assert sorted(params) == sorted(codes)                          # the five headers, every export once
    assert set(abi.declared_prototypes()) <= set(params)
    streamed = stream_order.streamed_exports()
    assert streamed == sorted(set(streamed))
    for name, ps in params.items():
        assert len(ps) == len(codes[name].partition(':')[2]), name
        ends_in_pointer = codes[name].endswith('p')
        named_stream = bool(ps) and ps[-1][1] == 'stream'
        assert (name in streamed) == (ends_in_pointer and named_stream), name
        assert not named_stream or ps[-1][0] == 'void *', (name, ps[-1])
        assert 'stream' not in [p for _, p in ps[:-1]], name         # (a stream anywhere but last would escape the proxy)
    assert not [n for n in streamed if n.endswith('_bytes') or n.endswith('_bytes_ex') or 'recorder' in n]
    for name in ('ssrs_traj_recorder_create', 'ssrs_traj_recorder_destroy', 'ssrs_traj_recorder_complete',
                 'ssrs_traj_recorder_used', 'ssrs_tracks_workspace_bytes_ex', 'ssrs_potential_workspace_bytes',
                 'ssrs_track_passage_workspace_bytes', 'ssrs_last_error', 'ssrs_track_params_init', 'ssrs_device_info',
                 'ssrs_projection_init_albers', 'ssrs_tracks_roam_feed_counts'):
        assert name in params and name not in streamed, name
    for name in ('ssrs_tracks_simulate', 'ssrs_tracks_simulate_h64', 'ssrs_tracks_simulate_rec', 'ssrs_tracks_gather',
                 'ssrs_potential_solve', 'ssrs_presence_count', 'ssrs_hist_reduce', 'ssrs_track_passage',
                 'ssrs_rotor_transits', 'ssrs_rotor_collision_risk', 'ssrs_site_collision_risk', 'ssrs_uniform_selftest',
                 'ssrs_roam_pair_word_selftest', 'ssrs_roam_tables_selftest'):
        assert name in streamed, name
    assert len(streamed) == 55
    assert set(stream_order.EXCLUSIONS) == {'ssrs_hist_reduce'} and set(stream_order.EXCLUSIONS) <= set(streamed)


class _FakeLib:
    """Two exports that record what they were given."""

    def __init__(self):
        self.got = []

    def ssrs_threshold_updraft(self, *args):
        self.got.append(('ssrs_threshold_updraft', args))
        return 7

    def ssrs_blur_workspace_bytes(self, *args):
        self.got.append(('ssrs_blur_workspace_bytes', args))
        return 4096


def test_handle_check_on_a_stand_in_library(monkeypatch):
    """A NULL stream and another stream than the thread's current one are refused by name before the library is called; the
    right handle goes through with its arguments unchanged; exports without a stream are not touched; watching() puts the
    library and _native.ptr back, also after an exception."""
    import torch
    from ssrs_amd import _native as nat
    fake = _FakeLib()
    monkeypatch.setattr(nat, '_lib', fake)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda: types.SimpleNamespace(cuda_stream=0x1230))
    real_ptr = nat.ptr
    with stream_order.watching('check') as proxy:
        assert nat.lib() is proxy and nat.ptr is not real_ptr
        args = (None, 0.75, None, 4, C.c_void_p(0x1230))
        assert nat.lib().ssrs_threshold_updraft(*args) == 7
        assert fake.got[-1][0] == 'ssrs_threshold_updraft' and all(a is b for a, b in zip(fake.got[-1][1], args))
        assert nat.lib().ssrs_blur_workspace_bytes(3, 5, 2.) == 4096 and fake.got[-1][1] == (3, 5, 2.)
        for bad, word in ((None, 'NULL stream'), (C.c_void_p(0), 'NULL stream'), (C.c_void_p(None), 'NULL stream'),
                          (C.c_void_p(0x4560), 'current stream')):
            with pytest.raises(AssertionError, match='ssrs_threshold_updraft.*' + word):
                nat.lib().ssrs_threshold_updraft(None, 0.75, None, 4, bad)
        assert len(fake.got) == 2 and len(proxy.problems) == 4
        assert [c[:2] for c in proxy.calls] == [('ssrs_threshold_updraft', 0x1230)] + [('ssrs_threshold_updraft', 0)] * 3 + \
            [('ssrs_threshold_updraft', 0x4560)]
        assert proxy.seen() == ['ssrs_threshold_updraft']
    assert nat._lib is fake and nat.ptr is real_ptr
    with pytest.raises(ZeroDivisionError):
        with stream_order.watching('late_null'):
            1 / 0
    assert nat._lib is fake and nat.ptr is real_ptr
