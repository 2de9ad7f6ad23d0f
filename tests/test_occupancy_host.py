"""Track occupancy (K13), the parts that need no device: the Config field and where it stands, the argument checks of
presence.compute_track_occupancy, the library's refusals, and compute_occupancy_map before any run."""
import ctypes as C
import os
from dataclasses import fields

import numpy as np
import pytest
import torch

from ssrs_amd import Config, Simulator, presence

import occupancy_ref as ref


def test_config_field():
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    assert cfg.track_occupancy is False
    names = [f.name for f in fields(Config)]
    assert names[names.index('max_tracks_file_gb') + 1] == 'track_occupancy'
    build = list(dict(_SECTIONS)['MI355X build'])
    assert build[build.index('max_tracks_file_gb') + 1] == 'track_occupancy'
    assert build[-1] == 'turbine_encounter_radius'
    text = str(Config(track_occupancy=True)).split(':::: MI355X build')[1]
    assert 'track_occupancy = True' in text
    assert 'track_occupancy = False' in str(cfg)


def test_reference_on_a_hand_made_case():
    """The reference itself, on a case small enough to count by hand."""
    tracks = [np.array([[0, 0], [0, 1], [0, 0], [5, 5]], dtype=np.int16),        # (5, 5) is outside a 2 x 3 raster
              np.array([[0, 1], [1, 2]], dtype=np.int16), np.zeros((0, 2), dtype=np.int16)]
    counts, per_track = ref.occupancy(tracks, (2, 3))
    assert counts.tolist() == [[1, 2, 0], [0, 0, 1]] and per_track.tolist() == [2, 2, 0]
    assert ref.visits(tracks, (2, 3)).tolist() == [[2, 2, 0], [0, 0, 1]]
    assert ref.clearing_paths(ref.case('memset_path'), 1) == ['memset', 'memset']
    assert ref.clearing_paths(ref.case('borders_33'), 1) == ['unset', 'unset']
    for c in ref.CASES:
        assert all(t.dtype == np.int16 and t.ndim == 2 and t.shape[1] == 2 for t in c['tracks']), c['name']


def test_argument_checks_need_no_device():
    good = [np.zeros((3, 2), dtype=np.int16)]
    for bad in ([np.zeros((3, 2), dtype=np.int32)], [np.zeros((3, 3), dtype=np.int16)], [np.zeros(6, dtype=np.int16)]):
        with pytest.raises(ValueError, match=r'expected int16 \(n, 2\)'):
            presence.compute_track_occupancy(bad, (4, 4))
    for planes in (0, 9, -1):
        with pytest.raises(ValueError, match='planes'):
            presence.compute_track_occupancy(good, (4, 4), planes=planes)
    pts = torch.zeros((3, 2), dtype=torch.int16)
    with pytest.raises(ValueError, match='needs offsets'):
        presence.compute_track_occupancy(pts, (4, 4))
    with pytest.raises(ValueError, match=r'expected int16 \(points, 2\)'):
        presence.compute_track_occupancy(pts.to(torch.int32), (4, 4), offsets=torch.tensor([0, 3]))
    with pytest.raises(ValueError, match=r'expected int16 \(points, 2\)'):
        presence.compute_track_occupancy(pts.reshape(-1), (4, 4), offsets=torch.tensor([0, 3]))
    with pytest.raises(ValueError, match='offsets must be int64'):
        presence.compute_track_occupancy(pts, (4, 4), offsets=torch.tensor([0, 3], dtype=torch.int32))
    with pytest.raises(ValueError, match='offsets goes with a device tensor'):
        presence.compute_track_occupancy(good, (4, 4), offsets=np.array([0, 3]))


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    assert _native.SSRS_OCCUPANCY_MAX_PLANES == presence.MAX_OCCUPANCY_PLANES == 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ssrs_hip.h')).read()
    assert '#define SSRS_OCCUPANCY_MAX_PLANES 8' in header
    assert lib.ssrs_track_occupancy_workspace_bytes(97, 131, 3) == -(-97 * 131 * 4 * 3 // 256) * 256
    assert lib.ssrs_track_occupancy_workspace_bytes(8, 8, 1) == 256
    buf = (C.c_char * 64)()
    good = dict(traj=buf, off=buf, ntracks=1, rows=2, cols=2, planes=1, counts=buf, per_track=None, ws=buf, nbytes=256)
    bad = [dict(traj=None), dict(off=None), dict(counts=None), dict(ws=None), dict(planes=0), dict(planes=9), dict(rows=0),
           dict(rows=32768), dict(cols=0), dict(cols=32768), dict(ntracks=-1), dict(ntracks=2 ** 31),
           dict(traj=C.c_void_p(C.addressof(buf) + 2)), dict(nbytes=255), dict(rows=8, cols=8, planes=2, nbytes=256)]
    for kw in bad:
        a = dict(good, **kw)
        rc = lib.ssrs_track_occupancy(a['traj'], a['off'], a['ntracks'], a['rows'], a['cols'], a['planes'], a['counts'],
                                      a['per_track'], a['ws'], a['nbytes'], None)
        assert rc == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_track_occupancy' in lib.ssrs_last_error(), kw
    # (no tracks: nothing to do, whatever the other arguments point at)
    assert lib.ssrs_track_occupancy(buf, buf, 0, 2, 2, 1, buf, None, buf, 256, None) == _native.SSRS_OK


def test_occupancy_map_before_any_run_raises():
    sim = object.__new__(Simulator)
    sim.track_occupancy_counts = {}
    with pytest.raises(ValueError, match='track_occupancy=True'):
        sim.compute_occupancy_map()
