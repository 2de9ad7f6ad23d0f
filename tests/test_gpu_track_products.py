"""The track products of Simulator.simulate_tracks (ssrs_amd/products.py) together: every product switched on at once
writes what each writes alone, whatever the number of sub-batches, and a track-sharded item issues its collectives in the
one order the module's docstring states.  Only the public API and the four rank hooks Simulator documents for tests are
used.  Every comparison is byte equality; every run is 64 tracks on 50 x 60 cells."""
import os
import shutil
from dataclasses import replace

import numpy as np
import pytest

from test_gpu_rotor_time import _turbines

pytestmark = pytest.mark.gpu

STEMS = [f's10d270_d0_t75_fluidflow_r{k}' for k in (0, 1)]
NTURB, CELLS = 5, 50 * 60

HEIGHTS = dict(flight_height=True, rotor_geometry='turbine', rotor_clearance=100.)
UNION = dict(turbine_encounter_radius=250., track_occupancy=True, track_passage_radius=250., flight_time=True,
             rotor_exposure_time=True, rotor_transits=True, collision_risk=True, site_collision_risk=True, **HEIGHTS)

# what every rank of a track-sharded run issues per (case, realisation), in this order: (collective, dtype, elements)
COLLECTIVES = [
    ('allreduce_sum', 'int64', NTURB),              # encounters: tracks per turbine
    ('reduce_histogram', 'int32', CELLS),           # occupancy
    ('reduce_histogram', 'int32', CELLS),           # passage
    ('reduce_histogram', 'int32', CELLS),           # heights: the rotor-zone raster
    ('allreduce_sum', 'int64', NTURB),              # rotor-zone encounters
    ('allreduce_sum', 'int64', 2 * NTURB),          # cylinders: [tracks, points]
    ('allreduce_sum', 'int64', NTURB),              # exposure time
    ('allreduce_sum', 'int64', 2 * NTURB),          # collision risk
    ('reduce_histogram', 'int64', 2 * CELLS),       # site risk
    ('reduce_histogram', 'int64', 2 * CELLS),       # site transits
    ('allreduce_sum', 'int64', 3 * NTURB),          # transits: [tracks, with, against]
    ('reduce_histogram', 'int64', CELLS),           # flight time
    ('reduce_histogram', 'int64', CELLS),           # flight time in the rotor zone
    ('reduce_histogram', 'int32', CELLS),           # last: the presence histogram
]


def _config(out_dir, name, **options):
    from ssrs_amd import Config
    return Config(run_name=name, out_dir=str(out_dir), sim_seed=7, region_width_km=(6., 5.), resolution=100., track_count=64,
                  track_start_region=(1, 5, 0.2, 0.6), track_direction=0., thermals_realization_count=1, **options)


def _run(out_dir, name, cls=None, **options):
    """The simulator of one finished run, with the number of sub-batches of every item in `sim.nparts`."""
    from ssrs_amd import Simulator
    sim = (cls or Simulator)(_config(out_dir, name, **options), terrain='synthetic', turbines=_turbines())
    step, sim.nparts = sim._step_case, []

    def counted(*args, **kwargs):
        batch = step(*args, **kwargs)
        sim.nparts.append(len(batch.parts))
        return batch
    sim._step_case = counted
    sim.simulate_tracks()
    return sim


def _files(sim):
    return {name: open(os.path.join(sim.mode_data_dir, name), 'rb').read() for name in os.listdir(sim.mode_data_dir)}


@pytest.fixture(scope='module')
def union(gpu, tmp_path_factory):
    sim = _run(tmp_path_factory.mktemp('union'), 'union', **UNION)
    files = _files(sim)
    products = ('turbine_encounters', 'occupancy', 'passage', 'rotor_presence', 'flight_heights', 'rotor_turbine_encounters',
                'turbine_rotor_encounters', 'turbine_rotor_time', 'turbine_collision_risk', 'track_collision_risk',
                'site_collision_risk', 'site_transits', 'turbine_rotor_transits', 'residence_time', 'rotor_residence_time',
                'flight_times')
    assert {f'{s}_{p}.npy' for s in STEMS for p in products} | {f'{s}_tracks.pkl' for s in STEMS} <= set(files)
    assert sim.nparts == [1, 1]
    return files


NARROWER = {
    'encounters': (dict(turbine_encounter_radius=250.), ('turbine_encounters.npy', 'tracks.pkl')),
    'occupancy': (dict(track_occupancy=True), ('occupancy.npy',)),
    'passage': (dict(track_passage_radius=250.), ('passage.npy',)),
    # (exposure and flight_time off: the rotor call right behind the heights)
    'cylinders': (HEIGHTS, ('rotor_presence.npy', 'flight_heights.npy', 'turbine_rotor_encounters.npy')),
    # (the transit kernel in place of the collision-risk kernel, which promises the same transits)
    'transits': ({**UNION, 'collision_risk': False},
                 ('turbine_rotor_transits.npy', 'turbine_rotor_time.npy', 'site_collision_risk.npy', 'flight_times.npy')),
    'no_pickle': ({**UNION, 'save_tracks': False}, ('turbine_collision_risk.npy', 'rotor_residence_time.npy')),
}


@pytest.mark.parametrize('name', list(NARROWER))
def test_products_do_not_see_each_other(gpu, tmp_path, union, name):
    """A run with fewer products writes, for each of its files, the bytes the run with all of them writes."""
    options, expected = NARROWER[name]
    files = _files(_run(tmp_path, name, **options))
    assert set(files) <= set(union), sorted(set(files) - set(union))
    assert {f'{s}_{e}' for s in STEMS for e in expected} <= set(files)
    assert ('save_tracks' in options) == (not [f for f in files if f.endswith('.pkl')])
    for fname, data in files.items():
        assert data == union[fname], fname


def test_sub_batches_accumulate(gpu, tmp_path, union):
    """hist_safe_tracks = 24 steps the 64 tracks as 22 + 22 + 20: every product file and the pickle are the one batch's."""
    sim = _run(tmp_path, 'parts', hist_safe_tracks=24, **UNION)
    assert sim.nparts == [3, 3]
    files = _files(sim)
    assert set(files) == set(union)
    for fname, data in files.items():
        assert data == union[fname], fname


def test_collective_order_of_a_track_sharded_item(gpu, tmp_path, monkeypatch):
    """Both ranks of a track-sharded pair issue COLLECTIVES for every item, and only rank 0 writes."""
    from ssrs_amd import Simulator, distributed
    log = []

    def record(kind):
        def collective(values, **kwargs):
            log.append((kind, str(values.dtype).replace('torch.', ''), int(np.prod(values.shape))))
            return values
        return collective
    monkeypatch.setattr(distributed, 'reduce_histogram', record('reduce_histogram'))

    def ranked(rank):
        class Ranked(Simulator):
            _world = staticmethod(lambda: 2)
            _rank = staticmethod(lambda: rank)
            _barrier = staticmethod(lambda: None)
            _allreduce_sum = staticmethod(record('allreduce_sum'))
        return Ranked

    options = {**UNION, 'save_tracks': False}
    first = _run(tmp_path, 'rank0', cls=ranked(0), **options)
    print(log)
    assert first._shards_tracks() and first.nparts == [1, 1]
    assert log == COLLECTIVES * 2
    written = set(os.listdir(first.mode_data_dir))
    assert {f'{s}_site_transits.npy' for s in STEMS} <= written
    # rank 1 reads the rasters rank 0 wrote (its constructor computes none) and writes nothing
    inputs = {f for f in written if f.endswith(('_orograph.npy', '_thermals.npy', '_potential.npy'))}
    second_dir = os.path.join(tmp_path, 'rank1', os.path.relpath(first.mode_data_dir, os.path.join(tmp_path, 'rank0')))
    os.makedirs(second_dir)
    for fname in inputs:
        shutil.copy(os.path.join(first.mode_data_dir, fname), second_dir)
    del log[:]
    second = _run(tmp_path, 'rank1', cls=ranked(1), **options)
    print(log)
    assert log == COLLECTIVES * 2
    assert set(os.listdir(second.mode_data_dir)) == inputs
    for key, three in first.turbine_rotor_transits.items():
        assert second.turbine_rotor_transits[key].shape == three.shape == (NTURB, 3)
