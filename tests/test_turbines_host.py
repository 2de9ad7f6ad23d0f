"""Turbines and turbine encounters, the parts that need no GPU: the `Turbines` table and its filter (the stand-in for
reference ssrs/turbines.py:68-95), the cull lists of the encounter kernel, the window and kernel radius of
the wind-plant presence map (simulator.py:557-592), Config / constructor checks, the library's argument validation and
the one collective of a track-sharded run."""
import ctypes as C
import os

import numpy as np
import pytest

from ssrs_amd import turbines as tb
from ssrs_amd import Config, presence
from ssrs_amd.simulator import Simulator


def _table():
    # bounds (0, 0, 7900, 5900): a 60 x 80 raster at 100 m
    return dict(x=np.array([0., 7900., 4000., 4000., 8000., 1000., 1000., -0.001]),
                y=np.array([0., 5900., 5900.0001, 3000., 3000., 2000., 2500., 100.]),
                p_name=np.array(['A', 'B', 'A', 'B', 'A', 'A', 'A', 'B'], dtype=object),
                t_hh=np.array([50., 80., 80., 50., 80., 49.999, 10000., 80.]),
                t_rd=np.full(8, 100.))


def test_filter_keeps_the_bounds_and_the_minimum_hub_height():
    t = tb.Turbines(_table(), bounds=(0., 0., 7900., 5900.), min_hubheight=50.)
    # 0: on the south-west corner, hub height == minimum; 1: on the north-east corner; 2: y just outside; 3: inside, hub ==
    # minimum; 4: x outside; 5: hub below; 6: hub 10000 (between(..., 'left') is open there); 7: x just outside
    x, y = t.get_locations()
    assert len(t) == 3 and np.array_equal(x, [0., 7900., 4000.]) and np.array_equal(y, [0., 5900., 3000.])
    assert list(t.get_project_names()) == ['A', 'B']
    xa, ya = t.get_locations_for_this_project('A')
    assert np.array_equal(xa, [0.]) and np.array_equal(ya, [0.])
    xb, yb = t.get_locations_for_this_project('B')
    assert np.array_equal(xb, [7900., 4000.]) and np.array_equal(yb, [5900., 3000.])
    xn, yn = t.get_locations_for_this_project('nowhere')
    assert xn.size == 0 and yn.size == 0
    cells = t.cell_coordinates((0., 0., 7900., 5900.), 100.)
    assert cells.dtype == np.float64 and np.array_equal(cells, [[0., 0.], [79., 59.], [40., 30.]])
    # no hub heights: only the bounds filter; no bounds: everything
    bare = tb.Turbines(dict(x=[1., 9000.], y=[1., 1.]), bounds=(0., 0., 7900., 5900.))
    assert len(bare) == 1
    assert len(tb.Turbines(dict(x=[1., 9000.], y=[1., 1.]))) == 2
    with pytest.raises(KeyError):
        bare.get_project_names()
    with pytest.raises(ValueError, match="'y'"):
        tb.Turbines(dict(x=[1.]))
    with pytest.raises(ValueError, match='shape'):
        tb.Turbines(dict(x=[1., 2.], y=[1., 2.], t_hh=[80.]))


def test_turbines_does_not_import_pandas_and_takes_a_dataframe():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from ssrs_amd import turbines as tb; "
            "t = tb.Turbines(dict(x=[1., 2.], y=[3., 4.], p_name=['P', 'Q'])); "
            "assert list(t.get_project_names()) == ['P', 'Q'] and t.get_locations_for_this_project('Q')[0][0] == 2.; "
            "assert 'pandas' not in sys.modules" % root)
    subprocess.run([sys.executable, '-c', code], check=True)
    pd = pytest.importorskip('pandas')
    frame = pd.DataFrame(_table())
    t = tb.Turbines(frame, bounds=(0., 0., 7900., 5900.), min_hubheight=50.)
    ref = frame[frame['x'].between(0., 7900., 'both') & frame['y'].between(0., 5900., 'both') &
                frame['t_hh'].between(50., 10000., 'left')]                     # turbines.py:68-71
    assert np.array_equal(t.get_locations()[0], ref['x'].values) and np.array_equal(t.get_locations()[1], ref['y'].values)
    assert list(t.get_project_names()) == list(ref['p_name'].unique())
    assert np.array_equal(t.get_locations_for_this_project('B')[0], ref.loc[ref['p_name'] == 'B', 'x'].values)
    assert t.dframe.shape == ref.shape and list(t.dframe.columns) == list(ref.columns)
    again = tb.Turbines(t)
    assert len(again) == len(t)


@pytest.mark.parametrize('radius', [0., 0.5, 2.5, 40.])
def test_build_bins_lists_every_turbine_that_can_reach_a_cell(radius):
    rows, cols = 70, 90                                      # neither a multiple of 32: 3 x 3 bins
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(-50., cols + 50., 40), rng.uniform(-50., rows + 50., 40)], 1)
    xy[:6] = [[0., 0.], [89., 69.], [31.5, 31.5], [32., 64.], [-0.5, 10.], [-45., -45.]]
    assert ((xy[:, 0] < 0) | (xy[:, 0] > cols - 1) | (xy[:, 1] < 0) | (xy[:, 1] > rows - 1)).sum() >= 5
    bin_start, bin_items = tb.build_bins(xy, radius, (rows, cols))
    assert bin_start.dtype == np.int32 and bin_items.dtype == np.int32
    assert bin_start.shape == (3 * 3 + 1,) and bin_start[0] == 0 and bin_start[-1] == bin_items.size
    lists = [bin_items[bin_start[b]:bin_start[b + 1]] for b in range(9)]
    for items in lists:
        assert (np.diff(items) > 0).all()                   # ascending, no duplicates
        assert items.size == 0 or (items.min() >= 0 and items.max() < 40)
    r, c = np.mgrid[0:rows, 0:cols]
    cell_bin = (r // 32) * 3 + c // 32
    reached = 0
    for t, (xt, yt) in enumerate(xy):
        inside = (c - xt) ** 2 + (r - yt) ** 2 <= radius * radius
        for b in np.unique(cell_bin[inside]):
            assert t in lists[b], (t, b)
        reached += int(inside.any())
    assert reached > 0 or radius == 0.
    again = tb.build_bins(xy, radius, (rows, cols))
    assert np.array_equal(again[0], bin_start) and np.array_equal(again[1], bin_items)
    assert tb.build_bins(np.array([[np.nan, 1.], [1e300, -1e300]]), radius, (rows, cols))[1].size == 0


def test_build_bins_refuses_a_bad_radius():
    for bad in (-1., float('nan')):
        with pytest.raises(ValueError, match='radius_cells'):
            tb.build_bins(np.zeros((1, 2)), bad, (70, 90))


def test_windplant_window_and_kernel_radius():
    bounds, res, grid = (1000., 2000., 1000. + 79 * 100., 2000. + 59 * 100.), 100., (60, 80)
    # centres x = 1000 + 100 c, y = 2000 + 100 r; turbines x in [3000, 3450], y in [4000, 4000]; pad 500
    win = tb.windplant_window([3000., 3450.], [4000., 4000.], 500., bounds, res, grid)
    # x in [2500, 3950] -> c 15 .. 29 (2500 = 1000 + 1500 included, 3950 < 4000); y in [3500, 4500] -> r 15 .. 25
    assert win == (15, 26, 15, 30)
    # clipped to the raster on every side
    assert tb.windplant_window([1000.], [2000.], 250., bounds, res, grid) == (0, 3, 0, 3)
    assert tb.windplant_window([8900.], [7900.], 1e9, bounds, res, grid) == (0, 60, 0, 80)
    with pytest.raises(ValueError, match='no cell'):
        tb.windplant_window([3040.], [4000.], 20., bounds, res, grid)        # between two columns of centres
    with pytest.raises(ValueError):
        tb.windplant_window([], [], 20., bounds, res, grid)
    # the wind-plant map truncates where the domain-wide map rounds
    assert presence.windplant_kernel_radius(270., 100., grid) == 2
    assert presence.presence_kernel_radius(270., 100., grid) == 3
    assert presence.windplant_kernel_radius(100., 100., grid) == 2           # the floor of 2 cells
    assert presence.windplant_kernel_radius(1e6, 100., grid) == 30           # half the shorter side


def test_config_field_and_constructor_checks(tmp_path):
    from dataclasses import fields
    cfg = Config()
    assert cfg.turbine_encounter_radius == 0.
    assert 'turbine_encounter_radius' in [f.name for f in fields(Config)]
    assert str(cfg).split(':::: MI355X build')[1].strip().splitlines()[-1] == 'turbine_encounter_radius = 0.0'
    base = dict(run_name='t', out_dir=str(tmp_path), region_width_km=(8., 6.), resolution=100., track_count=10, sim_seed=1)
    # all three are refused before any raster is computed (no GPU here)
    with pytest.raises(ValueError, match='turbine_encounter_radius'):
        Simulator(Config(**base, turbine_encounter_radius=-1.), terrain='synthetic')
    with pytest.raises(ValueError, match='none were given'):
        Simulator(Config(**base, turbine_encounter_radius=150.), terrain='synthetic')
    outside = dict(x=[9000., 1000.], y=[100., 100.], t_hh=[80., 20.])
    with pytest.raises(ValueError, match='none of those given'):
        Simulator(Config(**base, turbine_encounter_radius=150.), terrain='synthetic', turbines=outside)


INV = -1


def _encounters_call(lib, **kw):
    buf = (C.c_char * 64)()
    a = dict(traj=buf, off=buf, ntracks=1, turb=buf, nturb=1, radius=1.0, bin_start=buf, bin_items=buf, rows=70, cols=90,
             hits=buf, first=None)
    a.update(kw)
    return lib.ssrs_turbine_encounters(a['traj'], a['off'], C.c_int64(a['ntracks']), a['turb'], a['nturb'],
                                       C.c_double(a['radius']), a['bin_start'], a['bin_items'], a['rows'], a['cols'],
                                       a['hits'], a['first'], None)


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    assert _native.SSRS_TURBINE_BIN == tb.BIN == 32 and _native.SSRS_TURBINE_MAX == tb.MAX_TURBINES == 8192
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ssrs_hip.h')).read()
    assert '#define SSRS_TURBINE_BIN 32' in header and '#define SSRS_TURBINE_MAX 8192' in header
    bad = [dict(traj=None), dict(off=None), dict(turb=None), dict(bin_start=None), dict(bin_items=None), dict(hits=None),
           dict(ntracks=-1), dict(nturb=0), dict(nturb=8193), dict(rows=40000), dict(cols=40000), dict(rows=0), dict(cols=0),
           dict(radius=-1.0), dict(radius=float('nan'))]
    for kw in bad:
        assert _encounters_call(lib, **kw) == INV == _native.SSRS_ERR_INVALID, kw
        assert b'ssrs_turbine_encounters' in lib.ssrs_last_error(), kw
    buf = (C.c_char * 64)()
    for args in ((None, 1, 1, buf), (buf, 1, 1, None), (buf, -1, 1, buf), (buf, 1, 0, buf), (buf, 1, 8193, buf)):
        rc = lib.ssrs_turbine_encounter_counts(args[0], C.c_int64(args[1]), args[2], args[3], None, None)
        assert rc == INV, args
        assert b'ssrs_turbine_encounter_counts' in lib.ssrs_last_error(), args
    with pytest.raises(ValueError):
        _native.check(INV)


def test_track_sharded_runs_sum_the_per_turbine_counts_once_per_item(tmp_path):
    """Every rank of a track-sharded run hands its per-turbine counts to ONE all-reduce per (case, realisation); rank 0
    writes the sum; the per-track results stay the rank's own.  A case-sharded (or single) run reduces nothing.
    This drives the encounters product's store_counts (ssrs_amd/products.py: the host half of its store, and the one place
    that issues the collective) directly: that simulate_tracks calls store once per item from run(), in item order and before
    the histogram's reduce, needs a GPU and is checked in test_gpu_track_products.py."""
    from ssrs_amd.products import Encounters
    sim = object.__new__(Simulator)
    enc_product = object.__new__(Encounters)
    enc_product.sim = sim
    sim.mode_data_dir, sim.track_direction, sim.updraft_threshold, sim.movement_model = str(tmp_path), 0., 0.75, 'fluidflow'
    sim.turbine_encounters = {}
    calls = []

    def fake_sum(values):
        calls.append(np.array(values))
        return np.asarray(values, dtype=np.int64) * 4          # "four ranks with the same counts"
    sim._allreduce_sum = fake_sum
    sim._world = lambda: 4
    per_track, first = np.array([1, 0, 2], dtype=np.int32), np.array([5, -1, 0], dtype=np.int32)
    for rank in (1, 0):
        sim._rank = lambda rank=rank: rank
        calls.clear()
        for real_id, counts in enumerate(([3, 0, 1], [0, 2, 2])):
            enc_product.store_counts(('s10d270', real_id), np.array(counts, dtype=np.int64), per_track, first, sharded=True)
        assert len(calls) == 2
        assert [c.tolist() for c in calls] == [[3, 0, 1], [0, 2, 2]] and all(c.dtype == np.int64 for c in calls)
        enc = sim.turbine_encounters[('s10d270', 1)]
        assert enc['tracks_per_turbine'].tolist() == [0, 8, 8] and enc['tracks_per_turbine'].dtype == np.int64
        assert np.array_equal(enc['turbines_per_track'], per_track) and np.array_equal(enc['first_step'], first)
        files = sorted(os.listdir(tmp_path))
        if rank == 1:
            assert files == []                                  # only rank 0 writes the merged counts
        else:
            assert files == ['s10d270_d0_t75_fluidflow_r0_turbine_encounters.npy',
                             's10d270_d0_t75_fluidflow_r1_turbine_encounters.npy']
            saved = np.load(os.path.join(tmp_path, files[0]))
            assert saved.dtype == np.int64 and saved.tolist() == [12, 0, 4]
    # not track-sharded: no collective, the owning rank writes whatever its number
    calls.clear()
    sim._rank = lambda: 3
    enc_product.store_counts(('other', 0), np.array([7], dtype=np.int64), per_track, first, sharded=False)
    assert calls == [] and np.load(os.path.join(tmp_path, 'other_d0_t75_fluidflow_r0_turbine_encounters.npy')).tolist() == [7]
    # the summary: the mean over the items of counts / track_count
    sim.track_count, sim._world, sim._rank, sim._barrier = 10, (lambda: 1), (lambda: 0), (lambda: None)
    sim.case_ids = ['s10d270']
    sim.turbine_encounters = {k: v for k, v in sim.turbine_encounters.items() if k[0] == 's10d270'}
    got = sim.compute_turbine_encounters()
    want = np.mean([np.array([12, 0, 4]) / 10., np.array([0, 8, 8]) / 10.], axis=0)
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-15, atol=0)
    assert np.array_equal(np.load(os.path.join(tmp_path, 'summary_turbine_encounters.npy')), got)
    sim.turbine_encounters = {}
    with pytest.raises(ValueError, match='no turbine encounters'):
        sim.compute_turbine_encounters()
