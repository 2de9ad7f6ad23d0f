"""Rotor encounters (K15), the parts that need no GPU: the cull lists from a per-turbine radius, the cylinders of
turbines.rotor_geometry against hand-computed integers, the Config fields and the constructor's checks, and the library's
argument validation."""
import ctypes as C
import warnings

import numpy as np
import pytest

import rotor_ref as ref
from ssrs_amd import Config
from ssrs_amd import turbines as tb
from ssrs_amd.simulator import Simulator


def _lists(bins, nbins):
    return [bins[1][bins[0][b]:bins[0][b + 1]] for b in range(nbins)]


def test_build_bins_scalar_radius_is_unchanged():
    """A scalar, and the same number once per turbine, give the lists of the single-radius form (pinned here by their
    definition: the widened bounding box of every disk against the bins)."""
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(-50., 140., 40), rng.uniform(-50., 120., 40)], 1)
    for radius in (0., 0.5, 2.5, 40.):
        scalar = tb.build_bins(xy, radius, ref.SHAPE)
        vector = tb.build_bins(xy, np.full(40, radius), ref.SHAPE)
        assert np.array_equal(scalar[0], vector[0]) and np.array_equal(scalar[1], vector[1])
        assert scalar[0].dtype == np.int32 and scalar[1].dtype == np.int32
        want = [[] for _ in range(9)]
        for t, (x, y) in enumerate(xy):
            c0, c1 = max(np.floor(x - radius) - 1, 0), min(np.ceil(x + radius) + 1, ref.COLS - 1)
            r0, r1 = max(np.floor(y - radius) - 1, 0), min(np.ceil(y + radius) + 1, ref.ROWS - 1)
            if c0 <= c1 and r0 <= r1:
                for br in range(int(r0) // 32, int(r1) // 32 + 1):
                    for bc in range(int(c0) // 32, int(c1) // 32 + 1):
                        want[br * 3 + bc].append(t)
        assert [list(items) for items in _lists(scalar, 9)] == want
    for bad in (-1., float('nan'), np.float64(-0.5)):
        with pytest.raises(ValueError, match='radius_cells'):
            tb.build_bins(xy, bad, ref.SHAPE)
    with pytest.raises(ValueError, match='entries'):
        tb.build_bins(xy, np.ones(39), ref.SHAPE)


@pytest.mark.parametrize('name', ['planted', 'loiter'])
def test_build_bins_per_turbine_radius_is_conservative(name):
    """Every (point, turbine) pair the brute force accepts has the turbine in the list of the point's bin; NaN and negative
    entries, and NaN coordinates, are in no list."""
    c = ref.case(name)
    bins = tb.build_bins(c['xy'], c['reach'], ref.SHAPE)
    lists = _lists(bins, 9)
    for items in lists:
        assert (np.diff(items) > 0).all()
    traj, alt, off = ref.flat(c)
    inside = ref.inside_matrix(traj, alt, c['elev'], c['xy'], c['reach'], c['zband'], ref.SHAPE)
    pairs = np.argwhere(inside)
    assert len(pairs) > 500
    for k, t in pairs:
        r, col = int(traj[k, 0]), int(traj[k, 1])
        assert t in lists[(r // 32) * 3 + col // 32], (k, t)
    assert not np.isin([6, 7, 8], bins[1]).any()                 # NaN reach, NaN coordinate, negative reach
    assert np.isin([0, 1, 4, 5, 9], bins[1]).all()               # reach 0 and the one outside are listed; so is an empty band


def _turbines(**cols):
    return tb.Turbines(cols, min_hubheight=0.)


def test_rotor_geometry_against_hand_computed_integers():
    bounds, res = (1000., 2000., 1000. + 5 * 10., 2000. + 3 * 10.), 10.          # 4 x 6 cells of 10 m
    dem = np.arange(24, dtype=np.float64).reshape(4, 6) * 100. + 0.0004        # cell (r, c): 600 r + 100 c metres and a bit
    dem[3, 5] = np.nan
    dem[0, 1], dem[0, 2] = 1.08e6, -1.2e6                                     # clip to +-2^30 mm
    t = _turbines(
        #  on (2, 3)  ties: (0.5, 2.5) -> col 0, row 2  outside: clamped to (3, 0)  on nodata  NaN t_rd  bases that clip
        x=[1030., 1005., 900., 1050., 1020., 1010., 1020.],
        y=[2020., 2025., 2100., 2030., 2010., 2000., 2000.],
        t_hh=[80., 90.0005, 100., 80., 80., 80., 80.],
        t_rd=[100., 120.001, 50., 100., np.nan, 4e6, 4e6])
    assert len(t) == 7
    reach, zband = tb.rotor_geometry(t, dem, bounds, res)
    assert reach.dtype == np.float64 and zband.dtype == np.int32 and zband.shape == (7, 2)
    # 0: base rint(1500000.4) = 1500000; 80 -+ 50 m
    assert reach[0] == 5. and zband[0].tolist() == [1_500_000 + 30_000, 1_500_000 + 130_000]
    # 1: x 0.5 -> col 0 and y 2.5 -> row 2 (rint: ties to even); base 1200 m; rad 60.0005: the millimetres are rint of the
    # same f64 expressions
    rad = 120.001 / 2.
    assert zband[1].tolist() == [1_200_000 + int(np.rint(1000. * (90.0005 - rad))), 1_200_000 + int(np.rint(1000. * (90.0005 + rad)))]
    assert zband[1].tolist() == [1_230_000, 1_350_001] and reach[1] == rad / 10.
    # 2: outside the raster (x -10 cells, y +10 cells): the base cell is clamped to (3, 0): 1800 m
    assert zband[2].tolist() == [1_800_000 + 75_000, 1_800_000 + 125_000] and reach[2] == 2.5
    # 3: nodata base, 4: NaN rotor diameter: the empty band and a NaN reach
    assert zband[3].tolist() == [1, 0] and zband[4].tolist() == [1, 0] and np.isnan(reach[3]) and np.isnan(reach[4])
    # 5, 6: the bases clip to +-2^30 mm like cellinfo's elev, and the sums (2^30 + 2 000 080 000, -2^30 - 1 999 920 000)
    # clip to int32
    assert zband[5].tolist() == [2 ** 30 - 1_999_920_000, 2 ** 31 - 1] and reach[5] == 2e5
    assert zband[6].tolist() == [-2 ** 31, -2 ** 30 + 2_000_080_000]
    # clearance widens the cylinder in the plane and in height
    reach_c, zband_c = tb.rotor_geometry(t, dem, bounds, res, clearance=2.5)
    assert reach_c[0] == 5.25 and zband_c[0].tolist() == [1_500_000 + 27_500, 1_500_000 + 132_500]
    assert zband_c[3].tolist() == [1, 0] and np.isnan(reach_c[4])
    # an f32 DEM is widened to f64 before the product
    f32 = dem.astype(np.float32)
    want = int(np.rint(1000. * np.float64(f32[2, 3])))
    assert tb.rotor_geometry(t, f32, bounds, res)[1][0].tolist() == [want + 30_000, want + 130_000]
    # the columns it needs
    with pytest.raises(ValueError, match='t_rd'):
        tb.rotor_geometry(_turbines(x=[1000.], y=[2000.], t_hh=[80.]), dem, bounds, res)
    with pytest.raises(ValueError, match='t_hh / t_rd'):
        tb.rotor_geometry(_turbines(x=[1000.], y=[2000.]), dem, bounds, res)
    with pytest.raises(ValueError, match='clearance'):
        tb.rotor_geometry(t, dem, bounds, res, clearance=float('nan'))


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda unavailable, and any attempt to reach the device fails the test."""
    import torch
    from ssrs_amd import _device
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)

    def boom(*a, **k):
        raise AssertionError('device work before the argument check')
    monkeypatch.setattr(_device, 'device', boom)
    monkeypatch.setattr(_device, 'to_dev', boom)


def _table(**extra):
    cols = dict(x=[1500., 2550., 3000.], y=[700., 900., 1500.], t_hh=[80., 90., 100.], t_rd=[100., 110., 120.])
    cols.update(extra)
    return cols


def test_config_fields_and_constructor_checks(tmp_path, no_gpu):
    from dataclasses import fields
    from ssrs_amd.config import _SECTIONS
    cfg = Config()
    assert cfg.rotor_geometry == 'band' and cfg.rotor_clearance == 0.
    names = [f.name for f in fields(Config)]
    at = names.index('rotor_zone')
    assert names[at + 1:at + 3] == ['rotor_geometry', 'rotor_clearance']
    build = list(dict(_SECTIONS)['MI355X build'])
    at = build.index('rotor_zone')
    assert build[at + 1:at + 3] == ['rotor_geometry', 'rotor_clearance'] and build[-1] == 'turbine_encounter_radius'
    text = str(Config(rotor_geometry='turbine', rotor_clearance=5.)).split(':::: MI355X build')[1]
    assert 'rotor_geometry = turbine' in text and 'rotor_clearance = 5.0' in text

    base = dict(run_name='t', out_dir=str(tmp_path), region_width_km=(6., 5.), resolution=100., track_count=10, sim_seed=1)
    dem = np.zeros((50, 60))
    with pytest.raises(ValueError, match='rotor_geometry'):
        Simulator(Config(**base, rotor_geometry='disk'), terrain=dem)
    with pytest.raises(ValueError, match='flight_height=True'):
        Simulator(Config(**base, rotor_geometry='turbine'), terrain=dem, turbines=_table())
    with pytest.raises(ValueError, match='none were given'):
        Simulator(Config(**base, rotor_geometry='turbine', flight_height=True), terrain=dem)
    with pytest.raises(ValueError, match='rotor_clearance'):
        Simulator(Config(**base, rotor_geometry='turbine', flight_height=True, rotor_clearance=float('nan')), terrain=dem,
                  turbines=_table())
    with pytest.raises(ValueError, match='none of those given'):
        Simulator(Config(**base, rotor_geometry='turbine', flight_height=True), terrain=dem,
                  turbines=_table(x=[9000., 9100., 9200.]))
    with pytest.raises(ValueError, match='t_rd'):
        no_rd = _table()
        del no_rd['t_rd']
        Simulator(Config(**base, rotor_geometry='turbine', flight_height=True), terrain=dem, turbines=no_rd)
    many = dict(x=np.full(tb.MAX_TURBINES + 1, 1500.), y=np.full(tb.MAX_TURBINES + 1, 700.),
                t_hh=np.full(tb.MAX_TURBINES + 1, 80.), t_rd=np.full(tb.MAX_TURBINES + 1, 100.))
    with pytest.raises(ValueError, match=f'at most {tb.MAX_TURBINES}'):
        Simulator(Config(**base, rotor_geometry='turbine', flight_height=True), terrain=dem, turbines=many)


def test_resolve_turbines_builds_the_cylinders_and_band_leaves_it_as_it_was(tmp_path):
    """_resolve_turbines on a bare object (no constructor: nothing here needs the device): 'band' computes what it computed
    before -- the 2-D cull lists with turbine_encounter_radius, and nothing else -- 'turbine' adds the cylinders and the
    lists from the per-turbine reach, and says once how many turbines stand on nodata."""
    dem = np.add.outer(np.arange(50.), np.arange(60.))                       # (r, c): r + c metres
    dem[9, 26] = np.nan                                                        # under the second turbine (2550, 900)

    def bare(**kw):
        sim = object.__new__(Simulator)
        Config.__init__(sim, region_width_km=(6., 5.), resolution=100., **kw)
        sim.gridsize, sim.bounds = (50, 60), (0., 0., 5900., 4900.)
        sim._terrain = {'Elevation': dem}
        sim.projection = None
        return sim

    band = bare(turbine_encounter_radius=150.)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        kept = band._resolve_turbines(_table())
    assert len(kept) == 3 and not hasattr(band, '_rotor_cylinders')
    cells = kept.cell_coordinates(band.bounds, 100.)
    assert np.array_equal(band._turbine_cells, cells)
    want = tb.build_bins(cells, 1.5, (50, 60))
    assert np.array_equal(band._turbine_bins[0], want[0]) and np.array_equal(band._turbine_bins[1], want[1])
    plain = bare()
    assert len(plain._resolve_turbines(_table())) == 3
    assert not hasattr(plain, '_turbine_cells') and not hasattr(plain, '_rotor_cylinders')

    sim = bare(flight_height=True, rotor_geometry='turbine', rotor_clearance=10.)
    with pytest.warns(UserWarning, match='1 of the 3 turbines stand on a nodata cell') as seen:
        kept = sim._resolve_turbines(_table())
    assert len(seen) == 1 and not hasattr(sim, '_turbine_bins')               # no 2-D encounters were asked for
    xy, reach, zband, bins = sim._rotor_cylinders
    assert np.array_equal(xy, [[15., 7.], [25.5, 9.], [30., 15.]])
    assert np.array_equal(reach[[0, 2]], [0.6, 0.7]) and np.isnan(reach[1])
    # bases: cell (7, 15) = 22 m and (15, 30) = 45 m; rad 60 and 70 m
    assert zband.tolist() == [[22_000 + 20_000, 22_000 + 140_000], [1, 0], [45_000 + 30_000, 45_000 + 170_000]]
    want = tb.build_bins(xy, reach, (50, 60))
    assert np.array_equal(bins[0], want[0]) and np.array_equal(bins[1], want[1]) and sorted(set(bins[1])) == [0, 2]


INV = -1


def _call(lib, **kw):
    buf = (C.c_char * 64)()
    a = dict(traj=buf, off=buf, ntracks=1, alt=buf, info=buf, rows=70, cols=90, turb=buf, reach=buf, zband=buf, nturb=1,
             bin_start=buf, bin_items=buf, hits=buf, first=None, points=None)
    a.update(kw)
    return lib.ssrs_rotor_encounters(a['traj'], a['off'], C.c_int64(a['ntracks']), a['alt'], a['info'], a['rows'], a['cols'],
                                     a['turb'], a['reach'], a['zband'], a['nturb'], a['bin_start'], a['bin_items'], a['hits'],
                                     a['first'], a['points'], None)


def test_library_validates_without_a_gpu():
    from ssrs_amd import _native
    lib = _native.lib()
    assert 'ssrs_rotor_encounters' in _native.EXPORTS and lib.ssrs_version() == 109
    buf = (C.c_char * 64)()
    odd = C.c_void_p(C.addressof(buf) + 2)
    four = C.c_void_p(C.addressof(buf) + 4)
    for bad in (dict(traj=None), dict(off=None), dict(alt=None), dict(info=None), dict(turb=None), dict(reach=None),
                dict(zband=None), dict(bin_start=None), dict(bin_items=None), dict(hits=None),
                dict(ntracks=-1), dict(ntracks=2 ** 31), dict(nturb=0), dict(nturb=_native.SSRS_TURBINE_MAX + 1),
                dict(rows=0), dict(cols=0), dict(rows=32768), dict(cols=40000),
                dict(traj=odd), dict(alt=odd), dict(info=four), dict(zband=four), dict(points=four)):
        assert _call(lib, **bad) == INV, bad
        assert b'ssrs_rotor_encounters' in lib.ssrs_last_error(), bad
    # nothing to do is not an error, and is decided before the device is touched
    assert _call(lib, ntracks=0) == _native.SSRS_OK
