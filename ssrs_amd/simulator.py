"""`Simulator` -- the orchestrator of the hot path behind the reference's API
(/root/reference/ssrs/simulator.py:34-386, 508-546, 760-763).

Kept: constructor signature (`Simulator(in_config=None, **kwargs)`), the
methods and attributes listed in SURVEY.md section 8(b), and the on-disk file
contract (`<case>_orograph.npy` f32, `<id>_potential.npy` f32,
`<id>_tracks.pkl` list of int16 (n,2), `summary_presence.npy` f32).

Changed on purpose:
  * the reference constructor downloads terrain/wind from the network
    (simulator.py:88-125).  That L1 layer is out of scope; terrain and wind are
    INJECTED: `Simulator(cfg, terrain=..., wind=...)`.
  * the process pool over tracks (simulator.py:360-381) is one batched GPU call;
    the random stream is Philox keyed by (sim_seed + real_id, track id, step).
  * plotting methods are thin stubs (visualisation is out of scope).
"""
import json
import os
import pickle
import time
import warnings
from dataclasses import asdict
from types import SimpleNamespace

import numpy as np
import torch

from .config import Config
from . import distributed, flight, inputs, layers, movmodel, presence
from . import products as products_mod
from . import turbines as turbines_mod
from . import potential as potential_mod
from ._device import to_dev


def _elapsed(start):
    """'took' strings in the reference's format (utils.py:97-108)."""
    hours, rem = divmod(time.time() - start, 3600)
    mins, secs = divmod(rem, 60)
    if hours == 0:
        return f'{int(secs) + 1} sec' if mins == 0 else f'{int(mins)} min {int(secs)} sec'
    return f'{int(hours)} hr {int(mins)} min'


class Simulator(Config):
    """ Class for SSRS simulation """

    lonlat_crs = 'EPSG:4326'
    time_format = 'y%Ym%md%dh%H'

    def __init__(self, in_config: Config = None, *, terrain=None, wind=None,
                 origin=(0.0, 0.0), turbines=None, **kwargs) -> None:
        """terrain: 'synthetic' | elevation array (rows, cols) | dict with keys
        'Elevation' and optionally 'Slope', 'Aspect' | callable(gridsize, res).
        wind (snapshot / seasonal): list of dicts, each with 'datetime'
        (datetime or 4-tuple) or 'case_id', and 'wspeed', 'wdirn' given either as
        (rows, cols) rasters or as lattice samples with 'x_km', 'y_km' (or samples at
        scattered points: x_km[npts], y_km[npts], arrays (npts,)).  Samples are
        interpolated as `wtk_interp_type` says ('nearest' | 'linear' | 'cubic', scipy
        griddata's methods as in the reference); rasters are taken as they are.
        With thermal_model='wtk' (and with 'allen' while thermal_allen_zi or
        thermal_allen_wstar is 0) every entry also carries 'pressure', 'temperature',
        'blheight' and 'surfheatflux' (the keys of `wtk_layers`), all four as (rows, cols)
        rasters, as samples (npts,) at x_km / y_km, or on the lattice (ny, nx).
        origin: projected (west, south) of cell (0, 0), or 'southwest_lonlat': the image of
        `southwest_lonlat` under `projected_crs` (an Albers projection, ssrs_amd/georef.py), as the
        reference derives it through GDAL (simulator.py:77-85); `projection` and `lonlat_bounds` are
        then set, and inputs in degrees are accepted: terrain=LonLatRaster(...) (warped to the grid
        on the device), turbines with the USWTDB columns `xlong`, `ylat` instead of `x`, `y`, and
        wind entries with 'lon', 'lat' instead of 'x_km', 'y_km'.
        turbines: a `Turbines`, a dict of columns or a DataFrame with `x`, `y` in the projected frame of
        `origin` (optionally `p_name`, `t_hh`, `t_rd`): the stand-in for the reference's USWTDB download
        (simulator.py:101-105), filtered to `bounds` and `turbine_minimum_hubheight` like it."""
        if in_config is None:
            super().__init__(**kwargs)
        else:
            super().__init__(**asdict(in_config))
        self._check_thermal_model()
        self._check_orographic_model()
        if not float(self.turbine_encounter_radius) >= 0.:
            raise ValueError(f'turbine_encounter_radius = {self.turbine_encounter_radius!r}: expected metres >= 0 (0 = off)')
        if not float(self.track_passage_radius) >= 0.:
            raise ValueError(f'track_passage_radius = {self.track_passage_radius!r}: expected metres >= 0 (0 = off)')
        if float(self.track_passage_radius) > 0.:
            presence.passage_r2(self.track_passage_radius, self.resolution)       # (at most 255 cells)
        if self.flight_height:
            self._flight_params()
        if self.flight_time:
            self._time_params()
        self._check_rotor_exposure_time()
        self._check_rotor_transits(turbines)
        self._check_collision_risk(turbines)
        self._check_site_collision_risk()
        self._check_rotor_geometry(turbines)
        print(f'\n---- SSRS in {self.sim_mode} mode')
        print(f'Run name: {self.run_name}')
        if self.sim_seed >= 0:                                    # simulator.py:50-52
            print('Specified random number seed:', self.sim_seed)
            np.random.seed(self.sim_seed)

        print(f'Output dir: {os.path.join(self.out_dir, self.run_name)}')
        self.data_dir = os.path.join(self.out_dir, self.run_name, 'data/')
        self.fig_dir = os.path.join(self.out_dir, self.run_name, 'figs/')
        self.mode_data_dir = os.path.join(self.data_dir, self.sim_mode)
        self.mode_fig_dir = os.path.join(self.fig_dir, self.sim_mode)
        for dirname in (self.mode_data_dir, self.mode_fig_dir):
            os.makedirs(dirname, exist_ok=True)
        with open(os.path.join(self.out_dir, self.run_name, f'{self.run_name}.json'), 'w',
                  encoding='utf-8') as cfile:
            json.dump(self.__dict__, cfile, ensure_ascii=False, indent=2)

        print(f'Terrain resolution = {self.resolution} m')
        xsize = int(round((self.region_width_km[0] * 1000. / self.resolution)))
        ysize = int(round((self.region_width_km[1] * 1000. / self.resolution)))
        self.gridsize = (ysize, xsize)
        print(f'Terrain grid size = {self.gridsize}')
        self.projection = None
        if isinstance(origin, str):
            if origin != 'southwest_lonlat':
                raise ValueError(f"origin = {origin!r}: expected a pair (west, south) or 'southwest_lonlat'")
            # simulator.py:77-82: the projected image of the south-west corner
            from .georef import Projection
            self.projection = Projection.from_crs(self.projected_crs)
            west, south = (float(v) for v in self.projection.forward(*self.southwest_lonlat))
        else:
            west, south = float(origin[0]), float(origin[1])
        self.bounds = (west, south, west + (xsize - 1) * self.resolution,
                       south + (ysize - 1) * self.resolution)
        self.extent = (self.bounds[0], self.bounds[2], self.bounds[1], self.bounds[3])
        self.lonlat_bounds = None          # known only with origin='southwest_lonlat'
        if self.projection is not None:
            # transform_bounds, raster.py:52-84: the four corners, then min and max
            lon, lat = self.projection.inverse([self.bounds[0], self.bounds[0], self.bounds[2], self.bounds[2]],
                                               [self.bounds[1], self.bounds[3], self.bounds[1], self.bounds[3]])
            self.lonlat_bounds = [float(lon.min()), float(lat.min()), float(lon.max()), float(lat.max())]

        self.terrain_layers = {'Elevation': 'DEM', 'Slope': 'Slope Degrees',
                               'Aspect': 'Aspect Degrees'}
        self._terrain = self._resolve_terrain(terrain)
        self.turbines = self._resolve_turbines(turbines)
        self._site_class = self._resolve_site_class()
        self.turbine_encounters = {}      # (case_id, real_id) -> dict(tracks_per_turbine, turbines_per_track, first_step)
        self.track_occupancy_counts = {}  # (case_id, real_id) -> int32 (rows, cols): the distinct tracks through each cell
        self.track_passage_counts = {}    # (case_id, real_id) -> int32 (rows, cols): the distinct tracks within
        #                                     track_passage_radius of each cell
        self.rotor_presence_counts = {}   # (case_id, real_id) -> int32 (rows, cols) holding uint32: points in the rotor zone
        self.flight_heights = {}          # (case_id, real_id) -> int32 (this rank's tracks, 3): [in zone, h_min, h_max] in mm
        self.rotor_turbine_encounters = {}  # as turbine_encounters, of the points in the rotor zone only
        self.residence_time_counts = {}   # flight_time: (case_id, real_id) -> int64 (rows, cols) holding uint64 microseconds
        self.rotor_residence_time_counts = {}  # the same of the moves that leave a point in the rotor zone (flight_height too)
        self.flight_times = {}            # (case_id, real_id) -> int64 (this rank's tracks, 2): [total, in zone] microseconds
        self.turbine_rotor_encounters = {}  # rotor_geometry='turbine': (case_id, real_id) -> dict(tracks_per_turbine,
        #                                     points_per_turbine int64, turbines_per_track, first_step int32; with
        #                                     rotor_exposure_time also time_per_turbine int64, microseconds)
        self.turbine_rotor_transits = {}  # rotor_transits: (case_id, real_id) -> int64 (nturb, 3): [tracks, transits with the
        #                                     wind, against the wind]
        self.turbine_collision_risk = {}  # collision_risk: (case_id, real_id) -> int64 (nturb, 2): the summed collision
        #                                     probabilities of the transits in units of 2^-32 [with the wind, against the wind]
        self.track_collision_risk = {}    # (case_id, real_id) -> int64 (this rank's tracks,): the same per track
        self.site_collision_risk_sums = {}  # site_collision_risk: (case_id, real_id) -> int64 (rows, cols, 2): the summed
        #                                     collision probabilities of a turbine on each cell, in units of 2^-32
        self.site_transit_counts = {}     # (case_id, real_id) -> int64 (rows, cols, 2): its transits [with, against the wind]
        self.wtk_layers = {
            'wspeed': f'windspeed_{str(int(self.wtk_orographic_height))}m',
            'wdirn': f'winddirection_{str(int(self.wtk_orographic_height))}m',
            'pressure': f'pressure_{str(int(self.wtk_thermal_height))}m',
            'temperature': f'temperature_{str(int(self.wtk_thermal_height))}m',
            'blheight': 'boundary_layer_height',
            'surfheatflux': 'surface_heat_flux',
        }
        self._presence_counts = {}        # (case_id, real_id) -> device histogram
        self._nearest_index = (None, None)    # ('nearest': the sample points and their index raster, per wind geometry)

        if self.sim_mode.lower() != 'uniform':
            if wind is None:
                raise ValueError(f'{self.sim_mode} mode needs injected wind data (wind=[...]); '
                                 'the WIND Toolkit download is out of scope')
            self._wind = inputs.resolve_wind(wind, self.sim_mode, self.time_format, self.gridsize, self.wtk_interp_type,
                                             self._wtk_thermals() or self._allen_from_layers(), self.wtk_layers,
                                             self._wind_km, str(self.thermal_model).lower())
            self.dtimes = [w.datetime for w in self._wind]
            self.case_ids = [w.case_id for w in self._wind]
            self.compute_orographic_updrafts_using_wtk()
        else:
            print(f'Uniform mode: Wind speed = {self.uniform_windspeed} m/s')
            print(f'Uniform mode: Wind dirn = {self.uniform_winddirn} deg(cw)')
            self.case_ids = [self._get_uniform_id()]
            self.compute_orographic_updraft_uniform()
        if self._wtk_thermals():
            self.compute_thermal_updrafts_using_wtk()
        else:
            for case_id in self._cases_written_here():
                self.compute_thermal_updrafts(case_id)
        self._barrier()

        fig_aspect = self.region_width_km[0] / self.region_width_km[1]
        self.fig_size = (self.fig_height * fig_aspect, self.fig_height)
        self.km_bar = min([1, 5, 10], key=lambda x: abs(x - self.region_width_km[0] // 4))
        print('SSRS Simulator initiation done.')

    # ------------------------------------------------------------ injection
    def _resolve_terrain(self, terrain):
        if terrain is None:
            raise NotImplementedError(
                'Terrain download (USGS 3DEP / SRTM, simulator.py:88-99) is outside the '
                "hot-path scope: pass terrain='synthetic', an elevation array, a dict "
                "{'Elevation': ..., 'Slope': ..., 'Aspect': ...} or a callable.")
        from .georef import LonLatRaster
        if isinstance(terrain, LonLatRaster):
            # get_raster_in_projected_crs (raster.py:12-49) on the device; slope and aspect then come from the
            # Horn path, as in the reference when only the elevation could be had (simulator.py:152-159)
            from .georef import warp_to_grid
            projection = self._need_projection('terrain=LonLatRaster(...)')
            dem, uncovered = warp_to_grid(terrain, projection, self.bounds[0], self.bounds[1], self.gridsize,
                                          self.resolution)
            if uncovered > 0:
                raise ValueError(
                    f'terrain: {uncovered} of the {self.gridsize[0] * self.gridsize[1]} cells are not covered by the '
                    f'longitude / latitude raster (its pixel centres span {terrain.lonlat_bounds}) or need a missing '
                    f'pixel; the region needs lonlat_bounds = {self.lonlat_bounds}')
            terrain = dem
        if isinstance(terrain, str):
            if terrain != 'synthetic':
                raise ValueError(f'unknown terrain provider {terrain!r}')
            from .synthetic import synthetic_dem
            terrain = synthetic_dem(self.gridsize, self.resolution)
        if callable(terrain):
            terrain = terrain(self.gridsize, self.resolution)
        if not isinstance(terrain, dict):
            terrain = {'Elevation': terrain}
        out = {}
        for key, val in terrain.items():
            arr = inputs.host_f64(val)
            if arr.shape != tuple(self.gridsize):
                raise ValueError(f'terrain layer {key} has shape {arr.shape}, '
                                 f'expected {tuple(self.gridsize)}')
            out[key] = arr
        if 'Elevation' not in out:
            raise ValueError("terrain needs an 'Elevation' layer")
        return out

    def _need_projection(self, what):
        """The projection of a georeferenced run; ValueError for an input in degrees when the origin is numeric."""
        if self.projection is None:
            raise ValueError(f"{what} is given in longitude / latitude and needs the georeferenced origin: "
                             "Simulator(..., origin='southwest_lonlat') places cell (0, 0) at the projected image "
                             f'(projected_crs = {self.projected_crs!r}) of southwest_lonlat; a numeric origin says '
                             'nothing about where the grid lies on the ellipsoid')
        return self.projection

    def _rotor_per_turbine(self):
        return str(self.rotor_geometry).lower() == 'turbine'

    def _check_rotor_exposure_time(self):
        """rotor_exposure_time sums K16's durations over K15's cylinders along K14's heights: it needs all three.  (The
        turbines, and their t_hh / t_rd, are rotor_geometry = 'turbine''s to ask for.)"""
        if not self.rotor_exposure_time:
            return
        for ok, field, why in ((self.flight_height, 'flight_height=True', 'the cylinders are tested against the heights '
                                'along the tracks'),
                               (self._rotor_per_turbine(), "rotor_geometry='turbine'", 'the time is summed inside every '
                                "turbine's own cylinder (turbines with t_hh and t_rd)"),
                               (self.flight_time, 'flight_time=True', 'the time of every move is what is summed')):
            if not ok:
                raise ValueError(f'rotor_exposure_time = True needs {field}: {why}')

    def _check_rotor_yaw(self):
        yaw = float(self.rotor_yaw)
        if yaw != yaw or yaw in (float('inf'), float('-inf')):
            raise ValueError(f'rotor_yaw = {self.rotor_yaw!r}: expected degrees clockwise from north, or < 0 for the wind')

    def _check_disk_needs(self, option, turbines, twice):
        """What K18's disks need that can be told before anything is computed, for rotor_transits and collision_risk
        (`option`; `twice`: what the option takes the rotor diameter to be twice of)."""
        names = turbines_mod._column_names(turbines) if turbines is not None else []
        for ok, field, why in ((self.flight_height, 'flight_height=True', 'the disks are tested against the heights along '
                                'the tracks'),
                               (self._rotor_per_turbine(), "rotor_geometry='turbine'", "the disk is every turbine's own, "
                                'around its hub'),
                               (turbines is not None, 'turbines', 'none were given (Simulator(..., turbines=...))'),
                               ('t_hh' in names, 'turbines with t_hh', 'the hub height in metres, the centre of the disk'),
                               ('t_rd' in names, 'turbines with t_rd', f'the rotor diameter in metres, twice the {twice}')):
            if not ok:
                raise ValueError(f'{option} = True needs {field}: {why}')

    def _check_rotor_transits(self, turbines):
        """rotor_transits counts the moves through every turbine's disk along K14's heights.  (flight_time is not among what
        it needs.)"""
        if self.rotor_transits:
            self._check_rotor_yaw()
            self._check_disk_needs('rotor_transits', turbines, 'radius of the disk')

    def _check_collision_risk(self, turbines):
        """collision_risk weights K18's transits with Band's probability: it needs what rotor_transits needs (not
        rotor_transits itself), and a bird and a rotor the model can be evaluated for."""
        if self.collision_risk:
            self._check_disk_needs('collision_risk', turbines, 'length of a blade')
            self._check_band_model('collision_risk')

    def _check_band_model(self, who):
        """The bird and the rotor Band's model is evaluated for, and rotor_yaw: what collision_risk and site_collision_risk
        (`who`) both read."""
        self._check_rotor_yaw()
        for name in ('bird_length', 'bird_wingspan'):
            if not 0. < float(getattr(self, name)) < float('inf'):
                raise ValueError(f'{name} = {getattr(self, name)!r}: expected metres > 0 ({who})')
        if str(self.bird_flight).lower() not in ('gliding', 'flapping'):
            raise ValueError(f"bird_flight = {self.bird_flight!r}: expected 'gliding' or 'flapping' ({who})")
        if not 0. <= float(self.collision_avoidance) <= 1.:
            raise ValueError(f'collision_avoidance = {self.collision_avoidance!r}: expected a share in [0, 1] ({who})')
        for name, what in (('rotor_blades', 'a number of blades'), ('rotor_rpm', 'revolutions per minute'),
                           ('rotor_max_chord', 'metres')):
            if not 0. <= float(getattr(self, name)) < float('inf'):
                raise ValueError(f'{name} = {getattr(self, name)!r}: expected {what} >= 0 ({who})')
        pitch = float(self.rotor_pitch)
        if pitch != pitch or pitch in (float('inf'), float('-inf')):
            raise ValueError(f'rotor_pitch = {self.rotor_pitch!r}: expected degrees ({who})')
        profile = np.asarray(self.rotor_chord_profile, dtype=np.float64)
        if profile.shape != turbines_mod.BAND_CHORD_NODES.shape or not (profile >= 0.).all():
            raise ValueError(f'rotor_chord_profile: expected {turbines_mod.BAND_CHORD_NODES.size} values >= 0, the chord over '
                             f'rotor_max_chord at r / R = 0.05, 0.10, ..., 1.00 ({who})')

    def _check_site_collision_risk(self):
        """site_collision_risk puts one candidate turbine class on every cell: it needs K14's heights, a class the disk and
        Band's model can be evaluated for, and no turbines."""
        if not self.site_collision_risk:
            return
        if not self.flight_height:
            raise ValueError('site_collision_risk = True needs flight_height=True: the disks are tested against the heights '
                             'along the tracks')
        for name in ('site_hub_height', 'site_rotor_diameter'):
            if not 0. < float(getattr(self, name)) < float('inf'):
                raise ValueError(f'{name} = {getattr(self, name)!r}: expected metres > 0 (site_collision_risk)')
        clearance = float(self.rotor_clearance)
        if clearance != clearance or clearance in (float('inf'), float('-inf')):
            raise ValueError(f'rotor_clearance = {self.rotor_clearance!r}: expected metres (site_collision_risk)')
        self._check_band_model('site_collision_risk')
        radius = float(self.site_rotor_diameter) / 2.
        reach = (radius + clearance) / float(self.resolution)
        if not reach <= turbines_mod.SITE_MAX_REACH:
            raise ValueError(f'site_collision_risk: (site_rotor_diameter / 2 + rotor_clearance) / resolution = '
                             f'({float(self.site_rotor_diameter):g} / 2 + {clearance:g}) / {float(self.resolution):g} = {reach:g} '
                             f'cells, expected at most {turbines_mod.SITE_MAX_REACH:g}')
        if int(np.rint(1000. * float(self.site_hub_height))) >= 2 ** 31:
            raise ValueError(f'site_hub_height = {self.site_hub_height!r}: expected metres below 2^31 mm (site_collision_risk)')

    def _resolve_site_class(self):
        """(reach in cells, hub_mm, table uint32 (2, 256)) of the candidate class of site_collision_risk, once per run: the
        disk's reach and the hub's height as turbines.rotor_disks makes them, and the class's two rows of
        turbines.band_collision_table -- what collision_risk gives a fleet of this class.  None when the feature is off."""
        if not self.site_collision_risk:
            return None
        radius, clearance = float(self.site_rotor_diameter) / 2., float(self.rotor_clearance)
        reach = (radius + clearance) / float(self.resolution)
        hub_mm = int(np.rint(1000. * float(self.site_hub_height)))
        table = turbines_mod.band_collision_table(
            np.array([radius]), clearance,
            np.array([[float(self.rotor_rpm), float(self.rotor_max_chord), float(self.rotor_pitch), float(self.rotor_blades)]]),
            float(self.flight_airspeed), float(self.bird_length), float(self.bird_wingspan),
            str(self.bird_flight).lower() == 'flapping', bool(self.collision_model_3d), self.rotor_chord_profile)[1]
        return reach, hub_mm, np.ascontiguousarray(table[0])

    def _check_rotor_geometry(self, turbines):
        """rotor_geometry / rotor_clearance, and what 'turbine' needs that can be told before anything is computed."""
        if str(self.rotor_geometry).lower() not in ('band', 'turbine'):
            raise ValueError(f"rotor_geometry = {self.rotor_geometry!r}: expected 'band' or 'turbine'")
        if not self._rotor_per_turbine():
            return
        clearance = float(self.rotor_clearance)
        if clearance != clearance or clearance in (float('inf'), float('-inf')):
            raise ValueError(f'rotor_clearance = {self.rotor_clearance!r}: expected metres')
        if not self.flight_height:
            raise ValueError("rotor_geometry = 'turbine' needs flight_height=True: the cylinders are tested against the "
                             'heights along the tracks')
        if turbines is None:
            raise ValueError("rotor_geometry = 'turbine' needs turbines: none were given (Simulator(..., turbines=...))")

    def _resolve_turbines(self, turbines):
        """The injected turbines inside `bounds` at or above `turbine_minimum_hubheight` (None stays None); with
        turbine_encounter_radius > 0 also their cell coordinates and the cull lists of the encounter kernel; with
        rotor_geometry = 'turbine' their cylinders (turbines.rotor_geometry) and the cull lists from the per-turbine reach."""
        radius = float(self.turbine_encounter_radius)
        if turbines is not None and turbines_mod.has_lonlat_only(turbines):
            # the USWTDB columns, projected as turbines.py:52-62 of the reference does
            turbines = turbines_mod.with_projected_columns(turbines, self._need_projection('turbines= (xlong, ylat)'))
        if turbines is not None:
            turbines = turbines_mod.Turbines(turbines, self.bounds, float(self.turbine_minimum_hubheight),
                                             bool(self.print_verbose))
        if radius > 0.:
            if turbines is None or len(turbines) == 0:
                raise ValueError(f'turbine_encounter_radius = {radius:g} m needs turbines: ' +
                                 ('none were given (Simulator(..., turbines=...))' if turbines is None else
                                  'none of those given lies inside the bounds at or above turbine_minimum_hubheight'))
            if len(turbines) > turbines_mod.MAX_TURBINES:
                raise ValueError(f'{len(turbines)} turbines inside the bounds: encounters are counted for at most '
                                 f'{turbines_mod.MAX_TURBINES}')
            self._turbine_cells = turbines.cell_coordinates(self.bounds, self.resolution)
            self._turbine_bins = turbines_mod.build_bins(self._turbine_cells, radius / float(self.resolution),
                                                         self.gridsize)
        if self._rotor_per_turbine():
            if len(turbines) == 0:
                raise ValueError("rotor_geometry = 'turbine' needs turbines: none of those given lies inside the bounds at "
                                 'or above turbine_minimum_hubheight')
            if len(turbines) > turbines_mod.MAX_TURBINES:
                raise ValueError(f'{len(turbines)} turbines inside the bounds: rotor encounters are counted for at most '
                                 f'{turbines_mod.MAX_TURBINES}')
            dem = self._terrain['Elevation']
            reach, zband = turbines_mod.rotor_geometry(turbines, dem, self.bounds, self.resolution,
                                                       float(self.rotor_clearance))
            cells = turbines.cell_coordinates(self.bounds, self.resolution)
            rb, cb, known = turbines_mod.base_cells(cells, self.gridsize)
            nodata = int((np.isnan(dem[rb, cb]) | ~known).sum())
            if nodata:
                warnings.warn(f"rotor_geometry = 'turbine': {nodata} of the {len(turbines)} turbines stand on a nodata cell "
                              'of the DEM; their cylinders are empty and nothing encounters them')
            self._rotor_cylinders = (cells, reach, zband, turbines_mod.build_bins(cells, reach, self.gridsize))
            if self.rotor_transits or self.collision_risk:
                # the disks of K18 / K19: the cylinders' reach, the hubs, and cull lists of their own (a move is culled by
                # its first point: reach + 1.5)
                _, disk_reach, hub, _ = turbines_mod.rotor_disks(turbines, dem, self.bounds, self.resolution,
                                                                 float(self.rotor_clearance))
                self._rotor_disks = (cells, disk_reach, hub, turbines_mod.build_bins(
                    cells, disk_reach + turbines_mod.TRANSIT_CULL_MARGIN, self.gridsize))
            if self.collision_risk:
                # K19: the classes of the fleet and Band's probability per class, direction and ring, once per run
                self._collision_table = turbines_mod.band_collision_table(
                    np.asarray(turbines.columns['t_rd'], dtype=np.float64) / 2., float(self.rotor_clearance),
                    turbines_mod.band_parameters(turbines, self.rotor_blades, self.rotor_rpm, self.rotor_max_chord,
                                                 self.rotor_pitch),
                    float(self.flight_airspeed), float(self.bird_length), float(self.bird_wingspan),
                    str(self.bird_flight).lower() == 'flapping', bool(self.collision_model_3d), self.rotor_chord_profile)[:2]
        return turbines

    THERMAL_LAYERS = inputs.THERMAL_LAYERS      # keys of wtk_layers

    def _wind_km(self, lon, lat):
        """Wind samples at lon / lat (degrees) in kilometres from the centre of cell (0, 0)."""
        x, y = self._need_projection("wind samples at 'lon', 'lat'").forward(lon, lat)
        return (x - self.bounds[0]) / 1000., (y - self.bounds[1]) / 1000.

    def _wtk_thermals(self):
        return str(self.thermal_model).lower() == 'wtk'

    def _allen_thermals(self):
        return str(self.thermal_model).lower() == 'allen'

    def _allen_from_layers(self):
        """thermal_model = 'allen' with zi or w* left at 0: they come from the case's own WTK layers."""
        return self._allen_thermals() and not (float(self.thermal_allen_zi) > 0. and float(self.thermal_allen_wstar) > 0.)

    def _check_thermal_model(self):
        if str(self.thermal_model).lower() not in ('random', 'wtk', 'allen'):
            raise ValueError(f"thermal_model = {self.thermal_model!r}: expected 'random', 'wtk' or 'allen'")
        if self._allen_thermals():
            for name in ('thermal_allen_zi', 'thermal_allen_wstar'):
                v = float(getattr(self, name))
                if not (np.isfinite(v) and v >= 0.):
                    raise ValueError(f'{name} = {getattr(self, name)!r}: expected a finite number >= 0 (0 = from the WTK layers)')
            if not (np.isfinite(float(self.wtk_thermal_height)) and float(self.wtk_thermal_height) > 0.):
                raise ValueError(f"thermal_model = 'allen' evaluates the updrafts at wtk_thermal_height = "
                                 f'{self.wtk_thermal_height!r}: expected metres > 0')
            if int(self.thermals_realization_count) < 1:
                raise ValueError("thermal_model = 'allen' draws one field per realisation: thermals_realization_count must "
                                 f'be at least 1, not {self.thermals_realization_count!r}')
            if str(self.sim_mode).lower() == 'uniform':
                if self._allen_from_layers():
                    raise ValueError("thermal_model = 'allen' in uniform mode has no WTK layers to take them from: "
                                     'thermal_allen_zi and thermal_allen_wstar must both be > 0 '
                                     f'(got {self.thermal_allen_zi!r}, {self.thermal_allen_wstar!r})')
                self._allen_count(float(self.thermal_allen_zi), float(self.thermal_allen_wstar))
        if self._wtk_thermals():
            if str(self.sim_mode).lower() not in ('snapshot', 'seasonal'):
                raise ValueError("thermal_model = 'wtk' needs the WTK layers of a wind case: sim_mode must be 'snapshot' or "
                                 f"'seasonal', not {self.sim_mode!r}")
            if int(self.thermals_realization_count) != 1:
                raise ValueError("thermal_model = 'wtk' gives ONE thermal field per case: thermals_realization_count must "
                                 f'be 1, not {self.thermals_realization_count!r}')

    def _improved(self):
        return str(self.orographic_model).lower() == 'improved'

    def _check_orographic_model(self):
        """The orographic_* fields, on the host (no device work): ValueError names the one that does not fit."""
        if str(self.orographic_model).lower() not in ('original', 'improved'):
            raise ValueError(f"orographic_model = {self.orographic_model!r}: expected 'original' or 'improved'")
        if self._improved():
            layers.check_improved_parameters(self.orographic_sx_dmax, self.resolution, self.orographic_height,
                                             self.orographic_coeffs)
            layers.sector_rays(self.orographic_sx_sector, self.orographic_sx_step)
            if str(self.orographic_smoothing).lower() not in ('none', 'gaussian'):
                raise ValueError(f"orographic_smoothing = {self.orographic_smoothing!r}: expected 'none' or 'gaussian'")
            sigma_m = layers.smoothing_sigma_m(self.orographic_height, self.orographic_smooth_sigma)
            if str(self.orographic_smoothing).lower() == 'gaussian':
                layers.smoothing_radius(sigma_m / float(self.resolution),
                                        f'orographic_smooth_sigma = {sigma_m:g} m at resolution {self.resolution!r} m')

    def _smooth_sigma_m(self):
        """Width in metres of the Gaussian that smooths the improved orograph; 0 = no smoothing."""
        if not self._improved() or str(self.orographic_smoothing).lower() != 'gaussian':
            return 0.
        return layers.smoothing_sigma_m(self.orographic_height, self.orographic_smooth_sigma)

    def _improved_args(self):
        """Keyword arguments of layers.orographic_updraft_improved for this run.  The shelter ray lives in the frame of
        the aspect it multiplies: the Horn fallback computed from the DEM alone is transposed (+row = east, +col =
        north: DESIGN.md K9), injected Slope / Aspect layers are geographic (+row = north, +col = east).  With one layer
        injected and the other from the DEM, the aspect's frame decides."""
        given = 'Aspect' in self._terrain
        args = dict(dmax=float(self.orographic_sx_dmax), height=float(self.orographic_height),
                    coeffs=tuple(self.orographic_coeffs), ray_axes='row_north' if given else 'row_east', want_sx=True,
                    sector=float(self.orographic_sx_sector), sector_step=float(self.orographic_sx_step),
                    smooth_sigma=self._smooth_sigma_m())
        if 'Slope' in self._terrain or 'Aspect' in self._terrain:
            args.update(slope=to_dev(self.get_terrain_slope(), torch.float64),
                        aspect=to_dev(self.get_terrain_aspect(), torch.float64))
        return args

    def _get_sx_fname(self, case_id: str, dirname: str = './'):
        return os.path.join(dirname, f'{case_id}_sx')

    @staticmethod
    def _save_f32(fname, field):
        """`<fname>.npy` in the f32 the files hold, from a tensor or an array."""
        if isinstance(field, torch.Tensor):
            field = field.to(torch.float32).cpu().numpy()
        np.save(f'{fname}.npy', np.asarray(field, dtype=np.float32))

    # -------------------------------------------------------------- terrain
    def get_terrain_elevation(self):
        return self.get_terrain_layer('Elevation')

    def get_terrain_slope(self):
        """Injected 'Slope' layer, else the Horn-stencil fallback the reference
        takes when the GeoTIFF is unavailable (simulator.py:152-159)."""
        try:
            return self.get_terrain_layer('Slope')
        except KeyError:
            return layers.compute_slope_degrees(self.get_terrain_elevation(), self.resolution)

    def get_terrain_aspect(self):
        try:
            return self.get_terrain_layer('Aspect')
        except KeyError:
            return layers.compute_aspect_degrees(self.get_terrain_elevation(), self.resolution)

    def get_terrain_layer(self, lname: str):
        return self._terrain[lname]

    def get_terrain_grid(self):
        xgrid = np.linspace(self.bounds[0], self.bounds[0] + (self.gridsize[1] - 1) *
                            self.resolution, self.gridsize[1])
        ygrid = np.linspace(self.bounds[1], self.bounds[1] + (self.gridsize[0] - 1) *
                            self.resolution, self.gridsize[0])
        return xgrid, ygrid

    # ------------------------------------------------------------- updrafts
    def compute_orographic_updraft_uniform(self) -> None:
        """simulator.py:189-198.  With only a DEM injected this is ONE fused
        kernel (DEM -> orograph); with slope/aspect layers injected, the
        elementwise kernel on those layers."""
        print('Computing orographic updrafts..')
        if self.case_ids[0] not in self._cases_written_here():
            return
        if self._improved():
            orograph, _, sx = layers.orographic_updraft_improved(
                self.get_terrain_elevation(), self.resolution, float(self.uniform_windspeed),
                float(self.uniform_winddirn), **self._improved_args())
            self._save_f32(self._get_sx_fname(self.case_ids[0], self.mode_data_dir), sx)
        elif 'Slope' in self._terrain or 'Aspect' in self._terrain:
            orograph = layers.compute_orographic_updraft(
                float(self.uniform_windspeed), float(self.uniform_winddirn),
                self.get_terrain_slope(), self.get_terrain_aspect())
        else:
            orograph, _ = layers.updraft_from_dem(
                self.get_terrain_elevation(), self.resolution,
                float(self.uniform_windspeed), float(self.uniform_winddirn))
        self._save_f32(self._get_orograph_fname(self.case_ids[0], self.mode_data_dir), orograph)

    _CHUNK = 8          # wind cases per batched device call (the terrain, or the sample geometry, is read once for all)

    def compute_orographic_updrafts_using_wtk(self) -> None:
        """simulator.py:200-215: one orograph per wind case, batched so the
        terrain is read once for all cases."""
        print('Computing orographic updrafts..', end="")
        start_time = time.time()
        mine = set(self._cases_written_here())
        cases = [c for c in self._wind if c.case_id in mine]
        injected = 'Slope' in self._terrain or 'Aspect' in self._terrain
        # DEM-only terrain and wind on one regular lattice: the fused kernel (DEM read once
        # per batch, no per-cell wind rasters, no slope / aspect rasters)
        fused = not self._improved() and not injected and len(cases) > 0 and \
            str(self.wtk_interp_type).lower() == 'linear' and \
            all(c.wind.form == 'lattice' and c.wind.same_points(cases[0].wind) for c in cases)
        if fused or self._improved():
            # (improved: the per-cell wind rasters, always -- the fused lattice kernel has no shelter ray)
            dem = to_dev(self.get_terrain_elevation(), torch.float64)
            improved_args = self._improved_args() if self._improved() else None
        else:
            slope = to_dev(self.get_terrain_slope(), torch.float64)
            aspect = to_dev(self.get_terrain_aspect(), torch.float64)
        for b0 in range(0, len(cases), self._CHUNK):
            chunk = cases[b0:b0 + self._CHUNK]
            if fused:
                oro, _ = layers.updraft_from_dem_lattice(dem, self.resolution, chunk[0].wind.x_km, chunk[0].wind.y_km,
                                                         np.stack([c.wind.values[0] for c in chunk]),
                                                         np.stack([c.wind.values[1] for c in chunk]))
            else:
                ws, wd = (torch.stack(rasters) for rasters in zip(*(self._wind_rasters(c) for c in chunk)))
                if self._improved():
                    oro, _, sx = layers.orographic_updraft_improved(dem, self.resolution, ws, wd, **improved_args)
                    for case, x in zip(chunk, sx):
                        self._save_f32(self._get_sx_fname(case.case_id, self.mode_data_dir), x)
                else:
                    oro, _ = layers.orographic_updraft(ws, wd, slope, aspect)
            for case, o in zip(chunk, oro):
                self._save_f32(self._get_orograph_fname(case.case_id, self.mode_data_dir), o)
        self._nearest_index = (None, None)        # ('nearest': 4 B per cell of device memory, needed no longer)
        print(f'took {_elapsed(start_time)}', flush=True)

    def _wind_rasters(self, entry):
        """Per-cell wind speed / direction (f64 device tensors) of one resolved case: rasters as they are, samples
        through the reference's griddata (simulator.py:765-776) as `wtk_interp_type` says."""
        from .wind import interpolate_wind_lattice, interpolate_wind_scattered, nearest_sample_index
        wind, method = entry.wind, str(self.wtk_interp_type).lower()
        if wind.form == 'raster':
            return tuple(to_dev(v, torch.float64) for v in wind.values)
        if wind.form == 'lattice' and method == 'linear':
            return interpolate_wind_lattice(wind.x_km, wind.y_km, *wind.values, self.gridsize, self.resolution)
        pts = wind.as_points()        # the reference triangulates whatever points it gets: a lattice is its meshgrid points
        index = None
        if method == 'nearest':
            # the index raster depends on the points only: one per wind geometry, not one per case
            if self._nearest_index[0] is None or not pts.same_points(self._nearest_index[0]):
                self._nearest_index = (pts, nearest_sample_index(pts.x_km, pts.y_km, self.gridsize, self.resolution))
            index = self._nearest_index[1]
        ws_d, wd_d = interpolate_wind_scattered(pts.x_km, pts.y_km, *pts.values, self.gridsize, self.resolution,
                                                method=method, index=index)
        if method != 'nearest' and bool(torch.isnan(ws_d).any()):
            # griddata's behaviour (cells outside the samples' convex hull are NaN); the reference
            # prints rather than raises when NaNs turn up (simulator.py:286)
            print(f"{entry.case_id}: NANs in the interpolated wind (raster cells outside the convex "
                  'hull of the wind samples); their updraft is 0')
        return ws_d, wd_d

    def compute_thermal_updrafts_using_wtk(self) -> None:
        """thermal_model = 'wtk': `<case>_r0_thermals.npy` (f32) of every case this rank writes.  Cases that share
        their sample points go through the fused call in chunks (the sample geometry is located once per cell for the
        whole chunk), like the orographic updrafts of compute_orographic_updrafts_using_wtk."""
        print('Computing thermal updrafts from the WTK layers..', end="")
        start_time = time.time()
        mine = set(self._cases_written_here())
        todo = [(c.case_id, c.thermal.as_points()) for c in self._wind if c.case_id in mine]
        while todo:
            first = todo[0][1]
            same = todo[:1] if first.form == 'raster' else \
                [it for it in todo if it[1].form == first.form and it[1].same_points(first)][:self._CHUNK]
            self._write_wtk_thermals(same)
            todo = [it for it in todo if not any(it is s for s in same)]
        print(f'took {_elapsed(start_time)}', flush=True)

    def _write_wtk_thermals(self, items):
        """One device call for `items` = [(case_id, thermal layers as points or rasters), ...] of one form and one set
        of sample points -> their thermal files."""
        from .thermals import compute_wtk_thermals
        height = float(self.wtk_thermal_height)
        first = items[0][1]
        if first.form == 'raster':
            p, t, zi, q = (to_dev(a, torch.float64) for a in first.values)
            wstar = layers.deardoff_velocity_function(layers.compute_potential_temperature(p, t), zi, q)
            fields = layers.compute_thermal_updraft(height, wstar, zi).to(torch.float32)[None].cpu().numpy()
        else:
            stacked = np.stack([samples.values for _, samples in items], 1)            # (4, B, npts)
            fields = compute_wtk_thermals(first.x_km, first.y_km, *stacked, self.gridsize, self.resolution, height,
                                          method=str(self.wtk_interp_type).lower(), dtype=torch.float32)
        for (case_id, _), field in zip(items, fields):
            if np.isnan(field).any():
                # griddata's behaviour, as for the wind (cells outside the samples' convex hull are NaN)
                print(f"{case_id}: NANs in the interpolated thermal layers (raster cells outside the convex "
                      'hull of the samples); their updraft is 0')
            self._save_f32(self._get_thermal_fname(case_id, 0, self.mode_data_dir), field)

    def _thermal_seeds(self, case_id):
        """One key per realisation of a case.  The reference draws every case / realisation from one advancing numpy
        stream (layers.py:188-214), so all fields differ; here each gets its own key from (sim_seed, position of the
        case, realisation)."""
        base = (self.sim_seed if self.sim_seed >= 0 else
                int.from_bytes(os.urandom(4), 'little'))
        case_no = self.case_ids.index(case_id) if case_id in self.case_ids else 0
        return [base + 7919 * (real_id + 1) + 104729 * case_no
                for real_id in range(self.thermals_realization_count)]

    def _allen_count(self, zi, wstar):
        """The host scalars of an Allen field of this run; ValueError when its updrafts are too many."""
        from .thermals import allen_scalars, ALLEN_MAX_UPDRAFTS
        xsize = int(round((self.region_width_km[0] * 1000. / self.resolution)))
        ysize = int(round((self.region_width_km[1] * 1000. / self.resolution)))
        sc = allen_scalars(float(self.wtk_thermal_height), zi, wstar, (ysize, xsize), self.resolution,
                           sink=bool(self.thermal_allen_sink))
        if sc['N'] > ALLEN_MAX_UPDRAFTS:
            raise ValueError(f"thermal_model = 'allen': N = {sc['N']} updrafts for zi = {zi:g} m at wtk_thermal_height = "
                             f'{self.wtk_thermal_height!r} m on this region; at most {ALLEN_MAX_UPDRAFTS} are supported')
        return sc

    def allen_case_scalars(self, case_id: str):
        """(zi, wstar) of a case under thermal_model = 'allen': the positive thermal_allen_* fields, else the means over
        the case's WTK samples (or the finite cells of its rasters) of blheight.clip(min=100) and of
        deardoff_velocity_function(compute_potential_temperature(p, T), blheight, surfheatflux)."""
        zi, wstar = float(self.thermal_allen_zi), float(self.thermal_allen_wstar)
        if zi > 0. and wstar > 0.:
            return zi, wstar
        entry = next(c for c in self._wind if c.case_id == case_id)
        p, t, bl, q = (inputs.host_f64(a).ravel() for a in entry.thermal.values)
        if not zi > 0.:
            clipped = bl.clip(min=100.)
            zi = float(clipped[np.isfinite(clipped)].mean())
        if not wstar > 0.:
            w = np.asarray(layers.deardoff_velocity_function(layers.compute_potential_temperature(p, t), bl, q))
            wstar = float(w[np.isfinite(w)].mean())
        return zi, wstar

    def _write_allen_thermals(self, case_id):
        """thermal_model = 'allen': `<case>_r<k>_thermals.npy` (f32) of every realisation of a case, one device call
        each; the updrafts of realisation k come from its seed, their gains from the case's datetime."""
        from .thermals import allen_datetime_gains, allen_updrafts, compute_allen_thermals
        print('Computing thermal updrafts (Allen)...', flush=True)
        zi, wstar = self.allen_case_scalars(case_id)
        sc = self._allen_count(zi, wstar)
        dtime = None
        if str(self.sim_mode).lower() != 'uniform':
            dtime = next(c for c in self._wind if c.case_id == case_id).datetime
        gains = allen_datetime_gains(dtime)
        for real_id, seed in enumerate(self._thermal_seeds(case_id)):
            ups = allen_updrafts(sc['N'], self.gridsize, self.resolution, seed, gains)
            field = compute_allen_thermals(*ups, self.gridsize, self.resolution, float(self.wtk_thermal_height), zi, wstar,
                                           sink=bool(self.thermal_allen_sink), dtype=torch.float32)
            self._save_f32(self._get_thermal_fname(case_id, real_id, self.mode_data_dir), field)

    def compute_thermal_updrafts(self, case_id: str):
        """simulator.py:217-228; with thermal_model = 'wtk' the one field of the physical model instead, with 'allen'
        Allen's discrete updrafts."""
        if self._wtk_thermals():
            self._write_wtk_thermals([(c.case_id, c.thermal.as_points()) for c in self._wind if c.case_id == case_id])
            return
        if self._allen_thermals():
            self._write_allen_thermals(case_id)
            return
        if self.thermals_realization_count > 0:
            from .thermals import compute_thermals_batch
            print('Computing thermal updrafts...', flush=True)
            aspect = self.get_terrain_aspect()
            seeds = self._thermal_seeds(case_id)
            # one fused call per case, in the f32 the files hold; at most 1 GiB of fields at a time
            chunk = max(1, (1 << 30) // (4 * aspect.shape[0] * aspect.shape[1]))
            aspect = to_dev(aspect, torch.float64)
            for first in range(0, len(seeds), chunk):
                fields = compute_thermals_batch(aspect, 2.0, seeds[first:first + chunk], dtype=torch.float32)
                for k, field in enumerate(fields.cpu().numpy()):
                    self._save_f32(self._get_thermal_fname(case_id, first + k, self.mode_data_dir), field)
        else:
            print('No thermals requested!', flush=True)

    def _updraft_fields(self, case_id, load):
        """The orograph of a case, then orograph + thermal_k of every realisation (simulator.py:230-243), read through
        `load(file name)`."""
        orograph = load(f'{self._get_orograph_fname(case_id, self.mode_data_dir)}.npy')
        yield orograph
        for real_id in range(int(self.thermals_realization_count)):
            yield orograph + load(f'{self._get_thermal_fname(case_id, real_id, self.mode_data_dir)}.npy')

    def load_updrafts(self, case_id: str, apply_threshold=True):
        """simulator.py:230-243 -> [orograph] + [orograph + thermal_k], each
        passed through the threshold function (f64) when requested."""
        updrafts = list(self._updraft_fields(case_id, np.load))
        if apply_threshold:
            updrafts = [layers.get_above_threshold_speed(ix, self.updraft_threshold)
                        for ix in updrafts]
        return updrafts

    def _get_orograph_fname(self, case_id: str, dirname: str = './'):
        return os.path.join(dirname, f'{case_id}_orograph')

    def _get_thermal_fname(self, case_id: str, real_id: int, dirname: str = './'):
        return os.path.join(dirname, f'{case_id}_r{real_id}_thermals')

    # ------------------------------------------------------------ potential
    def get_directional_potential(self, updraft, case_id, real_id):
        """simulator.py:259-288: cached `<id>_potential.npy` when its shape
        matches, else the GPU solve; saved as f32."""
        potential = self._cached_potential(case_id, real_id)
        if potential is None:
            start_time = time.time()
            print(f'{self._get_id_string(case_id, real_id)}: Computing potential..', end="", flush=True)
            potential = potential_mod.solve_potential(np.asarray(updraft), self.track_direction)
            print(f'took {_elapsed(start_time)}', flush=True)
            np.save(f'{self._get_potential_fname(case_id, real_id, self.mode_data_dir)}.npy', potential.astype(np.float32))
        if np.isnan(potential).any():
            print('NANs found in potential!')
        return potential

    def _cached_potential(self, case_id, real_id):
        """The saved `<id>_potential.npy` (f32) when it fits this run, else None: its shape must be the grid's, and an
        unseeded run keeps only realisation 0 (simulator.py:262-270)."""
        try:
            potential = np.load(f'{self._get_potential_fname(case_id, real_id, self.mode_data_dir)}.npy')
        except FileNotFoundError:
            return None
        if potential.shape != self.gridsize or (self.sim_seed < 0) & (real_id != 0):
            return None
        print(f'{self._get_id_string(case_id, real_id)}: Found saved potential')
        return potential

    def _get_id_string(self, case_id: str, real_id=None):
        """simulator.py:290-298: <case>_d<dir>_t<thr*100>_<model>[_r<k>]."""
        model = self.movement_model
        if self._improved():
            # (a cached potential of the original model must never be picked up for the improved one)
            model = f'{self.movement_model}-sx{int(self.orographic_sx_dmax)}h{int(self.orographic_height)}'
            if float(self.orographic_sx_sector) > 0.:           # (nor that of a single-ray run for a sector's)
                model += f'a{float(self.orographic_sx_sector):g}s{float(self.orographic_sx_step):g}'
            if self._smooth_sigma_m() > 0.:                     # (nor that of an unsmoothed run for a smoothed one's)
                model += f'g{self._smooth_sigma_m():g}'
        if self._allen_thermals():                              # (nor a potential of another thermal model)
            model += '-allen'
        out_str = (f'{case_id}_d{int(self.track_direction % 360)}'
                   f'_t{int(self.updraft_threshold * 100)}_{model}')
        if real_id is not None:
            out_str += f'_r{int(real_id)}'
        return out_str

    def _get_potential_fname(self, case_id: str, real_id: int, dirname: str):
        return os.path.join(dirname, f'{self._get_id_string(case_id, real_id)}_potential')

    def _get_tracks_fname(self, case_id: str, real_id: int, dirname: str):
        return os.path.join(dirname, f'{self._get_id_string(case_id, real_id)}_tracks')

    def _get_presence_fname(self, case_id: str, real_id: int, dirname: str):
        return os.path.join(dirname, f'{self._get_id_string(case_id, real_id)}_presence')

    def _get_uniform_id(self):
        return f's{int(self.uniform_windspeed)}d{int(self.uniform_winddirn)}'

    # --------------------------------------------------------------- tracks
    def _stream_seed(self, real_id):
        """Key of the Philox stream of one realisation: sim_seed + real_id, the
        value the reference reseeds numpy with (simulator.py:351-352); a fresh
        random key when the run is unseeded (sim_seed < 0)."""
        if self.sim_seed >= 0:
            return int(self.sim_seed) + int(real_id)
        seed = int.from_bytes(os.urandom(7), 'little')
        if self._shards_tracks():
            # the shards of one case are ONE batch: every rank steps under rank 0's key (the items
            # are prepared in the same order on every rank, so the broadcasts pair up)
            seed = int(distributed.broadcast(np.array([seed], dtype=np.int64))[0])
        return seed

    # device-resident forms of load_updrafts / get_directional_potential: the public methods
    # keep the reference's numpy-in / numpy-out contract, the stepper takes these
    def _load_updrafts_dev(self, case_id):
        fields = self._updraft_fields(case_id, lambda fname: to_dev(np.load(fname), torch.float32))
        return [layers.get_above_threshold_speed(f, self.updraft_threshold) for f in fields]

    def _potential_dev(self, updraft, case_id, real_id):
        """get_directional_potential on device tensors: the cached .npy when valid, else
        the GPU solve (written to the cache by the rank that owns the case)."""
        fname = self._get_potential_fname(case_id, real_id, self.mode_data_dir)
        sharded = self._shards_tracks()
        if sharded and self._rank() != 0:
            self._barrier()                       # rank 0 solves (or finds the cache) and saves
            return to_dev(np.load(f'{fname}.npy'), torch.float32)
        potential = self._cached_potential(case_id, real_id)
        if potential is not None:
            pot = to_dev(potential, torch.float32)
        else:
            start_time = time.time()
            print(f'{self._get_id_string(case_id, real_id)}: Computing potential..', end="", flush=True)
            pot = potential_mod.solve_potential(updraft, self.track_direction)
            torch.cuda.current_stream().synchronize()
            print(f'took {_elapsed(start_time)}', flush=True)
            np.save(f'{fname}.npy', pot.cpu().numpy())
        if bool(torch.isnan(pot).any()):
            print('NANs found in potential!')
        if sharded:
            self._barrier()
        return pot

    def simulate_tracks(self):
        """simulator.py:332-386.  With a torch.distributed process group (one process per
        GPU) the work is sharded like SURVEY 8(e): wind cases over the ranks when there are
        at least as many cases as ranks (seasonal mode), otherwise the TRACKS of every case
        over the ranks by contiguous global id ranges (uniform / snapshot mode): each rank
        steps its share against its own replica of the rasters, the presence histograms are
        summed over the ranks and rank 0 writes the case's <id>_tracks.pkl."""
        print(f'Movement model = {self.movement_model}')
        print(f'Updraft threshold = {self.updraft_threshold} m/s')
        print(f'Movement direction = {self.track_direction} deg (cw)')
        starting_rows, starting_cols = movmodel.get_starting_indices(
            self.track_count, self.track_start_region, self.track_start_type,
            self.region_width_km, self.resolution)
        starts = np.stack([starting_rows, starting_cols], 1).astype(np.int32)
        use_table = {'auto': None, 'table': True, 'direct': False}[self.stepper_path]
        self.last_stats = {}
        self.last_seeds = {}
        sharded = self._shards_tracks()
        if sharded and self.sim_seed < 0:
            # unseeded: every rank drew its own start cells; the batch is rank 0's
            starts = distributed.broadcast(starts)
        lo, hi = 0, len(starts)
        if sharded:
            lo, hi = distributed.shard_range(len(starts), self._rank(), self._world())
        my_starts = to_dev(starts[lo:hi], torch.int32)
        # the largest share of any rank (shard sizes differ by one): whether the counts are kept in 64 bits
        # must not depend on the rank, or the ranks would meet in the reduce with different dtypes
        widest_share = -(-len(starts) // self._world()) if sharded else len(starts)

        # everything accumulated from the trajectory chunks (ssrs_amd/products.py), in the order of that module's docstring:
        # the constants and device uploads of this call, made once
        products = products_mod.enabled(self)
        # trajectories: for the pickle, or for the products (which read them on the device)
        want_tracks = bool(self.save_tracks) or bool(products)

        # (case, realisation) items are independent: like the reference's loop
        # they are prepared in order on this thread (file cache, reseeding), then
        # stepped concurrently, one HIP stream per worker thread (seasonal mode
        # has many small batches that cannot fill the GPU one at a time).
        def prepare():
            for case_id in self.my_case_ids():
                fluid = self.movement_model == 'fluidflow'
                if self.movement_model not in ('fluidflow', 'drw'):
                    raise ValueError(f'unknown movement_model {self.movement_model!r}')
                updrafts = self._load_updrafts_dev(case_id) if fluid else \
                    [None] * (1 + int(self.thermals_realization_count))
                # what the products read per case (the wind, the rotors' axes, the un-thresholded updrafts), once per case
                inputs = {}
                for product in products:
                    product.prepare(case_id, inputs)
                for real_id, updraft in enumerate(updrafts):
                    if self.sim_seed > 0:
                        np.random.seed(self.sim_seed + real_id)
                    fields = (updraft, self._potential_dev(updraft, case_id, real_id)) if fluid \
                        else (None, None)
                    yield SimpleNamespace(case_id=case_id, real_id=real_id, fields=fields, seed=self._stream_seed(real_id),
                                          inputs=inputs, state={})

        def run(item):
            key = (item.case_id, item.real_id)
            self.last_seeds[key] = item.seed
            id_str = self._get_id_string(*key)
            start_time = time.time()
            with torch.cuda.stream(torch.cuda.Stream()):
                batch = self._step_case(my_starts, lo, item.fields, item.seed, use_table, widest_share, want_tracks)
                torch.cuda.current_stream().synchronize()
                print(f'{id_str}: Simulating {hi - lo} tracks..took {_elapsed(start_time)}',
                      flush=True)
                for product in products:
                    item.state[product] = product.begin(item, hi - lo, my_starts.device)
                # every device chunk of the trajectories goes through the products on the device, then (save_tracks) on to
                # the pickle: a replay range is stepped ONCE for all
                chunks = self._device_chunks(batch, products, item.state) if products else None
                if self.save_tracks:
                    # (inside the stream's scope: long trajectories are stepped again range by range while written)
                    need = sum(b.total_points for b in batch.parts) * 4
                    if sharded:
                        # the limit is the merged file's, and every rank must reach the same verdict (a rank
                        # that raised alone would leave the others waiting in _write_tracks' barrier)
                        need = int(self._allreduce_sum(np.array([need], dtype=np.int64))[0])
                    if need > float(self.max_tracks_file_gb) * 2 ** 30:
                        raise ValueError(
                            f'{id_str}: the trajectories of these {len(starts)} tracks are {need / 2 ** 30:.1f} GiB '
                            f'(Sum lengths x 4 B; max_tracks_file_gb = {self.max_tracks_file_gb:g}): on fields where '
                            'tracks wander to max_moves run with save_tracks=False, or raise max_tracks_file_gb')
                    fname = self._get_tracks_fname(item.case_id, item.real_id, self.mode_data_dir)
                    tracks = (t for b in batch.parts for t in b.iter_tracks()) if chunks is None else \
                        (t for traj, off in chunks for t in movmodel.TrackBatch.host_tracks(traj, off))
                    self._write_tracks(fname, tracks, sharded)
                    torch.cuda.current_stream().synchronize()
                elif chunks is not None:
                    for _ in chunks:
                        pass
                # (track-sharded: every store is a collective or several, issued here in list and item order like the rest)
                for product in products:
                    product.store(item.state[product], key, sharded)
            if sharded:
                batch.hist = distributed.reduce_histogram(batch.hist, all_ranks=True)
            return key, batch

        nitems = max(1, len(self.my_case_ids())) * (1 + int(self.thermals_realization_count))
        # collectives of the track-sharded form must be issued in the same order on every rank
        workers = 1 if sharded else max(1, min(nitems, int(self.max_cores), 8))

        def collect(results):
            for key, batch in results:
                self._presence_counts[key] = batch.hist
                self.last_stats[key] = batch.stats

        if workers == 1:
            try:
                collect(run(it) for it in prepare())
            finally:
                # the stepper's scratch (13-15 GB with the pair / fine tables at 5000 x 6000) is cached per
                # thread between calls; K4, K5 and the next run size their own buffers from the free HBM
                movmodel.release_workspaces()
        else:
            # bounded pipeline: at most `workers` prepared items (device rasters) alive
            from concurrent.futures import ThreadPoolExecutor, wait, FIRST_COMPLETED
            with ThreadPoolExecutor(workers) as pool:
                pending = set()
                for it in prepare():
                    pending.add(pool.submit(run, it))
                    if len(pending) >= workers:
                        done, pending = wait(pending, return_when=FIRST_COMPLETED)
                        collect(f.result() for f in done)
                collect(f.result() for f in pending)

    @staticmethod
    def _device_chunks(batch, products, states):
        """The device chunks (traj, offsets) of every part of `batch` in track order, each one handed as a `Chunk` -- its
        track numbers within the batch -- to every product in list order before it is handed on."""
        base = 0
        for part in batch.parts:
            for t0, t1, traj, off in part.iter_device_chunks():
                chunk = products_mod.Chunk(base + t0, base + t1, traj, off)
                for product in products:
                    product.consume(states[product], chunk)
                del chunk                   # (its masked / alt / dt go before the chunk is handed on)
                yield traj, off
            base += int(part.lengths.numel())

    def _flight_params(self):
        """(heights in metres for flight.compute_track_altitudes, airspeed, sink rate) of the flight_* fields, checked."""
        airspeed = float(self.flight_airspeed)
        if not airspeed > 0.:
            raise ValueError(f'flight_airspeed = {self.flight_airspeed!r}: expected m/s > 0')
        sink = float(self.flight_sink_rate)
        if sink != sink:
            raise ValueError(f'flight_sink_rate = {self.flight_sink_rate!r}: expected m/s (< 0 = updraft_threshold)')
        if sink < 0.:
            sink = float(self.updraft_threshold)
        kw = dict(start=self.flight_height_start, floor=self.flight_height_floor, ceil=self.flight_height_ceiling,
                  band=self.rotor_zone)
        flight.height_params(who='Config.flight_height_* / rotor_zone', **kw)
        return kw, airspeed, sink

    def _time_params(self):
        """Keyword arguments of flight.compute_track_times from the resolution and the flight_* fields, checked."""
        kw = dict(resolution=self.resolution, airspeed=self.flight_airspeed, min_groundspeed=self.flight_min_groundspeed)
        flight.time_params(who='Config.resolution / flight_airspeed / flight_min_groundspeed', **kw)
        return kw

    def _time_ray_axes(self):
        """The frame of the wind's components: that of the aspect, as _improved_args chooses the shelter ray's."""
        return 'row_north' if 'Slope' in self._terrain or 'Aspect' in self._terrain else 'row_east'

    _MIN_SPLIT_TRACKS = 64          # a wrapped sub-batch smaller than twice this is an error, not a split
    _HIST64_FROM_TRACKS = 100_000   # sub-batches larger than this count in 64 bits (when no trajectories are asked for)

    def _step_case(self, my_starts, lo, fields, seed, use_table, widest_share=None, want_tracks=None):
        """The tracks of one (case, realisation) on this rank; want_tracks: with their trajectories, for the pickle or for
        the track products (None: as save_tracks says).  The presence histogram is uint32 (the
        reference's int16 wraps at 32 767, movmodel.py:415): a trap cell of the solved 10 m field takes
        ~1e9 visits per 100k tracks, so more than `hist_safe_tracks` tracks are stepped in sub-batches whose
        histograms are added up in 64 bits (K4 takes that form), and every sub-batch is checked by its
        checksum -- the counts must add up to the points of its tracks; a wrapped cell leaves 2^32 missing, and that
        sub-batch is stepped again as two halves (HistogramOverflow only below _MIN_SPLIT_TRACKS tracks)."""
        n = int(my_starts.shape[0])
        safe = max(1, int(self.hist_safe_tracks))
        widen = max(n, int(widest_share or 0)) > safe
        # equal sub-batches of at most hist_safe_tracks tracks: a pass lasts as long as its longest track chain, so a
        # short last sub-batch would cost a full pass's time for a fraction of the work
        step = max(1, -(-n // max(1, -(-n // safe))))
        parts, wide, stats = [], None, None
        if want_tracks is None:
            want_tracks = bool(self.save_tracks)
        # (start, length) of the sub-batches still to step, in track-id order; one whose uint32 counts wrapped is stepped
        # again as two halves, added up in 64 bits like the rest
        todo = [(t0, min(step, n - t0)) for t0 in range(0, max(n, 1), step)]
        while todo:
            t0, m = todo.pop(0)
            sub = my_starts[t0:t0 + m]
            # large sub-batches without trajectories count in 64 bits inside the library (the trap cells of a solved 10 m field
            # pass 2^32 visits from ~250 000 tracks on: ssrs_tracks_simulate_h64); the others keep the uint32 raster
            use64 = not want_tracks and m > self._HIST64_FROM_TRACKS
            b = movmodel.simulate_tracks(
                self.track_direction, sub, self.gridsize, self.track_dirn_restrict,
                self.track_stochastic_nu, fields[0], fields[1], seed=seed, track_id_base=lo + t0,
                use_table=use_table, want_tracks=want_tracks,
                steps_per_launch=self.steps_per_launch, hist64=use64)
            if b.hist.dtype == torch.int64:
                widen = True
                counted = int(b.hist.sum().item())
            else:
                counted = int((b.hist.view(torch.int32).to(torch.int64) & 0xFFFFFFFF).sum().item())
            if counted != b.total_points:
                if m < 2 * self._MIN_SPLIT_TRACKS:
                    raise distributed.HistogramOverflow(
                        f'presence histogram: {b.total_points - counted} visits are missing from the uint32 counts of '
                        f'{m} tracks (a cell passed 2^32 - 1)')
                import warnings
                warnings.warn(f'presence histogram: the uint32 counts of a sub-batch of {m} tracks wrapped '
                              f'({b.total_points - counted} visits missing); stepping it again as two halves '
                              f'(Config.hist_safe_tracks = {self.hist_safe_tracks} is too many for this field)', RuntimeWarning)
                todo[:0] = [(t0, m // 2), (t0 + m // 2, m - m // 2)]
                if not widen and parts:                       # (cannot happen: without `widen` there is one sub-batch)
                    raise distributed.HistogramOverflow('presence histogram: sub-batch wrapped after others were kept in 32 bits')
                widen = True
                del b
                continue
            parts.append(b)
            if widen:
                h64 = b.hist if b.hist.dtype == torch.int64 else b.hist.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
                wide = h64 if wide is None else wide.add_(h64)
                b.hist = None
            if stats is None:
                stats = dict(b.stats)
            else:
                for k, v in b.stats.items():
                    if isinstance(v, (int, float)) and not isinstance(v, bool):
                        stats[k] = stats.get(k, 0) + v
        first = parts[0]
        out = movmodel.TrackBatch(first.lengths if len(parts) == 1 else torch.cat([b.lengths for b in parts]),
                                  first.ends if len(parts) == 1 else torch.cat([b.ends for b in parts]),
                                  first.hist if wide is None else wide, None, None, stats)
        out.parts = parts
        return out

    class _TrackStream:
        """Pickles as a plain list whose items come from an iterator (pickle appends them in batches):
        <id>_tracks.pkl is written without ever holding all trajectories in memory."""

        def __init__(self, items):
            self.items = items

        def __reduce__(self):
            return (list, (), None, iter(self.items))

    @classmethod
    def _dump_tracks(cls, fobj, tracks):
        pickler = pickle.Pickler(fobj, protocol=4)
        pickler.fast = True            # no memo: nothing is shared between tracks, and a memo would keep them all alive
        pickler.dump(cls._TrackStream(tracks))

    def _write_tracks(self, fname, tracks, sharded):
        """<id>_tracks.pkl (simulator.py:382-385) = pickle of List[int16 (n_i, 2)], written as a stream
        (`tracks` may be a generator).  Track-sharded runs: every rank writes its share next to it as a
        sequence of pickled chunks, rank 0 streams the shares in rank order (= global track id order) into
        the one file of the contract and removes them."""
        if not sharded:
            with open(f'{fname}.pkl', "wb") as fobj:
                self._dump_tracks(fobj, tracks)
            return
        with open(f'{fname}.pkl.part{self._rank()}', "wb") as fobj:
            chunk = []
            for t in tracks:
                chunk.append(t)
                if len(chunk) >= 4096:
                    pickle.dump(chunk, fobj, protocol=4)
                    chunk = []
            pickle.dump(chunk, fobj, protocol=4)
        self._barrier()
        if self._rank() == 0:
            def parts():
                for r in range(self._world()):
                    with open(f'{fname}.pkl.part{r}', 'rb') as fobj:
                        while True:
                            try:
                                yield from pickle.load(fobj)
                            except EOFError:
                                break
                    os.remove(f'{fname}.pkl.part{r}')
            with open(f'{fname}.pkl', "wb") as fobj:
                self._dump_tracks(fobj, parts())
        self._barrier()

    # ------------------------------------------------------------- the score of observed tracks
    def _score_inputs(self, who, tracks, case_id, real_id, xy):
        """(tracks as cells, case_id, real_id, (updraft, potential)) of score_tracks and fit_tracks: the case and the
        realisation resolved as simulate_tracks resolves them, [x, y] metres walked to cells when xy."""
        if self.movement_model not in ('fluidflow', 'drw'):
            raise ValueError(f'unknown movement_model {self.movement_model!r}')
        case_id = self.case_ids[0] if case_id is None else case_id
        if case_id not in self.case_ids:
            raise ValueError(f'{who}: case_id {case_id!r} is not one of {self.case_ids}')
        real_id = int(real_id)
        if xy:
            cells = []
            for t in tracks:
                t = np.asarray(t, dtype=np.float64).reshape(-1, 2)
                cells.append(movmodel.rasterize_track((t[:, 1] - float(self.bounds[1])) / float(self.resolution),
                                                      (t[:, 0] - float(self.bounds[0])) / float(self.resolution)))
            tracks = cells
        fields = (None, None)
        if self.movement_model == 'fluidflow':
            updrafts = self._load_updrafts_dev(case_id)
            if not 0 <= real_id < len(updrafts):
                raise ValueError(f'{who}: real_id {real_id} outside the {len(updrafts)} realisations of {case_id}')
            updraft = updrafts[real_id]
            if self._shards_tracks():
                # (_potential_dev meets the other ranks in a barrier; here nothing is shared)
                cached = self._cached_potential(case_id, real_id)
                potential = to_dev(cached, torch.float32) if cached is not None else \
                    potential_mod.solve_potential(updraft, self.track_direction)
            else:
                potential = self._potential_dev(updraft, case_id, real_id)
            fields = (updraft, potential)
        return tracks, case_id, real_id, fields

    def score_tracks(self, tracks, case_id=None, real_id=0, xy=False):
        """The probability this run's movement model gives to every move of OBSERVED tracks (movmodel.score_tracks,
        DESIGN.md K21): the fields of `case_id` (default: the first case) and realisation `real_id`, resolved as
        simulate_tracks resolves them, with track_direction, track_dirn_restrict and track_stochastic_nu.

        tracks: a list of (n_i, 2) arrays, [row, col] cells of 8-connected sequences -- what <id>_tracks.pkl holds --
        or, with xy=True, [x, y] in projected metres of successive fixes, which are converted to cells like the turbine
        table's coordinates ((x - west) / resolution along columns, (y - south) / resolution along rows) and joined by
        movmodel.rasterize_track's line walk.  Returns the TrackScores and writes <id>_track_scores.npy, int64
        (ntracks, 6): S and the numbers of moves by status (movmodel.SCORE_COLUMNS).  Every rank that calls it scores all
        the tracks it is given; there are no collectives."""
        tracks, case_id, real_id, fields = self._score_inputs('score_tracks', tracks, case_id, real_id, xy)
        scores = movmodel.score_tracks(tracks, self.gridsize, self.track_direction, self.track_dirn_restrict,
                                       self.track_stochastic_nu, fields[0], fields[1])
        fname = os.path.join(self.mode_data_dir, f'{self._get_id_string(case_id, real_id)}_track_scores')
        np.save(f'{fname}.npy', scores.host_rows())
        return scores

    def fit_tracks(self, tracks, case_id=None, real_id=0, xy=False, memories=(1, 2, 3, 4), nus=None, rounds=3,
                   zero_bits=np.inf):
        """The memory (track_dirn_restrict) and nu (track_stochastic_nu) under which this run's movement model gives
        OBSERVED tracks the largest likelihood (movmodel.fit_tracks), on the fields and the heading that
        score_tracks uses; tracks, case_id, real_id and xy as score_tracks takes them.  It neither reads nor sets the run's
        own track_dirn_restrict and track_stochastic_nu.  Returns the TrackFit and writes <id>_track_fit.npz: memory, nu,
        bits, nu_lo, nu_hi, and of the last round memories, nus and rows_total, int64 (nmem, nnu, 6), its rows summed
        over the tracks.  No collectives."""
        tracks, case_id, real_id, fields = self._score_inputs('fit_tracks', tracks, case_id, real_id, xy)
        fit = movmodel.fit_tracks(tracks, self.gridsize, self.track_direction, fields[0], fields[1], memories=memories,
                                  nus=nus, rounds=rounds, zero_bits=zero_bits)
        last = fit.profiles[-1]
        fname = os.path.join(self.mode_data_dir, f'{self._get_id_string(case_id, real_id)}_track_fit')
        np.savez(f'{fname}.npz', memory=np.int64(fit.memory), nu=np.float64(fit.nu), bits=np.float64(fit.bits),
                 nu_lo=np.float64(fit.nu_lo), nu_hi=np.float64(fit.nu_hi), memories=np.array(last.memories, dtype=np.int64),
                 nus=last.nus, rows_total=last.host_rows().sum(0))
        return fit

    def score_fixes(self, fixes, moves=None, case_id=None, real_id=0, xy=False):
        """The probability this run's movement model gives to the gaps between successive fixes of SPARSE telemetry
        (movmodel.score_gaps): for every pair of fixes the sum over every path of `moves` moves between
        them, on the fields and the heading that score_tracks uses, with track_stochastic_nu.  The gap states are (cell,
        last move), so the run's track_dirn_restrict must be 1.

        fixes: a list of (n_i, 2) integer arrays, [row, col] cells that need not be adjacent, or, with xy=True, [x, y] in
        projected metres, rounded to their cells ((x - west) / resolution along columns, (y - south) / resolution along
        rows) and NOT joined by a line.  moves: None (the Chebyshev distance of every pair: the fewest moves, a lower
        bound) or a list of one (n_i - 1,) integer array per track, as movmodel.fix_gaps takes them.  Returns the GapScores
        with two more host arrays, track and pair (int64 (ngaps,): the track and the pair of it each gap came from), and
        writes <id>_gap_scores.npy, int64 (ngaps, 4): track, pair, status, surprisal.  No collectives."""
        if int(self.track_dirn_restrict) != 1:
            raise ValueError(f'score_fixes: track_dirn_restrict = {self.track_dirn_restrict} is not supported: the states of '
                             'a gap are (cell, last move), which is track_dirn_restrict = 1')
        fixes = list(fixes)
        if moves is not None and len(moves) != len(fixes):
            raise ValueError(f'score_fixes: {len(moves)} arrays of moves for {len(fixes)} tracks')
        if xy:
            cells = []
            for t in fixes:
                t = np.asarray(t, dtype=np.float64).reshape(-1, 2)
                if not np.isfinite(t).all():
                    raise ValueError('score_fixes: a fix is not finite')
                cells.append(np.stack([np.rint((t[:, 1] - float(self.bounds[1])) / float(self.resolution)),
                                       np.rint((t[:, 0] - float(self.bounds[0])) / float(self.resolution))], 1).astype(np.int64))
            fixes = cells
        fixes, case_id, real_id, fields = self._score_inputs('score_fixes', fixes, case_id, real_id, False)
        jobs, track, pair = [np.zeros((0, 6), dtype=np.int32)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
        for t, cells in enumerate(fixes):
            j, k = movmodel.fix_gaps(cells, None if moves is None else moves[t])
            jobs.append(j), pair.append(k), track.append(np.full(len(k), t, dtype=np.int64))
        scores = movmodel.score_gaps(np.concatenate(jobs), self.gridsize, self.track_direction, self.track_stochastic_nu,
                                     fields[0], fields[1])
        scores.track, scores.pair = np.concatenate(track), np.concatenate(pair)
        fname = os.path.join(self.mode_data_dir, f'{self._get_id_string(case_id, real_id)}_gap_scores')
        np.save(f'{fname}.npy', np.stack([scores.track, scores.pair, scores.status.cpu().numpy().astype(np.int64),
                                          scores.surprisal.cpu().numpy()], 1))
        return scores

    # ------------------------------------------------------------- presence
    def _counts_for(self, case_id, real_id):
        hist = self._presence_counts.get((case_id, real_id))
        if hist is not None:
            return hist
        fname = self._get_tracks_fname(case_id, real_id, self.mode_data_dir)
        with open(f'{fname}.pkl', 'rb') as fobj:
            tracks = pickle.load(fobj)
        flat = np.concatenate(tracks) if len(tracks) else np.zeros((0, 2), dtype=np.int16)
        return presence.compute_presence_counts(torch.from_numpy(flat).cuda(), self.gridsize)

    def _presence_summary(self, krad, counts_for=None, may_be_empty=False):
        """The normalisation ladder of plot_presence_map / plot_windplant_presence_map (simulator.py:521-546, :572-586)
        with a disk of `krad` cells: (the f32 summary map, the same on every rank; this rank's per-case maps).
        counts_for(case_id, real_id): the source of the counts, _counts_for (the visit histograms) by default.
        may_be_empty: a raster may be all zero (a visit histogram never is: every track has its first point); its
        division by the maximum is then left out, so it contributes zeros, and so on up the ladder."""
        counts_for = counts_for or self._counts_for
        some = (lambda t: bool((t != 0).any())) if may_be_empty else (lambda t: True)
        dev = self._presence_device()
        summary = torch.zeros(self.gridsize, dtype=torch.float64, device=dev)
        case_presence = {}
        for case_id in self.my_case_ids():
            nreal = 1 + int(self.thermals_realization_count)
            case_prob = torch.zeros(self.gridsize, dtype=torch.float64, device=dev)
            for real_id in range(nreal):
                counts = counts_for(case_id, real_id)
                if some(counts):
                    prprob = presence.smooth_presence_counts(counts, krad)
                    presence.normalise_add(prprob, case_prob)   # prprob /= amax; case += prprob
            if some(case_prob):
                presence.normalise_add(case_prob, summary)      # case /= amax; summary += case
            case_presence[case_id] = case_prob
        if not self._shards_tracks():
            distributed.reduce_presence_sum(summary)                        # cases of the other ranks
        if not some(summary):
            return np.zeros(self.gridsize, dtype=np.float32), case_presence
        return presence.normalise_to_f32(summary).cpu().numpy(), case_presence  # summary /= amax -> f32

    def compute_presence_map(self, radius: float = 1000.):
        """The numeric part of plot_presence_map (simulator.py:518-546): returns
        the f32 summary map and writes summary_presence.npy."""
        out, self.case_presence = self._presence_summary(
            presence.presence_kernel_radius(radius, self.resolution, self.gridsize))
        return self._save_summary('presence', out)

    def compute_rotor_presence_map(self, radius: float = 1000.):
        """compute_presence_map of the points in the rotor zone alone (flight_height=True): the same ladder
        over rotor_presence_counts.  A (case, realisation) without a point in the zone contributes zeros.  Returns the
        f32 summary map and writes summary_rotor_presence.npy.  ValueError when simulate_tracks computed no heights."""
        if not self.rotor_presence_counts:
            raise ValueError('no rotor-zone presence was computed: run simulate_tracks() with flight_height=True')
        out, self.case_rotor_presence = self._presence_summary(
            presence.presence_kernel_radius(radius, self.resolution, self.gridsize),
            counts_for=lambda case_id, real_id: to_dev(self.rotor_presence_counts[(case_id, real_id)], torch.int32),
            may_be_empty=True)
        return self._save_summary('rotor_presence', out)

    def _time_share_map(self, counts, radius, fname, what):
        if not counts:
            raise ValueError(f'no {what} was computed: run simulate_tracks() with flight_time=True'
                             + (' and flight_height=True' if 'rotor' in fname else ''))
        out, per_case = self._presence_summary(
            presence.presence_kernel_radius(radius, self.resolution, self.gridsize) if radius > 0. else 0,
            counts_for=lambda case_id, real_id: to_dev(counts[(case_id, real_id)], torch.int64), may_be_empty=True)
        total = float(out.sum(dtype=np.float64))
        if total > 0.:
            out = (out.astype(np.float64) / total).astype(np.float32)
        if self._rank() == 0:
            np.save(os.path.join(self.mode_data_dir, fname), out)
        self._barrier()
        return out, per_case

    def compute_residence_time_map(self, radius: float = 1000.):
        """Each cell's share of all flight time (flight_time=True): the ladder of compute_presence_map over
        residence_time_counts -- the 64-bit disk smoothing (ssrs_presence_smooth_u64) of every item's microseconds, the
        same normalisations over realisations and cases -- and the summary divided by its sum, so that the map adds up to
        1 (a run without a timed move gives zeros).  radius = 0: no smoothing; one item is then its raster over its
        total.  Returns the f32 map and writes summary_residence_time.npy.  ValueError when simulate_tracks timed nothing."""
        out, self.case_residence_time = self._time_share_map(self.residence_time_counts, float(radius),
                                                             'summary_residence_time.npy', 'flight time')
        return out

    def compute_rotor_residence_time_map(self, radius: float = 1000.):
        """compute_residence_time_map of the time spent in the rotor zone alone (flight_time=True and flight_height=True):
        each cell's share of it.  Writes summary_rotor_residence_time.npy."""
        out, self.case_rotor_residence_time = self._time_share_map(self.rotor_residence_time_counts, float(radius),
                                                                   'summary_rotor_residence_time.npy', 'rotor-zone flight time')
        return out

    def compute_windplant_presence_map(self, pname, radius: float = 100., pad: float = 2000.):
        """The numeric part of plot_windplant_presence_map (simulator.py:557-592): the same ladder with this method's
        radius -- handed on unrounded there, so int() truncates it (presence.windplant_kernel_radius) -- cropped to the
        axis limits of :589-590.  Returns (window, (r0, r1, c0, c1)): the f32 summary over the cells whose centres lie within
        `pad` of the project's turbines in x and in y, window = summary[r0:r1, c0:c1], clipped to the raster; writes
        presence_<pname>.npy.  ValueError for an unknown project or a window without cells."""
        if self.turbines is None:
            raise ValueError('compute_windplant_presence_map needs turbines (Simulator(..., turbines=...))')
        xloc, yloc = self.turbines.get_locations_for_this_project(pname)
        if len(xloc) == 0:
            raise ValueError(f'no turbines of a project {pname!r} inside the bounds '
                             f'(projects: {list(self.turbines.get_project_names())})')
        window = turbines_mod.windplant_window(xloc, yloc, float(pad), self.bounds, self.resolution, self.gridsize)
        r0, r1, c0, c1 = window
        summary, _ = self._presence_summary(presence.windplant_kernel_radius(radius, self.resolution, self.gridsize))
        out = np.ascontiguousarray(summary[r0:r1, c0:c1])
        if self._rank() == 0:
            np.save(os.path.join(self.mode_data_dir, f'presence_{pname}.npy'), out)
        self._barrier()
        return out, window

    def _item_mean(self, items):
        """The mean over all (case, realisation) items of the f64 arrays `items` (numpy, or tensors on the device), added up
        in the order given -- the callers give sorted keys -- with the number of items behind them; case-sharded runs sum
        both over the ranks, so the mean is over every rank's items."""
        total, nitems = 0., 0.
        for item in items:
            total, nitems = total + item, nitems + 1.
        if self._world() > 1 and not self._shards_tracks():
            # the cases of the other ranks
            flat = total.cpu().numpy() if torch.is_tensor(total) else total
            summed = np.asarray(self._allreduce_sum(np.append(flat.ravel(), nitems)))
            mean = summed[:-1].reshape(flat.shape)
            total, nitems = to_dev(mean, torch.float64) if torch.is_tensor(total) else mean, float(summed[-1])
        return total / nitems

    def _save_summary(self, name, out):
        """summary_<name>.npy, written by rank 0; every rank returns `out` behind the barrier."""
        if self._rank() == 0:
            np.save(os.path.join(self.mode_data_dir, f'summary_{name}.npy'), out)
        self._barrier()
        return out

    def _sorted_items(self, per_item):
        return [per_item[key] for key in sorted(per_item)]

    def compute_turbine_encounters(self):
        """Per turbine, the share of the simulated tracks that came within turbine_encounter_radius of it: the mean over
        all (case, realisation) items of tracks_per_turbine / track_count, f64 (nturb,) in the order of
        `turbines.get_locations()`; case-sharded runs take the mean over every rank's items.  Writes
        summary_turbine_encounters.npy.  ValueError when simulate_tracks computed no encounters."""
        if not self.turbine_encounters:
            raise ValueError('no turbine encounters were computed: run simulate_tracks() with turbine_encounter_radius > 0 '
                             'and turbines')
        return self._save_summary('turbine_encounters', self._item_mean(
            enc['tracks_per_turbine'] / float(self.track_count) for enc in self._sorted_items(self.turbine_encounters)))

    def compute_turbine_rotor_encounters(self):
        """Per turbine, the share of the simulated tracks that passed through its own rotor cylinder and the points they
        spent inside it per simulated track (rotor_geometry = 'turbine'): f64 (nturb, 2), the mean over all
        (case, realisation) items of [tracks_per_turbine, points_per_turbine] / track_count, in the order of
        `turbines.get_locations()`; case-sharded runs take the mean over every rank's items.  Writes
        summary_turbine_rotor_encounters.npy.  ValueError when simulate_tracks computed none."""
        if not self.turbine_rotor_encounters:
            raise ValueError("no rotor encounters were computed: run simulate_tracks() with flight_height=True, "
                             "rotor_geometry='turbine' and turbines")
        mean = self._item_mean(np.stack([enc['tracks_per_turbine'] / float(self.track_count),
                                         enc['points_per_turbine'] / float(self.track_count)])
                               for enc in self._sorted_items(self.turbine_rotor_encounters))
        return self._save_summary('turbine_rotor_encounters', np.ascontiguousarray(mean.T))

    def compute_turbine_rotor_transits(self):
        """Per turbine, the share of the simulated tracks that went through its rotor disk and the transits per simulated
        track, with and against the wind (rotor_transits = True; DESIGN.md K18, limit 17: flights through the disk, not
        collisions): f64 (nturb, 3), the mean over all (case, realisation) items of [tracks, with the wind, against the
        wind] / track_count, in the order of `turbines.get_locations()`; case-sharded runs take the mean over every
        rank's items.  Writes summary_turbine_rotor_transits.npy.  ValueError when simulate_tracks computed none."""
        if not self.turbine_rotor_transits:
            raise ValueError("no rotor transits were computed: run simulate_tracks() with rotor_transits=True "
                             "(flight_height=True, rotor_geometry='turbine' and turbines with t_hh and t_rd)")
        return self._save_summary('turbine_rotor_transits', self._item_mean(
            three / float(self.track_count) for three in self._sorted_items(self.turbine_rotor_transits)))

    def compute_turbine_collision_risk(self):
        """Per turbine, the expected collisions per simulated track (collision_risk = True; DESIGN.md K19, limit 18: Band's
        single-transit probability, recalled and not verified, summed over the transits): f64 (nturb, 3) [with the wind,
        against the wind, in total], the mean over all (case, realisation) items of the raw sums x 2^-32 x
        (1 - collision_avoidance) / track_count, in the order of `turbines.get_locations()`; case-sharded runs take the mean
        over every rank's items.  Writes summary_turbine_collision_risk.npy.  ValueError when simulate_tracks computed none."""
        if not self.turbine_collision_risk:
            raise ValueError("no collision risk was computed: run simulate_tracks() with collision_risk=True "
                             "(flight_height=True, rotor_geometry='turbine' and turbines with t_hh and t_rd)")
        scale = (1. - float(self.collision_avoidance)) / float(self.track_count)
        two = self._item_mean(risk.astype(np.float64) * 2. ** -32 * scale
                              for risk in self._sorted_items(self.turbine_collision_risk))
        return self._save_summary('turbine_collision_risk',
                                  np.ascontiguousarray(np.concatenate([two, two.sum(1, keepdims=True)], 1)))

    def compute_site_collision_risk_map(self):
        """For every cell, the expected collisions per simulated track of a turbine of the candidate class standing on it
        (site_collision_risk = True; DESIGN.md K20, limit 19): f64 (rows, cols), the mean over all (case, realisation) items
        of the raw sums of both directions x 2^-32 x (1 - collision_avoidance) / track_count; case-sharded runs take the mean
        over every rank's items.  Writes summary_site_collision_risk.npy.  ValueError when simulate_tracks computed none."""
        if not self.site_collision_risk_sums:
            raise ValueError('no site collision risk was computed: run simulate_tracks() with site_collision_risk=True '
                             '(flight_height=True)')
        scale = (1. - float(self.collision_avoidance)) / float(self.track_count)
        return self._save_summary('site_collision_risk', self._item_mean(
            risk.astype(np.float64).sum(2) * 2. ** -32 * scale for risk in self._sorted_items(self.site_collision_risk_sums)))

    def compute_turbine_rotor_time(self):
        """Per turbine, the seconds spent inside its own rotor cylinder per simulated track (rotor_exposure_time = True;
        DESIGN.md K15 timed): f64 (nturb,), the mean over all (case, realisation) items of time_per_turbine / 1e6 /
        track_count, in the order of `turbines.get_locations()`; case-sharded runs take the mean over every rank's items.
        Writes summary_turbine_rotor_time.npy.  ValueError when simulate_tracks computed none."""
        items = [enc for enc in self._sorted_items(self.turbine_rotor_encounters) if 'time_per_turbine' in enc]
        if not items:
            raise ValueError('no rotor exposure time was computed: run simulate_tracks() with rotor_exposure_time=True '
                             "(flight_height=True, rotor_geometry='turbine', flight_time=True and turbines)")
        return self._save_summary('turbine_rotor_time', self._item_mean(
            enc['time_per_turbine'] / 1e6 / float(self.track_count) for enc in items))

    def _share_of_tracks(self, counts):
        """uint32 counts (numpy int32) on the device as f64 / track_count: one item of the occupancy and passage means."""
        return (to_dev(counts, torch.int32).to(torch.int64) & 0xFFFFFFFF).to(torch.float64) / float(self.track_count)

    def compute_occupancy_map(self, radius: float = 0.):
        """Each cell's share of the simulated tracks that passed through it, in [0, 1]: the f32 mean over all kept
        (case, realisation) items of track_occupancy_counts / track_count (the per-cell analogue of
        compute_turbine_encounters); case-sharded runs take the mean over every rank's items.  radius > 0 (metres)
        applies the disk mean of the presence map (presence.smooth_presence_counts with
        presence.presence_kernel_radius) to each item's counts first: that is the disk MEAN OF THE PER-CELL SHARES, not
        the share of tracks that came within the radius of the cell (a track that crosses a disk touches several of its
        cells and enters the mean once for each).  Writes summary_occupancy.npy.  ValueError when simulate_tracks
        computed no occupancy."""
        if not self.track_occupancy_counts:
            raise ValueError('no track occupancy was computed: run simulate_tracks() with track_occupancy=True')
        share = self._share_of_tracks
        if float(radius) > 0.:
            krad = presence.presence_kernel_radius(float(radius), self.resolution, self.gridsize)
            share = lambda counts: presence.smooth_presence_counts(to_dev(counts, torch.int32), krad).to(torch.float64) / \
                float(self.track_count)
        mean = self._item_mean(share(counts) for counts in self._sorted_items(self.track_occupancy_counts))
        return self._save_summary('occupancy', mean.to(torch.float32).cpu().numpy())

    def compute_passage_map(self):
        """Each cell's share of the simulated tracks that came within track_passage_radius of it, in [0, 1]: the f32 mean
        over all kept (case, realisation) items of track_passage_counts / track_count; case-sharded runs take the mean
        over every rank's items.  Writes summary_passage.npy.  ValueError when simulate_tracks computed no passage."""
        if not self.track_passage_counts:
            raise ValueError('no track passage was computed: run simulate_tracks() with track_passage_radius > 0')
        mean = self._item_mean(self._share_of_tracks(counts) for counts in self._sorted_items(self.track_passage_counts))
        return self._save_summary('passage', mean.to(torch.float32).cpu().numpy())

    @staticmethod
    def _presence_device():
        return torch.device('cuda', torch.cuda.current_device())

    # ---------------------------------------------------------- multi-GPU
    # (host tests replace these four on an instance to stand in for the ranks of a group)
    _rank = staticmethod(distributed.rank)
    _world = staticmethod(distributed.world_size)
    _barrier = staticmethod(distributed.barrier)
    _allreduce_sum = staticmethod(distributed.all_reduce_sum)

    def _shards_tracks(self):
        """Fewer wind cases than ranks (uniform / snapshot mode: one case): the tracks of
        each case are sharded over the ranks instead of the cases (BASELINE configs[2])."""
        return self._world() > 1 and len(self.case_ids) < self._world()

    def my_case_ids(self):
        """Cases this rank simulates: with a torch.distributed process group (one process
        per GPU) the wind cases are sharded contiguously over the ranks and
        compute_presence_map sums the per-case maps over the ranks; with fewer cases than
        ranks every rank takes every case and a share of its tracks (simulate_tracks)."""
        if self._shards_tracks():
            return list(self.case_ids)
        return distributed.shard_cases(self.case_ids)

    def _cases_written_here(self):
        """Cases whose rasters (orograph, thermals) this rank computes and saves: its own
        cases, or -- track-sharded -- all of them on rank 0 (the other ranks read the
        files after the barrier that ends the constructor)."""
        if self._shards_tracks():
            return list(self.case_ids) if self._rank() == 0 else []
        return self.my_case_ids()

    def plot_presence_map(self, plot_turbs=True, radius: float = 1000., show=False,
                          minval=0.1, plot_all: bool = False) -> None:
        """simulator.py:508-550 up to and including summary_presence.npy; the
        matplotlib figures are out of scope."""
        print('Plotting presence density map..')
        self.compute_presence_map(radius)

    # ------------------------------------------------ out-of-scope plotting
    def _no_plot(self, name):
        print(f'{name}: plotting is outside the hot-path scope of this build (no-op)')

    def plot_terrain_features(self, *a, **k): self._no_plot('plot_terrain_features')
    def plot_terrain_elevation(self, *a, **k): self._no_plot('plot_terrain_elevation')
    def plot_terrain_slope(self, *a, **k): self._no_plot('plot_terrain_slope')
    def plot_terrain_aspect(self, *a, **k): self._no_plot('plot_terrain_aspect')
    def plot_wtk_layers(self, *a, **k): self._no_plot('plot_wtk_layers')
    def plot_updrafts(self, *a, **k): self._no_plot('plot_updrafts')
    def plot_directional_potentials(self, *a, **k): self._no_plot('plot_directional_potentials')
    def plot_simulated_tracks(self, *a, **k): self._no_plot('plot_simulated_tracks')

    def plot_windplant_presence_map(self, pname, radius: float = 100., plot_turbs=True, show=False, minval=0.05,
                                    pad: float = 2000., **k) -> None:
        """simulator.py:557-592 up to the summary map and its crop (presence_<pname>.npy); the figure is out of scope.
        Without injected turbines there is nothing to crop to: the no-op line of the other plotting methods."""
        if getattr(self, 'turbines', None) is None:
            self._no_plot('plot_windplant_presence_map')
            return
        print('Plotting presence density map..')
        self.compute_windplant_presence_map(pname, radius=radius, pad=pad)

    def plot_updraft_threshold_function(self, *a, **k): self._no_plot('plot_updraft_threshold_function')
