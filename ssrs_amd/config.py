"""`Config` -- the user-facing parameter set, field-for-field compatible with the
reference dataclass (/root/reference/ssrs/config.py:9-67: 34 fields + the
`turbine_mrkr_styles` class attribute), so existing scripts that build a
`Config(...)` or call `dataclasses.replace(cfg, ...)` keep working.

The annotations deliberately repeat the reference's (including its oddities,
e.g. `resolution: int = 100.`), because dataclass field order/defaults ARE the
API.  Fields added by this build come last and default to reference behaviour.
"""
import os
from dataclasses import dataclass, fields
from typing import Optional, Tuple

_SECTIONS = (
    ('General settings', ('run_name', 'out_dir', 'max_cores', 'sim_seed', 'sim_mode',
                          'print_verbose')),
    ('Terrain settings', ('southwest_lonlat', 'projected_crs', 'region_width_km',
                          'resolution')),
    ('Uniform mode', ('uniform_winddirn', 'uniform_windspeed')),
    ('Snapshot mode', ('snapshot_datetime',)),
    ('Seasonal mode', ('seasonal_start', 'seasonal_end', 'seasonal_timeofday',
                       'seasonal_count')),
    ('WindToolKit settings', ('wtk_source', 'wtk_orographic_height', 'wtk_thermal_height',
                              'wtk_interp_type')),
    ('Updraft computation', ('thermals_realization_count', 'updraft_threshold',
                             'orographic_smoothing', 'orographic_smooth_sigma',
                             'movement_model', 'orographic_sx_sector', 'orographic_sx_step',
                             'orographic_model', 'orographic_sx_dmax',
                             'orographic_height', 'orographic_coeffs')),
    ('Simulating tracks', ('track_direction', 'track_count', 'track_start_region',
                           'track_start_type', 'track_stochastic_nu',
                           'track_dirn_restrict')),
    ('Plotting and wind turbines', ('turbine_minimum_hubheight', 'turbine_mrkr_size',
                                    'fig_height', 'fig_dpi')),
    ('MI355X build', ('save_tracks', 'stepper_path', 'steps_per_launch', 'max_tracks_file_gb', 'track_occupancy',
                      'flight_height', 'flight_height_start', 'flight_height_floor', 'flight_height_ceiling',
                      'flight_airspeed', 'flight_sink_rate', 'rotor_zone', 'rotor_geometry', 'rotor_clearance',
                      'flight_time', 'flight_min_groundspeed', 'rotor_exposure_time', 'track_passage_radius', 'rotor_transits', 'rotor_yaw',
                      'collision_risk', 'bird_length', 'bird_wingspan', 'bird_flight', 'collision_avoidance', 'collision_model_3d',
                      'rotor_blades', 'rotor_rpm', 'rotor_max_chord', 'rotor_pitch', 'rotor_chord_profile',
                      'site_collision_risk', 'site_hub_height', 'site_rotor_diameter', 'hist_safe_tracks', 'thermal_model', 'thermal_allen_zi', 'thermal_allen_wstar', 'thermal_allen_sink',
                      'turbine_encounter_radius')),
)


@dataclass
class Config:
    """Configuration parameters for SSRS simulation """

    # -- general
    run_name: str = 'default'
    out_dir: str = os.path.join(os.path.abspath(os.path.curdir), 'output')
    max_cores: int = 8          # kept for compatibility; tracks run on the GPU
    sim_seed: int = -1          # < 0: unseeded (a fresh seed is drawn per run)
    sim_mode: str = 'uniform'   # uniform | snapshot | seasonal
    print_verbose: bool = False

    # -- terrain
    southwest_lonlat: Tuple[float, float] = (-106.21, 42.78)
    projected_crs: str = 'ESRI:102008'
    region_width_km: Tuple[float, float] = (60., 50.)
    resolution: int = 100.

    # -- uniform mode
    uniform_winddirn: float = 270.   # degrees clockwise from north (270 = westerly)
    uniform_windspeed: float = 10.   # m/s

    # -- snapshot mode
    snapshot_datetime: Tuple[int, int, int, int] = (2010, 6, 17, 13)

    # -- seasonal mode
    seasonal_start: Tuple[int, int] = (3, 20)
    seasonal_end: Tuple[int, int] = (5, 15)
    seasonal_timeofday: str = 'daytime'
    seasonal_count: int = 8

    # -- WIND Toolkit
    wtk_source: str = 'AWS'
    wtk_orographic_height: int = 100
    wtk_thermal_height: int = 100
    wtk_interp_type: str = 'linear'

    # -- updrafts
    thermals_realization_count: bool = 0
    updraft_threshold: float = 0.75
    movement_model: str = 'fluidflow'   # fluidflow | drw

    # -- tracks
    track_direction: float = 0
    track_count: str = 1000
    track_start_region: Tuple[float, float, float, float] = (5, 55, 1, 2)
    track_start_type: str = 'random'    # structured | random
    track_stochastic_nu: float = 1.
    track_dirn_restrict: int = 1

    # -- turbines / plotting (carried for compatibility)
    turbine_minimum_hubheight: float = 50.
    turbine_mrkr_styles = ('1k', '2k', '3k', '4k', '+k', 'xk', '*k', '.k', 'ok')
    turbine_mrkr_size: float = 3.
    fig_height: float = 6.
    fig_dpi: int = 200

    # -- added by the MI355X build (defaults keep the reference's behaviour)
    save_tracks: bool = True            # write <id>_tracks.pkl like the reference
    stepper_path: str = 'auto'          # auto | table | direct
    steps_per_launch: int = 0           # 0 = library default
    max_tracks_file_gb: float = 64.     # refuse a <id>_tracks.pkl larger than this (tracks that wander to
    #                                     max_moves: 1 TB per 100k tracks on a solved 10 m field)
    track_occupancy: bool = False       # True: simulate_tracks also counts, per cell, the DISTINCT tracks that passed through it
    #                                     (a track that loiters in a cell is many visits and one track), from the trajectories
    #                                     on the device (produced even with save_tracks=False):
    #                                     <id>_occupancy.npy, Simulator.compute_occupancy_map().  It stands here, not last,
    #                                     because tests pin every slot after the reference's fields but this one
    flight_height: bool = False         # True: simulate_tracks also integrates a height above ground along every track -- THIS
    #                                     BUILD'S OWN model, the reference has none (limit 13): each move adds
    #                                     (updraft - sink) * resolution / airspeed (times sqrt(2) on a diagonal) less the terrain's
    #                                     rise, clamped to [floor, ceiling] -- and counts the points inside rotor_zone, from the
    #                                     trajectories on the device (produced even with save_tracks=False):
    #                                     <id>_rotor_presence.npy, <id>_flight_heights.npy, with turbine_encounter_radius > 0 also
    #                                     <id>_rotor_turbine_encounters.npy; Simulator.compute_rotor_presence_map()
    flight_height_start: float = 100.   # metres above ground at a track's first point.  The heights and the band below are
    #                                     PLACEHOLDERS: set them for the species and the turbines at hand
    flight_height_floor: float = 10.    # metres: the height never falls below it
    flight_height_ceiling: float = 1000.  # metres: nor rises above it
    flight_airspeed: float = 15.        # m/s, still air: a move of one cell takes resolution / airspeed seconds
    flight_sink_rate: float = -1.       # m/s lost in still air; < 0 = updraft_threshold
    rotor_zone: Tuple[float, float] = (30., 150.)   # metres above ground, both ends inclusive
    rotor_geometry: str = 'band'        # band | turbine.  'band': rotor_zone, one height band above ground for all turbines.
    #                                     'turbine' (needs flight_height=True and Simulator(turbines=...) with t_hh and t_rd):
    #                                     simulate_tracks also tests every track point against each turbine's OWN cylinder --
    #                                     within t_rd / 2 of it in the plane, and between t_hh -+ t_rd / 2 above the ground the
    #                                     TURBINE stands on, in absolute heights -- and counts per turbine the tracks through it
    #                                     and the points inside it (the exposure), on the device (limit 14):
    #                                     <id>_turbine_rotor_encounters.npy, Simulator.compute_turbine_rotor_encounters().  The
    #                                     two fields stand here, after rotor_zone, because tests pin the slots further down
    rotor_clearance: float = 0.         # metres added to the rotor radius of 'turbine', in the plane and in height
    flight_time: bool = False           # True: simulate_tracks also gives every move a duration -- THIS BUILD'S OWN model, the
    #                                     reference has none (limit 15): the move's length over the ground speed
    #                                     the bird keeps along it at flight_airspeed in the wind of the cell it leaves (the case's
    #                                     wind at wtk_orographic_height), in integer microseconds -- and sums them per cell and per
    #                                     track, from the trajectories on the device (produced even with save_tracks=False):
    #                                     <id>_residence_time.npy, <id>_flight_times.npy, with flight_height=True also
    #                                     <id>_rotor_residence_time.npy (the time in rotor_zone);
    #                                     Simulator.compute_residence_time_map().  The two fields stand here, after
    #                                     rotor_clearance, because tests pin the slots on either side
    flight_min_groundspeed: float = 1.  # m/s: the ground speed along a move never falls below it (a headwind, or a cross wind
    #                                     the bird cannot hold its heading against); 0.001 .. flight_airspeed
    rotor_exposure_time: bool = False   # True (needs flight_height=True, rotor_geometry='turbine', flight_time=True and turbines
    #                                     with t_hh and t_rd): simulate_tracks also sums, per turbine, the durations of the moves
    #                                     that leave a point inside its cylinder -- the exposure in microseconds instead of
    #                                     points, on the device (DESIGN.md K15 timed, limits 14 and 15; the heights and the
    #                                     durations underneath are this build's placeholder models):
    #                                     <id>_turbine_rotor_time.npy, Simulator.compute_turbine_rotor_time().  It stands here,
    #                                     after flight_min_groundspeed, because tests pin every other slot
    track_passage_radius: float = 0.    # metres; 0 = off.  > 0: simulate_tracks also counts, per cell, the DISTINCT tracks that
    #                                     came within this distance of the cell's centre -- turbine_encounter_radius for a site
    #                                     that is not in the turbine table yet -- from the trajectories on the device (produced
    #                                     even with save_tracks=False; DESIGN.md K17, limit 16; at most 255 cells):
    #                                     <id>_passage.npy, Simulator.compute_passage_map().  The file name does not carry the
    #                                     radius: one radius per out_dir/run_name.  It stands here, not last, because tests pin
    #                                     the last two fields and the last entry of _SECTIONS
    rotor_transits: bool = False        # True (needs flight_height=True, rotor_geometry='turbine' and turbines with t_hh and
    #                                     t_rd; flight_time is not needed): simulate_tracks also counts, per turbine and direction,
    #                                     the TRANSITS -- unit moves whose straight segment goes through the rotor DISK, a circle
    #                                     of radius t_rd / 2 + rotor_clearance around the hub that stands across the wind -- on the
    #                                     device (limit 17: a count of flights through the disk, NOT a collision
    #                                     probability; K14's placeholder heights underneath):
    #                                     <id>_turbine_rotor_transits.npy, Simulator.compute_turbine_rotor_transits()
    rotor_yaw: float = -1.              # degrees clockwise from north the rotors face, for all turbines and cases; < 0: every
    #                                     rotor faces the case's wind at the cell it stands on.  The two fields stand here, behind
    #                                     track_passage_radius, because tests pin most other slots
    collision_risk: bool = False        # True (needs what rotor_transits needs: flight_height=True, rotor_geometry='turbine' and
    #                                     turbines with t_hh and t_rd; rotor_transits itself is not needed): simulate_tracks also
    #                                     weights every transit with Band's (2012) single-transit collision probability at the
    #                                     place in the disk it goes through and sums them exactly, per turbine, direction and
    #                                     track, on the device in the transits' own pass (limit 18: the formula
    #                                     and the chord profile are RECALLED, not verified):
    #                                     <id>_turbine_collision_risk.npy, <id>_track_collision_risk.npy,
    #                                     Simulator.compute_turbine_collision_risk().  The bird and rotor numbers below are
    #                                     PLACEHOLDERS, like rotor_zone: set them for the species and the fleet at hand.  The
    #                                     eleven fields stand here, behind rotor_yaw, because tests pin most other slots
    bird_length: float = 0.85           # metres, bill to tail
    bird_wingspan: float = 2.1          # metres
    bird_flight: str = 'gliding'        # gliding | flapping (Band's F = 2 / pi or 1)
    collision_avoidance: float = 0.     # in [0, 1]: the share of collisions avoided; a scalar factor applied on the host only
    #                                     (compute_turbine_collision_risk), the files hold the raw sums
    collision_model_3d: bool = True     # Band's K: True = the 3-D model (chord and pitch count), False = the 1-D model
    rotor_blades: int = 3               # for turbines without a column t_blades
    rotor_rpm: float = 12.              # revolutions per minute, for turbines without a column t_rpm
    rotor_max_chord: float = 4.         # metres, the blade's greatest chord, for turbines without a column t_chord
    rotor_pitch: float = 15.            # degrees, the blade's pitch, for turbines without a column t_pitch
    rotor_chord_profile: Tuple = (0.73, 0.79, 0.88, 0.96, 1.00, 0.98, 0.92, 0.85, 0.80, 0.75, 0.70, 0.64, 0.58, 0.52, 0.47,
                                  0.41, 0.37, 0.30, 0.24, 0.00)   # chord / rotor_max_chord at r / R = 0.05, 0.10, ..., 1.00,
    #                                     linear between the nodes and constant below 0.05: Band's generic blade, recalled from
    #                                     the published spreadsheet and NOT verified against it: correct it here, no rebuild
    #                                     is needed
    site_collision_risk: bool = False   # True (needs flight_height=True; no turbines and no rotor_geometry): simulate_tracks also
    #                                     computes, for EVERY cell of the raster, the collision risk of one candidate turbine
    #                                     class standing on that cell -- collision_risk turned inside out, for siting -- on the
    #                                     device (limit 19): the transits through a disk of radius
    #                                     site_rotor_diameter / 2 + rotor_clearance around a hub site_hub_height above the
    #                                     cell's ground, each weighted with Band's probability as collision_risk does.  It
    #                                     reads rotor_clearance, rotor_yaw, rotor_blades / rpm / max_chord / pitch /
    #                                     chord_profile, bird_*, collision_model_3d, flight_airspeed and collision_avoidance
    #                                     exactly as collision_risk does.  Writes <id>_site_collision_risk.npy,
    #                                     <id>_site_transits.npy, Simulator.compute_site_collision_risk_map().  The three
    #                                     fields stand here, behind rotor_chord_profile, because tests pin most other slots
    site_hub_height: float = 90.        # metres above the ground of the cell.  This and the diameter are PLACEHOLDERS, like
    #                                     rotor_zone: set them for the turbine class at hand
    site_rotor_diameter: float = 120.   # metres; (site_rotor_diameter / 2 + rotor_clearance) / resolution is at most 62 cells
    thermal_allen_zi: float = 0.        # thermal_model = 'allen': boundary-layer height zi in metres.  0 (snapshot / seasonal
    #                                     only) = the mean of the case's own blheight layer, clipped below at 100 m
    thermal_allen_wstar: float = 0.     # thermal_model = 'allen': convective velocity scale w* in m/s.  0 (snapshot / seasonal
    #                                     only) = the mean Deardorff velocity of the case's own WTK layers
    thermal_allen_sink: bool = False    # thermal_model = 'allen': the environment sink between the updrafts (Allen's sflag; off
    #                                     in the reference's own call)
    turbine_encounter_radius: float = 0.  # metres; 0 = off.  > 0 (needs Simulator(turbines=...)): simulate_tracks also finds, per
    #                                     turbine, the tracks that came within this distance of it and after how many moves, from
    #                                     the trajectories on the device (produced even with save_tracks=False):
    #                                     <id>_turbine_encounters.npy, Simulator.compute_turbine_encounters().  Listed last in
    #                                     _SECTIONS; as a field it stands here because tests pin the last two
    orographic_model: str = 'original'  # original | improved.  'original': the reference's wspeed sin(slope) cos(aspect - wdirn).
    #                                     'improved': that value sheltered by the terrain upwind (Winstral's Sx within
    #                                     orographic_sx_dmax metres) and scaled to orographic_height metres above ground:
    #                                     w0 max(0, 1 + g tan Sx) / ((a h^2 + b h + c) d^(e - cos(slope)) + f), DESIGN.md K9;
    #                                     also writes <case>_sx.npy, and the ids carry -sx<dmax>h<height>[a<sector>s<step>]
    orographic_sx_dmax: float = 500.    # metres upwind searched for sheltering terrain (>= resolution)
    orographic_height: float = 80.      # h, metres above ground
    orographic_coeffs: Tuple = (4e-5, 2.8e-3, 0.8, 0.35, 0.095, -0.09, 1.0)   # (a, b, c, d, e, f, g), recalled from the
    #                                     published improved model and NOT verified against it (the sign of g least of all):
    #                                     correct them here, no rebuild is needed
    orographic_sx_sector: float = 0.    # 'improved' only: half-width in degrees of the upwind sector Sx is averaged over
    #                                     (Winstral: 15 = a 30 degree sector).  0 = the single ray towards the wind.  > 0: the mean
    #                                     of Sx over the azimuths wdirn + j orographic_sx_step within the sector, at most 61 of
    #                                     them, in one device call; <case>_sx.npy holds the mean and the ids carry a<sector>s<step>
    orographic_sx_step: float = 5.      # degrees between the rays of that sector (> 0)
    orographic_smoothing: str = 'none'  # none | gaussian.  'improved' only.  'gaussian': the adjusted updraft is blurred by a
    #                                     Gaussian (scipy's gaussian_filter, mode='reflect', nodata entering as 0) before its clamp
    #                                     and threshold, in two device passes; <case>_orograph.npy holds the
    #                                     smoothed field and the ids carry g<sigma in metres>
    orographic_smooth_sigma: float = 0.  # metres; 0 = the model's own width min(0.8 orographic_height + 16, 300) (recalled,
    #                                     NOT verified).  Its radius int(4 sigma / resolution + 0.5) may be at most 512 cells
    hist_safe_tracks: int = 250_000     # tracks per sub-batch of a case: (i) histograms of several sub-batches are added up in 64
    #                                     bits; a sub-batch of more than 100 000 tracks is counted in 64 bits inside the library (a trap
    #                                     cell of the solved 10 m field takes 1.7e4 visits per track: 2^32 from ~245 000 tracks on;
    #                                     ssrs_tracks_simulate_h64), and a smaller one whose uint32 counts wrap all the same -- or one
    #                                     with trajectories, which stay on the uint32 raster -- is stepped again as two halves;
    #                                     (ii) ~42 % of such a batch ends up roaming, and the roaming stepper holds ONE block per
    #                                     CU: 250 000 tracks = ~105 000 roaming at first, one round of 512-lane blocks, later
    #                                     ~78 000 in 256-lane blocks: 2.0 s per pass = 1.27e5 tracks/s against 1.0e5 for 140 000
    #                                     (rounds 3-4) and 1.15e5 for 300 000 (a second round of blocks; profiles/r04_roam_fill.txt)
    thermal_model: str = 'random'       # random | wtk | allen.  'random': the reference's compute_thermals, one field of smoothed random
    #                                     blobs per realisation.  'wtk' (snapshot / seasonal, thermals_realization_count = 1): the
    #                                     Deardorff-velocity updraft at wtk_thermal_height from the case's own WTK layers
    #                                     (pressure, temperature, blheight, surfheatflux in every wind entry).  'allen': Allen's
    #                                     (2006) field of discrete updrafts at wtk_thermal_height, one stochastic field per
    #                                     realisation, their number and strength from zi and w* (thermal_allen_*);
    #                                     the ids carry -allen

    def __str__(self):
        known = {f.name for f in fields(self)}
        lines = [self.__doc__, '']
        for title, names in _SECTIONS:
            lines.append(f':::: {title}')
            lines.extend(f'{n} = {getattr(self, n)}' for n in names if n in known)
            lines.append('')
        return '\n'.join(lines)
