"""ctypes binding of libssrs_hip.so (include/ssrs_hip.h).

There is NO CPU fallback: if the library is missing or a call fails, the
functions raise.  The library is built in-tree by ssrs_amd/csrc/build.py
(hipcc, gfx950) and travels with the source tree.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SSRS_HIP_LIB') or os.path.join(_HERE, 'libssrs_hip.so')   # (override: timing probes only)

SSRS_F32, SSRS_F64 = 0, 1
SSRS_OK, SSRS_ERR_INVALID, SSRS_ERR_HIP, SSRS_ERR_START = 0, -1, -2, -3
SSRS_TRACKS_PROFILE = 1
SSRS_TRACKS_EXACT_ONLY = 2
SSRS_TRACKS_NO_SCHEDULE = 4
SSRS_TRACKS_NO_BINNING = 8
SSRS_TRACKS_RING_TABLE = 16
SSRS_TRACKS_SCATTERED = 32
SSRS_TRACKS_NO_SCATTERED = 64
SSRS_TRACKS_THR_TABLE = 128
SSRS_SOLVE_NO_AMG = 1
SSRS_TURBINE_BIN, SSRS_TURBINE_MAX = 32, 8192
SSRS_ROTOR_TIMED_LDS_TURBINES = 5120
SSRS_OCCUPANCY_MAX_PLANES = 8
SSRS_ALTITUDE_TILE = 4096
SSRS_RAY_AXES = {'row_north': 0, 'row_east': 1}                  # SSRS_RAY_ROW_NORTH / _ROW_EAST
SSRS_SHELTER_PATH = {'auto': 0, 'lds': 1, 'global': 2}           # SSRS_SHELTER_AUTO / _LDS / _GLOBAL
SSRS_SMOOTH_PATH = {'auto': 0, 'lds': 1, 'global': 2}            # SSRS_SMOOTH_AUTO / _LDS / _GLOBAL
SSRS_ALLEN_PATH = {'auto': 0, 'lds': 1, 'global': 2}             # SSRS_ALLEN_AUTO / _LDS / _GLOBAL
SSRS_ALLEN_MAX_UPDRAFTS, SSRS_ALLEN_TABLE_COLS = 1 << 22, 6
SSRS_INTERP = {'nearest': 0, 'linear': 1, 'cubic': 2}          # SSRS_INTERP_NEAREST / _LINEAR / _CUBIC

EXPORTS = (
    'ssrs_version', 'ssrs_build_flags', 'ssrs_last_error', 'ssrs_device_info', 'ssrs_slope_aspect',
    'ssrs_orographic_updraft', 'ssrs_threshold_updraft', 'ssrs_updraft_from_dem',
    'ssrs_lattice_workspace_bytes', 'ssrs_updraft_from_dem_lattice',
    'ssrs_wind_from_lattice', 'ssrs_wind_triangles_workspace_bytes', 'ssrs_wind_from_triangles',
    'ssrs_wind_nearest_workspace_bytes', 'ssrs_wind_nearest_index', 'ssrs_wind_from_nearest',
    'ssrs_wind_cubic_workspace_bytes', 'ssrs_wind_from_triangles_cubic', 'ssrs_thermal_seeds', 'ssrs_blur_workspace_bytes',
    'ssrs_gaussian_blur', 'ssrs_thermal_fields', 'ssrs_potential_temperature', 'ssrs_deardorff_velocity',
    'ssrs_thermal_updraft', 'ssrs_scalar_interp_workspace_bytes', 'ssrs_scalar_from_samples', 'ssrs_wtk_thermal_fields',
    'ssrs_track_params_init', 'ssrs_transition_table_build',
    'ssrs_transition_ring_bytes', 'ssrs_transition_ring_build',
    'ssrs_transition_thr_bytes', 'ssrs_transition_thr_build',
    'ssrs_tracks_workspace_bytes', 'ssrs_tracks_workspace_bytes_ex', 'ssrs_tracks_simulate', 'ssrs_uniform_selftest',
    'ssrs_traj_recorder_create', 'ssrs_traj_recorder_destroy', 'ssrs_traj_recorder_complete',
    'ssrs_traj_recorder_used', 'ssrs_tracks_simulate_rec', 'ssrs_tracks_gather', 'ssrs_tracks_simulate_h64',
    'ssrs_hist_reduce', 'ssrs_presence_count', 'ssrs_presence_workspace_bytes', 'ssrs_presence_smooth',
    'ssrs_presence_smooth_u64',
    'ssrs_presence_normalise_add', 'ssrs_presence_normalise_f32',
    'ssrs_potential_workspace_bytes', 'ssrs_potential_solve',
    'ssrs_turbine_encounters', 'ssrs_turbine_encounter_counts', 'ssrs_rotor_encounters', 'ssrs_rotor_encounters_timed',
    'ssrs_shelter_sx', 'ssrs_updraft_sheltered', 'ssrs_shelter_sx_sector', 'ssrs_updraft_sheltered_sector',
    'ssrs_smooth_workspace_bytes', 'ssrs_smooth_reflect',
    'ssrs_projection_init_albers', 'ssrs_warp_lonlat_raster',
    'ssrs_allen_workspace_bytes', 'ssrs_allen_thermal_field',
    'ssrs_track_occupancy_workspace_bytes', 'ssrs_track_occupancy',
    'ssrs_altitude_cellinfo', 'ssrs_track_altitude_workspace_bytes', 'ssrs_track_altitude',
    'ssrs_flight_windinfo', 'ssrs_track_time',
    'ssrs_roam_pair_word_selftest', 'ssrs_tracks_roam_feed_counts', 'ssrs_roam_tables_selftest',
    'ssrs_tracks_roam_stopped_waves',
)


class SsrsTrackParams(C.Structure):
    _fields_ = [('rows', C.c_int32), ('cols', C.c_int32), ('burnin', C.c_int32),
                ('memory_parameter', C.c_int32), ('max_moves', C.c_int64),
                ('scaling_parameter', C.c_double), ('prior', C.c_double * 9),
                ('steps_per_launch', C.c_int32), ('flags', C.c_int32)]


class SsrsTrackStats(C.Structure):
    _fields_ = [('total_steps', C.c_int64), ('launches', C.c_int32),
                ('kernel_ms', C.c_float), ('wall_ms', C.c_float), ('hist_ms', C.c_float),
                ('window_launches', C.c_int32), ('tile_launches', C.c_int32),
                ('block_window_launches', C.c_int32), ('wander_sorts', C.c_int32),
                ('timed_launches', C.c_int32), ('first_move_ms', C.c_float),
                ('block_window_ms', C.c_float), ('block_window_timed', C.c_int32),
                ('block_window_steps', C.c_int64), ('roam_launches', C.c_int32), ('reserved0', C.c_int32),
                ('roam_wave_pairs', C.c_int64), ('roam_slow_wave_pairs', C.c_int64),
                ('roam_shuffles', C.c_int32), ('roam_wide_launches', C.c_int32)]


class SsrsSolveStats(C.Structure):
    _fields_ = [('iterations', C.c_int32), ('converged', C.c_int32),
                ('residual', C.c_double), ('kernel_ms', C.c_float),
                ('amg_levels', C.c_int32), ('amg_coarsest', C.c_int32),
                ('setup_ms', C.c_float), ('workspace_used', C.c_uint64)]


class SsrsShelterParams(C.Structure):
    _fields_ = [('dmax', C.c_double), ('ray_axes', C.c_int32), ('path', C.c_int32), ('height', C.c_double),
                ('coef', C.c_double * 7)]


class SsrsProjection(C.Structure):
    _fields_ = [(name, C.c_double) for name in ('a', 'e2', 'lat_1', 'lat_2', 'lat_0', 'lon_0', 'x_0', 'y_0',
                                                'n', 'C', 'rho0', 'e')]


# ssrs_allen_thermal_field: xt, yt, wgain, rgain, n, bin_start, bin_items, bin_size_m, nbx, nby, rbar, wtbar, zzi, z_below_zi,
# we, res, rows, cols, path, out, out_type, nearest, table, workspace, workspace_bytes, stream
# ssrs_track_occupancy: traj, traj_offsets, ntracks, rows, cols, planes, counts, cells_per_track, workspace, workspace_bytes, stream
OCCUPANCY_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_size_t, C.c_void_p]

ALLEN_FIELD_ARGTYPES = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_int] + \
    [C.c_double] * 3 + [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                        C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]


class SsrsAltitudeParams(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ('start', 'floor', 'ceil', 'band_lo', 'band_hi')]


# ssrs_altitude_cellinfo: updraft, updraft_type, dem, dem_type, rows, cols, sink, scale, cellinfo, stream
ALTITUDE_CELLINFO_ARGTYPES = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p,
                              C.c_void_p]
# ssrs_track_altitude: traj, traj_offsets, ntracks, cellinfo, rows, cols, params, alt, band_hist, traj_band, in_band, h_min,
# h_max, workspace, workspace_bytes, stream
ALTITUDE_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.POINTER(SsrsAltitudeParams)] + \
    [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p]


class SsrsFlightTimeParams(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ('va', 'gmin', 'res_mm')]


# ssrs_flight_windinfo: wspeed, wdirn, type, rows, cols, ray_axes, windinfo, stream
FLIGHT_WINDINFO_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
# ssrs_track_time: traj, traj_offsets, ntracks, masked, windinfo, uniform_wr, uniform_wc, rows, cols, params, time_hist,
# band_time_hist, per_track, dt, stream
TRACK_TIME_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                       C.POINTER(SsrsFlightTimeParams)] + [C.c_void_p] * 5


# ssrs_rotor_encounters: traj, traj_offsets, ntracks, alt, cellinfo, rows, cols, turbines, reach, zband, nturb, bin_start,
# bin_items, hits, first_step, points_per_turbine, stream
ROTOR_ENCOUNTERS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + \
    [C.c_int] + [C.c_void_p] * 6
# ssrs_rotor_encounters_timed: traj, traj_offsets, ntracks, alt, dt, cellinfo, rows, cols, turbines, reach, zband, nturb,
# bin_start, bin_items, hits, first_step, points_per_turbine, time_per_turbine, stream
ROTOR_ENCOUNTERS_TIMED_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + \
    [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 7


class SsrsError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f'libssrs_hip error {code}: {message}')
        self.code = code


_lib = None


def lib():
    """Load libssrs_hip.so once; raise loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f'{LIB_PATH} is missing: build it with `python ssrs_amd/csrc/build.py` '
                '(hipcc, gfx950). ssrs_amd has no CPU fallback.')
        L = C.CDLL(LIB_PATH)
        L.ssrs_version.restype = C.c_int
        if L.ssrs_build_flags() & 1 and not os.environ.get('SSRS_ALLOW_PROBE_LIB'):
            raise ImportError(f'{LIB_PATH} is a timing-probe build (results are wrong on purpose); '
                              'set SSRS_ALLOW_PROBE_LIB=1 for timing runs only')
        L.ssrs_last_error.restype = C.c_char_p
        L.ssrs_tracks_workspace_bytes.restype = C.c_size_t
        L.ssrs_tracks_workspace_bytes.argtypes = [C.c_int64]
        L.ssrs_lattice_workspace_bytes.restype = C.c_size_t
        L.ssrs_wind_triangles_workspace_bytes.restype = C.c_size_t
        L.ssrs_wind_triangles_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.ssrs_lattice_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.ssrs_wind_nearest_workspace_bytes.restype = C.c_size_t
        L.ssrs_wind_nearest_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.ssrs_wind_nearest_index.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_size_t, C.c_void_p]
        L.ssrs_wind_cubic_workspace_bytes.restype = C.c_size_t
        L.ssrs_wind_cubic_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.ssrs_wind_from_triangles_cubic.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                                                        C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                                        C.c_void_p]
        L.ssrs_tracks_workspace_bytes_ex.restype = C.c_size_t
        L.ssrs_tracks_workspace_bytes_ex.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
        L.ssrs_traj_recorder_create.restype = C.c_void_p
        L.ssrs_traj_recorder_create.argtypes = [C.c_void_p, C.c_size_t]
        L.ssrs_traj_recorder_destroy.restype = None
        L.ssrs_traj_recorder_destroy.argtypes = [C.c_void_p]
        L.ssrs_traj_recorder_complete.argtypes = [C.c_void_p]
        L.ssrs_traj_recorder_used.restype = C.c_size_t
        L.ssrs_traj_recorder_used.argtypes = [C.c_void_p]
        L.ssrs_transition_thr_bytes.restype = C.c_size_t
        L.ssrs_transition_thr_bytes.argtypes = [C.c_int, C.c_int]
        L.ssrs_transition_ring_bytes.restype = C.c_size_t
        L.ssrs_transition_ring_bytes.argtypes = [C.c_int, C.c_int]
        if hasattr(L, 'ssrs_presence_workspace_bytes'):
            L.ssrs_presence_workspace_bytes.restype = C.c_size_t
            L.ssrs_presence_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        if hasattr(L, 'ssrs_blur_workspace_bytes'):
            L.ssrs_blur_workspace_bytes.restype = C.c_size_t
            L.ssrs_blur_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_double]
        L.ssrs_thermal_fields.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_uint64), C.c_int,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ssrs_potential_temperature.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ssrs_deardorff_velocity.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ssrs_thermal_updraft.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_size_t,
                                           C.c_void_p]
        L.ssrs_scalar_interp_workspace_bytes.restype = C.c_size_t
        L.ssrs_scalar_interp_workspace_bytes.argtypes = [C.c_int] * 5
        L.ssrs_scalar_from_samples.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int,
                                                                             C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ssrs_wtk_thermal_fields.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_double,
                                                                            C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                                            C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        if hasattr(L, 'ssrs_potential_workspace_bytes'):
            L.ssrs_potential_workspace_bytes.restype = C.c_size_t
            L.ssrs_potential_workspace_bytes.argtypes = [C.c_int, C.c_int]
        if hasattr(L, 'ssrs_turbine_encounters'):
            L.ssrs_turbine_encounters.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_double,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
            L.ssrs_turbine_encounter_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ssrs_shelter_sx.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ssrs_updraft_sheltered.argtypes = [C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 8 + \
            [C.c_int, C.POINTER(SsrsShelterParams), C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
             C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ssrs_shelter_sx_sector.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                             C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_int, C.c_int, C.c_void_p]
        L.ssrs_updraft_sheltered_sector.argtypes = [C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 8 + \
            [C.c_int, C.POINTER(SsrsShelterParams), C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
             C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ssrs_smooth_workspace_bytes.restype = C.c_size_t
        L.ssrs_smooth_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double]
        L.ssrs_smooth_reflect.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ssrs_projection_init_albers.argtypes = [C.POINTER(SsrsProjection)]
        L.ssrs_warp_lonlat_raster.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5 + \
            [C.POINTER(SsrsProjection)] + [C.c_double] * 3 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_int, C.c_int, C.c_void_p]
        L.ssrs_allen_workspace_bytes.restype = C.c_size_t
        L.ssrs_allen_workspace_bytes.argtypes = [C.c_int]
        L.ssrs_allen_thermal_field.argtypes = ALLEN_FIELD_ARGTYPES
        L.ssrs_track_occupancy_workspace_bytes.restype = C.c_size_t
        L.ssrs_track_occupancy_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.ssrs_track_occupancy.argtypes = OCCUPANCY_ARGTYPES
        L.ssrs_altitude_cellinfo.argtypes = ALTITUDE_CELLINFO_ARGTYPES
        L.ssrs_track_altitude_workspace_bytes.restype = C.c_size_t
        L.ssrs_track_altitude_workspace_bytes.argtypes = [C.c_int64]
        L.ssrs_track_altitude.argtypes = ALTITUDE_ARGTYPES
        L.ssrs_flight_windinfo.argtypes = FLIGHT_WINDINFO_ARGTYPES
        L.ssrs_track_time.argtypes = TRACK_TIME_ARGTYPES
        if hasattr(L, 'ssrs_rotor_encounters'):
            L.ssrs_rotor_encounters.argtypes = ROTOR_ENCOUNTERS_ARGTYPES
        if hasattr(L, 'ssrs_rotor_encounters_timed'):
            L.ssrs_rotor_encounters_timed.argtypes = ROTOR_ENCOUNTERS_TIMED_ARGTYPES
        L.ssrs_roam_pair_word_selftest.argtypes = [C.c_uint64] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
        L.ssrs_roam_tables_selftest.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 4
        L.ssrs_tracks_roam_feed_counts.restype = None
        L.ssrs_tracks_roam_feed_counts.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.ssrs_tracks_roam_stopped_waves.restype = C.c_int64
        L.ssrs_tracks_roam_stopped_waves.argtypes = []
        _lib = L
    return _lib


def check(rc):
    if rc != SSRS_OK:
        msg = lib().ssrs_last_error().decode('utf-8', 'replace')
        if rc == SSRS_ERR_INVALID or rc == SSRS_ERR_START:
            raise ValueError(f'libssrs_hip: {msg}')
        raise SsrsError(rc, msg)


def ptr(t):
    """void* of a torch tensor (None -> NULL)."""
    return C.c_void_p(0 if t is None else t.data_ptr())
