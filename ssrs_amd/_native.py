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

# One line per export of include/ssrs_hip.h: 'return:parameters', one character each (tests/test_native_abi.py checks
# every line against the header).  i int, d double, z size_t, q int64_t, Q uint64_t, p any pointer (NULL = None),
# s const char * (returned), v void.
_KINDS = {'i': C.c_int, 'd': C.c_double, 'z': C.c_size_t, 'q': C.c_int64, 'Q': C.c_uint64, 'p': C.c_void_p,
          's': C.c_char_p, 'v': None}
PROTOTYPES = {
    'ssrs_version': 'i:',
    'ssrs_build_flags': 'i:',
    'ssrs_last_error': 's:',
    'ssrs_device_info': 'i:ipzpp',
    'ssrs_slope_aspect': 'i:pidppiiip',
    'ssrs_orographic_updraft': 'i:ppippippdpdpiiip',
    'ssrs_threshold_updraft': 'i:pdpzp',
    'ssrs_updraft_from_dem': 'i:piddddpdpiip',
    'ssrs_lattice_workspace_bytes': 'z:iii',
    'ssrs_updraft_from_dem_lattice': 'i:pidppiidddddpdpiiipzp',
    'ssrs_wind_from_lattice': 'i:ppiidddddppiiip',
    'ssrs_wind_triangles_workspace_bytes': 'z:iiii',
    'ssrs_wind_from_triangles': 'i:pppppiidppiiipzp',
    'ssrs_wind_nearest_workspace_bytes': 'z:iii',
    'ssrs_wind_nearest_index': 'i:pidpiipzp',
    'ssrs_wind_from_nearest': 'i:pppippiiip',
    'ssrs_wind_cubic_workspace_bytes': 'z:iiiii',
    'ssrs_wind_from_triangles_cubic': 'i:ppppppppiidppiiipzp',
    'ssrs_thermal_seeds': 'i:pdQpiip',
    'ssrs_blur_workspace_bytes': 'z:iid',
    'ssrs_gaussian_blur': 'i:ppdiipzp',
    'ssrs_thermal_fields': 'i:pddpipiiip',
    'ssrs_potential_temperature': 'i:pppzp',
    'ssrs_deardorff_velocity': 'i:pppdpzp',
    'ssrs_thermal_updraft': 'i:pdppdpzp',
    'ssrs_scalar_interp_workspace_bytes': 'z:iiiii',
    'ssrs_scalar_from_samples': 'i:ipppppppiidpiiipzp',
    'ssrs_wtk_thermal_fields': 'i:ipppppppiidpddpiiiipzp',
    'ssrs_track_params_init': 'i:piiid',
    'ssrs_transition_table_build': 'i:pppiip',
    'ssrs_transition_ring_bytes': 'z:ii',
    'ssrs_transition_ring_build': 'i:pppiip',
    'ssrs_transition_thr_bytes': 'z:ii',
    'ssrs_transition_thr_build': 'i:ppppiip',
    'ssrs_tracks_workspace_bytes': 'z:q',
    'ssrs_tracks_workspace_bytes_ex': 'z:qiii',
    'ssrs_tracks_simulate': 'i:pppppqQQppppppzpp',
    'ssrs_tracks_simulate_h64': 'i:pppppqQQpppppzpp',
    'ssrs_traj_recorder_create': 'p:pz',
    'ssrs_traj_recorder_destroy': 'v:p',
    'ssrs_traj_recorder_complete': 'i:p',
    'ssrs_traj_recorder_used': 'z:p',
    'ssrs_tracks_simulate_rec': 'i:pppppqQQpppppzpp',
    'ssrs_tracks_gather': 'i:ppqpppzp',
    'ssrs_hist_reduce': 'i:pzipp',
    'ssrs_presence_count': 'i:pqpiipp',
    'ssrs_presence_workspace_bytes': 'z:iii',
    'ssrs_presence_smooth': 'i:pipiipzp',
    'ssrs_presence_smooth_u64': 'i:pipiipzp',
    'ssrs_presence_normalise_add': 'i:pipzpp',
    'ssrs_presence_normalise_f32': 'i:ppzpp',
    'ssrs_turbine_encounters': 'i:ppqpidppiippp',
    'ssrs_turbine_encounter_counts': 'i:pqippp',
    'ssrs_rotor_encounters': 'i:ppqppiipppipppppp',
    'ssrs_rotor_encounters_timed': 'i:ppqpppiipppippppppp',
    'ssrs_track_occupancy_workspace_bytes': 'z:iii',
    'ssrs_track_occupancy': 'i:ppqiiipppzp',
    'ssrs_altitude_cellinfo': 'i:pipiiiddpp',
    'ssrs_track_altitude_workspace_bytes': 'z:q',
    'ssrs_track_altitude': 'i:ppqpiippppppppzp',
    'ssrs_flight_windinfo': 'i:ppiiiipp',
    'ssrs_track_time': 'i:ppqppiiiipppppp',
    'ssrs_shelter_sx': 'i:pidpppdiippiiip',
    'ssrs_updraft_sheltered': 'i:pidppppppppipddpppiiip',
    'ssrs_shelter_sx_sector': 'i:pidpppdiiddppiiip',
    'ssrs_updraft_sheltered_sector': 'i:pidppppppppipddddpppiiip',
    'ssrs_smooth_workspace_bytes': 'z:iiid',
    'ssrs_smooth_reflect': 'i:pdiddpppiiipzp',
    'ssrs_allen_workspace_bytes': 'z:i',
    'ssrs_allen_thermal_field': 'i:ppppippdiidddiddiiipipppzp',
    'ssrs_projection_init_albers': 'i:p',
    'ssrs_warp_lonlat_raster': 'i:piiidddddpdddpipppiip',
    'ssrs_potential_workspace_bytes': 'z:ii',
    'ssrs_potential_solve': 'i:pppppiidiipzpp',
    'ssrs_uniform_selftest': 'i:Qpppzp',
    'ssrs_roam_pair_word_selftest': 'i:Qppppzp',
    'ssrs_roam_tables_selftest': 'i:ppppiipppp',
    'ssrs_tracks_roam_feed_counts': 'v:pp',
    'ssrs_tracks_roam_stopped_waves': 'q:',
}
EXPORTS = tuple(PROTOTYPES)
# The exports of include/ssrs_hip_passage.h (K17), in the same letter code; tests/test_passage_host.py checks them against
# that header.  They are bound after PROTOTYPES and stay out of it and of EXPORTS, which mirror ssrs_hip.h alone.
PASSAGE_PROTOTYPES = {
    'ssrs_track_passage_workspace_bytes': 'z:iii',
    'ssrs_track_passage': 'i:ppqiiqippppzp',
}
PASSAGE_MAX_PLANES, PASSAGE_MAX_RADIUS = 8, 255
# The export of include/ssrs_hip_transits.h (K18), bound the same way; tests/test_transit_host.py checks it against that header.
TRANSIT_PROTOTYPES = {
    'ssrs_rotor_transits': 'i:ppqppiippppdippppp',
}
ROTOR_TRANSIT_LDS_TURBINES = 7680
# The export of include/ssrs_hip_collision.h (K19), a group of its own bound the same way; tests/test_collision_host.py checks
# it against that header.
COLLISION_PROTOTYPES = {
    'ssrs_rotor_collision_risk': 'i:ppqppiippppdippppppippp',
}
COLLISION_RINGS, ROTOR_COLLISION_LDS_TURBINES = 256, 2560
# The export of include/ssrs_hip_sites.h (K20), a group of its own bound the same way; tests/test_site_host.py checks it
# against that header.
SITE_PROTOTYPES = {
    'ssrs_site_collision_risk': 'i:ppqppiidipidpppp',
}
SITE_MAX_REACH = 62.
# The export of include/ssrs_score.h (K21), a group of its own bound the same way; tests/test_score_host.py checks it against
# that header.
SCORE_PROTOTYPES = {
    'ssrs_tracks_score': 'i:pppppqpppppp',
}
SCORE_SCORED, SCORE_ZERO, SCORE_NOT_A_MOVE, SCORE_OUT, SCORE_UNDEFINED, SCORE_LAST = range(6)
SCORE_MAX_MEMORY, SCORE_ROW = 8, 6
# The export of include/ssrs_score_profile.h (K22), a group of its own bound the same way; tests/test_score_profile_host.py
# checks it against that header.
PROFILE_PROTOTYPES = {
    'ssrs_tracks_score_profile': 'i:pppppqpipipp',
}
PROFILE_MAX_MEMORIES, PROFILE_MAX_NUS = 8, 32
# The export of include/ssrs_bridge.h (K23), a group of its own bound the same way; tests/test_bridge_host.py checks it
# against that header.
BRIDGE_PROTOTYPES = {
    'ssrs_tracks_bridge': 'i:ppppqppppp',
}
BRIDGE_SCORED, BRIDGE_ZERO, BRIDGE_TOO_LONG, BRIDGE_OUT, BRIDGE_UNDEFINED = range(5)
BRIDGE_MAX_MOVES, BRIDGE_JOB = 32, 6


def argtypes(name):
    """The ctypes argtypes of export `name`, from its line of PROTOTYPES."""
    return [_KINDS[k] for k in {**PROTOTYPES, **PASSAGE_PROTOTYPES, **TRANSIT_PROTOTYPES, **COLLISION_PROTOTYPES, **SITE_PROTOTYPES,
                                **SCORE_PROTOTYPES, **PROFILE_PROTOTYPES, **BRIDGE_PROTOTYPES}[name].partition(':')[2]]


# read by the host tests that bind a CPU build of one kernel file by the library's own prototypes
OCCUPANCY_ARGTYPES, ALLEN_FIELD_ARGTYPES, ALTITUDE_CELLINFO_ARGTYPES, ALTITUDE_ARGTYPES, FLIGHT_WINDINFO_ARGTYPES, \
    TRACK_TIME_ARGTYPES, ROTOR_ENCOUNTERS_ARGTYPES, ROTOR_ENCOUNTERS_TIMED_ARGTYPES = map(argtypes, (
        'ssrs_track_occupancy', 'ssrs_allen_thermal_field', 'ssrs_altitude_cellinfo', 'ssrs_track_altitude',
        'ssrs_flight_windinfo', 'ssrs_track_time', 'ssrs_rotor_encounters', 'ssrs_rotor_encounters_timed'))
PASSAGE_ARGTYPES = argtypes('ssrs_track_passage')
ROTOR_TRANSITS_ARGTYPES = argtypes('ssrs_rotor_transits')
ROTOR_COLLISION_RISK_ARGTYPES = argtypes('ssrs_rotor_collision_risk')
SITE_COLLISION_RISK_ARGTYPES = argtypes('ssrs_site_collision_risk')
SCORE_ARGTYPES = argtypes('ssrs_tracks_score')
PROFILE_ARGTYPES = argtypes('ssrs_tracks_score_profile')
BRIDGE_ARGTYPES = argtypes('ssrs_tracks_bridge')


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
                ('roam_shuffles', C.c_int32), ('roam_wide_launches', C.c_int32),
                ('window_scans', C.c_int32)]


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


class SsrsAltitudeParams(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ('start', 'floor', 'ceil', 'band_lo', 'band_hi')]


class SsrsFlightTimeParams(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ('va', 'gmin', 'res_mm')]


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
        for name, proto in list(PROTOTYPES.items()) + list(PASSAGE_PROTOTYPES.items()) + list(TRANSIT_PROTOTYPES.items()) + \
                list(COLLISION_PROTOTYPES.items()) + list(SITE_PROTOTYPES.items()) + list(SCORE_PROTOTYPES.items()) + \
                list(PROFILE_PROTOTYPES.items()) + list(BRIDGE_PROTOTYPES.items()):
            fn = getattr(L, name)
            fn.restype = _KINDS[proto[0]]
            fn.argtypes = argtypes(name)
        if L.ssrs_build_flags() & 1 and not os.environ.get('SSRS_ALLOW_PROBE_LIB'):
            raise ImportError(f'{LIB_PATH} is a timing-probe build (results are wrong on purpose); '
                              'set SSRS_ALLOW_PROBE_LIB=1 for timing runs only')
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
