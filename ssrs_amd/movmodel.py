"""Track stepper host side (K2/K3), behind the reference's function names
(/root/reference/ssrs/movmodel.py).  The per-step work runs in
libssrs_hip.so; this module only prepares arguments (start cells, the
directional prior, which needs the host's cos) and owns the device buffers.

Random stream: the reference draws from numpy's global MT19937 inside a fork
pool (movmodel.py:312, simulator.py:360), which is irreproducible; here
u(seed, track_id, step) is Philox4x32-10 (include/ssrs_hip.h "Uniform
contract"), so results do not depend on how tracks are sharded.
"""
import ctypes as C
import os
import threading
from math import floor, ceil

import numpy as np
import torch

from . import _native as nat
from ._device import device, stream_ptr, to_dev, is_tensor

# movmodel.py:131-141
neighbour_deltas = [np.array([k // 3 - 1, k % 3 - 1]) for k in range(9)]
neighbour_delta_norms_inv = np.array(
    [[1 / np.sqrt(2.), 1., 1 / np.sqrt(2.)], [1., 0., 1.],
     [1 / np.sqrt(2.), 1., 1 / np.sqrt(2.)]], dtype=np.float32)


def get_starting_indices(ntracks, sbounds, stype, twidth, tres):
    """movmodel.py:144-182 -> (rows, cols) int arrays.  Host-side integer logic;
    'random' consumes numpy's legacy global stream with the same single
    np.random.randint call as the reference, so a seeded run picks the same
    start cells."""
    if (sbounds[1] < sbounds[0] or sbounds[3] < sbounds[2] or sbounds[0] < 0.
            or sbounds[2] < 0. or sbounds[1] > twidth[0] or sbounds[3] > twidth[1]):
        raise ValueError('track_start_region incompatible with terrain_width!')
    res_km = tres / 1000.
    x_max = ceil(twidth[0] / res_km)
    y_max = ceil(twidth[1] / res_km)
    x_lo = min(max(floor(sbounds[0] / res_km) - 1, 1), x_max - 2)
    x_hi = max(min(ceil(sbounds[1] / res_km), x_max - 1), 2)
    y_lo = min(max(floor(sbounds[2] / res_km) - 1, 1), y_max - 2)
    y_hi = max(min(ceil(sbounds[3] / res_km), y_max - 1), 2)
    nx, ny = x_hi - x_lo, y_hi - y_lo
    base_count = nx * ny

    def cell(idx):      # candidate list is x-major: idx = ix * ny + iy
        idx = np.asarray(idx, dtype=np.int64)
        return y_lo + idx % ny, x_lo + idx // ny

    if stype == 'structured':
        pick = np.round(np.linspace(0, base_count - 1, ntracks % base_count)).astype(np.int64)
        if ntracks > base_count:
            whole = np.tile(np.arange(base_count, dtype=np.int64), ntracks // base_count)
            idx = np.concatenate((whole, pick))
        else:
            idx = pick
    elif stype == 'random':
        idx = np.random.randint(0, base_count, ntracks)
    else:
        raise ValueError((f'Model:Invalid sim_start_type of {stype}\n'
                          'Options: structured, random'))
    rows, cols = cell(idx)
    return rows.astype(int), cols.astype(int)


def get_directional_probs(theta):
    """movmodel.py:247-257: cos lobe toward heading theta (radians), entries
    below 0.01 zeroed, row order flipped so that +row = north."""
    ang = np.array([[3 * np.pi / 4, np.pi, 5 * np.pi / 4],
                    [np.pi / 2, np.nan, 3 * np.pi / 2],
                    [np.pi / 4, 0., 7 * np.pi / 4]])
    lobe = np.cos(ang + theta)
    lobe[1, 1] = 0.
    lobe[lobe < 0.01] = 0.
    return lobe.flatten()


def make_track_params(grid_shape, move_dirn, memory_parameter=1, scaling_parameter=1.,
                      steps_per_launch=0, profile=False, exact_only=False, schedule=True,
                      binning=True, ring=False, scattered=None, thr=False):
    rows, cols = int(grid_shape[0]), int(grid_shape[1])
    p = nat.SsrsTrackParams()
    nat.check(nat.lib().ssrs_track_params_init(C.byref(p), rows, cols, int(memory_parameter), scaling_parameter))
    prior = get_directional_probs(move_dirn * np.pi / 180.)
    for k in range(9):
        p.prior[k] = float(prior[k])
    p.steps_per_launch = int(steps_per_launch)
    p.flags = (nat.SSRS_TRACKS_PROFILE if profile else 0) | \
        (nat.SSRS_TRACKS_EXACT_ONLY if exact_only else 0) | \
        (0 if schedule else nat.SSRS_TRACKS_NO_SCHEDULE) | \
        (0 if binning else nat.SSRS_TRACKS_NO_BINNING) | \
        (nat.SSRS_TRACKS_RING_TABLE if ring else 0) | \
        (nat.SSRS_TRACKS_THR_TABLE if thr else 0) | \
        (0 if scattered is None else (nat.SSRS_TRACKS_SCATTERED if scattered else nat.SSRS_TRACKS_NO_SCATTERED))
    return p


THR_MAX_CELLS = 1 << 26        # the threshold table is addressed with 32-bit offsets


def table_kind(table, rows=None, cols=None):
    """'f64' | 'ring' | 'thr' | None for a tensor made by build_transition_table.  The kind is the
    tensor's dtype (float64 rows, float32 ring records, int32 threshold dwords), so it survives
    clone / to / pickling; with rows, cols the size is checked against the library's layout."""
    if table is None:
        return None
    kind = {torch.float64: 'f64', torch.float32: 'ring', torch.int32: 'thr'}.get(table.dtype)
    if kind is None:
        raise ValueError(f'a transition table is float64, float32 (ring) or int32 (threshold), not {table.dtype}')
    if rows is not None:
        want = {'f64': rows * cols * 8, 'ring': nat.lib().ssrs_transition_ring_bytes(rows, cols) // 4,
                'thr': nat.lib().ssrs_transition_thr_bytes(rows, cols) // 4}[kind]
        if table.numel() != want or not table.is_contiguous():
            raise ValueError(f'this {table.dtype} tensor is not a {kind} table of a {rows} x {cols} raster '
                             f'({table.numel()} elements, expected {want} contiguous)')
    return kind


def build_transition_table(updraft, potential, ring=False, thr=False, move_dirn=None):
    """Per-cell move weights for the table stepper: 8 x f64 per cell (any
    memory_parameter); with ring=True the f32 ring table (10 x f32 per cell, a
    1-D float32 tensor) of the three-candidate stepper; with thr=True the threshold table
    (8 dwords per cell: the two 16-bit decision thresholds for each of the eight last moves, a 1-D
    int32 tensor) of the threshold stepper -- it belongs to ONE heading, `move_dirn` (degrees),
    recorded in the table's header and checked by the stepper.  Both compact forms serve
    memory_parameter 1 / nu 1 only."""
    upd = to_dev(updraft, torch.float64)
    pot = to_dev(potential, torch.float32)
    rows, cols = int(upd.shape[0]), int(upd.shape[1])
    if pot is not None and tuple(pot.shape) != (rows, cols):
        raise ValueError('updraft and potential shapes differ')
    if thr:
        if move_dirn is None:
            raise ValueError('the threshold table needs move_dirn (it holds the prior fallback of that heading)')
        prior = np.ascontiguousarray(get_directional_probs(float(move_dirn) * np.pi / 180.), dtype=np.float64)
        nbytes = nat.lib().ssrs_transition_thr_bytes(rows, cols)
        # int32: the kind travels with the tensor (the ring table is float32); the heading travels
        # in the table's own header, which ssrs_tracks_simulate checks against its prior
        table = torch.empty(nbytes // 4, dtype=torch.int32, device=upd.device)
        nat.check(nat.lib().ssrs_transition_thr_build(
            nat.ptr(upd), nat.ptr(pot), prior.ctypes.data_as(C.POINTER(C.c_double)), nat.ptr(table),
            rows, cols, stream_ptr()))
        return table
    if ring:
        nbytes = nat.lib().ssrs_transition_ring_bytes(rows, cols)
        table = torch.empty(nbytes // 4, dtype=torch.float32, device=upd.device)
        nat.check(nat.lib().ssrs_transition_ring_build(
            nat.ptr(upd), nat.ptr(pot), nat.ptr(table), rows, cols, stream_ptr()))
        return table
    table = torch.empty((rows, cols, 8), dtype=torch.float64, device=upd.device)
    nat.check(nat.lib().ssrs_transition_table_build(
        nat.ptr(upd), nat.ptr(pot), nat.ptr(table), rows, cols, stream_ptr()))
    return table


def ring_table_applies(memory_parameter, scaling_parameter, want_tracks, exact_only, steps_per_launch):
    """The f32 ring table serves the reference's default movement model only.
    `want_tracks` here means the two-pass trajectory form (the generic kernel writes the
    points itself); recorded trajectories (simulate_tracks' default) keep the ring path."""
    return (int(memory_parameter) == 1 and float(scaling_parameter) == 1.0 and not want_tracks
            and not exact_only and int(steps_per_launch) % 2 == 0)


def default_record_pool_bytes(n, rows, cols):
    """Pool for recorded trajectories: a launch of S = 512 steps needs 4 B x S x live slots,
    so a batch that crosses the raster in ~rows steps needs about n x rows x 4 B x 1.5;
    bounded by a quarter of the free HBM (the pool is only scratch: when it runs out the
    run falls back to the two-pass form)."""
    free, _ = torch.cuda.mem_get_info()
    want = max(int(n) * 4 * max(int(rows), int(cols)) * 3, 1 << 30)     # small batches: lists pad to 256 slots
    return int(max(1 << 20, min(want, free // 4))) // 256 * 256


# The stepper's scratch is large (8.3 KB per track + the pair / fine tables and histogram copies behind it:
# 13-15 GB for a million tracks at 5000 x 6000) and lives only for the duration of a call.  Allocating and
# freeing it around every call left the caching allocator with a freed block of that size which smaller
# requests of the next pass then split, so that the next 13 GB request went to hipMalloc again (~80 ms,
# inside somebody's timed region: profiles/r03_notes.md, the 105.8 ms outlier of round 2's 1 M-track
# sweep).  Each host thread keeps its last workspace per device instead (calls of one thread are serial
# and return synchronised; Simulator's worker threads each hold their own).
_ws_local = threading.local()


def _workspace(nbytes, dev):
    if os.environ.get('SSRS_NO_WS_CACHE'):
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cache = getattr(_ws_local, 'cache', None)
    if cache is None:
        cache = _ws_local.cache = {}
    key = (dev.type, dev.index)
    buf = cache.get(key)
    if buf is None or buf.numel() < nbytes or buf.numel() > 4 * max(nbytes, 1 << 26):
        cache.pop(key, None)
        buf = None                                  # (the old block goes back before the new one is asked for)
        buf = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return buf[:nbytes]


def release_workspaces():
    """Drop this thread's cached stepper workspaces."""
    _ws_local.cache = {}


class TrackBatch:
    """Result of simulate_tracks: device tensors + lazy host views."""

    def __init__(self, lengths, ends, hist, traj, offsets, stats, replay=None):
        self.lengths = lengths        # int32 (n)          trajectory points per track
        self.ends = ends              # int16 (n, 2)       last point [row, col]
        self.hist = hist              # uint32-in-int32 (rows, cols) or None
        self.traj = traj              # int16 (sum lengths, 2) or None
        self.offsets = offsets        # int64 (n + 1) or None
        self.stats = stats            # dict(total_steps, launches, kernel_ms, wall_ms)
        self._replay = replay         # chunked trajectories: callable(t0, t1) -> device (int16 (points, 2), int64 offsets)

    @property
    def total_points(self):
        """Sum of the trajectory lengths (4 bytes each as int16 pairs)."""
        return int(self.lengths.sum(dtype=torch.int64).item())

    def iter_device_chunks(self):
        """(t0, t1, traj, offsets) with the trajectories of tracks [t0, t1) ON THE DEVICE: traj int16 (points, 2) and
        offsets int64 (t1 - t0 + 1) from 0, in track order.  One chunk when the batch holds its trajectory tensor;
        otherwise one per replay range (see iter_tracks), each handed over before anything is copied to the host --
        a consumer on the device (turbines.turbine_encounters) and the pickle are served by ONE replay."""
        if self.traj is not None:
            yield 0, int(self.lengths.numel()), self.traj, self.offsets
            return
        if self._replay is None:
            raise ValueError('simulate_tracks was called with want_tracks=False')
        lengths = self.lengths.cpu().numpy().astype(np.int64)
        budget_points = max(int(self.stats['traj_chunk_bytes']) // 4, 1)
        t0, n = 0, lengths.size
        while t0 < n:
            t1, pts = t0, 0
            while t1 < n and (t1 == t0 or pts + lengths[t1] <= budget_points):
                pts += lengths[t1]
                t1 += 1
            traj, off = self._replay(t0, t1)
            yield t0, t1, traj, off
            t0 = t1

    @staticmethod
    def host_tracks(traj, offsets):
        """The tracks of one device chunk one by one, int16 (n_i, 2) host arrays."""
        traj = traj.cpu().numpy()
        off = offsets.cpu().numpy()
        for i in range(off.size - 1):
            yield traj[off[i]:off[i + 1]]

    def iter_tracks(self):
        """The tracks one by one, int16 (n_i, 2) each, in track order.  When the trajectories did not fit
        the device budget (Sum lengths x 4 B: 1 TB for 100k tracks on the solved 10 m field, where a
        third of them take max_moves = 7.5e6) they are produced range by range: the lengths of the
        finished pass give the ranges, and each range is stepped again with the generic kernel writing
        every point at its offset (the same counter-based streams: the same tracks)."""
        for _, _, traj, off in self.iter_device_chunks():
            yield from self.host_tracks(traj, off)

    def tracks(self, max_bytes=64 << 30):
        """List[int16 (n_i, 2)] like the reference's pool.map result (iter_tracks() streams them)."""
        need = self.total_points * 4
        if need > max_bytes:
            raise MemoryError(f'the trajectories of this batch are {need / 2**30:.1f} GiB (Sum lengths x 4 B): '
                              'stream them with iter_tracks() or run with save_tracks=False')
        return list(self.iter_tracks())


def simulate_tracks(move_dirn, starts, grid_shape, memory_parameter=1,
                    scaling_parameter=1., updraft_field=None, potential_field=None, *,
                    seed=0, track_id_base=0, table=None, use_table=None, hist=None,
                    want_hist=True, want_tracks=False, steps_per_launch=0, profile=False,
                    exact_only=False, schedule=True, binning=True, ring=None, scattered=None,
                    max_moves=None, record=True, record_pool_bytes=None, thr=None, traj_budget_bytes=None, hist64=False):
    """generate_simulated_tracks for a whole batch (movmodel.py:264-318 under
    simulator.py:360-369) + presence histogram (movmodel.py:410-419).

    starts: int (n, 2) [row, col].  updraft_field f64 / potential_field f32
    rasters (numpy or CUDA tensors); both None = 'drw'.  `table` (from
    build_transition_table) or use_table=True selects the one-fetch-per-step
    path; default: table when it pays (many steps per cell).  A float32
    `table` is the ring table (build_transition_table(..., ring=True)), an int32 one the
    threshold table; when the
    table is built here, the threshold table (build_transition_table(..., thr=True)) is
    picked whenever it applies (memory 1, nu 1, rows * cols < 2^26); ring=True / thr=False
    ask for the ring table, ring=False for the f64 table.
    `hist` (int32/uint32 CUDA tensor) is accumulated into when given.  hist64=True (no trajectories): the counts come back
    as an int64 tensor -- the kernels count into a uint32 scratch raster that the library empties into it every other batch
    (ssrs_tracks_simulate_h64): the trap cells of a solved 10 m field pass 2^32 visits from ~250 000 tracks of one call on;
    `hist`, when given, must then be int64 and is accumulated into.

    want_tracks: trajectories (TrackBatch.tracks()).  record=True (default) keeps every
    launch's visited cells in a device pool and assembles the trajectories afterwards
    (ssrs_tracks_simulate_rec + ssrs_tracks_gather): ONE simulation pass on whichever
    stepper path applies.  record=False, or a pool that ran out, takes the two-pass
    form: lengths first, then the same counter-based streams again with the generic
    kernel writing each point at its final offset.  When Sum lengths x 4 B exceeds
    `traj_budget_bytes` (default: a third of the free HBM, at most 16 GiB) no trajectory tensor is
    allocated at all: TrackBatch.iter_tracks() then steps the batch again range by range.
    """
    rows, cols = int(grid_shape[0]), int(grid_shape[1])
    dev = device()
    st = to_dev(np.asarray(starts) if not is_tensor(starts) else starts, torch.int32)
    st = st.reshape(-1, 2).contiguous()
    n = int(st.shape[0])
    upd = to_dev(updraft_field, torch.float64)
    pot = to_dev(potential_field, torch.float32)
    for name, f in (('updraft_field', upd), ('potential_field', pot)):
        if f is not None and tuple(f.shape) != (rows, cols):
            raise ValueError(f'{name} shape {tuple(f.shape)} != grid_shape {(rows, cols)}')
    if pot is not None and upd is None:
        raise ValueError('potential_field needs updraft_field')
    two_pass = bool(want_tracks) and not record
    if table is None and upd is not None:
        if use_table is None:
            # building the table is one streaming pass over the raster (0.5 ms at 5000 x 6000);
            # a batch pays for it with its first few hundred thousand steps -- and tracks that
            # wander in a basin of the potential take millions each (G11), so anything but a
            # handful of tracks takes the table
            use_table = n * max(rows, cols) >= rows * cols // 64 or n >= 4096
        if use_table:
            f32_ok = ring_table_applies(memory_parameter, scaling_parameter, two_pass,
                                        exact_only, steps_per_launch)
            if thr is None:
                thr = f32_ok and ring is None and rows * cols < THR_MAX_CELLS
            if ring is None:
                ring = f32_ok and not thr
            table = build_transition_table(upd, pot, ring=bool(ring) and not thr, thr=bool(thr),
                                           move_dirn=move_dirn)
    kind = table_kind(table, rows, cols)
    is_thr = kind == 'thr'
    is_ring = kind in ('ring', 'thr')          # the f32 / dword family: default movement model only
    if is_ring and not ring_table_applies(memory_parameter, scaling_parameter, two_pass,
                                          exact_only, steps_per_launch):
        raise ValueError('the ring table needs memory_parameter 1, scaling_parameter 1, no '
                         'two-pass trajectory output, exact_only=False and an even steps_per_launch')
    p = make_track_params((rows, cols), move_dirn, memory_parameter, scaling_parameter,
                          steps_per_launch, profile, exact_only, schedule, binning,
                          ring=is_ring and not is_thr, scattered=scattered, thr=is_thr)
    if max_moves is not None:          # probe hook: cap below the reference's R/2 * C/2 (movmodel.py:277)
        p.max_moves = int(max_moves)
    hist_scratch = None
    if hist64:
        if want_tracks:
            raise ValueError('hist64 goes with want_tracks=False')
        if hist is None:
            hist = torch.zeros((rows, cols), dtype=torch.int64, device=dev)
        elif hist.dtype != torch.int64:
            raise ValueError('hist64=True: `hist` must be an int64 tensor')
        hist_scratch = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
    if hist is None and want_hist:
        hist = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
    lengths = torch.empty(n, dtype=torch.int32, device=dev)
    ends = torch.empty((n, 2), dtype=torch.int16, device=dev)
    # room for private histogram copies (used only once a batch is scattered): up to 64,
    # within 4 GB
    copies = 0
    if hist is not None:
        copies = int(min(64, (4 << 30) // (rows * cols * 4)))
        copies = copies if copies >= 2 else 0
    ws_bytes = nat.lib().ssrs_tracks_workspace_bytes_ex(n, rows, cols, copies)
    ws = _workspace(ws_bytes, dev)
    stats = nat.SsrsTrackStats()

    def run(hist_t, traj_t, off_t):
        nat.check(nat.lib().ssrs_tracks_simulate(
            C.byref(p), nat.ptr(upd), nat.ptr(pot), nat.ptr(table), nat.ptr(st),
            n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(track_id_base), nat.ptr(hist_t), nat.ptr(ends),
            nat.ptr(lengths), nat.ptr(traj_t), nat.ptr(off_t), nat.ptr(ws), ws_bytes, C.byref(stats), stream_ptr()))

    traj = offsets = None
    recorded = simulated = False
    if traj_budget_bytes is None:
        traj_budget_bytes = min(16 << 30, torch.cuda.mem_get_info()[0] // 3)
    if want_tracks and record and n > 0:
        # one pass: every launch's visits stay in the pool, the gather assembles them
        pool_bytes = int(record_pool_bytes) if record_pool_bytes is not None else \
            default_record_pool_bytes(n, rows, cols)
        pool = torch.empty(max(256, pool_bytes // 256 * 256), dtype=torch.uint8, device=dev)
        rec = nat.lib().ssrs_traj_recorder_create(nat.ptr(pool), pool.numel())
        if not rec:
            nat.check(nat.SSRS_ERR_INVALID)
        try:
            nat.check(nat.lib().ssrs_tracks_simulate_rec(
                C.byref(p), nat.ptr(upd), nat.ptr(pot), nat.ptr(table), nat.ptr(st),
                n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(track_id_base), nat.ptr(hist), nat.ptr(ends),
                nat.ptr(lengths), rec, nat.ptr(ws), ws_bytes, C.byref(stats), stream_ptr()))
            if nat.lib().ssrs_traj_recorder_complete(rec) and \
                    int(lengths.sum(dtype=torch.int64).item()) * 4 <= int(traj_budget_bytes):
                offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                torch.cumsum(lengths, 0, out=offsets[1:])
                total = int(offsets[-1].item())
                traj = torch.empty((total, 2), dtype=torch.int16, device=dev)
                cursor = torch.empty(n, dtype=torch.int32, device=dev)
                nat.check(nat.lib().ssrs_tracks_gather(
                    rec, nat.ptr(st), n, nat.ptr(offsets), nat.ptr(traj), nat.ptr(cursor), 4 * n, stream_ptr()))
                torch.cuda.current_stream().synchronize()      # the pool dies with this scope
                recorded = True
            simulated = True                  # lengths, end cells and the histogram are final
        finally:
            nat.lib().ssrs_traj_recorder_destroy(rec)
            del pool
        if not recorded and is_ring:
            # the two-pass form runs the generic kernel, which reads the f64 table
            table = build_transition_table(upd, pot, ring=False)
            p = make_track_params((rows, cols), move_dirn, memory_parameter, scaling_parameter,
                                  steps_per_launch, profile, exact_only, schedule, binning, ring=False,
                                  scattered=scattered)
            if max_moves is not None:
                p.max_moves = int(max_moves)
    replay = None
    if want_tracks and not recorded:
        # pass 1: lengths only (done already when a recorded run ran out of pool); pass 2
        # replays the same counter-based streams and writes every point at its final
        # offset (no per-track cap).
        if not simulated:
            run(hist, None, None)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lengths, 0, out=offsets[1:])
        total = int(offsets[-1].item())
        if total * 4 <= int(traj_budget_bytes):
            traj = torch.empty((total, 2), dtype=torch.int16, device=dev)
            run(None, traj, offsets)
        else:
            # too long for one tensor (the reference would hold them as host lists, simulator.py:360-385):
            # range by range on demand, each range one second pass of its own tracks
            offsets = None
            two_table, two_p = table, p

            def replay(t0, t1):
                sub = st[t0:t1].contiguous()
                m = t1 - t0
                sub_len = torch.empty(m, dtype=torch.int32, device=dev)
                sub_end = torch.empty((m, 2), dtype=torch.int16, device=dev)
                off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
                torch.cumsum(lengths[t0:t1], 0, out=off[1:])
                out = torch.empty((int(off[-1].item()), 2), dtype=torch.int16, device=dev)
                wsb = nat.lib().ssrs_tracks_workspace_bytes(m)
                wss = torch.empty(wsb, dtype=torch.uint8, device=dev)
                st2 = nat.SsrsTrackStats()
                nat.check(nat.lib().ssrs_tracks_simulate(
                    C.byref(two_p), nat.ptr(upd), nat.ptr(pot), nat.ptr(two_table), nat.ptr(sub),
                    m, int(seed) & 0xFFFFFFFFFFFFFFFF, int(track_id_base) + t0, None, nat.ptr(sub_end), nat.ptr(sub_len),
                    nat.ptr(out), nat.ptr(off), nat.ptr(wss), wsb, C.byref(st2), stream_ptr()))
                if not torch.equal(sub_len, lengths[t0:t1]):
                    raise RuntimeError('trajectory replay: a track changed its length between the passes')
                return out, off
    elif hist64:
        nat.check(nat.lib().ssrs_tracks_simulate_h64(
            C.byref(p), nat.ptr(upd), nat.ptr(pot), nat.ptr(table), nat.ptr(st),
            n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(track_id_base), nat.ptr(hist_scratch), nat.ptr(hist),
            nat.ptr(ends), nat.ptr(lengths), nat.ptr(ws), ws_bytes, C.byref(stats), stream_ptr()))
    elif not want_tracks:
        run(hist, None, None)
    roam_fed, roam_own = C.c_int64(0), C.c_int64(0)      # of this thread's last stepper call, the one `stats` describes
    nat.lib().ssrs_tracks_roam_feed_counts(C.byref(roam_fed), C.byref(roam_own))
    return TrackBatch(lengths, ends, hist, traj, offsets, replay=replay, stats=
                      dict(total_steps=int(stats.total_steps), launches=int(stats.launches),
                           kernel_ms=float(stats.kernel_ms), wall_ms=float(stats.wall_ms),
                           hist_ms=float(stats.hist_ms), window_launches=int(stats.window_launches),
                           tile_launches=int(stats.tile_launches),
                           block_window_launches=int(stats.block_window_launches),
                           wander_sorts=int(stats.wander_sorts), timed_launches=int(stats.timed_launches),
                           first_move_ms=float(stats.first_move_ms), recorded=bool(recorded),
                           traj_chunk_bytes=int(traj_budget_bytes),
                           block_window_ms=float(stats.block_window_ms),
                           block_window_timed=int(stats.block_window_timed),
                           block_window_steps=int(stats.block_window_steps),
                           roam_launches=int(stats.roam_launches),
                           roam_fine_settled=int(stats.reserved0),
                           roam_wave_pairs=int(stats.roam_wave_pairs),
                           roam_slow_wave_pairs=int(stats.roam_slow_wave_pairs),
                           roam_fed_wave_pairs=int(roam_fed.value), roam_own_wave_pairs=int(roam_own.value),
                           roam_stopped_waves=int(nat.lib().ssrs_tracks_roam_stopped_waves()),
                           roam_shuffles=int(stats.roam_shuffles),
                           roam_wide_launches=int(stats.roam_wide_launches),
                           window_scans=int(stats.window_scans)))


def generate_simulated_tracks(move_dirn, start_location, grid_shape, memory_parameter=1,
                              scaling_parameter=1., updraft_field=None, potential_field=None,
                              *, seed=0, track_id=0):
    """Reference signature (movmodel.py:264-272) for ONE track -> int16 (n, 2).
    The two keyword-only arguments name the track's random stream."""
    res = simulate_tracks(move_dirn, [list(start_location)], grid_shape, memory_parameter,
                          scaling_parameter, updraft_field, potential_field, seed=seed,
                          track_id_base=track_id, use_table=False, want_hist=False,
                          want_tracks=True)
    return res.tracks()[0]


def uniforms(seed, track, step):
    """u(seed, track, step) evaluated on the device (rocRAND Philox engine)."""
    tr = to_dev(np.asarray(track, dtype=np.uint64).view(np.int64), torch.int64).reshape(-1)
    sp = to_dev(np.asarray(step, dtype=np.uint64).view(np.int64), torch.int64).reshape(-1)
    if tr.numel() != sp.numel():
        raise ValueError('track and step lengths differ')
    out = torch.empty(tr.numel(), dtype=torch.float64, device=tr.device)
    nat.check(nat.lib().ssrs_uniform_selftest(
        int(seed) & 0xFFFFFFFFFFFFFFFF, nat.ptr(tr), nat.ptr(sp), nat.ptr(out), tr.numel(), stream_ptr()))
    return out.cpu().numpy()


def roam_pair_words(seed, track, block):
    """The roaming stepper's hand-over word of each (track, Philox block) and the block's four words as rocRAND's engine
    gives them: (packed uint32 (n,), words uint32 (n, 4)), evaluated on the device."""
    tr = to_dev(np.asarray(track, dtype=np.uint64).view(np.int64), torch.int64).reshape(-1)
    bk = to_dev(np.asarray(block, dtype=np.uint64).view(np.int64), torch.int64).reshape(-1)
    if tr.numel() != bk.numel():
        raise ValueError('track and block lengths differ')
    packed = torch.empty(tr.numel(), dtype=torch.int32, device=tr.device)
    words = torch.empty((tr.numel(), 4), dtype=torch.int32, device=tr.device)
    nat.check(nat.lib().ssrs_roam_pair_word_selftest(
        int(seed) & 0xFFFFFFFFFFFFFFFF, nat.ptr(tr), nat.ptr(bk), nat.ptr(packed), nat.ptr(words),
        tr.numel(), stream_ptr()))
    return packed.cpu().numpy().view(np.uint32), words.cpu().numpy().view(np.uint32)


def roam_tables_selftest(updraft, potential, move_dirn, thr=None):
    """The roaming regime's pair and fine tables of a raster and heading (degrees), built by the stepper's own launches
    from the threshold table `thr` of the same fields and heading (default: a fresh one): numpy uint32 arrays
    (pair[rows, cols, 8, 4], fine[rows, cols, 8, 2], prior_words[38])."""
    upd = to_dev(updraft, torch.float64)
    pot = to_dev(potential, torch.float32)
    rows, cols = int(upd.shape[0]), int(upd.shape[1])
    if thr is None:
        thr = build_transition_table(upd, pot, thr=True, move_dirn=move_dirn)
    elif table_kind(thr, rows, cols) != 'thr':
        raise ValueError('thr is not a threshold table')
    prior = np.ascontiguousarray(get_directional_probs(float(move_dirn) * np.pi / 180.), dtype=np.float64)
    pair = torch.empty((rows, cols, 8, 4), dtype=torch.int32, device=upd.device)
    fine = torch.empty((rows, cols, 8, 2), dtype=torch.int32, device=upd.device)
    words = np.zeros(38, dtype=np.uint32)
    nat.check(nat.lib().ssrs_roam_tables_selftest(
        nat.ptr(upd), nat.ptr(pot), prior.ctypes.data_as(C.c_void_p), nat.ptr(thr), rows, cols, nat.ptr(pair), nat.ptr(fine),
        words.ctypes.data_as(C.c_void_p), stream_ptr()))
    return pair.cpu().numpy().view(np.uint32), fine.cpu().numpy().view(np.uint32), words


# ---------------------------------------------------------------- the score of observed tracks (K21)
SCORE_COLUMNS = ('S', 'scored', 'zero', 'not_a_move', 'out', 'undefined')


class TrackScores:
    """Result of score_tracks: device tensors + host views of the per-track sums.

    p          f64 (points,)     the model's probability of the move that LEAVES each point (0 where the status is
                                 LAST, OUT or NOT_A_MOVE, NaN where it is UNDEFINED); None when not asked for
    status     uint8 (points,)   nat.SCORE_SCORED / _ZERO / _NOT_A_MOVE / _OUT / _UNDEFINED / _LAST; None when not asked for
    rows       int64 (ntracks, 6)  per track: S (the surprisal of its SCORED moves in units of 2^-32 bit) and the numbers
                                 of moves by status, in the order of SCORE_COLUMNS
    surprisal_map, scored_map    int64 / int32 (rows, cols), accumulated at the base cell of each SCORED move; None when
                                 not asked for
    offsets    int64 (ntracks + 1)  into p and status
    p and status are parallel to the trajectory tensor; entries outside [offsets[0], offsets[-1]) are not written."""

    def __init__(self, p, status, rows, surprisal_map, scored_map, offsets):
        self.p, self.status, self.rows = p, status, rows
        self.surprisal_map, self.scored_map, self.offsets = surprisal_map, scored_map, offsets
        self._host = None

    def host_rows(self):
        """rows as int64 numpy (ntracks, 6), copied once."""
        if self._host is None:
            self._host = self.rows.cpu().numpy()
        return self._host

    def loglik(self):
        """The log-likelihood (natural log) of every track's SCORED moves: -ln 2 * S / 2^32, f64 (ntracks,).  A track with
        ZERO or UNDEFINED moves has, strictly, likelihood 0: counts() says whether it has any."""
        return -np.log(2.) * self.host_rows()[:, 0].astype(np.float64) / 4294967296.

    def bits_per_move(self):
        """The mean surprisal of every track's SCORED moves in bits (NaN for a track without one)."""
        rows = self.host_rows()
        with np.errstate(invalid='ignore', divide='ignore'):
            return rows[:, 0].astype(np.float64) / 4294967296. / rows[:, 1]

    def counts(self):
        """{'scored', 'zero', 'not_a_move', 'out', 'undefined': int64 (ntracks,)}."""
        rows = self.host_rows()
        return {name: rows[:, k].copy() for k, name in enumerate(SCORE_COLUMNS) if k > 0}


def _pack_tracks(who, tracks, offsets):
    """(traj int16 (points, 2), offsets int64 (ntracks + 1,), ntracks) on the device, from a list of (n_i, 2) arrays or from
    a device tensor with its offsets: what score_tracks and score_tracks_profile take, with their refusals under `who`."""
    if is_tensor(tracks):
        if offsets is None:
            raise ValueError(f'{who}: a trajectory tensor needs its offsets')
        if tracks.dtype != torch.int16 or tracks.dim() != 2 or tracks.shape[1] != 2:
            raise ValueError(f'{who}: the trajectory tensor is int16 (points, 2)')
        traj = to_dev(tracks)
        off = to_dev(offsets, torch.int64).reshape(-1)
        if off.numel() and not 0 <= int(off[0]) <= int(off[-1]) <= int(traj.shape[0]):
            raise ValueError(f'{who}: offsets {int(off[0])} .. {int(off[-1])} do not lie inside the '
                             f'{int(traj.shape[0])} points of the trajectory tensor')
    else:
        if offsets is not None:
            raise ValueError(f'{who}: offsets go with a trajectory tensor, not with a list of tracks')
        parts = [np.asarray(t).reshape(-1, 2) for t in tracks]
        for t in parts:
            if t.size and (t.min() < -32768 or t.max() > 32767):
                raise ValueError(f'{who}: a point does not fit int16')
        flat = np.concatenate([np.zeros((0, 2), dtype=np.int16)] + [t.astype(np.int16) for t in parts])
        traj = to_dev(flat, torch.int16)
        off = to_dev(np.concatenate([[0], np.cumsum([len(t) for t in parts])]).astype(np.int64), torch.int64)
    ntracks = int(off.numel()) - 1
    if ntracks < 0:
        raise ValueError(f'{who}: offsets is empty (ntracks + 1 entries)')
    return traj, off, ntracks


def _score_fields(updraft_field, potential_field, rows, cols):
    """The two rasters of a score on the device (None = not given), checked against the grid."""
    upd = to_dev(updraft_field, torch.float64)
    pot = to_dev(potential_field, torch.float32)
    for name, f in (('updraft_field', upd), ('potential_field', pot)):
        if f is not None and tuple(f.shape) != (rows, cols):
            raise ValueError(f'{name} shape {tuple(f.shape)} != grid_shape {(rows, cols)}')
    if pot is not None and upd is None:
        raise ValueError('potential_field needs updraft_field')
    return upd, pot


def score_tracks(tracks, grid_shape, move_dirn, memory_parameter=1, scaling_parameter=1., updraft_field=None,
                 potential_field=None, *, offsets=None, want_p=True, want_status=True, surprisal_map=None, scored_map=None):
    """The probability the movement model gives to every move of OBSERVED tracks (include/ssrs_score.h, K21): the
    stepper of simulate_tracks read backwards, with the same arguments -- heading, memory, nu and the two rasters
    (both None = 'drw').  Nothing is drawn.

    tracks: a list of int16 (n_i, 2) [row, col] arrays (TrackBatch.tracks(), the pickle), or a device int16 (points, 2)
    tensor with `offsets` (int64, ntracks + 1), as TrackBatch holds them.  surprisal_map / scored_map: True for a fresh
    map, or an int64 / int32 (rows, cols) device tensor that is accumulated into (a sweep over chunks).  One nu per call;
    memory_parameter 1..8 (0, the whole history, is not supported)."""
    rows, cols = int(grid_shape[0]), int(grid_shape[1])
    if int(memory_parameter) == 0:
        raise ValueError('score_tracks: memory_parameter = 0 (the whole history) is not supported; give 1..'
                         f'{nat.SCORE_MAX_MEMORY}')
    dev = device()
    traj, off, ntracks = _pack_tracks('score_tracks', tracks, offsets)
    upd, pot = _score_fields(updraft_field, potential_field, rows, cols)

    def a_map(given, dtype, name):
        if given is None or given is False:
            return None
        if given is True:
            return torch.zeros((rows, cols), dtype=dtype, device=dev)
        if not is_tensor(given) or given.dtype != dtype or tuple(given.shape) != (rows, cols) or not given.is_cuda \
                or not given.is_contiguous():
            raise ValueError(f'score_tracks: {name} is True or a contiguous {dtype} device tensor of shape {(rows, cols)}')
        return given

    smap = a_map(surprisal_map, torch.int64, 'surprisal_map')
    cmap = a_map(scored_map, torch.int32, 'scored_map')
    npts = int(traj.shape[0])
    p = torch.empty(npts, dtype=torch.float64, device=dev) if want_p else None
    status = torch.empty(npts, dtype=torch.uint8, device=dev) if want_status else None
    sums = torch.zeros((ntracks, nat.SCORE_ROW), dtype=torch.int64, device=dev)
    if not 1 <= int(memory_parameter) <= nat.SCORE_MAX_MEMORY:
        raise ValueError(f'score_tracks: memory_parameter = {int(memory_parameter)} outside [1, {nat.SCORE_MAX_MEMORY}]')
    prm = make_track_params((rows, cols), move_dirn, memory_parameter, scaling_parameter)
    if ntracks > 0 and npts > 0:                           # (an empty tensor has no address to hand over)
        nat.check(nat.lib().ssrs_tracks_score(
            C.byref(prm), nat.ptr(upd), nat.ptr(pot), nat.ptr(traj), nat.ptr(off), ntracks, nat.ptr(p),
            nat.ptr(status), nat.ptr(sums), nat.ptr(smap), nat.ptr(cmap), stream_ptr()))
    return TrackScores(p, status, sums, smap, cmap, off)


# ---------------------------------------------------------------- the likelihood profile and the fit (K22)
class TrackProfile:
    """Result of score_tracks_profile: K21's per-track rows over a grid of memories x nus.

    rows       int64 (ntracks, nmem, nnu, 6)  rows[t, a, b] is what score_tracks gives track t under memories[a] and nus[b],
                                 in the order of SCORE_COLUMNS
    memories   tuple of int, ascending;  nus  f64 numpy (nnu,), in the order given (repeats allowed)"""

    def __init__(self, rows, memories, nus):
        self.rows = rows
        self.memories = tuple(int(m) for m in memories)
        self.nus = np.array(nus, dtype=np.float64).reshape(-1)
        if tuple(rows.shape[1:]) != (len(self.memories), self.nus.size, nat.SCORE_ROW):
            raise ValueError(f'TrackProfile: rows of shape {tuple(rows.shape)} for {len(self.memories)} memories and '
                             f'{self.nus.size} nus')
        self._host = None

    def host_rows(self):
        """rows as int64 numpy (ntracks, nmem, nnu, 6), copied once."""
        if self._host is None:
            self._host = self.rows.cpu().numpy() if is_tensor(self.rows) else np.asarray(self.rows, dtype=np.int64)
        return self._host

    def row(self, memory, nu):
        """The int64 numpy (ntracks, 6) slice of one combination (the first of equal nus)."""
        if int(memory) not in self.memories:
            raise ValueError(f'TrackProfile.row: memory {memory} is not one of {self.memories}')
        hits = np.nonzero(self.nus == float(nu))[0]
        if not hits.size:
            raise ValueError(f'TrackProfile.row: nu {nu} is not one of {self.nus.tolist()}')
        return self.host_rows()[:, self.memories.index(int(memory)), int(hits[0])]

    def forbidden(self):
        """int64 (nmem, nnu): the observed moves a combination gives no probability, zero + undefined over the tracks."""
        total = self.host_rows().sum(0)
        return total[..., 2] + total[..., 5]

    def total_bits(self, zero_bits=np.inf):
        """f64 (nmem, nnu): sum_t S / 2^32 + zero_bits * sum_t (zero + undefined), the surprisal of all tracks in bits.
        A move the model forbids has likelihood 0: with the default inf, a combination that forbids any observed move is
        out.  A finite zero_bits is the price per such move, a telemetry-error allowance the caller owns.  0 * inf is 0."""
        bits = self.host_rows()[..., 0].sum(0).astype(np.float64) / 4294967296.
        forbidden = self.forbidden()
        penalty = np.zeros_like(bits)
        penalty[forbidden > 0] = float(zero_bits) * forbidden[forbidden > 0]
        return bits + penalty

    def best(self, zero_bits=np.inf):
        """(memory, nu, bits) of the smallest total_bits; ties go to the first in order of ascending memory, then ascending
        nu.  ValueError when every combination forbids a move and zero_bits is inf."""
        total = self.total_bits(zero_bits)
        order = np.argsort(self.nus, kind='stable')
        ranked = total[:, order]
        if not np.isfinite(ranked).any():
            forbidden = self.forbidden()[:, order]
            a, b = np.unravel_index(int(np.argmin(forbidden)), forbidden.shape)
            raise ValueError(f'TrackProfile.best: every combination forbids an observed move; the fewest, '
                             f'{int(forbidden[a, b])}, under memory {self.memories[a]} and nu {self.nus[order[b]]:g} '
                             '(a finite zero_bits prices them)')
        a, b = np.unravel_index(int(np.argmin(ranked)), ranked.shape)      # (argmin: the first of equal values, row-major)
        return self.memories[a], float(self.nus[order[b]]), float(ranked[a, b])


def _profile_grid(memories, nus):
    """(sorted distinct memories as int32, nus as f64), refused as the library refuses them."""
    mem = np.unique(np.asarray(memories, dtype=np.int64).reshape(-1))
    if not mem.size:
        raise ValueError('score_tracks_profile: memories is empty')
    if mem[0] < 1 or mem[-1] > nat.SCORE_MAX_MEMORY:
        raise ValueError(f'score_tracks_profile: memories {mem.tolist()} outside [1, {nat.SCORE_MAX_MEMORY}] (0, the whole '
                         'history, is not supported)')
    nu = np.ascontiguousarray(nus, dtype=np.float64).reshape(-1)
    if not 1 <= nu.size <= nat.PROFILE_MAX_NUS:
        raise ValueError(f'score_tracks_profile: {nu.size} nus (1 .. {nat.PROFILE_MAX_NUS} a call)')
    if not (nu >= 0.).all():
        raise ValueError(f'score_tracks_profile: nus {nu.tolist()} (not negative, not NaN)')
    return np.ascontiguousarray(mem, dtype=np.int32), nu


def score_tracks_profile(tracks, grid_shape, move_dirn, memories, nus, updraft_field=None, potential_field=None, *,
                         offsets=None):
    """score_tracks' per-track rows for every combination of `memories` (1..8, sorted and de-duplicated on the way in) and
    `nus` (1..32 values, any order) in ONE pass over the points (include/ssrs_score_profile.h, K22): what calibrating
    track_dirn_restrict and track_stochastic_nu on telemetry needs.  tracks, offsets and the fields as score_tracks takes
    them.  Returns a TrackProfile; p, status and the maps come from score_tracks at the fitted values."""
    rows, cols = int(grid_shape[0]), int(grid_shape[1])
    mem, nu = _profile_grid(memories, nus)
    dev = device()
    traj, off, ntracks = _pack_tracks('score_tracks_profile', tracks, offsets)
    upd, pot = _score_fields(updraft_field, potential_field, rows, cols)
    sums = torch.zeros((ntracks, mem.size, nu.size, nat.SCORE_ROW), dtype=torch.int64, device=dev)
    prm = make_track_params((rows, cols), move_dirn, 1, 1.)
    if ntracks > 0 and int(traj.shape[0]) > 0:             # (an empty tensor has no address to hand over)
        nat.check(nat.lib().ssrs_tracks_score_profile(
            C.byref(prm), nat.ptr(upd), nat.ptr(pot), nat.ptr(traj), nat.ptr(off), ntracks, mem.ctypes.data_as(C.c_void_p),
            int(mem.size), nu.ctypes.data_as(C.c_void_p), int(nu.size), nat.ptr(sums), stream_ptr()))
    return TrackProfile(sums, mem.tolist(), nu)


class TrackFit:
    """Result of fit_tracks: the maximum-likelihood memory and nu on the last round's grid.

    memory, nu, bits     TrackProfile.best of the last round
    nu_lo, nu_hi         the last bracket, ONE spacing of the last round's grid wide.  For fixed statuses the surprisal of
                         `memory` is convex in nu, so its minimum lies between the neighbours of nu on that grid; the closing
                         profile at the two midpoints beside nu says in which half: [left neighbour, nu] when the left
                         midpoint is lower than nu, [nu, right neighbour] when the right one is, else between the midpoints.
                         nu lies inside or on its rim.  At an end of the grid nu itself bounds that side
    at_edge              True when round 1's best nu is its grid's largest: the bracket is then ONE-SIDED -- the rounds zoom
                         in below that nu and say nothing about larger ones; give a grid that reaches further
    profiles             one TrackProfile per round
    closing              the TrackProfile of all the memories at the midpoints (None for a grid of one nu); a lower total
                         there moves the bracket, not nu and bits"""

    def __init__(self, memory, nu, bits, nu_lo, nu_hi, at_edge, profiles, closing=None):
        self.memory, self.nu, self.bits, self.nu_lo, self.nu_hi = memory, nu, bits, nu_lo, nu_hi
        self.at_edge, self.profiles, self.closing = at_edge, profiles, closing


def _nu_bracket(nus, nu):
    """The neighbours of `nu` on the sorted grid `nus`; at an end of the grid, nu itself."""
    grid = np.unique(np.asarray(nus, dtype=np.float64))
    k = int(np.searchsorted(grid, nu))
    return float(grid[max(k - 1, 0)]), float(grid[min(k + 1, grid.size - 1)])


def _close_bracket(lo, nu, hi, bits, left, right):
    """The half of [lo, hi] that holds the minimum of a convex function with the value `bits` at nu, `left` at the midpoint
    of [lo, nu] and `right` at that of [nu, hi] (None: that side is an end of the grid, lo or hi is nu)."""
    mid_lo = nu if left is None else .5 * (lo + nu)
    mid_hi = nu if right is None else .5 * (nu + hi)
    if left is not None and left < bits and (right is None or left <= right):
        return lo, nu
    if right is not None and right < bits:
        return nu, hi
    return mid_lo, mid_hi


def fit_tracks(tracks, grid_shape, move_dirn, updraft_field=None, potential_field=None, *, memories=(1, 2, 3, 4), nus=None,
               rounds=3, zero_bits=np.inf, offsets=None):
    """The memory and nu under which the movement model gives OBSERVED tracks the largest likelihood: a coarse grid and a
    zoom, every round one score_tracks_profile.  Round 1 profiles memories x nus (default np.linspace(0, 4, 17)); every
    later round profiles ALL the memories again on np.linspace(lo, hi, len(nus)) between the neighbours of the best nu on
    the sorted grid of the round before.  A closing profile at the two midpoints beside the last best nu halves the last
    bracket (TrackFit.nu_lo, .nu_hi).  zero_bits as TrackProfile.total_bits takes it.  No derivative, no other parameter, no
    collectives.  Returns a TrackFit."""
    nus = np.linspace(0., 4., 17) if nus is None else np.asarray(nus, dtype=np.float64).reshape(-1)
    if int(rounds) < 1:
        raise ValueError(f'fit_tracks: rounds = {rounds} (at least 1)')
    profiles = []
    for _ in range(int(rounds)):
        profiles.append(score_tracks_profile(tracks, grid_shape, move_dirn, memories, nus, updraft_field, potential_field,
                                             offsets=offsets))
        memory, nu, bits = profiles[-1].best(zero_bits)
        lo, hi = _nu_bracket(nus, nu)
        if len(profiles) == 1:
            at_edge = nu == float(np.max(nus))
        nus = np.linspace(lo, hi, len(nus))
    mids = [.5 * (lo + nu)] * (lo < nu) + [.5 * (nu + hi)] * (nu < hi)
    closing = None
    if mids:
        closing = score_tracks_profile(tracks, grid_shape, move_dirn, memories, mids, updraft_field, potential_field,
                                       offsets=offsets)
        at = [float(v) for v in closing.total_bits(zero_bits)[closing.memories.index(memory)]]
        lo, hi = _close_bracket(lo, nu, hi, bits, at[0] if lo < nu else None, at[-1] if nu < hi else None)
    return TrackFit(memory, nu, bits, lo, hi, at_edge, profiles, closing)


def rasterize_track(rows, cols):
    """Real-valued cell coordinates of successive fixes (telemetry already converted to the grid) -> the 8-connected cell
    sequence that score_tracks takes, int16 (n, 2).  Every fix is rounded to its cell (numpy's rint); between two cells a and
    b with d = b - a and N = max(|d_row|, |d_col|) the cells a + sgn(d) * ((2 i |d| + N) // (2 N)), i = 1..N, are emitted
    per axis: the straight line, the minor axis rounded half up.  Repeated cells are dropped, so every consecutive pair is a
    unit move; the first and the last fix keep their cells.  A plain line walk, not a resampling model: a fix interval
    longer than a cell is filled with a line the bird may not have flown."""
    r = np.rint(np.asarray(rows, dtype=np.float64)).reshape(-1)
    c = np.rint(np.asarray(cols, dtype=np.float64)).reshape(-1)
    if r.size != c.size:
        raise ValueError('rasterize_track: rows and cols differ in length')
    if not (np.isfinite(r).all() and np.isfinite(c).all()):
        raise ValueError('rasterize_track: a fix is not finite')
    if r.size and (min(r.min(), c.min()) < -32768 or max(r.max(), c.max()) > 32767):
        raise ValueError('rasterize_track: a fix does not fit int16 cell coordinates')
    cells = np.stack([r, c], 1).astype(np.int64)
    if len(cells) == 0:
        return np.zeros((0, 2), dtype=np.int16)
    out = [cells[:1]]
    for a, b in zip(cells[:-1], cells[1:]):
        d = b - a
        n = int(np.abs(d).max())
        if n == 0:
            continue
        i = np.arange(1, n + 1, dtype=np.int64)[:, None]
        out.append(a + np.sign(d) * ((2 * i * np.abs(d) + n) // (2 * n)))
    return np.concatenate(out).astype(np.int16)


# ---------------------------------------------------------------- gaps between sparse fixes (K23)
GAP_STATUSES = ('scored', 'zero', 'too_long', 'out', 'undefined')


class GapScores:
    """Result of score_gaps: device tensors + host views.

    g          f64 (ngaps, 9)    the probability of being at B after the job's moves, by the move k = 3 (dr + 1) + (dc + 1)
                                 that arrived there (what a later gap would take as its incoming state); 0 where the job
                                 was not evaluated
    status     uint8 (ngaps,)    nat.BRIDGE_SCORED / _ZERO / _TOO_LONG / _OUT / _UNDEFINED
    surprisal  int64 (ngaps,)    rint(-log2(P) * 2^32) of a SCORED gap, 0 otherwise: score_tracks' unit
    arrivals   f64 (ngaps, 32)   the probability of being at B after 1, 2, ... moves, 0 past the job's own number; None when
                                 not asked for
    jobs       int32 (ngaps, 6)  what was scored: row_a, col_a, incoming, row_b, col_b, moves"""

    def __init__(self, g, status, surprisal, arrivals, jobs):
        self.g, self.status, self.surprisal, self.arrivals, self.jobs = g, status, surprisal, arrivals, jobs
        self._host = None

    def _views(self):
        if self._host is None:
            self._host = (self.g.cpu().numpy(), self.status.cpu().numpy(), self.surprisal.cpu().numpy())
        return self._host

    def p(self):
        """P of every gap, f64 (ngaps,): the sum of g in numpy's pairwise order, as the library forms it."""
        g = self._views()[0]
        return (((g[:, 0] + g[:, 1]) + (g[:, 2] + g[:, 3])) + ((g[:, 4] + g[:, 5]) + (g[:, 6] + g[:, 7]))) + g[:, 8]

    def bits(self):
        """The surprisal of every gap in bits, f64 (ngaps,): inf where the model forbids the gap (ZERO, UNDEFINED), NaN where
        it was not evaluated (TOO_LONG, OUT)."""
        _, status, s = self._views()
        out = s.astype(np.float64) / 4294967296.
        out[(status == nat.BRIDGE_ZERO) | (status == nat.BRIDGE_UNDEFINED)] = np.inf
        out[(status == nat.BRIDGE_TOO_LONG) | (status == nat.BRIDGE_OUT)] = np.nan
        return out

    def total_bits(self, zero_bits=np.inf):
        """sum S / 2^32 + zero_bits * (zero + undefined), with the meaning TrackProfile.total_bits gives it: a forbidden
        gap has likelihood 0, a finite zero_bits is the price per such gap; 0 * inf is 0.  Gaps that were not evaluated
        (TOO_LONG, OUT) add nothing: counts() says whether there are any."""
        _, status, s = self._views()
        forbidden = int(((status == nat.BRIDGE_ZERO) | (status == nat.BRIDGE_UNDEFINED)).sum())
        return float(int(s.sum()) / 4294967296.) + (float(zero_bits) * forbidden if forbidden else 0.)

    def counts(self):
        """{'scored', 'zero', 'too_long', 'out', 'undefined': int}."""
        n = np.bincount(self._views()[1], minlength=len(GAP_STATUSES))
        return {name: int(n[k]) for k, name in enumerate(GAP_STATUSES)}


def score_gaps(jobs, grid_shape, move_dirn, scaling_parameter=1., updraft_field=None, potential_field=None, *,
               want_arrivals=False):
    """The probability that the movement model with memory 1 is at cell B `moves` moves after it was at cell A, for every
    job (include/ssrs_bridge.h, K23): the sum over EVERY path between two fixes of sparse telemetry, where score_tracks on
    rasterize_track's line gives the probability of one.  jobs: int32 (ngaps, 6) rows of row_a, col_a, incoming, row_b,
    col_b, moves (fix_gaps makes them), numpy or a device tensor; heading, nu and the two rasters as score_tracks takes them
    (both None = 'drw').  One nu per call, 1 <= moves <= 32, gaps independent of each other.  Returns a GapScores."""
    rows, cols = int(grid_shape[0]), int(grid_shape[1])
    if not is_tensor(jobs):
        jobs = np.ascontiguousarray(jobs)
        if jobs.dtype.kind not in 'iu':
            raise ValueError(f'score_gaps: jobs is an integer array, not {jobs.dtype}')
        if jobs.size and (jobs.min() < -2 ** 31 or jobs.max() >= 2 ** 31):
            raise ValueError('score_gaps: a job does not fit int32')
    elif jobs.dtype != torch.int32:
        raise ValueError(f'score_gaps: a jobs tensor is int32, not {jobs.dtype}')
    if jobs.ndim != 2 or jobs.shape[1] != nat.BRIDGE_JOB:
        raise ValueError(f'score_gaps: jobs of shape {tuple(jobs.shape)}, not (ngaps, {nat.BRIDGE_JOB}): row_a, col_a, '
                         'incoming, row_b, col_b, moves')
    if not float(scaling_parameter) >= 0.:
        raise ValueError(f'score_gaps: scaling_parameter = {scaling_parameter} (not negative, not NaN)')
    dev = device()
    jobs = to_dev(jobs, torch.int32)
    ngaps = int(jobs.shape[0])
    upd, pot = _score_fields(updraft_field, potential_field, rows, cols)
    g = torch.empty((ngaps, 9), dtype=torch.float64, device=dev)
    status = torch.empty(ngaps, dtype=torch.uint8, device=dev)
    surprisal = torch.empty(ngaps, dtype=torch.int64, device=dev)
    arrivals = torch.empty((ngaps, nat.BRIDGE_MAX_MOVES), dtype=torch.float64, device=dev) if want_arrivals else None
    prm = make_track_params((rows, cols), move_dirn, 1, scaling_parameter)
    if ngaps > 0:                                          # (an empty tensor has no address to hand over)
        nat.check(nat.lib().ssrs_tracks_bridge(C.byref(prm), nat.ptr(upd), nat.ptr(pot), nat.ptr(jobs), ngaps, nat.ptr(g),
                                               nat.ptr(status), nat.ptr(surprisal), nat.ptr(arrivals), stream_ptr()))
    return GapScores(g, status, surprisal, arrivals, jobs)


def fix_gaps(fixes, moves=None):
    """One track's successive fix cells, int (n, 2) [row, col], NOT necessarily adjacent -> (jobs int32 (m, 6), pair int64
    (m,)): one job of score_gaps per pair (fixes[j], fixes[j + 1]) and the j it came from.

    moves[j] is the number of moves of pair j (n - 1 of them).  The default is the Chebyshev distance of its cells: the
    FEWEST moves that join them -- a lower bound, not an estimate of what the bird flew, and the probability of a gap
    depends strongly on it; give the number that the fix interval and the bird's speed suggest.  A pair of equal cells has
    no such number and is left out unless `moves` is given.  A pair of more than 32 moves is kept, so that it comes back
    TOO_LONG and is seen.  incoming is the move of the pair before when that pair was a single unit move (one move between
    adjacent cells), else 4, no last move: the track's first pair, after a longer gap, after a repeated cell."""
    cells = np.asarray(fixes)
    if cells.size and cells.dtype.kind not in 'iu':
        raise ValueError(f'fix_gaps: fixes are integer cells, not {cells.dtype} (Simulator.score_fixes takes metres)')
    cells = cells.astype(np.int64).reshape(-1, 2)
    npairs = max(len(cells) - 1, 0)
    d = cells[1:] - cells[:-1]
    cheb = np.abs(d).max(1) if npairs else np.zeros(0, dtype=np.int64)
    if moves is None:
        n = cheb
        keep = cheb > 0
    else:
        n = np.asarray(moves).astype(np.int64).reshape(-1)
        if n.size != npairs:
            raise ValueError(f'fix_gaps: {n.size} moves for {npairs} pairs of fixes')
        keep = np.ones(npairs, dtype=bool)
    unit = keep & (n == 1) & (cheb <= 1)
    incoming = np.full(npairs, 4, dtype=np.int64)
    incoming[1:][unit[:-1]] = (3 * (d[:, 0] + 1) + (d[:, 1] + 1))[:-1][unit[:-1]]
    jobs = np.stack([cells[:-1, 0], cells[:-1, 1], incoming, cells[1:, 0], cells[1:, 1], n], 1)[keep]
    if jobs.size and (jobs.min() < -2 ** 31 or jobs.max() >= 2 ** 31):
        raise ValueError('fix_gaps: a cell or a number of moves does not fit int32')
    return np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, nat.BRIDGE_JOB), np.nonzero(keep)[0].astype(np.int64)


def thin_track(track, every):
    """Every `every`-th point of an 8-connected track, and its last one -> (fixes (m, 2), moves int64 (m - 1,)): what a
    logger that fixes every `every` moves would have kept, with the true number of moves between the fixes, as fix_gaps
    takes them."""
    track = np.asarray(track).reshape(-1, 2)
    every = int(every)
    if every < 1:
        raise ValueError(f'thin_track: every = {every} (at least 1)')
    idx = np.arange(0, len(track), every, dtype=np.int64)
    if len(track) and idx[-1] != len(track) - 1:
        idx = np.append(idx, len(track) - 1)
    return track[idx], np.diff(idx)


# ---------------------------------------------------------------- re-exports
from .presence import (compute_presence_counts, compute_smooth_presence_counts)  # noqa: E402
from . import potential as _potential  # noqa: E402


class MovModel:
    """Fluid-flow movement model (movmodel.py:10-128).  Same constructor; the
    three-call sequence of the reference (boundary nodes, assemble, solve)
    is kept for compatibility, but nothing is assembled: `solve` runs the
    matrix-free GPU solver."""

    def __init__(self, move_dirn, grid_shape):
        self.move_dirn = move_dirn
        self.grid_shape = grid_shape

    def get_boundary_nodes(self):
        return _potential.get_boundary_nodes(self.move_dirn, self.grid_shape)

    def assemble_sparse_linear_system(self):
        """No-op placeholder: the operator is applied matrix-free on the GPU."""
        return None, None, None

    def solve_sparse_linear_system(self, conductivity, bnodes=None, benergy=None,
                                   row_inds=None, col_inds=None, facs=None, **kwargs):
        """Potential f32 (rows, cols).  bnodes/benergy are re-derived from
        move_dirn (they are a pure function of it in the reference too)."""
        return _potential.solve_potential(conductivity, self.move_dirn, **kwargs)
