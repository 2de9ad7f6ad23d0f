"""ssrs_tracks_simulate_h64 (include/ssrs_hip.h) on every stepper path, driven through ctypes as a C-ABI caller drives it.

The kernels count into the caller's uint32 scratch, the private histogram copies of a scattered batch and the transposed
raster of an east / west front; the library must empty all three into the 64-bit counts before any cell can wrap.  A
wrapped cell raises no fault: it is 2^32 short, and only the counts themselves show it.  Two ways to get there:

(a) a scratch preloaded with 2^32 - P at the cells the trap fills (the header: whatever the scratch holds is counted too),
    then a small trapped batch in short launches that adds more than 2P visits to them: against the C oracle, cell for
    cell, on each path;
(b) a batch that takes one cell past 2^32 by stepping alone (the copies' own 32-bit sums): against the same tracks in
    sub-batches on the 32-bit ssrs_tracks_simulate, added up in int64."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, COLS = 96, 128
S = 8                        # steps per launch of (a), with SSRS_TRACKS_FIXED_STEPS
N_A = 8192                   # tracks of (a): enough for the row window / transposed window to bin
MOVES_A = 24_000
TWO32 = 1 << 32


def _trap_field():
    """A circular trough of radius 7 around the raster's centre whose floor falls clockwise by 6 per radian: tracks run
    round it (with memory 2 too, which forbids reversing either of the last two moves; a one-cell pit does not hold
    those), 84 % (memory 1) / 65 % (memory 2) of them until max_moves.  Zero updraft: the weights are the potential's."""
    rr, cc = np.arange(ROWS, dtype=np.float64)[:, None], np.arange(COLS, dtype=np.float64)[None, :]
    dy, dx = rr - ROWS // 2, cc - COLS // 2
    d = np.sqrt(dy ** 2 + dx ** 2)
    theta = np.mod(np.arctan2(dx, -dy), 2 * np.pi)
    return np.zeros((ROWS, COLS)), (5. * (d - 7.) ** 2 + 6. * theta).astype(np.float32)


def _starts(n, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(ROWS // 2 - 10, ROWS // 2 + 10, n),
                     rng.integers(COLS // 2 - 10, COLS // 2 + 10, n)], 1).astype(np.int32)


class _Env:
    def __init__(self, names):
        self.names = list(names)

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.names}
        for k in self.names:
            os.environ[k] = '1'

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _inputs(memory, heading, table_kind):
    from ssrs_amd import movmodel
    upd, pot = _trap_field()
    upd_t = torch.from_numpy(upd).cuda()
    pot_t = torch.from_numpy(pot).cuda()
    table = None
    if table_kind == 'f64':
        table = movmodel.build_transition_table(upd_t, pot_t)
    elif table_kind == 'ring':
        table = movmodel.build_transition_table(upd_t, pot_t, ring=True)
    elif table_kind == 'thr':
        table = movmodel.build_transition_table(upd_t, pot_t, thr=True, move_dirn=heading)
    return upd, pot, upd_t, pot_t, table


def _params(memory, heading, table_kind, flags, steps, max_moves):
    from ssrs_amd import movmodel, _native as nat
    p = movmodel.make_track_params((ROWS, COLS), heading, memory, 1., steps_per_launch=steps,
                                   ring=table_kind == 'ring', thr=table_kind == 'thr')
    p.flags |= flags
    p.max_moves = int(max_moves)
    return p


def _workspace(n, copies):
    from ssrs_amd import _native as nat
    nb = int(nat.lib().ssrs_tracks_workspace_bytes_ex(n, ROWS, COLS, copies) if copies
             else nat.lib().ssrs_tracks_workspace_bytes(n))
    return torch.empty(nb, dtype=torch.uint8, device='cuda'), nb


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _h64(p, upd_t, pot_t, table, starts, seed, base, scratch, hist64, copies):
    """One ssrs_tracks_simulate_h64 call -> (lengths, end cells, stats)."""
    from ssrs_amd import _native as nat
    n = int(starts.shape[0])
    st = torch.from_numpy(starts).cuda()
    lengths = torch.empty(n, dtype=torch.int32, device='cuda')
    ends = torch.empty((n, 2), dtype=torch.int16, device='cuda')
    ws, nb = _workspace(n, copies)
    stats = nat.SsrsTrackStats()
    nat.check(nat.lib().ssrs_tracks_simulate_h64(
        C.byref(p), nat.ptr(upd_t), nat.ptr(pot_t), nat.ptr(table), nat.ptr(st), C.c_int64(n), C.c_uint64(seed),
        C.c_uint64(base), nat.ptr(scratch), nat.ptr(hist64), nat.ptr(ends), nat.ptr(lengths), nat.ptr(ws),
        C.c_size_t(nb), C.byref(stats), _stream()))
    torch.cuda.synchronize()
    return lengths.cpu().numpy(), ends.cpu().numpy(), stats


def _h32(p, upd_t, pot_t, table, starts, seed, base, copies):
    """One 32-bit ssrs_tracks_simulate call -> (lengths, end cells, uint32 counts, total steps)."""
    from ssrs_amd import _native as nat
    n = int(starts.shape[0])
    st = torch.from_numpy(starts).cuda()
    lengths = torch.empty(n, dtype=torch.int32, device='cuda')
    ends = torch.empty((n, 2), dtype=torch.int16, device='cuda')
    hist = torch.zeros((ROWS, COLS), dtype=torch.int32, device='cuda')
    ws, nb = _workspace(n, copies)
    stats = nat.SsrsTrackStats()
    nat.check(nat.lib().ssrs_tracks_simulate(
        C.byref(p), nat.ptr(upd_t), nat.ptr(pot_t), nat.ptr(table), nat.ptr(st), C.c_int64(n), C.c_uint64(seed),
        C.c_uint64(base), nat.ptr(hist), nat.ptr(ends), nat.ptr(lengths), None, None, nat.ptr(ws), C.c_size_t(nb),
        C.byref(stats), _stream()))
    torch.cuda.synchronize()
    return lengths.cpu().numpy(), ends.cpu().numpy(), hist.cpu().numpy().view(np.uint32), int(stats.total_steps)


_ORACLE = {}


def _oracle(memory, heading, n):
    from oracle import c_oracle
    key = (memory, heading, n)
    if key not in _ORACLE:
        upd, pot = _trap_field()
        _ORACLE[key] = c_oracle.simulate_tracks(float(heading), _starts(n), (ROWS, COLS), memory, 1., upd, pot, seed=7,
                                                max_moves=MOVES_A, want_traj=False)
    return _ORACLE[key]


def _missing(got, want):
    """Multiples of 2^32 the 64-bit counts lack, summed over the cells."""
    d = want.astype(np.int64) - got.astype(np.int64)
    return int(d[d > 0].sum() // TWO32)


# case: (memory, heading, table, flag, environment switches, hist copies, expected path).  Without
# SSRS_TRACKS_NO_BLOCK_WINDOW a threshold-table batch that scatters turns to block windows, the one path that drained
# mid-call before: the control case, and the east / west fronts, whose transposed raster is added up at the end.
CASES = {
    'direct_f64': (1, 0., None, 0, (), 0, None),
    'f64_table': (2, 0., 'f64', 0, (), 0, None),
    'ring_table': (1, 0., 'ring', 0, (), 0, None),
    'thr_no_block_window': (1, 0., 'thr', 0, ('SSRS_TRACKS_NO_BLOCK_WINDOW',), 0, 'no_block_window'),
    'thr_not_scattered': (1, 0., 'thr', 'NO_SCATTERED', ('SSRS_TRACKS_NO_BLOCK_WINDOW',), 0, 'no_block_window'),
    'scattered_copies': (1, 0., 'thr', 'SCATTERED', ('SSRS_TRACKS_NO_BLOCK_WINDOW',), 64, 'no_block_window'),
    'scattered_no_copies': (1, 0., 'thr', 'SCATTERED', ('SSRS_TRACKS_NO_BLOCK_WINDOW',), 0, 'no_block_window'),
    'per_step_atomics': (1, 0., 'thr', 'NO_BINNING', ('SSRS_TRACKS_NO_BLOCK_WINDOW',), 0, 'no_window'),
    'east_front_transposed': (1, 90., 'thr', 0, (), 64, 'window'),
    'west_front_transposed': (1, 270., 'thr', 0, (), 64, 'window'),
    'cached_control': (1, 0., 'thr', 0, (), 0, 'block_window'),
}


@pytest.mark.parametrize('case', list(CASES))
def test_preloaded_scratch_counts_exactly_on_every_path(gpu, case):
    """The scratch holds 2^32 - P at every cell the oracle's batch visits.  With SSRS_TRACKS_FIXED_STEPS every launch is
    S = 8 steps deep and a batch is at most kBatch = 2 launches, so two batches add at most 4 (S + 1) = 36 points per
    track to one cell, 36 N = 294 912 for N = 8192 tracks; P = 4 x that = 1 179 648.  The trap's hottest cells receive
    ~3.8e6 > 2P visits: a library that drains the scratch only at the end (or lets a 32-bit sum wrap) comes out 2^32
    short there.  hist64 - preload must equal the oracle's counts cell for cell; lengths and end cells too."""
    from ssrs_amd import _native as nat
    memory, heading, kind, flags, env, copies, path = CASES[case]
    flags = getattr(nat, 'SSRS_TRACKS_' + flags) if flags else 0
    upd, pot, upd_t, pot_t, table = _inputs(memory, heading, kind)
    ref = _oracle(memory, heading, N_A)
    want = ref['hist'].astype(np.int64)
    per_two_batches = 2 * 2 * (S + 1) * N_A
    P = 4 * per_two_batches
    assert want.max() > 2 * P, (case, int(want.max()), P)          # the trap is hot enough for the test to bite
    preload = np.where(want > 0, TWO32 - P, 0).astype(np.int64)
    scratch = torch.from_numpy(preload.astype(np.uint32).view(np.int32)).cuda()
    hist64 = torch.zeros((ROWS, COLS), dtype=torch.int64, device='cuda')
    p = _params(memory, heading, kind, flags, S, MOVES_A)
    with _Env(('SSRS_TRACKS_FIXED_STEPS',) + tuple(env)):
        lengths, ends, st = _h64(p, upd_t, pot_t, table, _starts(N_A), 7, 0, scratch, hist64, copies)
    got = hist64.cpu().numpy() - preload
    assert np.array_equal(lengths, ref['lengths']), case
    assert np.array_equal(ends, ref['ends']), case
    assert np.array_equal(got, want), f'{case}: {_missing(got, want)} multiples of 2^32 missing'
    assert not scratch.any(), 'the scratch is handed back empty'
    if path == 'no_block_window':
        assert st.block_window_launches == 0, case
    elif path == 'block_window':
        assert st.block_window_launches > 0, case
    elif path == 'window':
        assert st.window_launches > 0 and st.tile_launches == 0, case
    elif path == 'no_window':
        assert st.window_launches == 0 and st.tile_launches == 0 and st.block_window_launches == 0, case


# (b): name -> (memory, table, flag, switches, copies, tracks, max_moves, sub-batches of the reference).  The trap's
# hottest cell takes 2.5 % of all steps (both memories), so one cell passes 2^32 from ~1.7e11 steps on.  Memory 1: tracks
# leave the trough after 2.4e5 steps on average, whatever max_moves -> 786 432 tracks, 1.9e11 steps.  Memory 2: two
# thirds stay until max_moves -> 65 536 tracks x 4.4e6 moves, 1.9e11 steps.  Both paths step this trapped batch at
# ~1.6e10 steps/s on the MI355X (same-cell atomics, 64 copies): ~12 s per call, as long again for the reference.
PAST = {
    'thr_scattered_copies': (1, 'thr', 'SCATTERED', ('SSRS_TRACKS_NO_BLOCK_WINDOW',), 64, 3 << 18, 1_000_000, 8),
    'f64_table_copies': (2, 'f64', 'SCATTERED', (), 64, 1 << 16, 4_400_000, 8),
}


@pytest.mark.parametrize('case', list(PAST))
def test_counts_past_2_32_by_stepping(gpu, case):
    """One call whose hottest cell passes 2^32 visits on its own: the private copies' sums and the scratch would wrap.
    Against the same tracks in sub-batches (consecutive track ids) on the 32-bit ssrs_tracks_simulate, each far below
    2^32 per cell (its own checksum says so), added up in int64: identical lengths, end cells and counts."""
    from ssrs_amd import _native as nat
    memory, kind, flags, env, copies, n, moves, nsub = PAST[case]
    flags = getattr(nat, 'SSRS_TRACKS_' + flags) if flags else 0
    upd, pot, upd_t, pot_t, table = _inputs(memory, 0., kind)
    starts = _starts(n, seed=11)
    p = _params(memory, 0., kind, flags, 0, moves)
    scratch = torch.zeros((ROWS, COLS), dtype=torch.int32, device='cuda')
    hist64 = torch.zeros((ROWS, COLS), dtype=torch.int64, device='cuda')
    with _Env(env):
        lengths, ends, st = _h64(p, upd_t, pot_t, table, starts, 30, 0, scratch, hist64, copies)
        want = np.zeros((ROWS, COLS), dtype=np.int64)
        ref_len, ref_end = [], []
        step = -(-n // nsub)
        for b0 in range(0, n, step):
            sub = starts[b0:b0 + step]
            l, e, h, steps = _h32(p, upd_t, pot_t, table, sub, 30, b0, copies)
            assert int(h.astype(np.int64).sum()) == steps + len(sub), 'a reference sub-batch wrapped'
            want += h
            ref_len.append(l)
            ref_end.append(e)
    got = hist64.cpu().numpy()
    assert np.array_equal(lengths, np.concatenate(ref_len))
    assert np.array_equal(ends, np.concatenate(ref_end))
    assert int(got.sum()) == int(st.total_steps) + n
    assert int(got.max()) > TWO32, int(got.max())
    assert np.array_equal(got, want), f'{case}: {_missing(got, want)} multiples of 2^32 missing'
