"""Every kernel family on a side stream, and from two host threads, under tests/stream_order.py.

include/ssrs_hip.h promises of every export that takes a `stream`: asynchronous on it, or one wait for it with the launches
put to it in order; and the library is thread-safe for distinct streams.  Simulator runs every (case, realisation) item
under torch.cuda.stream(torch.cuda.Stream()) from a thread pool, so the product lives on side streams -- and on the null
stream, where the rest of the suite runs, a launch, memset or copy that forgets its stream is ordered by accident.

Here every family's existing checker (the thunks of test_gpu_dirty_memory.FAMILIES and five more; references, tolerances and
cases are those of the families' own modules) runs inside torch.cuda.stream(S) with the library behind stream_order's proxy:
every streamed call must carry S, and a device-side delay sits in front of it, on S ('late_stream') or on the null stream
('late_null').  profiles/stream_contract.md has the measured delay, the stream that was chosen, the exports seen and the
two mutations under which these tests were seen to fail."""
import threading

import numpy as np
import pytest
import torch

import stream_order
from test_gpu_dirty_memory import FAMILIES as DIRTY_FAMILIES

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the positive controls
def test_controls_fire_on_the_side_stream_and_not_on_the_null_stream(gpu):
    """torch only, no library code.  On the chosen side stream a copy enqueued on the null stream holds the stale values
    (a), and a consumer on the side stream does not see what a late null stream produced (b); with the null stream in the
    side stream's place both give the producer's values."""
    side, index = stream_order.side_stream()
    assert side is not None, f'none of {stream_order.CANDIDATES} fresh streams separates from the null stream'
    null = torch.cuda.default_stream()
    assert side.cuda_stream != 0 and null.cuda_stream == 0
    print(f'side stream: candidate {index} of {stream_order.CANDIDATES}, handle {side.cuda_stream:#x}; '
          f'{stream_order.cycles_per_ms():.0f} sleep cycles per ms, delay {stream_order.DELAY_MS} ms')
    assert stream_order.control_copy_off_the_stream(side) == 0.
    assert stream_order.control_consumer_on_the_stream(side) == 0.
    assert stream_order.control_copy_off_the_stream(null) == 1.
    assert stream_order.control_consumer_on_the_stream(null) == 1.
    a, b = stream_order.delay(side, timed=True)
    b.synchronize()
    assert a.elapsed_time(b) >= stream_order.DELAY_MS, a.elapsed_time(b)


# ------------------------------------------------------------------------------------------------ the families
# The five that test_gpu_dirty_memory.FAMILIES does not have, each through the device checker of its own module, without
# the dirty arena (one hostile condition per test).
def _passage(gpu, golden):
    """A raster smaller than a window, a chunk that begins inside its buffer, and 33 = 1 mod 32 tracks on 70 x 130; the
    three plane counts and the buffer's placements between them."""
    import passage_ref as ref
    import test_gpu_passage as t
    picks = (('basic_5x3_r2', 1, 0), ('lead_2', 3, 1), ('borders_33', 8, 3), ('borders_33', 1, 2))
    return [lambda n=n, p=p, s=s: t.run_case(ref.case(n), gpu, p, s) for n, p, s in picks]


def _transits(gpu, golden):
    import transit_ref as ref
    import test_gpu_rotor_transits as t
    return [lambda n=n: t.check(t.run(ref.case(n), gpu), ref.expected(n)) for n in ('short', 'planted')]


def _collision(gpu, golden):
    import collision_ref as ref
    import test_gpu_collision_risk as t
    return [lambda n=n: t.check(t.run(ref.case(n), gpu), ref.expected(n)) for n in ('short', 'rings')]


def _site(gpu, golden):
    """The three tiny rasters with their classes, and the short tracks on 70 x 90."""
    import collision_ref as cref
    import site_ref as ref
    import test_gpu_site_risk as t
    combos = [(c, k) for c in ref.TINY_CASES for k in ref.TINY_CLASSES] + [(cref.case('short'), 'r4')]
    return [lambda c=c, k=k: t.check(t.run(c, k, gpu), ref.expected(c, k)) for c, k in combos]


def _potential(gpu, golden):
    """3 x 3, the 62 columns of a wave, and 65 x 97: AMG set-up, the scans and the graph capture on a side stream."""
    import potential_cases as pc
    import test_gpu_potential_shapes as t

    def solve(case):
        d = pc.load_case(golden('g16_potential_shapes.npz'), case)
        d['system'] = pc.assemble(d['cond'], case.heading)
        pot, st = t.run(case, d)
        assert st['converged'], (pc.case_id(case), st)
        t.check_field(case, d, pot, ' side stream')
    return [lambda c=c: solve(c) for c in pc.QUIRK_CASES if (c.rows, c.cols) in ((3, 3), (9, 62), (65, 97))]


def _misc(gpu, golden):
    """The exports no other family is there for, or reaches only in passing: the three self-tests, ssrs_presence_count and
    ssrs_tracks_simulate_h64; and the two that the header-derived list showed no family to call at all, the plain
    ssrs_tracks_simulate (the wrappers of the other families record or count in 64 bits) and ssrs_wind_from_lattice."""
    import test_gpu_hist64 as h
    import test_gpu_interp_edges as ie
    import test_gpu_roam_feed as rf
    import test_gpu_tables as tb
    import test_gpu_tracks as tr

    def presence_counts():
        from ssrs_amd import movmodel
        from test_gpu_presence_potential import split
        g = golden('g9_presence.npz')
        assert np.array_equal(movmodel.compute_presence_counts(split(g['tracks'], g['lengths']), (40, 50)), g['counts'])
    return [lambda: tr.test_uniform_contract_matches_oracle(gpu),
            lambda: rf.test_hand_over_word_is_the_top_halves_of_words_x_and_z(gpu),
            lambda: tb.test_roam_tables_every_state(gpu, ('magnitudes', (17, 65), True)),
            presence_counts,
            lambda: h.test_preloaded_scratch_counts_exactly_on_every_path(gpu, 'ring_table'),
            lambda: tr.test_privatised_histogram_in_the_generic_kernels(gpu, 1, False),
            lambda: ie.test_wind_lattice_edges(gpu, (4, 3))]


FAMILIES = dict(DIRTY_FAMILIES, passage=_passage, transits=_transits, collision=_collision, site=_site,
                potential=_potential, misc=_misc)
SEEN = {mode: {} for mode in stream_order.MODES}             # mode -> {family: the streamed exports its thunks called}


def run_family(family, mode, gpu, golden):
    from ssrs_amd import movmodel
    side, _ = stream_order.side_stream()
    assert side is not None, f'none of {stream_order.CANDIDATES} fresh streams separates from the null stream'
    SEEN[mode][family] = set()
    movmodel.release_workspaces()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side), stream_order.watching(mode) as proxy:
            try:
                for thunk in FAMILIES[family](gpu, golden):
                    thunk()
                side.synchronize()
            finally:
                SEEN[mode][family] = set(proxy.seen())
        assert not proxy.problems, proxy.problems
        assert proxy.calls, f'{family}: no streamed export was called'
        strays = sorted({name for name, handle, _ in proxy.calls if handle != side.cuda_stream})
        assert not strays, f'{family}: not on the side stream: {strays}'
        torch.cuda.synchronize()
        host = sorted(seconds for _, _, seconds in proxy.calls)
        print(f'{family} [{mode}]: {len(proxy.calls)} streamed calls of {len(proxy.seen())} exports, host time of a call '
              f'median {1e3 * host[len(host) // 2]:.3f} ms, first delay {proxy.achieved_ms():.3f} ms')
        assert proxy.achieved_ms() >= stream_order.DELAY_MS, (proxy.achieved_ms(), stream_order.DELAY_MS)
    finally:
        torch.cuda.synchronize()                  # (a delay still queued on the null stream ends with its own test)
        movmodel.release_workspaces()


@pytest.mark.parametrize('mode', stream_order.MODES)
@pytest.mark.parametrize('family', list(FAMILIES))
def test_family_is_ordered_on_a_side_stream(gpu, golden, family, mode):
    """Every thunk of the family inside torch.cuda.stream(S) with a delay in front of every streamed call, S alone
    synchronised by the checkers: their references and tolerances hold, every streamed call carried S."""
    run_family(family, mode, gpu, golden)


# ------------------------------------------------------------------------------------------------ two host threads
# Simulator's shape: each worker thread enters a stream of its own and runs the stepper's consumers there.  Three rounds,
# every family once; the two threads of a round share no reference module (the references' caches are per module).
ROUNDS = ((('tracks_recorded',), ('turbines', 'rotor')),
          (('occupancy', 'passage'), ('altitude', 'flight_time')),
          (('transits', 'collision', 'site'), ('presence',)))


def _refusal(which):
    """One host-side refusal (nothing is launched) -> (the export's name, its return code)."""
    from ssrs_amd import _native as nat
    from ssrs_amd._device import stream_ptr
    if which == 0:
        return 'ssrs_slope_aspect', nat.lib().ssrs_slope_aspect(None, 1, 10., None, None, 1, 10, 10, stream_ptr())
    return 'ssrs_threshold_updraft', nat.lib().ssrs_threshold_updraft(None, 0.75, None, 4, stream_ptr())


@pytest.mark.parametrize('families', ROUNDS, ids=['+'.join(a) + '|' + '+'.join(b) for a, b in ROUNDS])
def test_consumers_from_two_host_threads(gpu, golden, families):
    """Two host threads, each inside its own side stream, run different families at the same time under the handle check:
    every checker passes, no thread raises, every call carried its own thread's stream, and ssrs_last_error() of a thread
    shows its own refusal and not the other's."""
    from ssrs_amd import _native as nat
    from ssrs_amd import movmodel
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert streams[0].cuda_stream != streams[1].cuda_stream and all(s.cuda_stream for s in streams)
    errors, messages, idents = [], [None, None], [None, None]
    both_refused = threading.Barrier(2, timeout=60)

    def work(i):
        try:
            idents[i] = threading.get_ident()
            with torch.cuda.stream(streams[i]):
                name, rc = _refusal(i)
                assert rc == nat.SSRS_ERR_INVALID, (name, rc)
                both_refused.wait()                                  # the other thread's refusal has happened by now
                messages[i] = nat.lib().ssrs_last_error().decode()
                for family in families[i]:
                    for thunk in FAMILIES[family](gpu, golden):
                        thunk()
                streams[i].synchronize()
        except BaseException as exc:
            both_refused.abort()
            errors.append((i, families[i], exc))
        finally:
            movmodel.release_workspaces()

    with stream_order.watching('check') as proxy:
        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    assert not proxy.problems, proxy.problems
    assert 'ssrs_slope_aspect' in messages[0] and 'ssrs_threshold_updraft' not in messages[0], messages
    assert 'ssrs_threshold_updraft' in messages[1] and 'ssrs_slope_aspect' not in messages[1], messages
    handles = {handle for _, handle, _ in proxy.calls}
    assert handles == {s.cuda_stream for s in streams}, (handles, [s.cuda_stream for s in streams])
    print(f'{families}: {len(proxy.calls)} streamed calls of {len(proxy.seen())} exports on two streams')


def test_two_thread_rounds_name_every_consumer_once():
    named = [f for pair in ROUNDS for group in pair for f in group]
    assert sorted(named) == sorted(['tracks_recorded', 'turbines', 'rotor', 'occupancy', 'passage', 'altitude',
                                    'flight_time', 'transits', 'collision', 'site', 'presence'])
    assert set(named) <= set(FAMILIES)


# ------------------------------------------------------------------------------------------------ what was seen
def test_every_streamed_export_of_the_headers_was_seen(gpu, golden):
    """Under each delay mode the families call every export of include/ssrs_hip*.h that takes a stream, but the documented
    exclusions.  (A family that has not run in this process -- a selection with -k -- runs here.)"""
    streamed = set(stream_order.streamed_exports())
    for mode in stream_order.MODES:
        for family in FAMILIES:
            if family not in SEEN[mode]:
                run_family(family, mode, gpu, golden)
        seen = set().union(*SEEN[mode].values())
        print(f'[{mode}] {len(seen)} of {len(streamed)} streamed exports seen:')
        for name in sorted(streamed):
            where = sorted(f for f, names in SEEN[mode].items() if name in names)
            print(f'  {name}: {", ".join(where) if where else "not seen -- " + stream_order.EXCLUSIONS.get(name, "?")}')
        assert seen <= streamed
        assert streamed - seen == set(stream_order.EXCLUSIONS), sorted(streamed - seen ^ set(stream_order.EXCLUSIONS))
