"""Every kernel family through the library's own Python entry point on dirty, guarded memory (tests/dirty_memory.py).

torch.empty in a test process is usually a fresh block; in a Simulator run it is a recycled one.  Here every workspace and
every output of a wrapper comes from the arena, filled with 0x00, with the leavings of an earlier call of the same family
on OTHER inputs, or with 0xFF (NaN / -1 / all bits set), between canary guards.  Under every fill

  * the family's existing checker passes (references and tolerances are those of the case modules the suite shares);
  * the guards are clean: nothing was written before or after a workspace or an output;
  * where include/ssrs_hip.h or DESIGN.md documents the result as exact or order-independent, the bits equal those of the
    0x00 run.

A family that reads a workspace region before writing it goes right on zeros and wrong on leavings; an OVERWRITE output
with an unwritten cell shows NaN / -1 under 0xFF; a write a little outside a buffer changes a canary.

Outputs that include/ssrs_hip.h documents as partly written, sliced by the existing checks that run here exactly as they
slice them in their own modules (under 0xFF the rest of such a buffer stays -1 / NaN, which nothing asserts):
  * ssrs_track_altitude: alt and traj_band, "the per-point ones are indexed like traj and written for the points
    [traj_offsets[0], traj_offsets[ntracks]) only" -- the lead points of a shifted buffer;
  * ssrs_track_flight_time: "dt is indexed like traj and written for [traj_offsets[0], traj_offsets[ntracks]) only";
  * ssrs_updraft_from_dem and its kin: "threshold < 0 -> `usable` is not written" (no tensor is allocated then).
Every other output here is OVERWRITTEN in full, or ACCUMULATED into a tensor its wrapper takes from torch.zeros."""
import numpy as np
import pytest
import torch

from dirty_memory import CANARY, GUARD, dirty

pytestmark = pytest.mark.gpu

FILLS = (0x00, 'leavings', 0xFF)
FILL_IDS = ('zeros', 'leavings', 'ones')
_CLEAN = {}                                  # family -> the outputs of its 0x00 run, computed once, read-only


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def same_bits(key, fill, arrays, clean):
    """The outputs of this fill are, byte for byte, those of the 0x00 run of the same case (clean(): that run, made here
    when the 0x00 parameter of the test has not run in this process)."""
    arrays = [np.ascontiguousarray(host(a)) for a in arrays]
    if fill == 0x00 or key not in _CLEAN:
        _CLEAN[key] = arrays if fill == 0x00 else [np.ascontiguousarray(host(a)) for a in clean()]
        for a in _CLEAN[key]:
            a.setflags(write=False)
    assert len(arrays) == len(_CLEAN[key])
    for k, (got, want) in enumerate(zip(arrays, _CLEAN[key])):
        assert got.dtype == want.dtype and got.shape == want.shape, (key, k)
        bad = got.view(np.uint8) != want.view(np.uint8)
        assert not bad.any(), f'{key} output {k}: {int(bad.sum())} bytes differ from the 0x00 run'


# ------------------------------------------------------------------------------------------------ the arena itself
def test_arena_sees_a_stray_device_write(gpu):
    """torch only: one element past a guarded device tensor, and one before another, written through the raw buffer."""
    with dirty(0xFF) as arena:
        a = torch.empty((5, 7), dtype=torch.float32, device=gpu)            # 140 bytes: the pad begins at byte 140
        b = torch.zeros(64, dtype=torch.int32, device=gpu)
        c = torch.empty(3, dtype=torch.float64)                             # host: not the arena's
        assert len(arena.buffers) == 2 and a.is_cuda and a.data_ptr() % 256 == 0 and b.data_ptr() % 256 == 0
        assert bool(a.isnan().all()) and bool((b == 0).all()) and not c.is_cuda
        arena.assert_clean()
        ra, rb = arena.buffers[0], arena.buffers[1]
        assert ra.raw.data_ptr() + ra.lead == a.data_ptr() and bool((ra.raw[:ra.lead] == CANARY).all())
        ra.raw[ra.lead + 140:ra.lead + 144].view(torch.float32).fill_(1.0)   # a[5, 0], were there a sixth row
        rb.raw[rb.lead - 4:rb.lead].view(torch.int32).fill_(7)               # b[-1]
        found = {v['shape']: v for v in arena.violations()}
        assert set(found) == {(5, 7), (64,)}
        assert found[(5, 7)]['offset'] == 140 and found[(5, 7)]['side'] == 'after'
        assert found[(5, 7)]['dtype'] == torch.float32 and found[(5, 7)]['changed_bytes'] == 4
        assert found[(64,)]['offset'] == -4 and found[(64,)]['side'] == 'before' and found[(64,)]['changed_bytes'] == 4
        with pytest.raises(AssertionError, match='writes outside a buffer'):
            arena.assert_clean()
    assert GUARD >= 64 * 1024


# ------------------------------------------------------------------------------------------------ the families
# A family is a list of thunks, each one case run through the library's Python entry point and judged by the checker the
# suite already has for it: the thunks call the existing test functions of the family's own module, whose references,
# tolerances and cases are thereby the ones in force -- nothing is restated here.  The arena replaces torch's factories
# globally, so the workspaces and outputs those functions allocate themselves (the C-ABI drivers of test_gpu_hist64.py,
# test_gpu_smooth.dev_smooth, ...) are dirty and guarded as well, each of exactly the size its query reported: the guard
# begins at the first byte past it.
def _raster(gpu, golden):
    import test_gpu_raster_edges as t
    return [lambda n=n: t.test_g14_every_entry_point(gpu, golden, n) for n in ('nodata', 'terraced')] + \
           [lambda n=n: t.test_slope_aspect_variants(gpu, golden, n) for n in ('nodata', 'terraced')] + \
           [lambda lat=lat: t.test_lattice_kernel_vs_independent_reference(gpu, golden, 'terraced', lat)
            for lat in ('cover', 'nx1', 'one')]


def _interp(gpu, golden):
    import g15_cases
    import test_gpu_interp_edges as t
    import test_gpu_wtk_thermals as w
    g15 = g15_cases.load()
    tiny = ('line_1x7', 'line_7x1', 'line_1x1', 'duplicates', 'one_triangle')
    return [lambda n=n: t.test_scalar_methods_on_tiny_geometries(gpu, n) for n in tiny] + \
           [lambda n=n: t.test_wind_methods_on_tiny_geometries(gpu, n) for n in tiny] + \
           [lambda m=m: w.test_fused_equals_the_chain_bit_for_bit(gpu, g15, 'C', m) for m in g15_cases.METHODS] + \
           [lambda m=m: w.test_fused_vs_the_reference_chain(gpu, g15, 'C', m) for m in g15_cases.METHODS]


def _thermal_case(name):
    """test_gpu_thermal_parity's three checks of one case, without its cached device tensors."""
    import test_gpu_thermal_parity as t
    import thermals_ref as ref
    from ssrs_amd import thermals
    _, shape, aspect_of, seeds = t.CASE[name]
    aspect = aspect_of(shape)
    fields = [thermals.thermal_seeds(aspect, ref.SCALE, seed) for seed in seeds]
    for seed, got, (want, hit) in zip(seeds, fields, t.ref_seed_fields(name)):
        t.check_seed_field(got, want, hit, (name, seed))
    for sigma in ref.sigmas_of(shape):
        chain = []
        for seed, x in zip(seeds, fields):
            t.check_blur(x, sigma, (name, seed))
            chain.append(thermals.gaussian_blur(x, sigma))
        f64 = thermals.compute_thermals_batch(aspect, ref.SCALE, seeds, sigma=sigma)
        f32 = thermals.compute_thermals_batch(aspect, ref.SCALE, seeds, dtype=torch.float32, sigma=sigma)
        for k, (values, _) in enumerate(t.ref_seed_fields(name)):
            assert t.same_bits(f64[k], chain[k]) and t.same_bits(f32[k], chain[k].astype(np.float32)), (name, sigma, k)
            want = ref.blur_kernel_order(values, sigma)
            assert (np.abs(f64[k] - want) <= t.RTOL_AMP * want + ref.bound(sigma, values)).all(), (name, sigma, k)


def _thermals(gpu, golden):
    import test_gpu_thermal_fields as f
    import thermals_ref as ref
    return [lambda n=n: _thermal_case(n) for n in ['%dx%d-flat' % shape for shape, _ in ref.TINY]] + \
           [lambda: f.test_more_realisations_than_one_launch_holds(gpu)]          # 40 seeds: two launches, one tensor


def _allen(gpu, golden):
    import allen_ref as ref
    import test_gpu_allen as t
    cases = {c['name']: c for c in ref.CASES}
    return [lambda n=n: t.test_field(gpu, cases[n]) for n in ('ragged', 'tiles', 'dense')]   # auto, lds, global each


def _shelter(gpu, golden):
    import test_gpu_shelter as t
    import test_gpu_shelter_sector as s
    return [lambda K=K: t.test_sx_uniform_wind_is_bit_identical(gpu, (20, 23), K) for K in (5, 50)] + \
           [lambda K=K: t.test_sx_per_cell_wind(gpu, (20, 23), K) for K in (5, 50)] + \
           [lambda: s.test_sector_uniform_wind(gpu, (33, 65), 6, 15., 5.),
            lambda: s.test_sector_per_cell_wind(gpu, (33, 65), 10., 2.5),
            lambda: t.test_improved_model_against_the_reference(gpu, 'nan'),
            lambda: s.test_sector_updraft(gpu)]


def _smooth(gpu, golden):
    import smooth_ref as ref
    import test_gpu_smooth as t
    names = ('3x5-s2', '1x7-s1.3', '33x65-s8', '150x140-s4.5-holes', '40x50-s40')     # the last: the global path
    return [lambda c=c: t.test_smoothing(gpu, *c) for c in ref.CASES if c[0] in names] + \
           [lambda: t.test_batch_of_3_equals_single_calls(gpu)]


def _warp(gpu, golden):
    import test_gpu_warp_dem as t
    return [lambda: t.test_inverse_gather_and_full_chain(gpu), lambda: t.test_overhang_is_nan_and_counted(gpu),
            lambda: t.test_outputs_may_be_left_out(gpu)]


def _tables(gpu, golden):
    import test_gpu_tables as t
    cases = [(recipe, shape, True) for shape in ((5, 5), (17, 65)) for recipe in ('benign', 'poison', 'half_way')]
    return [lambda f=f, c=c: f(gpu, c) for c in cases
            for f in (t.test_f64_table_is_the_oracles_weights, t.test_ring_table_records_and_zero_mask,
                      t.test_threshold_table_every_state, t.test_roam_tables_every_state)]


def _presence(gpu, golden):
    import test_gpu_presence_potential as t
    return [lambda: t.test_presence_counts_and_smoothing_vs_golden(gpu, golden),
            lambda: t.test_presence_smoothing_u64_counts_past_2_32(gpu, (37, 300)),
            lambda: t.test_presence_smoothing_u64_counts_past_2_32(gpu, (7, 9)),
            lambda: t.test_presence_c1_golden(gpu, golden)]                            # _normalise_add, _normalise_f32


def _turbines(gpu, golden):
    import test_gpu_turbines as t
    tracks, xy = t._synthetic()
    traj, off = t._pack(tracks)
    syn = dict(traj=traj, off=off, xy=xy, traj_dev=torch.from_numpy(traj).to(gpu), off_dev=torch.from_numpy(off).to(gpu))
    return [lambda: t.test_synthetic_trajectories_against_brute_force(syn, 70, 2.5),
            lambda: t.test_synthetic_trajectories_against_brute_force(syn, 33, 2.5),           # nturb = 1 mod 32
            lambda: t.test_unaligned_buffer_and_caller_bins(syn, gpu)]                          # the 4-byte shift


def _rotor(gpu, golden):
    import rotor_ref
    import test_gpu_rotor_encounters as e
    import test_gpu_rotor_time as r
    return [lambda c=c: e.test_cases_on_the_device(gpu, c) for c in rotor_ref.CASES] + \
           [lambda c=c: r.test_cases_on_the_device(gpu, c) for c in rotor_ref.CASES]


def _occupancy(gpu, golden):
    """The workspace of ssrs_track_occupancy must be ZERO on entry (include/ssrs_hip.h): flight.track_occupancy takes it
    from torch.zeros, which the arena leaves zero and guards; the existing test's 'left zero' assertion runs as it is."""
    import occupancy_ref as ref
    import test_gpu_occupancy as t
    return [lambda c=c: t.test_cases_on_the_device(gpu, c) for c in ref.CASES]


def _altitude(gpu, golden):
    """`alt` is written for the points of [off[0], off[n]) only (include/ssrs_hip.h, ssrs_track_altitude: "alt ... of the
    chunk's points"); the existing check slices it so, and so it does here."""
    import altitude_ref as ref
    import test_gpu_altitude as t
    return [lambda c=c: t.test_cases_on_the_device(gpu, c) for c in ref.CASES] + \
           [lambda d=d: t.test_cellinfo_on_the_device(gpu, d) for d in ((np.float32, np.float64), (np.float64, np.float32))]


def _flight_time(gpu, golden):
    import flight_time_ref as ref
    import test_gpu_flight_time as t
    return [lambda c=c: t.test_cases_on_the_device(gpu, c) for c in ref.CASES] + \
           [lambda: t.test_windinfo_on_the_device(gpu, np.float64, 'row_east')]


def _stepper_paths(names):
    def family(gpu, golden):
        import test_gpu_hist64 as t
        return [lambda n=n: t.test_preloaded_scratch_counts_exactly_on_every_path(gpu, n) for n in names]
    return family


def _tracks_recorded(gpu, golden):
    """The C1 golden tracks and the G7 trajectories with the recorder pool and ssrs_tracks_gather."""
    import test_gpu_tracks as t
    return [lambda: t.test_c1_golden_1000_tracks(gpu, golden),
            lambda: t.test_g7_reference_trajectories(gpu, golden, 'ff_m1', True),
            lambda: t.test_g7_reference_trajectories(gpu, golden, 'drw_m1', False)]


FAMILIES = {
    'raster': _raster, 'interp': _interp, 'thermals': _thermals, 'allen': _allen, 'shelter': _shelter, 'smooth': _smooth,
    'warp': _warp, 'tables': _tables, 'presence': _presence, 'turbines': _turbines, 'rotor': _rotor,
    'occupancy': _occupancy, 'altitude': _altitude, 'flight_time': _flight_time,
    'stepper_generic': _stepper_paths(('direct_f64', 'f64_table', 'ring_table')),
    'stepper_thr': _stepper_paths(('thr_no_block_window', 'thr_not_scattered', 'per_step_atomics', 'cached_control')),
    'stepper_scattered': _stepper_paths(('scattered_copies', 'scattered_no_copies')),
    'stepper_transposed': _stepper_paths(('east_front_transposed', 'west_front_transposed')),
    'tracks_recorded': _tracks_recorded,
}


@pytest.mark.parametrize('fill', FILLS, ids=FILL_IDS)
@pytest.mark.parametrize('family', list(FAMILIES))
def test_family_on_dirty_guarded_memory(gpu, golden, family, fill):
    """Every case of the family under its existing checker, guards clean.  'leavings': the family runs twice in one arena,
    and a case of the second pass inherits the buffers that the case before it dropped (another case's workspace and
    results, of any size that fits)."""
    from ssrs_amd import movmodel
    movmodel.release_workspaces()                 # the stepper's cached workspace: allocated inside the arena, dirty
    thunks = FAMILIES[family](gpu, golden)
    try:
        with dirty(fill) as arena:
            if fill == 'leavings':
                for thunk in thunks:
                    thunk()
                first_pass = len(arena.buffers) + arena.reused
            for thunk in thunks:
                thunk()
                arena.assert_clean()
            assert arena.buffers and not arena.passed, (len(arena.buffers), arena.passed)
            if fill == 'leavings' and (arena.reused or any(b.factory.startswith('empty') for b in arena.buffers)):
                # (a family whose wrappers allocate with zeros / full only -- turbines -- has nothing to inherit)
                assert arena.reused > 0, 'no buffer was handed out again: the second pass ran on fresh memory'
                print(f'{family}: {arena.reused} of {len(arena.buffers) + arena.reused} requests inherited a buffer '
                      f'({first_pass} in the first pass)')
    finally:
        movmodel.release_workspaces()


# ------------------------------------------------------------------------------------------------ bits of the 0x00 run
# The checkers of the integer scans (turbines, rotor, occupancy, altitude, flight time), of the presence counts, of the
# threshold / pair / fine tables and of the stepper (lengths, end cells, counts against the C oracle) are equalities with
# a reference: a dirty run that passes them has the bits of the 0x00 run.  The families below are judged within a bound,
# so their bits are compared here.  Each sums in a fixed order, whatever the launch order (include/ssrs_hip.h: "All paths
# give the same bits" for smooth and Allen, "bit for bit" for the thermal fields; the interpolators and the raster kernels
# evaluate a cell in one thread), so a difference from the 0x00 run can only come from memory the call did not write.
def _bits_smooth():
    import smooth_ref as ref
    from ssrs_amd import layers
    out = []
    for name, shape, sigma, holes in ref.CASES:
        if name in ('3x5-s2', '33x65-s8', '150x140-s4.5-holes', '40x50-s40'):
            out += list(layers.smooth_orograph(ref.case_input(shape, holes), sigma, threshold=ref.THRESHOLD, want_smooth=True))
    return out


def _bits_allen():
    import allen_ref as ref
    import test_gpu_allen as t
    cases = {c['name']: c for c in ref.CASES}
    return [a for n, path in (('ragged', 'auto'), ('ragged', 'global'), ('tiles', 'lds'), ('dense', 'auto'))
            for a in t.gpu_field(cases[n], path)[:3]]


def _bits_interp():
    import interp_ref as ir
    import test_gpu_interp_edges as t
    out = []
    for name in ('line_1x7', 'duplicates', 'one_triangle', 'overhang'):
        pts, rows, cols, cell = ir.CASES[name]
        vals = np.stack([ir.case_values(name, k) for k in range(3)])
        ws, wd = (np.stack(v) for v in zip(*(ir.sample_wind(pts, k) for k in range(3))))
        for method in t.METHODS:
            out.append(t._scalar(pts, vals, rows, cols, cell, method))
            out += list(t._wind(pts, ws, wd, rows, cols, cell, method))
    return out


def _bits_thermals():
    import thermals_ref as ref
    from ssrs_amd import thermals
    out = []
    for shape, seeds in ref.TINY:
        aspect = ref.flat_aspect(shape)
        out.append(thermals.compute_thermals_batch(aspect, ref.SCALE, seeds))
        out += [thermals.gaussian_blur(thermals.thermal_seeds(aspect, ref.SCALE, s), ref.SIGMA) for s in seeds]
    aspect = np.random.default_rng(2).uniform(0., 360., (150, 130))
    out.append(thermals.compute_thermals_batch(aspect, 2.0, list(range(100, 140))))
    return out


def _bits_tables():
    """The tables' documented contents: every f64 weight, the ring records and zero-mask bytes, the threshold table's
    header and eight planes.  The buffers hold more than that -- 8 bytes between the ring records and the mask and up to 3
    at the end (ssrs_transition_ring_bytes rounds to whole floats), the dwords between a threshold plane's last cell and
    the next plane at its power-of-two stride, the guard bands behind the header -- which no comment of the header promises
    and the builders need not write: on the (5, 5) ring table 11 of 1036 bytes kept the arena's 0xFF.  The stepper's
    results do not depend on them (the families above build their tables on 0xFF and match the oracle)."""
    import table_ref as tr
    from ssrs_amd import movmodel
    from ssrs_amd._device import to_dev
    out = []
    for shape in ((5, 5), (17, 65)):
        f = tr.field_ref('magnitudes', shape, True)
        upd, pot = to_dev(f.updraft, torch.float64), to_dev(f.potential, torch.float32)
        out.append(movmodel.build_transition_table(upd, pot))
        out += list(tr.ring_decode(movmodel.build_transition_table(upd, pot, ring=True).cpu().numpy(), *shape))
        header, planes = tr.thr_decode(movmodel.build_transition_table(upd, pot, thr=True, move_dirn=30.).cpu().numpy(), *shape)
        out += [np.frombuffer(header['magic'], dtype=np.uint8), np.array([header['rows'], header['cols']]), header['prior'],
                planes]
    return out


def _bits_raster():
    from conftest import load_golden
    import test_gpu_raster_edges as t
    from ssrs_amd import layers
    g = load_golden('g14_raster_edges.npz')
    z, res = g['nodata_dem'].astype(np.float64), float(g['res'])
    x, y, ws, wd = t.lattices('cover', z.shape[0], z.shape[1], res)
    return list(layers.slope_aspect(z, res)) + list(layers.updraft_from_dem(z, res, 7.5, 265., threshold=0.75)) + \
        list(layers.updraft_from_dem_lattice(z, res, x, y, ws, wd, threshold=0.75))


BITS = {'smooth': _bits_smooth, 'allen': _bits_allen, 'interp': _bits_interp, 'thermals': _bits_thermals,
        'tables': _bits_tables, 'raster': _bits_raster}


@pytest.mark.parametrize('fill', FILLS, ids=FILL_IDS)
@pytest.mark.parametrize('family', list(BITS))
def test_bits_equal_those_of_the_zero_filled_run(gpu, family, fill):
    with dirty(fill) as arena:
        if fill == 'leavings':
            BITS[family]()
        arrays = BITS[family]()
        arena.assert_clean()
        assert fill != 'leavings' or arena.reused > 0

    def clean():
        with dirty(0x00):
            return BITS[family]()
    same_bits(family, fill, arrays, clean)


# ------------------------------------------------------------------------------------------------ the potential solver
_POTENTIAL = {}                              # case.idx -> (inputs, the clean solve, whether a second clean solve had its bits)


def _potential_cases():
    import potential_cases as pc
    shapes = pc.SMALL_SHAPES + ((3, 250), (251, 3), (33, 31))                # small, odd and thin
    return [c for c in pc.QUIRK_CASES if (c.rows, c.cols) in shapes]


@pytest.mark.parametrize('fill', FILLS, ids=FILL_IDS)
def test_potential_solver_on_dirty_guarded_memory(gpu, golden, fill):
    """potential.solve_potential on the small, odd and thin shapes of potential_cases (one heading each), judged by
    check_field of test_gpu_potential_shapes.py.  At these sizes the wrapper's first-try reservation (1.1 KB per cell +
    96 MiB) is not below ssrs_potential_workspace_bytes, so the one workspace it allocates is the full bound, exactly.
    Repeatability is measured, not assumed: every case is first solved twice on ordinary memory; where those two agree
    bit for bit the dirty solve must have the same bits, otherwise check_field alone judges it.  The run prints which:
    on the MI355X all 11 cases repeated bit for bit, so every dirty solve here is held to the clean solve's bits."""
    import potential_cases as pc
    import test_gpu_potential_shapes as t
    g16 = golden('g16_potential_shapes.npz')
    cases = _potential_cases()
    for case in cases:
        if case.idx not in _POTENTIAL:
            d = pc.load_case(g16, case)
            d['system'] = pc.assemble(d['cond'], case.heading)
            a, b = t.run(case, d)[0], t.run(case, d)[0]
            _POTENTIAL[case.idx] = (d, a, np.array_equal(a.view(np.int32), b.view(np.int32)))
    print('potential: clean solves repeat bit for bit on', sum(r for _, _, r in _POTENTIAL.values()), 'of', len(cases), 'cases')
    with dirty(fill) as arena:
        for sweep in range(2 if fill == 'leavings' else 1):
            for case in cases:
                d, clean, repeats = _POTENTIAL[case.idx]
                pot, st = t.run(case, d)
                arena.assert_clean()
                assert st['converged'], (pc.case_id(case), st)
                t.check_field(case, d, pot, f' dirty {fill!r}')
                if repeats:
                    assert np.array_equal(pot.view(np.int32), clean.view(np.int32)), (pc.case_id(case), fill)
        assert arena.buffers and (fill != 'leavings' or arena.reused > 0)


# ------------------------------------------------------------------------------------------------ a stale stepper workspace
STALE_SHAPE, STALE_N = (9, 150), 9000        # the boundary-ring set-up of test_gpu_roam_feed.py: it roams within a few launches


def _stale_field(seed, n=STALE_N):
    rows, cols = STALE_SHAPE
    rng = np.random.default_rng(seed)
    upd = np.abs(rng.normal(0.8, 0.6, (rows, cols)))
    pot = (1000. * (1 - np.arange(rows)[:, None] / (rows - 1.)) + rng.normal(0, 30., (rows, cols))).astype(np.float32)
    ring_r = rng.choice([0, 1, rows - 2, rows - 1], STALE_N)
    ring_c = rng.choice([0, 1, cols - 2, cols - 1], STALE_N)
    on_row = rng.random(STALE_N) < 0.7
    starts = np.stack([np.where(on_row, ring_r, rng.integers(0, rows, STALE_N)),
                       np.where(on_row, rng.integers(0, cols, STALE_N), ring_c)], 1).astype(np.int32)
    return upd, pot, np.ascontiguousarray(starts[:n])


_STALE_REF = {}


def _stale_oracle(field, heading, n=STALE_N):
    from oracle import c_oracle
    if (field, heading, n) not in _STALE_REF:
        upd, pot, starts = _stale_field(field, n)
        _STALE_REF[field, heading, n] = c_oracle.simulate_tracks(heading, starts, STALE_SHAPE, 1, 1., upd, pot, seed=11,
                                                              want_traj=False)
    return _STALE_REF[field, heading, n]


def _stale_call(ws, field, heading, kind, flag=None, env=(), n=STALE_N):
    """One ssrs_tracks_simulate through the C ABI into the caller's workspace `ws`; lengths, end cells and counts must be
    the C oracle's.  Returns the call's SsrsTrackStats."""
    import ctypes as C
    import test_gpu_hist64 as th
    from ssrs_amd import movmodel, _native as nat
    upd, pot, starts = _stale_field(field, n)
    ref = _stale_oracle(field, heading, n)
    upd_t, pot_t, st_t = torch.from_numpy(upd).cuda(), torch.from_numpy(pot).cuda(), torch.from_numpy(starts).cuda()
    table = None if kind is None else movmodel.build_transition_table(
        upd_t, pot_t, ring=kind == 'ring', thr=kind == 'thr', move_dirn=heading if kind == 'thr' else None)
    p = movmodel.make_track_params(STALE_SHAPE, heading, 1, 1., steps_per_launch=16, ring=kind == 'ring', thr=kind == 'thr')
    p.flags |= getattr(nat, 'SSRS_TRACKS_' + flag) if flag else 0
    lengths = torch.empty(n, dtype=torch.int32, device='cuda')
    ends = torch.empty((n, 2), dtype=torch.int16, device='cuda')
    hist = torch.zeros(STALE_SHAPE, dtype=torch.int32, device='cuda')
    stats = nat.SsrsTrackStats()
    with th._Env(env):
        nat.check(nat.lib().ssrs_tracks_simulate(
            C.byref(p), nat.ptr(upd_t), nat.ptr(pot_t), nat.ptr(table), nat.ptr(st_t), C.c_int64(n), C.c_uint64(11),
            C.c_uint64(0), nat.ptr(hist), nat.ptr(ends), nat.ptr(lengths), None, None, nat.ptr(ws), C.c_size_t(ws.numel()),
            C.byref(stats), th._stream()))
    torch.cuda.synchronize()
    tag = (field, heading, kind, flag, env, n)
    assert np.array_equal(lengths.cpu().numpy(), ref['lengths']), tag
    assert np.array_equal(ends.cpu().numpy(), ref['ends']), tag
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), ref['hist']), tag
    print('stale', tag, 'launches', stats.launches, 'window', stats.window_launches, 'tile', stats.tile_launches,
          'block window', stats.block_window_launches, 'roam', stats.roam_launches)
    return stats


@pytest.mark.parametrize('fill', (0x00, 0xFF), ids=('zeros', 'ones'))
def test_stepper_inherits_the_workspace_of_another_call(gpu, fill):
    """ONE workspace of ssrs_tracks_workspace_bytes_ex(n, rows, cols, 64) bytes, guarded, never touched between the calls
    -- what movmodel._workspace hands Simulator from case to case.  Field A roams (pair and fine tables, private copies and
    wander windows are really written); field B of the SAME shape has another updraft and potential, so that A's tables sit
    at B's offsets and look valid.  Then the paths of test_gpu_hist64.CASES in the pairs block window -> scattered copies,
    scattered copies -> east front transposed, threshold -> ring -> direct.  Every call: the C oracle's lengths, end cells
    and counts."""
    from ssrs_amd import _native as nat
    rows, cols = STALE_SHAPE
    no_bw = ('SSRS_TRACKS_NO_BLOCK_WINDOW',)
    with dirty(fill) as arena:
        nb = int(nat.lib().ssrs_tracks_workspace_bytes_ex(STALE_N, rows, cols, 64))
        ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
        st = _stale_call(ws, 5, 0., 'thr', 'SCATTERED')                       # A: roams
        assert st.roam_launches > 0 and st.block_window_launches > 0, (st.roam_launches, st.block_window_launches)
        _stale_call(ws, 77, 0., 'thr', 'SCATTERED')                           # B, same shape, same switches
        st = _stale_call(ws, 5, 0., 'thr', 'SCATTERED', no_bw)                # block window -> scattered copies
        assert st.block_window_launches == 0
        _stale_call(ws, 77, 90., 'thr')                                       # scattered copies -> east front (transposed raster)
        _stale_call(ws, 5, 0., 'thr', None, no_bw)                            # threshold ...
        _stale_call(ws, 77, 0., 'ring')                                       # ... -> ring ...
        _stale_call(ws, 5, 0., None)                                          # ... -> direct
        arena.assert_clean()


@pytest.mark.parametrize('fill', (0x00, 0xFF), ids=('zeros', 'ones'))
def test_stepper_workspace_of_exactly_the_reported_size(gpu, fill):
    """ssrs_tracks_workspace_bytes and _ex to the byte, the guard at the first byte past them, for 8193 tracks: one above
    the step at which the eight lists grow by four blocks each (track_plan.h, list_cap), so the last list holds one track
    and every buffer sized by the slots has its longest unused tail; odd rows and cols (9 x 150 is no multiple of a
    window or a tile), 64 and 2 histogram copies.  The other *_workspace_bytes exports are called to the byte by the
    wrappers and C-ABI drivers of the families above (each passes exactly what its query reported), at shapes that are
    no multiple of their tiles: a lattice of 1 x 5 samples, owner rasters of 9 x 13 and 1 x 7 cells, blur and smooth on
    3 x 5, presence on 7 x 9 with krad 0 .. 12, Allen with 149 updrafts, occupancy on 1 x 40, the full potential bound."""
    from ssrs_amd import _native as nat
    rows, cols = STALE_SHAPE
    n = 8193
    lib = nat.lib()
    sizes = (int(lib.ssrs_tracks_workspace_bytes(n)), int(lib.ssrs_tracks_workspace_bytes_ex(n, rows, cols, 2)),
             int(lib.ssrs_tracks_workspace_bytes_ex(n, rows, cols, 64)))
    assert sizes[0] < sizes[1] < sizes[2]
    with dirty(fill) as arena:
        for nb in sizes:
            ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
            _stale_call(ws, 5, 0., 'thr', 'SCATTERED', n=n)
            _stale_call(ws, 77, 90., 'thr', n=n)
            _stale_call(ws, 5, 0., 'ring', n=n)
            arena.assert_clean()
            del ws
