"""ssrs_potential_solve on the small, odd and thin rasters of fixture G16, against the exact solutions
of the reference's systems (tests/golden/generate_g16_potential_shapes.py): the ABI minimum 3 x 3, odd
rows and columns, the widths around the 62 columns of a wave and the 248 of a block of the fused
level-0 cycle, rasters three cells thin; every heading quadrant; nine media.  The gates are those the
suite already states elsewhere (potential_cases.gate); the measured figures of the first run are in
profiles/potential_shapes.md."""
import contextlib
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import potential_cases as pc

pytestmark = pytest.mark.gpu

LO, HI = -1e-3, 1000.001                      # the range bound of test_potential_two_phase_raster_iteration_budget


@pytest.fixture(scope='module')
def g16(golden):
    return golden('g16_potential_shapes.npz')


@contextlib.contextmanager
def switch(env, val):
    """One of the solver's environment switches, read at the start of every call."""
    os.environ[env] = val
    try:
        yield
    finally:
        del os.environ[env]


def run(case, d, max_iterations=3000, **kw):
    from ssrs_amd.potential import solve_potential
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')           # `converged` is asserted, not warned about
        pot, st = solve_potential(d['cond'], case.heading, max_iterations=max_iterations, return_stats=True, **kw)
    assert pot.dtype == np.float32 and pot.shape == (case.rows, case.cols)
    return pot, st


_COLD = {}


def cold(g16, case):
    """The solve at the library's defaults, once per case and left unchanged."""
    if case.idx not in _COLD:
        d = pc.load_case(g16, case)
        d['system'] = pc.assemble(d['cond'], case.heading)
        pot, st = run(case, d)
        pot.setflags(write=False)
        _COLD[case.idx] = (d, pot, st)
    return _COLD[case.idx]


def dirichlet_exact(case, d, pot):
    r, c = d['bnodes'] % case.rows, d['bnodes'] // case.rows
    return np.array_equal(pot[r, c].view(np.int32), d['benergy'].astype(np.float32).view(np.int32))


def check_field(case, d, pot, tag=''):
    """Items 2-4: distance from the exact solution, true residual, Dirichlet cells and range."""
    gate = pc.gate(case, d['ref_max_err'])
    err = float(np.abs(pot.astype(np.float64) - d['exact']).max())
    res = pc.relative_residual(d['system'], pot)
    figures = dict(err=err, gate=gate, share=pc.one_ulp_share(pot, d['exact']), res=res)
    print(f'G16{tag} | {pc.case_id(case)} | err {err:.2e} | gate {gate:.1e} | one-ulp {figures["share"]:.3f} | '
          f'res {res:.2e} | floor {d["floor_residual"]:.2e} | ref err {d["ref_max_err"]:.2e} | '
          f'ref one-ulp {pc.one_ulp_share(d["ref"], d["exact"]):.3f}')
    assert np.isfinite(pot).all()
    assert err <= gate, (pc.case_id(case), tag, err, gate)
    assert res <= pc.GATE_RESIDUAL, (pc.case_id(case), tag, res, d['floor_residual'])
    assert dirichlet_exact(case, d, pot), (pc.case_id(case), tag)
    assert pot.min() >= LO and pot.max() <= HI, (pc.case_id(case), tag, pot.min(), pot.max())
    return figures


@pytest.mark.parametrize('case', pc.CASES, ids=pc.case_id)
def test_potential_vs_exact(gpu, g16, case):
    """Converged at the defaults, within the gate of the exact solution, a true residual (computed on the
    CPU in f64 in the reference's system, not the solver's carried one) of at most 1e-5, Dirichlet cells
    bit for bit, values in range; the hierarchy's figures are sane."""
    d, pot, st = cold(g16, case)
    print(f'G16 stats | {pc.case_id(case)} | it {st["iterations"]} | levels {st["amg_levels"]} | '
          f'coarsest {st["amg_coarsest"]} | carried {st["residual"]:.1e} | converged {int(st["converged"])}')
    assert st['converged'], (pc.case_id(case), st)
    check_field(case, d, pot)
    assert st['amg_levels'] >= 1 and st['amg_coarsest'] >= 1, st
    assert 0 < st['workspace_used'] <= st['workspace_bytes'], st


@pytest.mark.parametrize('case', pc.QUIRK_CASES, ids=pc.case_id)
def test_fused_level0_is_bit_identical(gpu, g16, case):
    """The fused level-0 kernels (two raster rows per wave, 62 columns per wave, 248 per block) against the
    unfused ones on every shape: same bits, same iteration count; a second plain call as well."""
    d, pot, st = cold(g16, case)
    with switch('SSRS_AMG_NO_FUSE', '1'):
        unfused, st1 = run(case, d)
    again, st2 = run(case, d)
    assert st1['converged'] == st['converged'] and st1['iterations'] == st['iterations'], (st, st1)
    assert np.array_equal(unfused.view(np.int32), pot.view(np.int32))
    assert st2['iterations'] == st['iterations'] and np.array_equal(again.view(np.int32), pot.view(np.int32))


@pytest.mark.parametrize('env, val', [('SSRS_AMG_NU', '2,2'), ('SSRS_AMG_NO_BLOCKS', '1')])
@pytest.mark.parametrize('case', pc.QUIRK_CASES, ids=pc.case_id)
def test_other_cycles_reach_the_exact_solution(gpu, g16, case, env, val):
    """V(2,2) and the pairwise first level, each against the exact solution (not against each other)."""
    d, _, _ = cold(g16, case)
    with switch(env, val):
        pot, st = run(case, d)
    print(f'G16 {env}={val} stats | {pc.case_id(case)} | it {st["iterations"]} | levels {st["amg_levels"]} | '
          f'coarsest {st["amg_coarsest"]}')
    assert st['converged'], (env, st)
    check_field(case, d, pot, tag=f' {env}={val}')


GUESS_CASES = tuple(pc.find(r, c, m) for r, c in ((9, 62), (33, 31)) for m in ('speckle50', 'live'))


@pytest.mark.parametrize('case', GUESS_CASES, ids=pc.case_id)
def test_initial_guess_exact_and_garbage(gpu, g16, case):
    """initial_guess is part of the ABI: the exact solution as a guess costs no more iterations than the
    cold start; a guess of N(0, 1e6), wrong on the Dirichlet cells too, still converges to the same gates
    (the stop rule is on |b|, and the Dirichlet cells never take the guess)."""
    d, _, st = cold(g16, case)
    assert st['converged']
    warm, st_w = run(case, d, initial_guess=d['exact'])
    print(f'G16 guess | {pc.case_id(case)} | cold {st["iterations"]} | exact guess {st_w["iterations"]}')
    assert st_w['converged'] and st_w['iterations'] <= st['iterations'], (st, st_w)
    check_field(case, d, warm, tag=' guess=exact')
    garbage = np.random.default_rng(case.idx).normal(0., 1e6, (case.rows, case.cols))
    wild, st_g = run(case, d, initial_guess=garbage)
    print(f'G16 guess | {pc.case_id(case)} | garbage guess {st_g["iterations"]}')
    assert st_g['converged'], st_g
    check_field(case, d, wild, tag=' guess=garbage')


def test_abi_refusals_leave_the_output_alone(gpu, g16):
    """Host-side refusals: SSRS_ERR_INVALID, a message, and not a byte written to the output."""
    from ssrs_amd import _native as nat
    from ssrs_amd._device import to_dev, stream_ptr
    from ssrs_amd.potential import dirichlet_rasters
    L = nat.lib()
    assert L.ssrs_potential_workspace_bytes(0, 5) == 0
    rows = cols = 5
    cond = to_dev(np.ones((rows, cols)), torch.float64)
    mask_h, vals_h = dirichlet_rasters(0., (rows, cols))
    mask, vals = to_dev(mask_h), to_dev(vals_h)
    sentinel = -12345.5
    out = torch.full((rows, cols), sentinel, dtype=torch.float32, device='cuda')
    nbytes = L.ssrs_potential_workspace_bytes(rows, cols)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 256 == 0
    good = dict(cond=nat.ptr(cond), rows=rows, cols=cols, rel_tol=1e-15, max_iterations=100, ws=nat.ptr(ws))
    refusals = (('rows = 2', dict(rows=2)), ('cols = 2', dict(cols=2)), ('rel_tol = 0', dict(rel_tol=0.)),
                ('max_iterations = 0', dict(max_iterations=0)),
                ('workspace 128- but not 256-byte aligned', dict(ws=C.c_void_p(ws.data_ptr() + 128))),
                ('NULL conductivity', dict(cond=None)))
    for what, change in refusals:
        a = dict(good, **change)
        stats = nat.SsrsSolveStats()
        rc = L.ssrs_potential_solve(a['cond'], nat.ptr(mask), nat.ptr(vals), None, nat.ptr(out), a['rows'], a['cols'],
                                    C.c_double(a['rel_tol']), a['max_iterations'], 0, a['ws'], C.c_size_t(nbytes),
                                    C.byref(stats), stream_ptr())
        msg = L.ssrs_last_error()
        torch.cuda.synchronize()
        assert rc == nat.SSRS_ERR_INVALID, (what, rc)
        assert msg and b'ssrs_potential_solve' in msg, (what, msg)
        assert bool((out == sentinel).all().item()), what
    # and the unchanged arguments are accepted: the refusals above were each about their one change
    stats = nat.SsrsSolveStats()
    rc = L.ssrs_potential_solve(good['cond'], nat.ptr(mask), nat.ptr(vals), None, nat.ptr(out), rows, cols,
                                C.c_double(1e-15), 100, 0, good['ws'], C.c_size_t(nbytes), C.byref(stats), stream_ptr())
    torch.cuda.synchronize()
    assert rc == nat.SSRS_OK and stats.converged == 1
    ramp = 1000. * (1 - np.arange(rows)[:, None] / (rows - 1.)) * np.ones((1, cols))
    np.testing.assert_allclose(out.cpu().numpy(), ramp, rtol=0, atol=pc.GATE_SMOOTH)


def test_capped_solve_returns_a_usable_field(gpu, g16):
    """max_iterations = 5 on 33 x 31 speckle70: SSRS_OK with converged == 0, solve_potential warns, and the
    field is finite, exact on the Dirichlet cells and in range.  Regression test twice over: the solver used to
    give BiCGStab at least 50 iterations whatever the cap (15 iterations and converged == 1 here), and PCG's fifth
    iterate, 8.06 from the exact solution, reaches 1000.00275; a solve that does not converge now writes its
    iterate projected onto the range of the Dirichlet values."""
    from ssrs_amd import _native as nat
    from ssrs_amd._device import to_dev, stream_ptr
    from ssrs_amd.potential import solve_potential
    case = pc.find(33, 31, 'speckle70')
    d = pc.load_case(g16, case)
    cond = to_dev(d['cond'], torch.float64)
    mask_h = np.zeros((case.rows, case.cols), dtype=np.uint8)
    vals_h = np.zeros((case.rows, case.cols))
    mask_h[d['bnodes'] % case.rows, d['bnodes'] // case.rows] = 1
    vals_h[d['bnodes'] % case.rows, d['bnodes'] // case.rows] = d['benergy']
    mask, vals = to_dev(mask_h), to_dev(vals_h)
    out = torch.full((case.rows, case.cols), float('nan'), dtype=torch.float32, device='cuda')
    nbytes = nat.lib().ssrs_potential_workspace_bytes(case.rows, case.cols)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    stats = nat.SsrsSolveStats()
    rc = nat.lib().ssrs_potential_solve(nat.ptr(cond), nat.ptr(mask), nat.ptr(vals), None, nat.ptr(out), case.rows, case.cols,
                                        C.c_double(1e-15), 5, 0, nat.ptr(ws), C.c_size_t(nbytes), C.byref(stats), stream_ptr())
    torch.cuda.synchronize()
    assert rc == nat.SSRS_OK and stats.converged == 0, (rc, stats.converged, stats.iterations)
    with pytest.warns(UserWarning, match='potential solve stopped'):
        pot, st = solve_potential(d['cond'], case.heading, max_iterations=5, return_stats=True)
    assert not st['converged']
    raw = out.cpu().numpy()
    print(f'G16 capped | {pc.case_id(case)} | it {stats.iterations} / {st["iterations"]} | carried {st["residual"]:.1e} | '
          f'min {raw.min():.6g} | max {raw.max():.6g} | err {np.abs(raw - d["exact"]).max():.2e}')
    assert stats.iterations <= 5 and st['iterations'] <= 5
    for field in (raw, pot):
        assert np.isfinite(field).all()
        assert dirichlet_exact(case, d, field)
        assert field.min() >= LO and field.max() <= HI, (field.min(), field.max())
