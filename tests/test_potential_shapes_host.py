"""Host side of the potential solver on the small, odd and thin rasters of fixture G16 (reference
results; tests/golden/generate_g16_potential_shapes.py): the Dirichlet sets, the oracle, and the proof
that the fixture's yardstick tells the reference's east-edge weights from the natural ones."""
import numpy as np
import pytest

import potential_cases as pc


@pytest.fixture(scope='module')
def g16(golden):
    return golden('g16_potential_shapes.npz')


def test_case_table_and_media_are_the_fixtures(g16):
    assert len(g16['rows']) == len(pc.CASES) == 151
    assert {(c.rows, c.cols) for c in pc.CASES} == set(pc.SHAPES)
    for shape in pc.SMALL_SHAPES:
        assert [c.heading for c in pc.CASES if (c.rows, c.cols) == shape] == list(pc.HEADINGS)
    for shape in pc.LARGER_SHAPES:
        quadrants = {int(c.heading % 360 // 90) for c in pc.CASES if (c.rows, c.cols) == shape and c.heading % 90}
        assert quadrants == {0, 1, 2, 3}, shape
    for name in pc.MEDIA:
        uses = [c for c in pc.CASES if c.medium == name]
        assert len(uses) >= 8 and any((c.rows, c.cols) in pc.LARGER_SHAPES for c in uses), name
    for case in pc.CASES:
        d = pc.load_case(g16, case)                          # asserts shape, heading and medium
        assert g16[f'c{case.idx:03d}_cond'].dtype == np.float32 and d['exact'].dtype == np.float64
        assert np.array_equal(d['cond'], pc.medium(case)), pc.case_id(case)
        assert d['floor_residual'] < pc.GATE_RESIDUAL / 10 and np.isfinite(d['exact']).all()


def test_boundary_nodes_and_dirichlet_rasters_vs_reference(g16):
    """Every quadrant's slices and the midpoint split of the energies, at odd node counts too."""
    from ssrs_amd.potential import get_boundary_nodes, dirichlet_rasters
    odd = 0
    for case in pc.CASES:
        d = pc.load_case(g16, case)
        bn, be = get_boundary_nodes(case.heading, (case.rows, case.cols))
        assert np.array_equal(bn, d['bnodes']) and np.array_equal(be, d['benergy']), pc.case_id(case)
        odd += bn.size % 2
        mask, vals = dirichlet_rasters(case.heading, (case.rows, case.cols))
        want_mask = np.zeros((case.rows, case.cols), dtype=np.uint8)
        want_vals = np.zeros((case.rows, case.cols))
        want_mask[d['bnodes'] % case.rows, d['bnodes'] // case.rows] = 1
        want_vals[d['bnodes'] % case.rows, d['bnodes'] // case.rows] = d['benergy']
        assert mask.dtype == np.uint8 and np.array_equal(mask, want_mask), pc.case_id(case)
        assert np.array_equal(vals, want_vals), pc.case_id(case)
        assert int(mask.sum()) == bn.size                  # no node twice
    assert odd >= 10                                        # the split at size // 2 is exercised


def test_oracle_reproduces_reference_fields(g16):
    """The tolerance of generate_golden.g5_potential.  The fixture was made under NumPy >= 2, where a
    raster without any live pair is assembled in f32 (oracle.solve_potential: numpy2); on every other
    medium the oracle's default form, the one the device implements, holds the same tolerance."""
    from oracle import ssrs_oracle as orc
    for case in pc.CASES:
        d = pc.load_case(g16, case)
        np.testing.assert_allclose(orc.solve_potential(d['cond'], case.heading, numpy2=True), d['ref'],
                                   rtol=2e-6, atol=1e-4, err_msg=pc.case_id(case))
        if case.medium != 'alldead':
            np.testing.assert_allclose(orc.solve_potential(d['cond'], case.heading), d['ref'],
                                       rtol=2e-6, atol=1e-4, err_msg=pc.case_id(case))


def test_natural_weights_differ_on_the_east_column_only():
    from oracle import ssrs_oracle as orc
    for shape in pc.SHAPES:
        nrow, ncol = shape
        r, c, facs = orc.neighbour_lists(shape)
        r, c = r.astype(np.int64), c.astype(np.int64)
        differ = pc.natural_facs(shape) != facs
        assert differ.any(), shape
        # the S and the SW link of every interior node of the east column, nothing else
        assert np.all(r[differ] // nrow == ncol - 1) and np.all((r[differ] % nrow > 0) & (r[differ] % nrow < nrow - 1))
        assert np.all(c[differ] % nrow == r[differ] % nrow - 1)
        assert differ.sum() == 2 * (nrow - 2), shape


@pytest.mark.parametrize('case', pc.QUIRK_CASES, ids=pc.case_id)
def test_yardstick_separates_natural_east_edge_weights(g16, case):
    """The exact solution tells an operator without the reference's east-edge quirk from the right one
    by at least ten times the gate the device field is held to; the same solve with the reference's
    weights lies within the reference field's own error plus one f32 ulp (negative control)."""
    d = pc.load_case(g16, case)
    assert pc.shows_quirk(case, d['bnodes'])
    gate = pc.gate(case, d['ref_max_err'])
    natural = pc.solve(pc.assemble(d['cond'], case.heading, pc.natural_facs((case.rows, case.cols))))
    control = pc.solve(pc.assemble(d['cond'], case.heading))
    dist, ctl = np.abs(natural - d['exact']).max(), np.abs(control - d['exact']).max()
    print(f'{pc.case_id(case)}: natural weights {dist:.3e} from exact (gate {gate:.1e}), reference weights {ctl:.3e}')
    assert dist >= 10 * gate
    assert ctl <= d['ref_max_err'] + pc.ULP_RANGE


def test_every_shape_has_a_quirk_case():
    assert sorted((c.rows, c.cols) for c in pc.QUIRK_CASES) == sorted(pc.SHAPES)
    assert all(c.medium not in ('uniform', 'alldead') for c in pc.QUIRK_CASES)
