#!/usr/bin/env python3
"""G16 generator: runs the REFERENCE's potential solve (ssrs/movmodel.py:21-128: boundary nodes,
assembly, SuperLU) in the build container on the rasters the other goldens never contain -- the ABI
minimum, odd rows and columns, widths around the 62 columns of a wave and the 248 of a block of the
fused level-0 cycle, rasters three cells thin -- over all heading quadrants and nine media, and stores
inputs and results as tests/golden/g16_potential_shapes.npz.  The fixture is data; the reference's
source never enters the repo and no test reads the reference.

How the reference is loaded: through generate_golden.py (by file path after the two in-process shims
`numpy.int = int` and an empty `richdem` module), whose reference_system and exact_potential give the
yardstick: the exact solution (SuperLU + extended-precision refinement) of the system with f64
dead-pair entries, the one ssrs_potential_solve solves (as in G12).

Every vector is compared with oracle/ssrs_oracle.py while it is generated (boundary nodes and energies
exactly, the field to rtol 2e-6 / atol 1e-4 as g5_potential does, the system of
tests/potential_cases.py:assemble entry for entry), so a fixture can only be written by an oracle
that agrees with the reference on it.  Conditions on the case table, asserted here:
  (a) every shape has a case on a non-uniform medium whose east column has free interior cells
      (potential_cases.QUIRK_HEADINGS names it: the case that shows the reference's east-edge quirk;
      tests/test_potential_shapes_host.py proves that it does -- free cells alone are not enough where the
      field is flat at the east end, as behind a dead row or far from the high boundary of a thin raster);
  (b) every case has a free node and |b| > 0;
  (c) exact_potential's refinement converges (its own max |dx| < 1e-6 assertion);
  every medium occurs at least eight times and on at least one of the larger shapes.

Content: the case table of tests/potential_cases.py as rows, cols, headings (f64), media (str), and
ref_max_err = max |f32 reference field - exact|, floor_residual = relative residual of the f32-rounded
exact solution in that system (no f32 field does better); per case `cNNN_`:
  cond (f32), bnodes (i8) and benergy (f64) of the reference, ref (f32, the reference's SuperLU field),
  exact_minus_ref (f32): the exact solution is f64(ref) + f64(exact_minus_ref) to 1e-8 (asserted), the
  form that keeps the archive under the size limit of a committed file (potential_cases.load_case).

Usage:  python tests/golden/generate_g16_potential_shapes.py [--out PATH]
The archive is written with fixed member timestamps: a rerun reproduces it byte for byte.
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

MAX_BYTES = 1 << 20          # the limit for a committed file (g8_c1.npz, the largest golden, has 1.29 MB)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'g16_potential_shapes.npz'))
    args = ap.parse_args()
    import generate_golden as gg
    from generate_g14_raster_edges import save_deterministic
    import potential_cases as pc
    from oracle import ssrs_oracle as orc

    out = {'rows': np.array([c.rows for c in pc.CASES], dtype=np.int32),
           'cols': np.array([c.cols for c in pc.CASES], dtype=np.int32),
           'headings': np.array([c.heading for c in pc.CASES], dtype=np.float64),
           'media': np.array([c.medium for c in pc.CASES])}
    ref_max_err, floor_residual = [], []
    quirk_shapes, failed = set(), []
    for case in pc.CASES:
        shape = (case.rows, case.cols)
        cond = pc.medium(case)
        cond32 = cond.astype(np.float32)
        assert np.array_equal(cond32.astype(np.float64), cond)
        model = gg.mm.MovModel(case.heading, shape)
        bn, be = model.get_boundary_nodes()
        ri, ci, fa = model.assemble_sparse_linear_system()
        ref = model.solve_sparse_linear_system(cond, bn, be, ri, ci, fa)
        assert ref.dtype == np.float32 and ref.shape == shape
        obn, obe = orc.get_boundary_nodes(case.heading, shape)
        assert np.array_equal(bn, obn) and np.array_equal(be, obe), f'{pc.case_id(case)}: oracle boundary differs'
        ori, oci, ofa = orc.neighbour_lists(shape)
        assert np.array_equal(ri, ori) and np.array_equal(ci, oci) and np.array_equal(fa, ofa)
        np.testing.assert_allclose(orc.solve_potential(cond, case.heading, numpy2=True), ref, rtol=2e-6, atol=1e-4)
        # the helper's system is the reference's with f64 dead-pair entries, entry for entry
        a_mat, b_vec, inodes, _, _ = gg.reference_system(cond, case.heading, numpy2=False)
        system = pc.assemble(cond, case.heading)
        assert np.array_equal(system.inodes, inodes) and np.array_equal(system.b, b_vec)
        assert (system.a != a_mat).nnz == 0, f'{pc.case_id(case)}: assembled system differs'
        assert inodes.size > 0 and np.linalg.norm(b_vec) > 0, f'{pc.case_id(case)}: condition (b)'
        with contextlib.redirect_stdout(io.StringIO()) as log:
            try:
                exact = gg.exact_potential(cond, case.heading, numpy2=False)          # condition (c)
            except AssertionError:
                sys.stderr.write(log.getvalue())
                failed.append(pc.case_id(case))
                print(f'  {pc.case_id(case):34s} condition (c): the refinement does not converge', flush=True)
                ref_max_err.append(np.nan)
                floor_residual.append(np.nan)
                continue
        if case in pc.QUIRK_CASES:
            assert pc.shows_quirk(case, bn), f'{pc.case_id(case)}: condition (a)'
            quirk_shapes.add(shape)
        k = f'c{case.idx:03d}_'
        out[k + 'cond'], out[k + 'bnodes'], out[k + 'benergy'] = cond32, bn, be
        # exact = f64(ref) + f64(exact_minus_ref): an f64 field does not deflate, this pair does
        diff = (exact - ref.astype(np.float64)).astype(np.float32)
        assert np.abs(ref.astype(np.float64) + diff - exact).max() <= 1e-8
        out[k + 'ref'], out[k + 'exact_minus_ref'] = ref, diff
        ref_max_err.append(np.abs(ref.astype(np.float64) - exact).max())
        floor_residual.append(pc.relative_residual(system, exact.astype(np.float32)))
        print(f'  {pc.case_id(case):34s} free {inodes.size:5d}  ref_max_err {ref_max_err[-1]:.2e}  '
              f'floor_residual {floor_residual[-1]:.2e}', flush=True)
    assert not failed, f'condition (c) fails on {failed}: give these slots another medium'
    assert quirk_shapes == set(pc.SHAPES), f'condition (a) fails on {set(pc.SHAPES) - quirk_shapes}'
    for name in pc.MEDIA:
        uses = [c for c in pc.CASES if c.medium == name]
        assert len(uses) >= 8 and any((c.rows, c.cols) in pc.LARGER_SHAPES for c in uses), name
    out['ref_max_err'] = np.array(ref_max_err)
    out['floor_residual'] = np.array(floor_residual)
    save_deterministic(args.out, out)
    size = os.path.getsize(args.out)
    print(f'wrote {args.out}: {len(pc.CASES)} cases, {size / 1024:.1f} KiB; worst ref_max_err '
          f'{max(ref_max_err):.2e}, worst floor_residual {max(floor_residual):.2e}')
    assert size <= MAX_BYTES, 'archive too large for a committed file'


if __name__ == '__main__':
    main()
