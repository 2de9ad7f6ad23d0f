#!/usr/bin/env python3
"""G15 generator: runs the REFERENCE's physical thermal model (ssrs/layers.py: compute_potential_temperature :40-48,
deardoff_velocity_function :25-37, compute_thermal_updraft :51-60) in the build container, behind scipy's griddata as
ssrs/simulator.py:765-776 calls it, and stores inputs and outputs as tests/golden/g15_wtk_thermals.npz.  The fixture
is data; the reference's source never enters the repo and no test reads the reference.

How the reference is loaded: as in generate_g13_thermals.py, ssrs/layers.py is imported by file path after two
in-process shims (`numpy.int = int`, an empty `richdem` module).

Content
(i) sweep_*: a 1-D sweep of 4096 inputs for the three functions with the reference's outputs:
      sweep_pressure, sweep_temperature, sweep_blheight, sweep_flux, sweep_z (a per-element height)
      sweep_theta   = compute_potential_temperature(pressure, temperature)
      sweep_wstar   = deardoff_velocity_function(theta, blheight, flux)
      sweep_updraft = compute_thermal_updraft(sweep_z, wstar, blheight)
      sweep_updraft_z100 = compute_thermal_updraft(100., wstar, blheight)
    The first 64 entries are hand-placed special cases (q <= 0, zi < 100, zi <= 0, z = 0, z > zi, p <= 0, NaN in each
    argument); the rest are drawn from default_rng(150) over and somewhat beyond the physical ranges.
(ii) three geometries A, B, C (rows x cols, cell km, npts, seed: see GEOMETRIES), drawn as
      rng = default_rng(seed); x ~ U(-0.05 W, 1.04 W), y likewise with H, pressure ~ U(8e4, 9.5e4),
      temperature ~ U(-5, 30), blheight ~ U(20, 2500), surfheatflux ~ U(-100, 500); W, H = (cols - 1, rows - 1) * cell
    For each: <g>_shape (rows, cols), <g>_cell, <g>_x, <g>_y, <g>_layers (4, npts), and for each griddata method m
      <g>_<m>_updraft  (rows, cols) f32   griddata of the four layers -> the three functions at z = 100
      <g>_<m>_mask     (rows, cols) bool  sensitive cells: interpolated flux in (0, 1e-3), |blheight| < 1e-3 or
                                          |pressure| < 1 -- where rounding of the interpolation alone decides the result
    The generator asserts that a mask covers at most 1e-4 of the cells and that the pressure stays positive.

Usage:  python tests/golden/generate_g15_wtk_thermals.py [--out PATH]
Every draw comes from a seeded Generator: a rerun reproduces the arrays exactly.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
from scipy.interpolate import griddata

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/ssrs'
GEOMETRIES = (('A', 96, 128, 0.1, 60, 15), ('B', 37, 53, 0.25, 24, 16), ('C', 120, 150, 0.08, 150, 17))
METHODS = ('nearest', 'linear', 'cubic')
SWEEP, HEIGHT = 4096, 100.


def load_reference_layers():
    np.int = int                                                    # shim (i)
    sys.modules.setdefault('richdem', types.ModuleType('richdem'))  # shim (ii)
    spec = importlib.util.spec_from_file_location('ref_layers', os.path.join(REF, 'layers.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sweep_inputs():
    """(pressure, temperature, blheight, flux, z), SWEEP values each."""
    nan, inf = np.nan, np.inf
    #          pressure temperature blheight flux     z
    special = [(9e4,    15.,        800.,    0.,      100.),     # q = 0
               (9e4,    15.,        800.,    -50.,    100.),     # q < 0
               (9e4,    15.,        800.,    -0.,     100.),
               (9e4,    15.,        50.,     200.,    100.),     # zi < 100, z > zi
               (9e4,    15.,        99.999,  200.,    40.),
               (9e4,    15.,        100.,    200.,    100.),     # z = zi
               (9e4,    15.,        0.,      200.,    100.),     # zi = 0, z > 0
               (9e4,    15.,        0.,      200.,    0.),       # 0 / 0
               (9e4,    15.,        -0.,     200.,    100.),
               (9e4,    15.,        -300.,   200.,    100.),     # zi < 0
               (9e4,    15.,        800.,    200.,    0.),       # z = 0
               (9e4,    15.,        800.,    200.,    -20.),     # z < 0
               (9e4,    15.,        800.,    200.,    800.),     # z = zi
               (9e4,    15.,        800.,    200.,    2000.),    # z > zi
               (0.,     15.,        800.,    200.,    100.),     # p = 0
               (-0.,    15.,        800.,    200.,    100.),
               (-9e4,   15.,        800.,    200.,    100.),     # p < 0
               (-1.,    15.,        800.,    200.,    100.),
               (3e4,    15.,        800.,    200.,    100.),     # a low pressure
               (nan,    15.,        800.,    200.,    100.),     # NaN in each argument
               (9e4,    nan,        800.,    200.,    100.),
               (9e4,    15.,        nan,     200.,    100.),
               (9e4,    15.,        800.,    nan,     100.),
               (9e4,    15.,        800.,    200.,    nan),
               (nan,    nan,        nan,     nan,     nan),
               (9e4,    15.,        nan,     -5.,     100.),     # NaN beside a clipped argument
               (9e4,    15.,        50.,     nan,     100.),
               (inf,    15.,        800.,    200.,    100.),     # infinities
               (9e4,    inf,        800.,    200.,    100.),
               (9e4,    15.,        inf,     200.,    100.),
               (9e4,    15.,        800.,    inf,     100.),
               (9e4,    15.,        800.,    200.,    inf),
               (9e4,    -273.15,    800.,    200.,    100.),     # 0 K
               (9e4,    -300.,      800.,    200.,    100.),     # below 0 K: a negative base of the cube root
               (9e4,    15.,        800.,    1e-300,  100.),     # tiny positive flux
               (9e4,    15.,        800.,    1e-12,   100.),
               (9e4,    15.,        2500.,   500.,    100.),
               (1e5,    0.,         100.,    1.,      100.)]
    rng = np.random.default_rng(150)
    pad = 64 - len(special)
    assert pad >= 0
    special += [(9e4, 15., 800., 200., 100.)] * pad
    sp = np.asarray(special, dtype=np.float64).T
    n = SWEEP - 64
    pressure = rng.uniform(5e4, 1.1e5, n)
    temperature = rng.uniform(-40., 45., n)
    blheight = rng.uniform(-50., 3500., n)
    flux = rng.uniform(-200., 800., n)
    z = rng.uniform(-10., 3000., n)
    # a tenth of the random part close to the clipping points
    k = n // 10
    blheight[:k] = rng.uniform(95., 105., k)
    flux[k:2 * k] = rng.uniform(-1e-3, 1e-3, k)
    z[2 * k:3 * k] = blheight[2 * k:3 * k] * rng.uniform(0.99, 1.01, k)
    return [np.concatenate([sp[i], a]) for i, a in enumerate((pressure, temperature, blheight, flux, z))]


def geometry(rows, cols, cell, npts, seed):
    rng = np.random.default_rng(seed)
    w, h = (cols - 1) * cell, (rows - 1) * cell
    x = rng.uniform(-0.05 * w, 1.04 * w, npts)
    y = rng.uniform(-0.05 * h, 1.04 * h, npts)
    layers = np.stack([rng.uniform(8e4, 9.5e4, npts), rng.uniform(-5., 30., npts), rng.uniform(20., 2500., npts),
                       rng.uniform(-100., 500., npts)])
    return x, y, layers


def reference_chain(ly, x, y, layers, rows, cols, cell, method):
    """(updraft f64, sensitive mask, the four interpolated rasters) as the reference would compute them."""
    xm, ym = np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)
    pts = np.array([x, y]).T
    p, t, zi, q = (griddata(pts, v, (xm, ym), method=method) for v in layers)       # simulator.py:765-776
    theta = ly.compute_potential_temperature(p, t)
    wstar = ly.deardoff_velocity_function(theta, zi, q)
    updraft = ly.compute_thermal_updraft(HEIGHT, wstar, zi)
    with np.errstate(invalid='ignore'):
        mask = ((q > 0.) & (q < 1e-3)) | (np.abs(zi) < 1e-3) | (np.abs(p) < 1.)
    return updraft, mask, (p, t, zi, q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'g15_wtk_thermals.npz'))
    args = ap.parse_args()
    ly = load_reference_layers()
    out = {}
    with np.errstate(all='ignore'):
        p, t, zi, q, z = sweep_inputs()
        theta = ly.compute_potential_temperature(p, t)
        wstar = ly.deardoff_velocity_function(theta, zi, q)
        out.update(sweep_pressure=p, sweep_temperature=t, sweep_blheight=zi, sweep_flux=q, sweep_z=z, sweep_theta=theta,
                   sweep_wstar=wstar, sweep_updraft=ly.compute_thermal_updraft(z, wstar, zi),
                   sweep_updraft_z100=ly.compute_thermal_updraft(HEIGHT, wstar, zi))
    for name, rows, cols, cell, npts, seed in GEOMETRIES:
        x, y, layers = geometry(rows, cols, cell, npts, seed)
        out.update({f'{name}_shape': np.asarray([rows, cols], dtype=np.int32), f'{name}_cell': np.float64(cell),
                    f'{name}_x': x, f'{name}_y': y, f'{name}_layers': layers})
        for method in METHODS:
            with np.errstate(all='ignore'):
                updraft, mask, (pr, _, _, _) = reference_chain(ly, x, y, layers, rows, cols, cell, method)
            hull = np.isnan(updraft)
            assert mask.mean() <= 1e-4, (name, method, int(mask.sum()))
            assert np.nanmin(pr) > 0., (name, method, float(np.nanmin(pr)))
            assert method != 'nearest' or not hull.any()
            print(f'  {name} {method}: {int(mask.sum())} sensitive of {mask.size} cells, {int(hull.sum())} hull-NaN cells, '
                  f'updraft in [{np.nanmin(updraft):.3g}, {np.nanmax(updraft):.3g}]')
            out[f'{name}_{method}_updraft'] = updraft.astype(np.float32)
            out[f'{name}_{method}_mask'] = mask
    np.savez_compressed(args.out, **out)
    print(f'wrote {args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
