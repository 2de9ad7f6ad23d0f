#!/usr/bin/env python3
"""G14 generator: runs the REFERENCE's raster functions (ssrs/layers.py:11-22, :63-128,
:171-185) in the build container on the DEMs the smooth fixtures never contain -- plateaus
(interior cells with dz_dx == 0, where layers.py:124 substitutes 1e-10), ridges and nodata
(NaN) cells -- and stores inputs and results as tests/golden/g14_raster_edges.npz.  The
fixture is data; the reference's source never enters the repo and no test reads the reference.

How the reference is loaded: as in generate_golden.py, ssrs/layers.py is imported by file
path after two in-process shims (`numpy.int = int`, an empty `richdem` module).

Every vector is compared with oracle/ssrs_oracle.py while it is generated (slope, aspect and
orograph bit for bit, the usable updraft to rtol 1e-14), so a fixture can only be written by
an oracle that agrees with the reference on it.

Content: rasters of 97 x 161 cells at 30 m (97 = 3 x 32 + 1, 161 = 2 x 64 + 33: ragged
against the kernels' 32 x 64 tile on both axes), from base = synthetic_dem((97, 161), 30., 14):
  integer      rint(base)                                       int16
  terraced     floor(base / 5) * 5                              int16
  ridge_cols   row 48 of `integer` repeated over all rows       int16
  ridge_rows   column 80 of `integer` repeated over all columns int16
  nodata       `integer` with NaN in one interior cell, a 3 x 3 block, a corner cell and one
               cell of row 1 (NODATA_CELLS)                     float32 (exact)
The reference raises on an integer *dtype* DEM (np.nan into an int array): it is fed f64.
Per DEM `k`:
  k_dem, k_slope, k_aspect (f64)
  k_oro<j> (f32, the raster the Simulator saves) and k_use<j> (f64,
  get_above_threshold_speed(f32 orograph, THRESHOLD)) for case j of CASES
plus res, threshold, cases (5, 3) = (wspeed, wdirn, min_updraft_val), nodata_cells (12, 2).

Usage:  python tests/golden/generate_g14_raster_edges.py [--out PATH]
The archive is written with fixed member timestamps: a rerun reproduces it byte for byte.
"""
import argparse
import importlib.util
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
REF = '/root/reference/ssrs'
ROWS, COLS, RES, SEED, THRESHOLD = 97, 161, 30., 14, 0.75
# (wspeed, wdirn, min_updraft_val): 270 and 265 are the winds that tell the dz_dx == 0
# formula from the main one (the 1e-10 is visible only close to the ridge direction)
CASES = ((7.5, 0., 0.), (7.5, 270., 0.), (7.5, 265., 0.), (7.5, 45., 0.), (123.4, 123.4, 0.05))
NODATA_CELLS = [(40, 70)] + [(r, c) for r in (60, 61, 62) for c in (100, 101, 102)] + [(0, 0), (1, 120)]


def load_reference_layers():
    np.int = int                                                    # shim (i)
    sys.modules.setdefault('richdem', types.ModuleType('richdem'))  # shim (ii)
    spec = importlib.util.spec_from_file_location('ref_layers', os.path.join(REF, 'layers.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dems():
    from ssrs_amd.synthetic import synthetic_dem
    base = synthetic_dem((ROWS, COLS), RES, seed=SEED)
    integer = np.rint(base)
    nodata = integer.copy()
    for r, c in NODATA_CELLS:
        nodata[r, c] = np.nan
    out = {
        'integer': integer.astype(np.int16),
        'terraced': (np.floor(base / 5.) * 5.).astype(np.int16),
        'ridge_cols': np.repeat(integer[48:49], ROWS, axis=0).astype(np.int16),
        'ridge_rows': np.repeat(integer[:, 80:81], COLS, axis=1).astype(np.int16),
        'nodata': nodata.astype(np.float32),
    }
    assert np.array_equal(out['integer'], integer) and np.array_equal(out['nodata'], nodata, equal_nan=True)
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the current time)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asarray(a), allow_pickle=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'g14_raster_edges.npz'))
    args = ap.parse_args()
    ly = load_reference_layers()
    from oracle import ssrs_oracle as orc

    out = {'res': np.float64(RES), 'threshold': np.float64(THRESHOLD),
           'cases': np.asarray(CASES, dtype=np.float64),
           'nodata_cells': np.asarray(NODATA_CELLS, dtype=np.int16)}
    for name, dem in dems().items():
        z = dem.astype(np.float64)
        slope, aspect = ly.compute_slope_degrees(z, RES), ly.compute_aspect_degrees(z, RES)
        assert not np.isnan(slope).any() and not np.isnan(aspect).any()
        assert same_bits(orc.compute_slope_degrees(z, RES), slope), f'{name}: oracle slope differs'
        assert same_bits(orc.compute_aspect_degrees(z, RES), aspect), f'{name}: oracle aspect differs'
        out[f'{name}_dem'], out[f'{name}_slope'], out[f'{name}_aspect'] = dem, slope, aspect
        gx, gy = orc._horn_gradients(z, RES)
        share = float(((gx == 0) & (gy != 0)).mean())
        for j, (ws, wd, mn) in enumerate(CASES):
            # the reference's call shape: constant-filled wind rasters (simulator.py:194-195)
            oro = ly.compute_orographic_updraft(np.full_like(z, ws), np.full_like(z, wd), slope, aspect, mn)
            assert same_bits(orc.compute_orographic_updraft(ws, wd, slope, aspect, mn), oro), \
                f'{name} case {j}: oracle orograph differs'
            oro32 = oro.astype(np.float32)
            use = ly.get_above_threshold_speed(oro32, THRESHOLD)
            assert use.dtype == np.float64
            np.testing.assert_allclose(orc.get_above_threshold_speed(oro32, THRESHOLD), use, rtol=1e-14, atol=0)
            out[f'{name}_oro{j}'], out[f'{name}_use{j}'] = oro32, use
        print(f'  {name:10s} {str(dem.dtype):8s} dz_dx == 0 != dz_dy on {100 * share:5.2f} % of the interior', flush=True)
    save_deterministic(args.out, out)
    print(f'wrote {args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
