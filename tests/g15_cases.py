"""Fixture G15 (tests/golden/g15_wtk_thermals.npz, written by tests/golden/generate_g15_wtk_thermals.py from the
reference's ssrs/layers.py behind scipy's griddata) unpacked for the tests: the sweep of the three physical functions
and the geometries A, B, C with the reference chain at z = 100 for griddata's three methods."""
import numpy as np

from conftest import load_golden

GEOMETRIES = ('A', 'B', 'C')
METHODS = ('nearest', 'linear', 'cubic')
HEIGHT = 100.
MASK_SHARE = 1e-4          # the share of cells a sensitive-cell mask may cover (the allowance of the hull-edge cells)


def load():
    return load_golden('g15_wtk_thermals.npz')


def geometry(g15, name):
    """(rows, cols, cell_km, x, y, layers (4, npts): pressure, temperature, blheight, surfheatflux)"""
    rows, cols = (int(v) for v in g15[f'{name}_shape'])
    return rows, cols, float(g15[f'{name}_cell']), g15[f'{name}_x'], g15[f'{name}_y'], g15[f'{name}_layers']


def griddata_layers(x, y, layers, rows, cols, cell, method):
    """The four layers on the raster's cell centres as the reference interpolates them (ssrs/simulator.py:765-776)."""
    from scipy.interpolate import griddata
    xm, ym = np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)
    pts = np.array([x, y]).T
    return np.stack([griddata(pts, v, (xm, ym), method=method) for v in layers])


def same_class(got, want):
    """NaN where NaN, +-inf where +-inf (same sign), finite where finite."""
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and
            np.array_equal(np.isneginf(got), np.isneginf(want)))
