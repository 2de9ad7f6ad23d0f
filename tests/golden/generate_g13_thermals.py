#!/usr/bin/env python3
"""G13 generator: runs the REFERENCE's compute_thermals (ssrs/layers.py:188-214) in the
build container and stores what it drew and what it returned as tests/golden/g13_thermals.npz.
The fixture is data; the reference's source never enters the repo and no test reads the
reference.

How the reference is loaded: as in generate_golden.py, ssrs/layers.py is imported by file
path after two in-process shims (`numpy.int = int`, an empty `richdem` module).

How the seed field is learnt: `np.random.randint` and `np.random.lognormal` are wrapped *in
this process* by recorders that pass every call through to the legacy generator unchanged.
compute_thermals draws one randint per interior cell in row-major order, so the ordinal of a
randint call is the cell, and a lognormal call belongs to the cell of the randint before it.
`check_recording()` proves that the recorded field, blurred by scipy, is the returned field.

Content (200 x 240 raster, aspect = default_rng(13).uniform(0, 360), scale 2.0):
  aspect, thermal_intensity_scale, sigma
  band_counts   (256, 4) int32   seeded cells per run and aspect band b = min(int(|a-180|/45), 3)
  logamp        (N,) f64         log of every seeded amplitude, runs concatenated
  logamp_offsets (257,) int64    run s owns logamp[offsets[s]:offsets[s+1]]
  field_max, field_var (256,) f64  per run max and (population) variance of the returned field
  seed0_index (flat, int32), seed0_value (f64)   the recorded seed field of run 0, sparse
  field0        (200, 240) f64   the field the reference returned for run 0

Usage:  python tests/golden/generate_g13_thermals.py [--out PATH]
Legacy np.random.seed streams are deterministic: a rerun reproduces the arrays exactly.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/ssrs'
ROWS, COLS, SCALE, SIGMA, RUNS = 200, 240, 2.0, 4.0, 256


def load_reference_layers():
    np.int = int                                                    # shim (i)
    sys.modules.setdefault('richdem', types.ModuleType('richdem'))  # shim (ii)
    spec = importlib.util.spec_from_file_location('ref_layers', os.path.join(REF, 'layers.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class DrawRecorder:
    """Pass-through wrappers of the two legacy draws that remember what was drawn."""

    def __init__(self):
        self.randint, self.lognormal = np.random.randint, np.random.lognormal
        self.calls = 0
        self.cells, self.values = [], []

    def __enter__(self):
        def _randint(*a, **k):
            self.calls += 1
            return self.randint(*a, **k)

        def _lognormal(*a, **k):
            v = self.lognormal(*a, **k)
            self.cells.append(self.calls - 1)      # the cell of the randint just before
            self.values.append(v)
            return v
        np.random.randint, np.random.lognormal = _randint, _lognormal
        return self

    def __exit__(self, *exc):
        np.random.randint, np.random.lognormal = self.randint, self.lognormal


def reference_run(ly, aspect, s):
    """(flat indices, amplitudes, returned field) of the reference's run np.random.seed(s)."""
    rows, cols = aspect.shape
    by, bx = int(0.1 * rows), int(0.1 * cols)
    w = cols - 2 * bx
    np.random.seed(s)
    with DrawRecorder() as rec:
        field = ly.compute_thermals(aspect, SCALE)
    assert rec.calls == (rows - 2 * by) * w, rec.calls
    k = np.asarray(rec.cells, dtype=np.int64)
    flat = (by + k // w) * cols + (bx + k % w)
    return flat.astype(np.int32), np.asarray(rec.values, dtype=np.float64), field


def check_recording(shape, flat, values, field):
    seeds = np.zeros(shape)
    seeds.flat[flat] = values
    blurred = ndimage.gaussian_filter(seeds, sigma=SIGMA, mode='constant')
    assert np.array_equal(blurred, field), 'recorded seed field does not reproduce the reference output'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(HERE, 'g13_thermals.npz'))
    args = ap.parse_args()
    ly = load_reference_layers()
    aspect = np.random.default_rng(13).uniform(0, 360, (ROWS, COLS))
    band = np.minimum((np.abs(aspect - 180.) / 45.).astype(np.int64), 3).ravel()

    band_counts = np.zeros((RUNS, 4), dtype=np.int32)
    logamp, offsets = [], [0]
    field_max, field_var = np.zeros(RUNS), np.zeros(RUNS)
    keep = None
    for s in range(RUNS):
        flat, values, field = reference_run(ly, aspect, s)
        check_recording(aspect.shape, flat, values, field)
        band_counts[s] = np.bincount(band[flat], minlength=4)
        logamp.append(np.log(values))
        offsets.append(offsets[-1] + len(values))
        field_max[s], field_var[s] = field.max(), field.var()
        if s == 0:
            keep = (flat, values, field)
        if s % 32 == 31:
            print(f'  run {s + 1}/{RUNS}', flush=True)
    np.savez_compressed(args.out, aspect=aspect, thermal_intensity_scale=np.float64(SCALE),
                        sigma=np.float64(SIGMA), band_counts=band_counts,
                        logamp=np.concatenate(logamp), logamp_offsets=np.asarray(offsets, dtype=np.int64),
                        field_max=field_max, field_var=field_var,
                        seed0_index=keep[0], seed0_value=keep[1], field0=keep[2])
    print(f'wrote {args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
