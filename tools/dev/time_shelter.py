"""K9 alone: ssrs_shelter_sx and ssrs_updraft_sheltered on the 5000 x 6000 synthetic DEM at 10 m with dmax = 500 m
(K = 50: 1.5e9 bilinear samples), HIP events, a warm-up and the median of 5 runs, next to updraft_from_dem (K1) on the
same raster on the same box.  Uniform wind from 237.3 degrees (a general direction: four neighbours per sample) and from
270 (an axis wind: one), per-cell wind, and the LDS path against the global one.  --rows / --cols / --dmax scale it
down for a quick look; --out writes the markdown table as well.  Nothing asserts a time."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd import layers                      # noqa: E402
from ssrs_amd.synthetic import synthetic_dem     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=5000)
ap.add_argument('--cols', type=int, default=6000)
ap.add_argument('--res', type=float, default=10.)
ap.add_argument('--dmax', type=float, default=500.)
ap.add_argument('--out', default=None)
args = ap.parse_args()

rows, cols, res, dmax = args.rows, args.cols, args.res, args.dmax
K = int(np.floor(dmax / res))
dev = torch.device('cuda', 0)
dem = torch.from_numpy(synthetic_dem((rows, cols), res)).to(dev)
r, c = torch.meshgrid(torch.arange(rows, device=dev, dtype=torch.float64),
                      torch.arange(cols, device=dev, dtype=torch.float64), indexing='ij')
wd = 200. + 110. * torch.sin(c / 1900. + r / 2900.)
ws = 8. + 3. * torch.sin(c / 1700.) * torch.cos(r / 1300.)
del r, c
print(f'{rows} x {cols} cells at {res:g} m, dmax {dmax:g} m: K = {K}, {rows * cols * K:.3e} samples per case '
      f'on {torch.cuda.get_device_name(0)}', flush=True)


def timed(fn):
    ms = []
    for rep in range(6):                                         # the first is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms[1:])), ms[1:]


variants = [
    ('updraft_from_dem (K1), 237.3', lambda: layers.updraft_from_dem(dem, res, 10., 237.3, threshold=0.75)),
    ('compute_sx, uniform 237.3', lambda: layers.compute_sx(dem, res, 237.3, dmax=dmax)),
    ('compute_sx, uniform 270', lambda: layers.compute_sx(dem, res, 270., dmax=dmax)),
    ('compute_sx, uniform 237.3, global path', lambda: layers.compute_sx(dem, res, 237.3, dmax=dmax, path='global')),
    ('compute_sx, per-cell wind', lambda: layers.compute_sx(dem, res, wd, dmax=dmax)),
    ('compute_sx, per-cell wind, global path', lambda: layers.compute_sx(dem, res, wd, dmax=dmax, path='global')),
    ('orographic_updraft_improved, uniform 237.3',
     lambda: layers.orographic_updraft_improved(dem, res, 10., 237.3, dmax=dmax, threshold=0.75, want_sx=True)),
    ('orographic_updraft_improved, per-cell wind',
     lambda: layers.orographic_updraft_improved(dem, res, ws, wd, dmax=dmax, threshold=0.75, want_sx=True)),
]
lines = ['| call | median ms | samples / s | runs (ms) |', '|---|---|---|---|']
for name, fn in variants:
    try:
        med, runs = timed(fn)
    except ValueError as exc:                                    # e.g. a forced path that does not fit
        lines.append(f'| {name} | - | - | {exc} |')
        continue
    rate = '' if 'K1' in name else f'{rows * cols * K / med / 1e-3:.3e}'
    lines.append(f'| {name} | {med:.3f} | {rate} | {", ".join(f"{m:.3f}" for m in runs)} |')
    print(lines[-1], flush=True)
text = '\n'.join(lines)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
