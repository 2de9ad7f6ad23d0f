"""The sector-averaged Sx of K9 alone: layers.compute_sx(..., sector=15, sector_step=5) (one fused call,
ssrs_shelter_sx_sector: M = 7 rays on one staging of the tile) on the 5000 x 6000 synthetic DEM at 10 m with dmax = 500 m
(K = 50: 1.05e10 bilinear samples), next to the unfused route of the same tree: M calls of compute_sx, one per azimuth,
and the mean of the M rasters on the device.  Uniform wind from 237.3 degrees and per-cell wind; HIP events, a warm-up and
the median of 5 runs.  The two routes are compared once before they are timed.  --rows / --cols / --dmax / --sector /
--step scale it; --out writes the markdown table as well.  Nothing asserts a time."""
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
ap.add_argument('--sector', type=float, default=15.)
ap.add_argument('--step', type=float, default=5.)
ap.add_argument('--out', default=None)
args = ap.parse_args()

rows, cols, res, dmax = args.rows, args.cols, args.res, args.dmax
K = int(np.floor(dmax / res))
H, M = layers.sector_rays(args.sector, args.step)
dev = torch.device('cuda', 0)
dem = torch.from_numpy(synthetic_dem((rows, cols), res)).to(dev)
r, c = torch.meshgrid(torch.arange(rows, device=dev, dtype=torch.float64),
                      torch.arange(cols, device=dev, dtype=torch.float64), indexing='ij')
wd = 200. + 110. * torch.sin(c / 1900. + r / 2900.)
del r, c
print(f'{rows} x {cols} cells at {res:g} m, dmax {dmax:g} m, sector +-{args.sector:g} in steps of {args.step:g}: K = {K}, '
      f'M = {M}, {rows * cols * K * M:.3e} samples per case on {torch.cuda.get_device_name(0)}', flush=True)


def fused(wdirn, path='auto'):
    return layers.compute_sx(dem, res, wdirn, dmax=dmax, sector=args.sector, sector_step=args.step, path=path)


def unfused(wdirn):
    acc = torch.zeros((rows, cols), dtype=torch.float64, device=dev)
    for m in range(M):
        acc += layers.compute_sx(dem, res, wdirn + float(m - H) * args.step, dmax=dmax)
    return acc / float(M)


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


for name, wdirn in (('uniform 237.3', 237.3), ('per-cell wind', wd)):
    diff = float((fused(wdirn) - unfused(wdirn)).abs().max())
    print(f'{name}: largest |fused - mean of {M} calls| = {diff:.3e} degrees', flush=True)

variants = [
    ('fused, uniform 237.3', lambda: fused(237.3)),
    (f'{M} x compute_sx + mean, uniform 237.3', lambda: unfused(237.3)),
    ('fused, uniform 237.3, global path', lambda: fused(237.3, 'global')),
    ('fused, per-cell wind', lambda: fused(wd)),
    (f'{M} x compute_sx + mean, per-cell wind', lambda: unfused(wd)),
    ('fused, per-cell wind, global path', lambda: fused(wd, 'global')),
]
lines = ['| call | median ms | samples / s | runs (ms) |', '|---|---|---|---|']
for name, fn in variants:
    try:
        med, runs = timed(fn)
    except ValueError as exc:                                    # e.g. a forced path that does not fit
        lines.append(f'| {name} | - | - | {exc} |')
        continue
    lines.append(f'| {name} | {med:.3f} | {rows * cols * K * M / med / 1e-3:.3e} | {", ".join(f"{m:.3f}" for m in runs)} |')
    print(lines[-1], flush=True)
text = '\n'.join(lines)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
