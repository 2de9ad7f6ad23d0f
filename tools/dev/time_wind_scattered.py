"""Scattered wind samples at BASELINE's size: a jittered 2 km lattice (31 x 26 points + margin) onto the 5000 x 6000
raster at 10 m -- ssrs_wind_from_triangles against scipy griddata (what the reference calls), seconds for each.
--method nearest | cubic times the other two griddata methods the same way (device kernels: one
`rocprofv3 --kernel-trace --stats` run of this script per method); --batch B interpolates B snapshots in one call,
--no-scipy leaves the host comparison out (it takes 6 - 26 s per snapshot)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd.wind import interpolate_wind_scattered, nearest_sample_index       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--method', default='linear', choices=('linear', 'nearest', 'cubic'))
ap.add_argument('--batch', type=int, default=1)
ap.add_argument('--no-scipy', action='store_true')
args = ap.parse_args()

rows, cols, cell = 5000, 6000, 0.01
rng = np.random.default_rng(1)
gx, gy = np.meshgrid(np.arange(-2., 63., 2.), np.arange(-2., 53., 2.))
x = (gx + rng.uniform(-0.3, 0.3, gx.shape)).ravel()
y = (gy + rng.uniform(-0.3, 0.3, gy.shape)).ravel()
ws = rng.uniform(2., 14., x.size)
wd = (270. + rng.normal(0., 40., x.size)) % 360.
if args.batch > 1:                                      # (snapshot 0 stays the one compared with scipy)
    ws = np.stack([ws] + [rng.uniform(2., 14., x.size) for _ in range(args.batch - 1)])
    wd = np.stack([wd] + [(270. + rng.normal(0., 40., x.size)) % 360. for _ in range(args.batch - 1)])
kw = {} if args.method == 'linear' else dict(method=args.method)
name = {'linear': 'ssrs_wind_from_triangles', 'nearest': 'ssrs_wind_nearest_index + ssrs_wind_from_nearest',
        'cubic': 'ssrs_wind_from_triangles_cubic'}[args.method]
what = '' if args.batch == 1 else f' x {args.batch} snapshots'
for rep in range(3):
    torch.cuda.synchronize(); t = time.time()
    s, d = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., **kw)
    torch.cuda.synchronize(); dt = time.time() - t
    host = 'host triangulation + copies included' if args.method != 'cubic' else 'host triangulation, gradients + copies included'
    print(f'{name}, {x.size} points -> {rows} x {cols}{what}: {dt * 1e3:.1f} ms ({host})', flush=True)
if args.method == 'nearest':
    torch.cuda.synchronize(); t = time.time()
    index = nearest_sample_index(x, y, (rows, cols), cell * 1000.)
    torch.cuda.synchronize(); dt_i = time.time() - t
    torch.cuda.synchronize(); t = time.time()
    s, d = interpolate_wind_scattered(x, y, ws, wd, (rows, cols), cell * 1000., method='nearest', index=index)
    torch.cuda.synchronize(); dt = time.time() - t
    print(f'  index raster alone (once per geometry): {dt_i * 1e3:.1f} ms; with it prebuilt{what}: {dt * 1e3:.1f} ms', flush=True)
if args.no_scipy:
    sys.exit(0)
if args.batch > 1:
    s, ws, wd = s[0], ws[0], wd[0]
from scipy.interpolate import griddata                     # noqa: E402
t = time.time()
xm, ym = np.meshgrid(np.arange(cols) * cell, np.arange(rows) * cell)
east = ws * np.sin(wd * np.pi / 180.); north = ws * np.cos(wd * np.pi / 180.)
pts = np.array([x, y]).T
ie = griddata(pts, east, (xm, ym), method=args.method); inn = griddata(pts, north, (xm, ym), method=args.method)
spd = np.sqrt(ie * ie + inn * inn)
print(f'scipy griddata (two components) + speed: {time.time() - t:.1f} s on one host core')
got = s.cpu().numpy()
print('max |speed - scipy|', float(np.nanmax(np.abs(got - spd))), 'NaN cells', int(np.isnan(got).sum()), int(np.isnan(spd).sum()))
