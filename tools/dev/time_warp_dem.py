"""K10 alone: ssrs_warp_lonlat_raster on a 5000 x 6000 destination at 10 m (ESRI:102008, the default southwest_lonlat)
from a synthetic 1/3 arc-second longitude / latitude source that just covers it (about 6500 x 8500 pixels).  HIP events
around `--reps` back-to-back launches on preallocated buffers, a warm-up first, the median of 5 such windows.  Variants
separate the inverse projection (lon / lat only, no source) from the gather, and f32 from f64.  The bytes column is what
the call must move: the source once and every output once; price it against tools/microbench/stream on the same
device.  --rows / --cols scale it down for a quick look; --out writes the markdown table.  Nothing asserts a time."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd import _native as nat              # noqa: E402
from ssrs_amd.georef import Projection           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=5000)
ap.add_argument('--cols', type=int, default=6000)
ap.add_argument('--res', type=float, default=10.)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--out', default=None)
args = ap.parse_args()

rows, cols, res = args.rows, args.cols, args.res
dev = torch.device('cuda', 0)
proj = Projection.from_crs('ESRI:102008')
west, south = (float(v) for v in proj.forward(-106.21, 42.78))
lon, lat = proj.inverse([west, west, west + (cols - 1) * res] * 2, [south, south + (rows - 1) * res] * 3)
step = 1. / 10800.
lon0, lat0 = (np.floor(lon.min() / step) - 2) * step, (np.floor(lat.min() / step) - 2) * step
nx, ny = int(np.ceil((lon.max() - lon0) / step)) + 3, int(np.ceil((lat.max() - lat0) / step)) + 3
jj = torch.arange(nx, device=dev, dtype=torch.float64)[None, :]
ii = torch.arange(ny, device=dev, dtype=torch.float64)[:, None]
src64 = 1500. + 300. * torch.sin(jj / 700.) * torch.cos(ii / 900.) + 40. * torch.sin(jj / 37. + ii / 53.)
del ii, jj
src32 = src64.to(torch.float32)
out = {torch.float32: torch.empty((rows, cols), dtype=torch.float32, device=dev),
       torch.float64: torch.empty((rows, cols), dtype=torch.float64, device=dev)}
lon_d, lat_d = (torch.empty((rows, cols), dtype=torch.float64, device=dev) for _ in range(2))
counter = torch.zeros(1, dtype=torch.int64, device=dev)
struct = proj.as_struct()
lib = nat.lib()
print(f'{rows} x {cols} cells at {res:g} m from a {ny} x {nx} source on {torch.cuda.get_device_name(0)}', flush=True)


def call(src, dst, want_lonlat):
    nat.check(lib.ssrs_warp_lonlat_raster(
        nat.ptr(src), nat.SSRS_F64 if src is not None and src.dtype == torch.float64 else nat.SSRS_F32, ny, nx,
        lon0, lat0, step, step, float('nan'), C.byref(struct), west, south, res, nat.ptr(dst),
        nat.SSRS_F64 if dst is not None and dst.dtype == torch.float64 else nat.SSRS_F32,
        nat.ptr(lon_d if want_lonlat else None), nat.ptr(lat_d if want_lonlat else None), nat.ptr(counter), rows, cols,
        C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def timed(fn):
    fn()                                                         # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.reps)
    return float(np.median(ms)), ms


ncell = rows * cols
variants = [
    ('f32 source -> f64 dst (the Simulator path)', src32, torch.float64, False),
    ('f32 source -> f32 dst', src32, torch.float32, False),
    ('f64 source -> f64 dst', src64, torch.float64, False),
    ('lon / lat only (the inverse projection, no source)', None, None, True),
    ('f32 source -> f64 dst + lon / lat', src32, torch.float64, True),
]
lines = ['| call | median ms per launch | Mcell / s | bytes moved, MB | windows (ms) |', '|---|---|---|---|---|']
for name, src, dtype, want in variants:
    dst = None if dtype is None else out[dtype]
    med, runs = timed(lambda: call(src, dst, want))
    moved = (0 if src is None else src.numel() * src.element_size()) + \
        (0 if dst is None else dst.numel() * dst.element_size()) + (2 * 8 * ncell if want else 0)
    lines.append(f'| {name} | {med:.3f} | {ncell / med / 1e3:.0f} | {moved / 1e6:.0f} | {", ".join(f"{m:.3f}" for m in runs)} |')
    print(lines[-1], flush=True)
assert int(counter.item()) == 0, 'the synthetic source does not cover the destination'
text = '\n'.join(lines)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
