"""The Gaussian smoothing of K11 alone: ssrs_smooth_reflect (f32 in; smooth f64 is not asked for, so 4 B read and 8 B
written by the first pass, 8 B read and 4 B written by the second: 24 B per cell) on a 5000 x 6000 raster with sigma 8
and 30 cells (R = 32 and 120) and batches of 1 and 8, next to the chain the tree had before it: ssrs_gaussian_blur on an
f64 copy of the same raster, same sigma, one call per case back to back.  That chain does strictly less (zero padding,
no clamp, no threshold function).  HIP events, a warm-up and the median of 5 runs, the two alternating.  The interior of
the two results is compared once before they are timed.  --rows / --cols / --sigmas / --batches scale it; --out writes the
markdown table as well.  Nothing asserts a time."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd import _native as nat              # noqa: E402
from ssrs_amd._device import stream_ptr          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=5000)
ap.add_argument('--cols', type=int, default=6000)
ap.add_argument('--sigmas', type=float, nargs='+', default=[8., 30.])
ap.add_argument('--batches', type=int, nargs='+', default=[1, 8])
ap.add_argument('--out', default=None)
args = ap.parse_args()

rows, cols = args.rows, args.cols
dev = torch.device('cuda', 0)
lib = nat.lib()
nmax = max(args.batches)
r, c = torch.meshgrid(torch.arange(rows, device=dev, dtype=torch.float64),
                      torch.arange(cols, device=dev, dtype=torch.float64), indexing='ij')
x64 = torch.stack([1.9 * torch.sin(r / 33. + b) * torch.cos(c / 41.) + 0.8 * torch.sin((r + 2. * c) / 27.) - 0.3 for b in range(nmax)])
del r, c
x32 = x64.to(torch.float32)
x64 = x32.to(torch.float64)
oro = torch.empty_like(x32)
use = torch.empty_like(x64)
old = torch.empty_like(x64)
print(f'{rows} x {cols} cells on {torch.cuda.get_device_name(0)}', flush=True)


def new_call(sigma, batch, path='auto', want_usable=True):
    nbytes = lib.ssrs_smooth_workspace_bytes(rows, cols, batch, sigma)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def fn():
        nat.check(lib.ssrs_smooth_reflect(nat.ptr(x32), sigma, nat.SSRS_SMOOTH_PATH[path], 0., 0.75, None, nat.ptr(oro),
                                          nat.ptr(use) if want_usable else None, rows, cols, batch, nat.ptr(work), nbytes,
                                          stream_ptr()))
    return fn


def old_call(sigma, batch):
    nbytes = lib.ssrs_blur_workspace_bytes(rows, cols, sigma)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def fn():
        for b in range(batch):
            nat.check(lib.ssrs_gaussian_blur(nat.ptr(x64[b]), nat.ptr(old[b]), C.c_double(sigma), rows, cols, nat.ptr(work),
                                             C.c_size_t(nbytes), stream_ptr()))
    return fn


def timed(fns):
    """Median ms of 5 runs of each, alternating, after one warm-up round."""
    ms = [[] for _ in fns]
    for rep in range(6):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if rep:
                ms[i].append(a.elapsed_time(b))
    return [(float(np.median(m)), m) for m in ms]


lines = ['| sigma (R) | batch | call | median ms | GB/s of the 24 B per cell | runs (ms) |', '|---|---|---|---|---|---|']
for sigma in args.sigmas:
    R = int(4. * sigma + 0.5)
    # once: away from the edges (where the old chain pads with zeros) the two are the same blur of the same values
    smooth = torch.empty_like(x64[:1])
    nbytes = lib.ssrs_smooth_workspace_bytes(rows, cols, 1, sigma)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nat.check(lib.ssrs_smooth_reflect(nat.ptr(x32), sigma, 0, 0., 0.75, nat.ptr(smooth), None, None, rows, cols, 1,
                                      nat.ptr(work), nbytes, stream_ptr()))
    old_call(sigma, 1)()
    torch.cuda.synchronize()
    if rows > 2 * R and cols > 2 * R:
        diff = float((smooth[0, R:rows - R, R:cols - R] - old[0, R:rows - R, R:cols - R]).abs().max())
        print(f'sigma {sigma:g}: largest interior |new - old| = {diff:.3e}', flush=True)
    del smooth, work
    for batch in args.batches:
        calls = [('ssrs_smooth_reflect, orograph + usable', new_call(sigma, batch)),
                 ('ssrs_smooth_reflect, orograph only', new_call(sigma, batch, want_usable=False)),
                 ('ssrs_smooth_reflect, global path', new_call(sigma, batch, 'global')),
                 ('ssrs_gaussian_blur on f64', old_call(sigma, batch))]
        for (name, _), (med, runs) in zip(calls, timed([fn for _, fn in calls])):
            lines.append(f'| {sigma:g} ({R}) | {batch} | {name} | {med:.3f} | {24. * rows * cols * batch / med / 1e6:.0f} | '
                         f'{", ".join(f"{m:.3f}" for m in runs)} |')
            print(lines[-1], flush=True)
text = '\n'.join(lines)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
