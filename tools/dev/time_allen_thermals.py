"""K12 alone: ssrs_allen_thermal_field on the 5000 x 6000 raster at 10 m for the two updraft counts of the 60 x 50 km
region -- N = 38 994 (z = 100 m, zi = 1000 m) and N = 1 077 378 (zi = 150 m) -- on the LDS path (auto) and on the global
path, HIP events around the library call (table kernel + field kernel; updrafts and bins already on the device), a
warm-up and the median of 5 runs.  Beside each: the share of cells that left the LDS path (the workspace's counter).
--scale shrinks the raster's sides for a quick look."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd import _native as nat, thermals       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--scale', type=float, default=1.)
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

rows, cols, res = int(5000 * args.scale), int(6000 * args.scale), 10.
dev = torch.device('cuda', 0)
lib = nat.lib()


def timed(z, zi, wstar, path, dtype):
    sc = thermals.allen_scalars(z, zi, wstar, (rows, cols), res)
    n = sc['N']
    ups = thermals.allen_updrafts(n, (rows, cols), res, 12)
    start, items, bin_m, nbx, nby = thermals.allen_bins(ups[0], ups[1], (rows, cols), res)
    d = [torch.from_numpy(a).to(dev) for a in ups]
    d_start, d_items = torch.from_numpy(start).to(dev), torch.from_numpy(items).to(dev)
    out = torch.empty((rows, cols), dtype=dtype, device=dev)
    nbytes = lib.ssrs_allen_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = []
    for rep in range(6):                                         # the first is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        nat.check(lib.ssrs_allen_thermal_field(
            *(nat.ptr(t) for t in d), n, nat.ptr(d_start), nat.ptr(d_items), bin_m, nbx, nby, sc['rbar'], sc['wtbar'],
            sc['zzi'], int(sc['z_below_zi']), 0., res, rows, cols, nat.SSRS_ALLEN_PATH[path], nat.ptr(out),
            nat.SSRS_F32 if dtype == torch.float32 else nat.SSRS_F64, None, None, nat.ptr(ws), nbytes, stream))
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    left = int(ws[:8].view(torch.int64).item())
    return n, (bin_m, nbx, nby), float(np.median(ms[1:])), ms[1:], left / (rows * cols), float(out.double().abs().max())


lines = [f'{rows} x {cols} at {res:g} m, f32 out, {torch.cuda.get_device_name(0)}', '',
         '| N | zi (m) | bin (m), bins | path | median ms | runs (ms) | cells that left the LDS path | max abs w |',
         '|---|---|---|---|---|---|---|---|']
for zi in (1000., 150.):
    for path in ('auto', 'global'):
        n, (bin_m, nbx, nby), med, runs, share, top = timed(100., zi, 2., path, torch.float32)
        lines.append(f'| {n} | {zi:g} | {bin_m:.1f}, {nbx} x {nby} | {path} | {med:.3f} | {", ".join(f"{m:.3f}" for m in runs)} | '
                     f'{"-" if path == "global" else f"{100 * share:.2f} %"} | {top:.4f} |')
        print(lines[-1], flush=True)
text = '\n'.join(lines)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
