"""Thermal fields at 5000 x 6000, four realisations: (a) the two-stage chain ssrs_thermal_seeds +
ssrs_gaussian_blur per realisation (buffers and workspace allocated once, outside the timing)
against (b) one ssrs_thermal_fields call, count = 4, in f32 and in f64.  HIP events around each
leg after a warm-up of every leg, legs alternating, REPS repeats; prints median, min and max per
leg and whether (b) is slower than (a) beyond (a)'s own spread.  Outputs are compared bit for bit
first.  Numbers kept in profiles/thermals_fused.md."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from ssrs_amd import _native as nat
from ssrs_amd._device import stream_ptr

ROWS, COLS, COUNT, REPS = 5000, 6000, 4, 9
lib = nat.lib()
dev = torch.device('cuda', 0)
aspect = torch.from_numpy(np.random.default_rng(1).uniform(0., 360., (ROWS, COLS))).to(dev)
seeds = [1000 + k for k in range(COUNT)]
keys = (C.c_uint64 * COUNT)(*seeds)
seed_buf = torch.empty((ROWS, COLS), dtype=torch.float64, device=dev)
out_chain = torch.empty((COUNT, ROWS, COLS), dtype=torch.float64, device=dev)
out64 = torch.empty_like(out_chain)
out32 = torch.empty((COUNT, ROWS, COLS), dtype=torch.float32, device=dev)
nbytes = lib.ssrs_blur_workspace_bytes(ROWS, COLS, C.c_double(4.0))
ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)


def chain():
    for k in range(COUNT):
        nat.check(lib.ssrs_thermal_seeds(nat.ptr(aspect), C.c_double(2.0), C.c_uint64(seeds[k]), nat.ptr(seed_buf),
                                         ROWS, COLS, stream_ptr()))
        nat.check(lib.ssrs_gaussian_blur(nat.ptr(seed_buf), nat.ptr(out_chain[k]), C.c_double(4.0), ROWS, COLS,
                                         nat.ptr(ws), C.c_size_t(nbytes), stream_ptr()))


def fused(out, is_f32):
    nat.check(lib.ssrs_thermal_fields(nat.ptr(aspect), C.c_double(2.0), C.c_double(4.0), keys, COUNT, nat.ptr(out),
                                      is_f32, ROWS, COLS, stream_ptr()))


legs = {'chain f64 (a)': chain, 'fused f32 (b)': lambda: fused(out32, 1), 'fused f64 (b)': lambda: fused(out64, 0)}


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


for fn in legs.values():          # warm-up: code objects, every shape of the timed window
    fn(), fn()
torch.cuda.synchronize()
assert torch.equal(out64, out_chain) and torch.equal(out32, out_chain.to(torch.float32)), 'outputs differ'
print(f'{torch.cuda.get_device_name(0)}: {ROWS} x {COLS}, {COUNT} realisations, outputs bit-identical; '
      f'{int((out_chain[0] > 0).sum())} non-zero cells in field 0')
ms = {name: [] for name in legs}
for _ in range(REPS):
    for name, fn in legs.items():
        ms[name].append(timed(fn))
for name, v in ms.items():
    print(f'{name}: median {np.median(v):8.3f} ms   min {min(v):8.3f}   max {max(v):8.3f}   '
          f'({np.median(v) / COUNT:.3f} ms per realisation)')
a = ms['chain f64 (a)']
spread = max(a) - min(a)
for name in ('fused f32 (b)', 'fused f64 (b)'):
    slower = np.median(ms[name]) > np.median(a) + spread
    print(f'{name}: {np.median(a) / np.median(ms[name]):.2f}x the chain; spread of (a) {spread:.3f} ms -> '
          f'{"SLOWER than the chain" if slower else "not slower than the chain"}')
