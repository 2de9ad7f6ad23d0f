"""K17 alone: ssrs_track_passage over synthetic trajectory points on the 5000 x 6000 raster, HIP events, a warm-up and the
median of 5 runs, at radii of 0, 5 and 20 cells -- each next to K13 (ssrs_track_occupancy) on the same points in the same
run, THE YARDSTICK (no rate is promised for K17; the figure is its time over K13's), with stats[0] per point: the mask
words a set kernel tested, that is the L2 loads a point cost.
The two inputs of time_track_occupancy.py:
  short       40 000 tracks of 5000 points that cross the raster northwards, mostly self-avoiding: nearly every cell of
              every crescent is a first visit (a load, an atomicOr and an atomicAdd)
  loiter      40 tracks of --loiter-length points that go round four cells until the step cap.  The round is four
              DIFFERENT moves, two more than a lane remembers, so every move pays its crescent in loads that find the
              bit set
and one that shows what the memo is for:
  pingpong    40 tracks of the same length that alternate between two cells: two moves, both remembered
--points scales the size (default 2e8 points = 0.8 GB per input)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd import presence       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=2e8)
ap.add_argument('--loiter-length', type=float, default=5e6)
ap.add_argument('--planes', type=int, default=8)
ap.add_argument('--radii', type=int, nargs='+', default=[0, 5, 20], help='cells')
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

rows, cols = 5000, 6000
dev = torch.device('cuda', 0)
rng = np.random.default_rng(8)


def short_tracks(n, length=5000):
    j = torch.arange(length, device=dev)
    c0 = torch.from_numpy(rng.uniform(600., 5400., n)).to(dev)
    slope = torch.from_numpy(rng.uniform(-0.05, 0.05, n)).to(dev)
    traj = torch.empty((n, length, 2), dtype=torch.int16, device=dev)
    traj[:, :, 0] = j[None, :].clamp(0, rows - 1).to(torch.int16)
    traj[:, :, 1] = (c0[:, None] + slope[:, None] * j[None, :]).clamp(0, cols - 1).to(torch.int16)
    return traj.view(-1, 2), torch.arange(n + 1, dtype=torch.int64, device=dev) * length


def loiter_tracks(n, length, four=True):
    j = torch.arange(length, device=dev)
    traj = torch.empty((n, length, 2), dtype=torch.int16, device=dev)
    for k in range(n):
        r0, c0 = int(rng.integers(30, rows - 30)), int(rng.integers(30, cols - 30))
        traj[k, :, 0] = (r0 + (j & 1)).to(torch.int16)
        traj[k, :, 1] = (c0 + ((j >> 1) & 1) * int(four)).to(torch.int16)
    return traj.view(-1, 2), torch.arange(n + 1, dtype=torch.int64, device=dev) * length


def median_ms(fn):
    ms = []
    for rep in range(6):                                         # the first is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms[1:])), ms[1:]


occ_ws = presence.occupancy_workspace((rows, cols), args.planes)
pas_ws = presence.passage_workspace((rows, cols), args.planes)
lines = [f'{rows} x {cols}, {args.planes} planes, {torch.cuda.get_device_name(0)}', '',
         '| input | pass | median ms | G points/s | runs (ms) | over K13 | words tested per point |', '|---|---|---|---|---|---|---|']
len_loiter = int(args.loiter_length)
nloiter = max(int(args.points) // len_loiter, 2)
inputs = (('short', lambda: short_tracks(max(int(args.points) // 5000, 1))),
          ('loiter', lambda: loiter_tracks(nloiter, len_loiter)),
          ('pingpong', lambda: loiter_tracks(nloiter, len_loiter, four=False)))
for name, make in inputs:
    traj, off = make()
    n, total = off.numel() - 1, int(traj.shape[0])
    print(f'{name}: {total:.3e} points ({total * 4 / 1e9:.2f} GB) in {n} tracks', flush=True)
    counts = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)

    def passage(r2):
        return lambda: presence.compute_track_passage(traj, (rows, cols), r2, offsets=off, counts=counts, planes=args.planes,
                                                      workspace=pas_ws, stats=stats)
    passes = [('K13 occupancy', lambda: presence.compute_track_occupancy(traj, (rows, cols), offsets=off, counts=counts,
                                                                        planes=args.planes, workspace=occ_ws), None)]
    passes += [(f'K17 radius {r} (r2 = {r * r})', passage(r * r), r * r) for r in args.radii]
    base = None
    for what, fn, r2 in passes:
        stats.zero_()
        med, runs = median_ms(fn)
        base = med if base is None else base
        tested, won = (int(v) // 6 for v in stats.tolist())       # six equal runs
        per_point = '' if r2 is None else f'{tested / total:.3f}'
        lines.append(f'| {name}: {total:.2e} points, {n} tracks | {what} | {med:.3f} | {total / med / 1e6:.2f} | '
                     f'{", ".join(f"{m:.3f}" for m in runs)} | {med / base:.2f} | {per_point} |')
        print(lines[-1], flush=True)
    del traj, off, counts
text = '\n'.join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
