"""K13 alone: ssrs_track_occupancy over synthetic trajectory points on the 5000 x 6000 raster, HIP events, a warm-up and
the median of 5 runs -- next to the two other passes over the same points, measured in the same run:
  occupancy   ssrs_track_occupancy, 8 planes, the workspace allocated once (presence.compute_track_occupancy)
  histogram   presence.compute_presence_counts: the plain visit histogram, one atomic per point.  THE YARDSTICK: no
              rate is promised for K13, the figure is its time over this one's
  encounters  ssrs_turbine_encounters against 500 turbines at 15 cells (K8: the streaming pass K13's layout is taken from)
Two inputs:
  short       tracks of 5000 points that cross the raster northwards, mostly self-avoiding: nearly every point is a
              first visit (a load, an atomicOr and an atomicAdd), and the clearing pass writes as many words again
  loiter      tracks of --loiter-length points that oscillate in four cells until the step cap, what a trap cell of a
              solved 10 m field does: every point but a handful finds its bit set (one L2 load)
--points scales the size (default 2e8 points = 0.8 GB per input)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd import presence, turbines as tb       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=2e8)
ap.add_argument('--loiter-length', type=float, default=5e6)
ap.add_argument('--planes', type=int, default=8)
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

rows, cols, nturb, radius = 5000, 6000, 500, 15.
dev = torch.device('cuda', 0)
rng = np.random.default_rng(8)
centres = np.stack([rng.uniform(800., 5200., 20), rng.uniform(500., 4500., 20)], 1)
xy = (centres[:, None, :] + rng.uniform(-150., 150., (20, 25, 2))).reshape(-1, 2)
xy_dev = torch.from_numpy(xy).to(dev)
bins = tuple(torch.from_numpy(b).to(dev) for b in tb.build_bins(xy, radius, (rows, cols)))


def short_tracks(n, length=5000):
    j = torch.arange(length, device=dev)
    c0 = torch.from_numpy(rng.uniform(600., 5400., n)).to(dev)
    slope = torch.from_numpy(rng.uniform(-0.05, 0.05, n)).to(dev)
    traj = torch.empty((n, length, 2), dtype=torch.int16, device=dev)
    traj[:, :, 0] = j[None, :].clamp(0, rows - 1).to(torch.int16)
    traj[:, :, 1] = (c0[:, None] + slope[:, None] * j[None, :]).clamp(0, cols - 1).to(torch.int16)
    return traj.view(-1, 2), torch.arange(n + 1, dtype=torch.int64, device=dev) * length


def loiter_tracks(n, length):
    j = torch.arange(length, device=dev)
    traj = torch.empty((n, length, 2), dtype=torch.int16, device=dev)
    for k in range(n):
        r0, c0 = int(rng.integers(0, rows - 1)), int(rng.integers(0, cols - 1))
        traj[k, :, 0] = (r0 + (j & 1)).to(torch.int16)
        traj[k, :, 1] = (c0 + ((j >> 1) & 1)).to(torch.int16)
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


workspace = presence.occupancy_workspace((rows, cols), args.planes)
lines = [f'{rows} x {cols}, {args.planes} planes, {torch.cuda.get_device_name(0)}', '',
         '| input | pass | median ms | G points/s | runs (ms) | over histogram |', '|---|---|---|---|---|---|']
len_loiter = int(args.loiter_length)
inputs = (('short', lambda: short_tracks(max(int(args.points) // 5000, 1))),
          ('loiter', lambda: loiter_tracks(max(int(args.points) // len_loiter, 2), len_loiter)))
for name, make in inputs:
    traj, off = make()
    n, total = off.numel() - 1, int(traj.shape[0])
    print(f'{name}: {total:.3e} points ({total * 4 / 1e9:.2f} GB) in {n} tracks', flush=True)
    counts = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
    hits = torch.zeros((n, (nturb + 31) // 32), dtype=torch.int32, device=dev)
    first = torch.full((n,), -1, dtype=torch.int32, device=dev)
    passes = (
        ('histogram', lambda: presence.compute_presence_counts(traj, (rows, cols))),
        ('occupancy', lambda: presence.compute_track_occupancy(traj, (rows, cols), offsets=off, counts=counts,
                                                               planes=args.planes, workspace=workspace)),
        ('encounters', lambda: tb.turbine_encounters(traj, off, xy_dev, radius, (rows, cols), bins=bins, hits=hits,
                                                     first_step=first)))
    base = None
    for what, fn in passes:
        med, runs = median_ms(fn)
        base = med if base is None else base
        lines.append(f'| {name}: {total:.2e} points, {n} tracks | {what} | {med:.3f} | {total / med / 1e6:.2f} | '
                     f'{", ".join(f"{m:.3f}" for m in runs)} | {med / base:.2f} |')
        print(lines[-1], flush=True)
    assert not bool(workspace.any()), 'the workspace is not zero after the calls'
    del traj, off, counts, hits, first
text = '\n'.join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
