"""K14 alone: ssrs_track_altitude (its three launches and the read-back of two offsets) over synthetic trajectories of the
contract's shape -- --points points (default 1e8), half of them in tracks of 5000 points that cross the 5000 x 6000 raster
northwards, half in tracks of --long-length points (default 7.5e6: the step cap of a 10 m run) that wander with king's
moves -- HIP events, a warm-up and the median of 5 runs, for each set of per-point outputs:
  rasters    band_hist and the per-track rows only (what Simulator asks for without turbines): 8 B/point algorithmic
  + masked   traj_band as well (Simulator with turbine_encounter_radius > 0): 12 B/point
  + alt      alt and traj_band: 16 B/point
Algorithmic bytes: traj is read by the "ops" and by the "emit" launch, 4 B each; alt and traj_band are
4 B written each; the cellinfo gathers (two 8-byte loads a point and launch, neighbours in the raster) and the atomics are
left out.  The yardstick is tools/microbench/stream on buffers of the same size, run next to it."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd import flight       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=1e8)
ap.add_argument('--long-length', type=float, default=7.5e6)
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

rows, cols = 5000, 6000
dev = torch.device('cuda', 0)
rng = np.random.default_rng(14)
gen = torch.Generator(device=dev).manual_seed(14)


def short_tracks(n, length=5000):
    j = torch.arange(length, device=dev)
    c0 = torch.from_numpy(rng.uniform(600., 5400., n)).to(dev)
    slope = torch.from_numpy(rng.uniform(-0.05, 0.05, n)).to(dev)
    traj = torch.empty((n, length, 2), dtype=torch.int16, device=dev)
    traj[:, :, 0] = j[None, :].clamp(0, rows - 1).to(torch.int16)
    traj[:, :, 1] = (c0[:, None] + slope[:, None] * j[None, :]).clamp(0, cols - 1).to(torch.int16)
    return traj.view(-1, 2)


def long_track(length):
    steps = torch.randint(-1, 2, (length, 2), generator=gen, device=dev, dtype=torch.int32)
    steps[0, 0], steps[0, 1] = int(rng.integers(1000, rows - 1000)), int(rng.integers(1000, cols - 1000))
    pts = torch.cumsum(steps, 0)
    return torch.stack([pts[:, 0].clamp(0, rows - 1), pts[:, 1].clamp(0, cols - 1)], 1).to(torch.int16)


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


length = int(args.long_length)
nshort = max(int(args.points / 2) // 5000, 1)
nlong = max(int(args.points / 2) // length, 1)
parts = [short_tracks(nshort)] + [long_track(length) for _ in range(nlong)]
lengths = [5000] * nshort + [length] * nlong
order = rng.permutation(len(lengths))                            # long tracks between the short ones
traj = torch.cat([parts[0][k * 5000:(k + 1) * 5000] if k < nshort else parts[1 + k - nshort] for k in order])
off = torch.from_numpy(np.concatenate([[0], np.cumsum([lengths[k] for k in order])]).astype(np.int64)).to(dev)
del parts
total = int(traj.shape[0])
print(f'{total:.3e} points ({total * 4 / 1e9:.2f} GB) in {nshort} tracks of 5000 and {nlong} of {length}', flush=True)

updraft = torch.randn((rows, cols), generator=gen, device=dev, dtype=torch.float32) + 0.75
dem = torch.rand((rows, cols), generator=gen, device=dev, dtype=torch.float32) * 3. + \
    torch.arange(rows, device=dev, dtype=torch.float32)[:, None] * 0.2
cellinfo = flight.altitude_cellinfo(updraft, dem, 10., 15., 0.75)
workspace = flight.altitude_workspace(total)
band_hist = torch.zeros((rows, cols), dtype=torch.int32, device=dev)
kw = dict(start=100., floor=10., ceil=1000., band=(30., 150.), band_hist=band_hist, workspace=workspace)

lines = [f'{rows} x {cols}, {total:.2e} points, {nshort} tracks of 5000 points and {nlong} of {length}, '
         f'{torch.cuda.get_device_name(0)}', '',
         '| outputs | B/point | median ms | G points/s | algorithmic GB/s | runs (ms) |', '|---|---|---|---|---|---|']
for what, nbytes, extra in (('rasters', 8, {}), ('+ masked', 12, dict(want_masked=True)),
                            ('+ alt', 16, dict(want_masked=True, want_alt=True))):
    band_hist.zero_()
    med, runs = median_ms(lambda: flight.compute_track_altitudes(traj, cellinfo, (rows, cols), offsets=off, **kw, **extra))
    lines.append(f'| {what} | {nbytes} | {med:.3f} | {total / med / 1e6:.2f} | {total * nbytes / med / 1e6:.0f} | '
                 f'{", ".join(f"{m:.3f}" for m in runs)} |')
    print(lines[-1], flush=True)
out = flight.compute_track_altitudes(traj, cellinfo, (rows, cols), offsets=off, start=100., floor=10., ceil=1000.,
                                     band=(30., 150.))
in_zone = int(out['heights'][:, 0].sum(dtype=torch.int64))
assert in_zone == int((out['band_hist'].to(torch.int64) & 0xFFFFFFFF).sum()), 'the checksum does not hold'
lines += ['', f'points in the zone: {in_zone} of {total}; (the timed calls include torch.full / torch.zeros of the per-point '
          'outputs they return)']
text = '\n'.join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')
