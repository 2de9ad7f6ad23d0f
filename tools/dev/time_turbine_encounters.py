"""K8 alone: ssrs_turbine_encounters over 1e9 synthetic trajectory points (4 GB) against 500 turbines at 15 cells on the
5000 x 6000 raster, HIP events, a warm-up and the median of 5 runs; next to it what a plain 16-byte read of the same
bytes reaches (`tools/microbench/stream 4`, run from here when --stream-bin names the built yardstick).  The kernel
is expected to stream at 4 B per point, so the ratio of the two is the figure.

The points: 100 000 tracks of 5000 points that cross the raster northwards (the turbines lie on their way), and 100
tracks of 5e6 points that oscillate in four cells until the step cap, half of them inside a turbine's disk -- what a trap
cell of a solved 10 m field does.  Three variants tell the parts apart:
  full        the above
  far         the same points, the turbines moved off the tracks' columns: no bin walk, no atomics -- stream + track
              lookup + mask lookup
  one-track   the same points as ONE track, turbines far: no span crosses a track end -- stream + mask lookup
--points scales everything down for a quick look."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ssrs_amd import turbines as tb       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=1e9)
ap.add_argument('--stream-bin', default=None, help='built tools/microbench/stream.hip; run as `<bin> 4`')
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

rows, cols, nturb, radius = 5000, 6000, 500, 15.
scale = args.points / 1e9
n_cross, len_cross = int(100_000 * scale), 5000
n_trap, len_trap = max(int(100 * scale), 2), 5_000_000
dev = torch.device('cuda', 0)
rng = np.random.default_rng(8)
# turbines: 20 plants of 25 on the tracks' way (columns 600 .. 5400)
centres = np.stack([rng.uniform(800., 5200., 20), rng.uniform(500., 4500., 20)], 1)
xy = (centres[:, None, :] + rng.uniform(-150., 150., (20, 25, 2))).reshape(-1, 2)
xy_far = xy.copy()
xy_far[:, 0] = rng.uniform(0., 300., nturb)                     # west of every track

total = n_cross * len_cross + n_trap * len_trap
traj = torch.empty((total, 2), dtype=torch.int16, device=dev)
lengths = []
pos = 0
slabs = 10
j_c = torch.arange(len_cross, device=dev)
j_t = torch.arange(len_trap, device=dev)
for s in range(slabs):
    k0, k1 = n_cross * s // slabs, n_cross * (s + 1) // slabs
    c0 = torch.from_numpy(rng.uniform(600., 5400., k1 - k0)).to(dev)
    slope = torch.from_numpy(rng.uniform(-0.05, 0.05, k1 - k0)).to(dev)
    block = traj[pos:pos + (k1 - k0) * len_cross].view(k1 - k0, len_cross, 2)
    block[:, :, 0] = j_c[None, :].to(torch.int16)
    block[:, :, 1] = (c0[:, None] + slope[:, None] * j_c[None, :]).clamp(0, cols - 1).to(torch.int16)
    pos += (k1 - k0) * len_cross
    lengths += [len_cross] * (k1 - k0)
    k0, k1 = n_trap * s // slabs, n_trap * (s + 1) // slabs
    for k in range(k0, k1):
        # even ones sit ON a turbine (every point inside its disk: the case that must cost no atomics); odd ones 40 cells
        # east of one, in an occupied bin but mostly outside the disks (every point walks a list and hits nothing)
        xt, yt = xy[(k * 7) % nturb]
        r0, c0 = int(round(yt)), int(round(xt)) + (40 if k & 1 else 0)
        block = traj[pos:pos + len_trap]
        block[:, 0] = (r0 + (j_t & 1)).clamp(0, rows - 1).to(torch.int16)
        block[:, 1] = (c0 + ((j_t >> 1) & 1)).clamp(0, cols - 1).to(torch.int16)
        pos += len_trap
        lengths.append(len_trap)
assert pos == total
off = torch.zeros(len(lengths) + 1, dtype=torch.int64, device=dev)
off[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64, device=dev), 0)
off_one = torch.tensor([0, total], dtype=torch.int64, device=dev)
print(f'{total:.3e} points ({total * 4 / 1e9:.2f} GB) in {len(lengths)} tracks; {nturb} turbines, radius {radius:g} cells, '
      f'{rows} x {cols}', flush=True)


def timed(offsets, turbines):
    xy_dev = torch.from_numpy(turbines).to(dev)
    bins = tuple(torch.from_numpy(b).to(dev) for b in tb.build_bins(turbines, radius, (rows, cols)))
    n = offsets.numel() - 1
    ms = []
    for rep in range(6):                                         # the first is the warm-up
        hits = torch.zeros((n, (nturb + 31) // 32), dtype=torch.int32, device=dev)
        first = torch.full((n,), -1, dtype=torch.int32, device=dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tb.turbine_encounters(traj, offsets, xy_dev, radius, (rows, cols), bins=bins, hits=hits, first_step=first)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    per_turbine, _ = tb.encounter_counts(hits, nturb)
    return float(np.median(ms[1:])), ms[1:], int(per_turbine.sum().item()), int((first >= 0).sum().item())


lines = ['| variant | median ms | TB/s | runs (ms) | encounters | tracks with one |', '|---|---|---|---|---|---|']
rates = {}
for name, offsets, turbines in (('full', off, xy), ('far', off, xy_far), ('one-track', off_one, xy_far)):
    med, runs, enc, met = timed(offsets, turbines)
    rates[name] = total * 4 / med / 1e9
    lines.append(f'| {name} | {med:.3f} | {rates[name]:.3f} | {", ".join(f"{m:.3f}" for m in runs)} | {enc} | {met} |')
    print(lines[-1], flush=True)

stream = None
if args.stream_bin:
    out = subprocess.run([args.stream_bin, '4'], capture_output=True, text=True, timeout=300).stdout
    print(out, flush=True)
    found = re.findall(r'grid\s+(\d+): read x4 ([\d.]+)', out)
    if found:
        stream = max(float(v) for _, v in found)
        lines.append(f'| stream: 16-byte read of 4 GiB, best grid | | {stream:.3f} | | | |')
        lines.append('')
        lines.append(f'ratio full / stream = {rates["full"] / stream:.3f}; far / stream = {rates["far"] / stream:.3f}; '
                     f'one-track / stream = {rates["one-track"] / stream:.3f}')
text = '\n'.join(lines)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
