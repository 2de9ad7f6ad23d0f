"""K16 alone: ssrs_track_time over the point set of profiles/flight_height.md -- --points points (default 1e8, which gives
9.5e7) on a 5000 x 6000 raster, half of them in tracks of 5000 points that cross the raster northwards, half in whole tracks of
--long-length points (default 7.5e6: the step cap of a 10 m run) -- with a random windinfo raster (8 B a cell), and K14
(ssrs_track_altitude, rasters and traj_band) on the same points.  HIP events, a warm-up and the median of 5 runs for
  K16           time_hist and the per-track rows, from the windinfo raster
  K16 uniform   the same with one wind everywhere (no gathers)
  K16 zone      + masked (K14's traj_band) and band_time_hist
  K16 zone dt   + dt
  K14           band_hist, the per-track rows and traj_band: the yardstick
in two steps:
  spread   the long tracks wander with king's moves (the set of profiles/flight_height.md)
  parked   the long tracks go round three cells: every lane of theirs adds to the same three cells of the rasters, the worst
           case of the register cache
and `tools/microbench/stream 1` (--stream-bin, the built yardstick) in the same visit.  Without --step this is the driver: it
runs each step as a child under its own `timeout -k 10`, stops at the first that fails, and writes the table to --out.
Algorithmic bytes: traj 4 B a point, masked and dt 4 B each where used; the windinfo gathers and the atomics are left out."""
import argparse
import json
import os
import re
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=1e8)
ap.add_argument('--long-length', type=float, default=7.5e6)
ap.add_argument('--step', choices=('spread', 'parked'), default=None)
ap.add_argument('--stream-bin', default=None, help='built tools/microbench/stream.hip; run as `<bin> 1`')
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_SECONDS = 300
CALLS = (('K16', 4), ('K16 uniform', 4), ('K16 zone', 8), ('K16 zone dt', 12), ('K14', 12))


def driver():
    lines, results = [], {}
    for step in ('spread', 'parked'):
        cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', step,
               '--points', repr(args.points), '--long-length', repr(args.long_length)]
        run = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(run.stdout)
        if run.returncode != 0:
            sys.stderr.write(run.stderr)
            sys.exit(f'step {step} ended with status {run.returncode}: nothing more is started')
        results[step] = json.loads(run.stdout.strip().splitlines()[-1])
    head = results['spread']
    lines += [f'{head["rows"]} x {head["cols"]}, {head["points"]:.2e} points, {head["nshort"]} tracks of 5000 points and '
              f'{head["nlong"]} of {head["long_length"]}, {head["device"]}', '',
              '| step | call | B/point | median ms | G points/s | algorithmic GB/s | x K14 | runs (ms) |',
              '|---|---|---|---|---|---|---|---|']
    for step, res in results.items():
        k14 = res['calls']['K14']['median']
        for call, nbytes in CALLS:
            t = res['calls'][call]
            lines.append(f'| {step} | {call} | {nbytes} | {t["median"]:.3f} | {res["points"] / t["median"] / 1e6:.2f} | '
                         f'{res["points"] * nbytes / t["median"] / 1e6:.0f} | {t["median"] / k14:.2f} | '
                         f'{", ".join(f"{m:.3f}" for m in t["runs"])} |')
    lines.append('')
    for call, _ in CALLS[:-1]:
        lines.append(f'{call}: parked / spread = '
                     f'{results["parked"]["calls"][call]["median"] / results["spread"]["calls"][call]["median"]:.2f}')
    lines.append('')
    for step, res in results.items():
        lines.append(f'{step}: {res["total_us"]} us in all, {res["zone_us"]} us in the zone ({res["in_zone"]} points); '
                     f'checksums {"hold" if res["checksums"] else "FAIL"}')
    if args.stream_bin:
        run = subprocess.run(['timeout', '-k', '10', '120', args.stream_bin, '1'], capture_output=True, text=True)
        sys.stdout.write(run.stdout)
        if run.returncode != 0:
            sys.exit(f'stream ended with status {run.returncode}')
        found = re.findall(r'grid\s+(\d+): read x4 ([\d.]+)\s+read dword ([\d.]+)', run.stdout)
        lines += ['', '| stream 1: grid | read 16 B (TB/s) | read 4 B (TB/s) |', '|---|---|---|']
        lines += [f'| {g} | {a} | {b} |' for g, a, b in found]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


def step(which):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from ssrs_amd import flight

    rows, cols, res = 5000, 6000, 10.
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(16)
    gen = torch.Generator(device=dev).manual_seed(16)

    def short_tracks(n, length=5000):
        j = torch.arange(length, device=dev)
        c0 = torch.from_numpy(rng.uniform(600., 5400., n)).to(dev)
        slope = torch.from_numpy(rng.uniform(-0.05, 0.05, n)).to(dev)
        traj = torch.empty((n, length, 2), dtype=torch.int16, device=dev)
        traj[:, :, 0] = j[None, :].clamp(0, rows - 1).to(torch.int16)
        traj[:, :, 1] = (c0[:, None] + slope[:, None] * j[None, :]).clamp(0, cols - 1).to(torch.int16)
        return traj.view(-1, 2)

    def long_track(length, k):
        if which == 'parked':
            r0, c0 = int(rng.integers(1000, rows - 1000)), int(rng.integers(1000, cols - 1000))
            j = torch.arange(length, device=dev) % 3                   # (r0, c0) -> (r0 + 1, c0 + 1) -> (r0, c0 + 1) -> ...
            return torch.stack([r0 + (j == 1).to(torch.int64), c0 + (j >= 1).to(torch.int64)], 1).to(torch.int16)
        steps = torch.randint(-1, 2, (length, 2), generator=gen, device=dev, dtype=torch.int32)
        steps[0, 0], steps[0, 1] = int(rng.integers(1000, rows - 1000)), int(rng.integers(1000, cols - 1000))
        pts = torch.cumsum(steps, 0)
        return torch.stack([pts[:, 0].clamp(0, rows - 1), pts[:, 1].clamp(0, cols - 1)], 1).to(torch.int16)

    length = int(args.long_length)
    nshort = max(int(args.points / 2) // 5000, 1)
    nlong = max(int(args.points / 2) // length, 1)
    parts = [short_tracks(nshort)] + [long_track(length, k) for k in range(nlong)]
    lengths = [5000] * nshort + [length] * nlong
    order = rng.permutation(len(lengths))                            # long tracks between the short ones
    traj = torch.cat([parts[0][k * 5000:(k + 1) * 5000] if k < nshort else parts[1 + k - nshort] for k in order])
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([lengths[k] for k in order])]).astype(np.int64)).to(dev)
    del parts
    total = int(traj.shape[0])

    updraft = torch.randn((rows, cols), generator=gen, device=dev, dtype=torch.float32) + 0.75
    dem = torch.rand((rows, cols), generator=gen, device=dev, dtype=torch.float32) * 3. + \
        torch.arange(rows, device=dev, dtype=torch.float32)[:, None] * 0.2
    cellinfo = flight.altitude_cellinfo(updraft, dem, res, 15., 0.75)
    wspeed = torch.rand((rows, cols), generator=gen, device=dev, dtype=torch.float32) * 20.
    wdirn = torch.rand((rows, cols), generator=gen, device=dev, dtype=torch.float32) * 360.
    windinfo = flight.wind_cellinfo(wspeed, wdirn, 'row_east')
    del updraft, wspeed, wdirn
    heights = dict(start=100., floor=10., ceil=1000., band=(30., 150.))
    workspace = flight.altitude_workspace(total)
    state = {}

    def fresh():
        state['time_hist'] = torch.zeros((rows, cols), dtype=torch.int64, device=dev)
        state['band_time_hist'] = torch.zeros((rows, cols), dtype=torch.int64, device=dev)
        state['band_hist'] = torch.zeros((rows, cols), dtype=torch.int32, device=dev)

    def k14():
        state['k14'] = flight.compute_track_altitudes(traj, cellinfo, (rows, cols), offsets=off, want_masked=True,
                                                      band_hist=state['band_hist'], workspace=workspace, **heights)

    fresh()
    k14()
    masked = state['k14']['masked']
    in_zone = int(state['k14']['heights'][:, 0].sum())
    scalars = dict(resolution=res, airspeed=15., min_groundspeed=1.)

    def k16(wind, zone, dt):
        state['k16'] = flight.compute_track_times(traj, (rows, cols), offsets=off, wind=wind, masked=masked if zone else None,
                                                  want_dt=dt, time_hist=state['time_hist'],
                                                  band_time_hist=state['band_time_hist'] if zone else None, **scalars)

    def median_ms(fn):
        ms = []
        for rep in range(6):                                         # the first is the warm-up
            fresh()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return dict(median=float(np.median(ms[1:])), runs=ms[1:])

    calls = {'K14': median_ms(k14)}
    calls['K16'] = median_ms(lambda: k16(windinfo, False, False))
    calls['K16 uniform'] = median_ms(lambda: k16((8., 250.), False, False))
    calls['K16 zone dt'] = median_ms(lambda: k16(windinfo, True, True))
    calls['K16 zone'] = median_ms(lambda: k16(windinfo, True, False))
    times = state['k16']['times']
    ok = int(state['time_hist'].sum()) == int(times[:, 0].sum()) and int(state['band_time_hist'].sum()) == int(times[:, 1].sum())
    print(json.dumps(dict(rows=rows, cols=cols, points=total, nshort=nshort, nlong=nlong, long_length=length,
                          device=torch.cuda.get_device_name(0), calls=calls, total_us=int(times[:, 0].sum()),
                          zone_us=int(times[:, 1].sum()), in_zone=in_zone, checksums=bool(ok))), flush=True)


if args.step:
    step(args.step)
else:
    driver()
