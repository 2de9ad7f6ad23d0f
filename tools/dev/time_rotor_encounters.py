"""K15 alone: ssrs_rotor_encounters over the point set of profiles/flight_height.md -- --points points (default 1e8, which gives
9.5e7) on a 5000 x 6000 raster, half of them in tracks of 5000 points that cross the raster northwards, half in whole tracks of
--long-length points (default 7.5e6: the step cap of a 10 m run) -- against 300 turbines (20 plants of 15 on the tracks' way, rotor radii of
40 .. 80 m at 10 m a cell, hubs at 80 .. 120 m), with the heights K14 computes for these points.  HIP events, a warm-up and
the median of 5 runs for
  K15          hits, first_step and points_per_turbine
  K15 bitmap   the same call without points_per_turbine
  K8           ssrs_turbine_encounters on the same points and turbines at the mean reach: the yardstick, 4 B a point
in two steps:
  spread   the long tracks wander with king's moves (the set of profiles/flight_height.md)
  parked   the long tracks oscillate among four cells inside a cylinder that holds every height: every one of their points
           counts for the exposure, the worst case of its combining
and `tools/microbench/stream 1` (--stream-bin, the built yardstick) in the same visit.  Without --step this is the driver: it
runs each step as a child under its own `timeout -k 10`, stops at the first that fails, and writes the table to --out.
Algorithmic bytes: 8 B per point for K15 (traj and alt), 4 B for K8; the elevation gathers, the turbine tables and the atomics
are left out.

--timed adds the leg of the timed form (ssrs_rotor_encounters_timed): `K15 timed`, the same call with the dt K16 computes for
these points in a uniform wind and time_per_turbine (8 B a point plus 4 B per point inside a cylinder).  --parent-lib <a
libssrs_hip.so built from the parent commit> makes the driver run every step four times in one visit -- the parent's library,
this tree's with the timed leg, the parent's again (SSRS_HIP_LIB selects the library of a child) -- and print, per step, the
parent's two medians of the untimed K15, their difference (the run-to-run spread), this tree's median, and whether it lies
within that spread of the parent's."""
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
ap.add_argument('--timed', action='store_true', help='also time ssrs_rotor_encounters_timed')
ap.add_argument('--parent-lib', default=None, help="the parent commit's library: the untimed K15 of both, side by side")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_SECONDS = 300


def run_step(step, timed, lib=None):
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', step,
           '--points', repr(args.points), '--long-length', repr(args.long_length)] + (['--timed'] if timed else [])
    env = dict(os.environ, SSRS_HIP_LIB=os.path.abspath(lib)) if lib else None
    run = subprocess.run(cmd, capture_output=True, text=True, env=env)
    sys.stdout.write(run.stdout)
    if run.returncode != 0:
        sys.stderr.write(run.stderr)
        sys.exit(f'step {step} ended with status {run.returncode}: nothing more is started')
    return json.loads(run.stdout.strip().splitlines()[-1])


def driver():
    lines, results, parent = [], {}, {}
    for step in ('spread', 'parked'):
        if args.parent_lib:
            parent[step] = [run_step(step, False, args.parent_lib)]
        results[step] = run_step(step, args.timed)
        if args.parent_lib:
            parent[step].append(run_step(step, False, args.parent_lib))
    head = results['spread']
    lines += [f'{head["rows"]} x {head["cols"]}, {head["points"]:.2e} points, {head["nshort"]} tracks of 5000 points and '
              f'{head["nlong"]} of {head["long_length"]}, {head["nturb"]} turbines, {head["device"]}', '',
              '| step | call | B/point | median ms | G points/s | algorithmic GB/s | x K8 | runs (ms) |',
              '|---|---|---|---|---|---|---|---|']
    for step, res in results.items():
        k8 = res['calls']['K8']['median']
        for call, nbytes in (('K15 timed', 8), ('K15', 8), ('K15 bitmap', 8), ('K8', 4)):
            if call not in res['calls']:
                continue
            t = res['calls'][call]
            lines.append(f'| {step} | {call} | {nbytes} | {t["median"]:.3f} | {res["points"] / t["median"] / 1e6:.2f} | '
                         f'{res["points"] * nbytes / t["median"] / 1e6:.0f} | {t["median"] / k8:.2f} | '
                         f'{", ".join(f"{m:.3f}" for m in t["runs"])} |')
    lines.append('')
    for step, res in results.items():
        lines.append(f'{step}: {res["inside"]} (point, turbine) pairs inside a cylinder, {res["tracks_hit"]} tracks with one, '
                     f'{res["turbines_hit"]} turbines met; K8 at {res["radius"]:.2f} cells: {res["k8_tracks_hit"]} tracks')
    for step, res in results.items():
        if 'K15 timed' in res['calls']:
            lines.append(f'{step}: K15 timed / K15 = {res["calls"]["K15 timed"]["median"] / res["calls"]["K15"]["median"]:.3f}; '
                         f'{res["time_us"]} us inside the cylinders over {res["inside"]} (point, turbine) pairs')
    if parent:
        lines += ['', '| step | untimed K15 | median ms | runs (ms) |', '|---|---|---|---|']
        for step, (first, second) in parent.items():
            for label, res in (('parent, first', first), ('this tree', results[step]), ('parent, second', second)):
                t = res['calls']['K15']
                lines.append(f'| {step} | {label} | {t["median"]:.4f} | {", ".join(f"{m:.4f}" for m in t["runs"])} |')
        lines.append('')
        for step, (first, second) in parent.items():
            a, b, new = (r['calls']['K15']['median'] for r in (first, second, results[step]))
            spread, centre = abs(a - b), (a + b) / 2.
            lines.append(f'{step}: the parent\'s medians {a:.4f} and {b:.4f} ms differ by {spread:.4f} ms (the run-to-run spread); '
                         f'this tree\'s {new:.4f} ms lies {abs(new - centre):.4f} ms from their mean {centre:.4f}: '
                         f'{"within" if abs(new - centre) <= spread else "OUTSIDE"} the spread')
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
    from ssrs_amd import turbines as tb

    rows, cols, res = 5000, 6000, 10.
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(15)
    gen = torch.Generator(device=dev).manual_seed(15)
    nplants, per_plant = 20, 15
    nturb = nplants * per_plant
    centres = np.stack([rng.uniform(800., 5200., nplants), rng.uniform(500., 4500., nplants)], 1)
    xy = (centres[:, None, :] + rng.uniform(-150., 150., (nplants, per_plant, 2))).reshape(-1, 2)
    hub, rad = rng.uniform(80., 120., nturb), rng.uniform(40., 80., nturb)

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
            xt, yt = xy[(k * 7) % nturb]
            j = torch.arange(length, device=dev)
            return torch.stack([(int(round(yt)) + (j & 1)).clamp(0, rows - 1), (int(round(xt)) + ((j >> 1) & 1)).clamp(0, cols - 1)],
                               1).to(torch.int16)
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
    alt = flight.compute_track_altitudes(traj, cellinfo, (rows, cols), offsets=off, want_alt=True, start=100., floor=10.,
                                         ceil=1000., band=(30., 150.))['alt']
    table = tb.Turbines(dict(x=xy[:, 0] * res, y=xy[:, 1] * res, t_hh=hub, t_rd=2. * rad))
    reach, zband = tb.rotor_geometry(table, dem, (0., 0., (cols - 1) * res, (rows - 1) * res), res)
    if which == 'parked':
        zband[[(k * 7) % nturb for k in range(nlong)]] = (-2 ** 31, 2 ** 31 - 1)
    radius = float(np.mean(reach))
    xy_dev, reach_dev, zband_dev = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xy, reach, zband))
    bins = tuple(torch.from_numpy(b).to(dev) for b in tb.build_bins(xy, reach, (rows, cols)))
    bins8 = tuple(torch.from_numpy(b).to(dev) for b in tb.build_bins(xy, radius, (rows, cols)))
    ntracks, words = len(lengths), (nturb + 31) // 32
    state = {}

    def fresh():
        state['hits'] = torch.zeros((ntracks, words), dtype=torch.int32, device=dev)
        state['first'] = torch.full((ntracks,), -1, dtype=torch.int32, device=dev)
        state['points'] = torch.zeros(nturb, dtype=torch.int64, device=dev)
        state['time'] = torch.zeros(nturb, dtype=torch.int64, device=dev)

    def k15(points):
        tb.rotor_encounters(traj, alt, off, cellinfo, xy_dev, reach_dev, zband_dev, (rows, cols), bins=bins, hits=state['hits'],
                            first_step=state['first'], points=state['points'] if points else False)

    if args.timed:
        # the dt K16 gives these points in a uniform wind: every point inside a cylinder then costs one more 4-byte load
        dt = flight.compute_track_times(traj, (rows, cols), offsets=off, resolution=res, airspeed=15., wind=(8., 240.),
                                        want_dt=True)['dt']

    def k15_timed():
        tb.rotor_encounters(traj, alt, off, cellinfo, xy_dev, reach_dev, zband_dev, (rows, cols), bins=bins, hits=state['hits'],
                            first_step=state['first'], points=state['points'], dt=dt, time=state['time'])

    def k8():
        tb.turbine_encounters(traj, off, xy_dev, radius, (rows, cols), bins=bins8, hits=state['hits'], first_step=state['first'])

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

    calls = {'K8': median_ms(k8)}
    k8_tracks_hit = int((state['first'] >= 0).sum())
    calls['K15 bitmap'] = median_ms(lambda: k15(False))
    calls['K15'] = median_ms(lambda: k15(True))
    per_turbine, _ = tb.encounter_counts(state['hits'], nturb)
    extra = {}
    if args.timed:
        untimed = {k: state[k].clone() for k in ('hits', 'first', 'points')}
        calls['K15 timed'] = median_ms(k15_timed)
        assert all(torch.equal(state[k], v) for k, v in untimed.items()), 'the timed call changed hits, first_step or points'
        extra = dict(time_us=int(state['time'].sum()))
    print(json.dumps(dict(**extra, rows=rows, cols=cols, points=total, nshort=nshort, nlong=nlong, long_length=length, nturb=nturb,
                          device=torch.cuda.get_device_name(0), radius=radius, calls=calls,
                          inside=int(state['points'].sum()), tracks_hit=int((state['first'] >= 0).sum()),
                          turbines_hit=int((per_turbine > 0).sum()), k8_tracks_hit=k8_tracks_hit)), flush=True)


if args.step:
    step(args.step)
else:
    driver()
