"""K18 beside K15: ssrs_rotor_transits and the untimed ssrs_rotor_encounters of the same build over the point set of
profiles/rotor_encounters.md -- --points points (default 1e8, which gives 9.5e7) on a 5000 x 6000 raster, half of them in
tracks of 5000 points that cross the raster northwards, half in whole tracks of --long-length points (default 7.5e6) --
against 300 turbines (20 plants of 15 on the tracks' way, rotor radii of 40 .. 80 m at 10 m a cell, hubs at 80 .. 120 m),
with the heights K14 computes for these points and every rotor facing a wind from 240 degrees.  HIP events, a warm-up and
the median of 5 runs for
  K18   hits and transits
  K15   hits, first_step and points_per_turbine: the yardstick, the same 8 B a point
in two steps, each a child of its own under `timeout -k 10`:
  spread   the long tracks wander with king's moves
  parked   the long tracks oscillate among four cells on a turbine: every one of their points lies in an occupied bin and
           half of their moves cross its plane
Without --step this is the driver: it stops at the first step that fails and writes the table to --out.  Algorithmic bytes:
8 B per point for both (traj and alt); the elevation gathers, the turbine tables and the atomics are left out."""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=1e8)
ap.add_argument('--long-length', type=float, default=7.5e6)
ap.add_argument('--step', choices=('spread', 'parked'), default=None)
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_SECONDS = 300


def run_step(step):
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', step,
           '--points', repr(args.points), '--long-length', repr(args.long_length)]
    run = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(run.stdout)
    if run.returncode != 0:
        sys.stderr.write(run.stderr)
        sys.exit(f'step {step} ended with status {run.returncode}: nothing more is started')
    return json.loads(run.stdout.strip().splitlines()[-1])


def driver():
    results = {step: run_step(step) for step in ('spread', 'parked')}
    head = results['spread']
    lines = [f'{head["rows"]} x {head["cols"]}, {head["points"]:.2e} points, {head["nshort"]} tracks of 5000 points and '
             f'{head["nlong"]} of {head["long_length"]}, {head["nturb"]} turbines, {head["device"]}', '',
             '| step | call | B/point | median ms | G points/s | algorithmic GB/s | x K15 | runs (ms) |',
             '|---|---|---|---|---|---|---|---|']
    for step, res in results.items():
        k15 = res['calls']['K15']['median']
        for call in ('K18', 'K15'):
            t = res['calls'][call]
            lines.append(f'| {step} | {call} | 8 | {t["median"]:.3f} | {res["points"] / t["median"] / 1e6:.2f} | '
                         f'{res["points"] * 8 / t["median"] / 1e6:.0f} | {t["median"] / k15:.2f} | '
                         f'{", ".join(f"{m:.3f}" for m in t["runs"])} |')
    lines.append('')
    for step, res in results.items():
        lines.append(f'{step}: K18 {res["transits"][0]} transits with the wind and {res["transits"][1]} against it, '
                     f'{res["transit_tracks"]} tracks with one, {res["transit_turbines"]} turbines transited; K15 '
                     f'{res["inside"]} (point, turbine) pairs inside a cylinder, {res["tracks_hit"]} tracks with one')
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

    # the point set and the turbines of time_rotor_encounters.py, draw by draw
    rows, cols, res = 5000, 6000, 10.
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(15)
    gen = torch.Generator(device=dev).manual_seed(15)
    nplants, per_plant = 20, 15
    nturb = nplants * per_plant
    centres = np.stack([rng.uniform(800., 5200., nplants), rng.uniform(500., 4500., nplants)], 1)
    xy = (centres[:, None, :] + rng.uniform(-150., 150., (nplants, per_plant, 2))).reshape(-1, 2)
    hub_m, rad = rng.uniform(80., 120., nturb), rng.uniform(40., 80., nturb)

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
    table = tb.Turbines(dict(x=xy[:, 0] * res, y=xy[:, 1] * res, t_hh=hub_m, t_rd=2. * rad))
    bounds = (0., 0., (cols - 1) * res, (rows - 1) * res)
    reach, zband = tb.rotor_geometry(table, dem, bounds, res)
    _, disk_reach, hub, _ = tb.rotor_disks(table, dem, bounds, res)
    if which == 'parked':
        # the parked tracks' turbines hold every height: K15's worst case, and a disk of 10 km for K18
        held = [(k * 7) % nturb for k in range(nlong)]
        zband[held] = (-2 ** 31, 2 ** 31 - 1)
        disk_reach[held] = 1000.
    axis = tb.rotor_axes(240., 'row_north', nturb)
    xy_dev, reach_dev, zband_dev, disk_dev, hub_dev, axis_dev = (
        torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xy, reach, zband, disk_reach, hub, axis))
    bins = tuple(torch.from_numpy(b).to(dev) for b in tb.build_bins(xy, reach, (rows, cols)))
    # (the parked turbines' huge reach is for the test alone: their cull lists are those of their real reach, or every bin
    # of the raster would be occupied)
    bins18 = tuple(torch.from_numpy(b).to(dev) for b in tb.build_bins(xy, reach + tb.TRANSIT_CULL_MARGIN, (rows, cols)))
    ntracks, words = len(lengths), (nturb + 31) // 32
    state = {}

    def fresh():
        state['hits'] = torch.zeros((ntracks, words), dtype=torch.int32, device=dev)
        state['first'] = torch.full((ntracks,), -1, dtype=torch.int32, device=dev)
        state['points'] = torch.zeros(nturb, dtype=torch.int64, device=dev)
        state['transits'] = torch.zeros((nturb, 2), dtype=torch.int64, device=dev)

    def k15():
        tb.rotor_encounters(traj, alt, off, cellinfo, xy_dev, reach_dev, zband_dev, (rows, cols), bins=bins, hits=state['hits'],
                            first_step=state['first'], points=state['points'])

    def k18():
        # the library call alone: turbines.rotor_transits also counts the bitmap, which K15's wrapper does not
        from ssrs_amd import _native as nat
        from ssrs_amd._device import stream_ptr
        nat.check(nat.lib().ssrs_rotor_transits(
            nat.ptr(traj), nat.ptr(off), ntracks, nat.ptr(alt), nat.ptr(cellinfo), rows, cols, nat.ptr(xy_dev),
            nat.ptr(disk_dev), nat.ptr(hub_dev), nat.ptr(axis_dev), 1000. * res, nturb, nat.ptr(bins18[0]),
            nat.ptr(bins18[1]), nat.ptr(state['hits']), nat.ptr(state['transits']), stream_ptr()))

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

    calls = {'K15': median_ms(k15)}
    inside, tracks_hit = int(state['points'].sum()), int((state['first'] >= 0).sum())
    calls['K18'] = median_ms(k18)
    per_turbine, per_track = tb.encounter_counts(state['hits'], nturb)
    print(json.dumps(dict(rows=rows, cols=cols, points=total, nshort=nshort, nlong=nlong, long_length=length, nturb=nturb,
                          device=torch.cuda.get_device_name(0), calls=calls, inside=inside, tracks_hit=tracks_hit,
                          transits=[int(v) for v in state['transits'].sum(0)], transit_tracks=int((per_track > 0).sum()),
                          transit_turbines=int((per_turbine > 0).sum()))), flush=True)


if args.step:
    step(args.step)
else:
    driver()
