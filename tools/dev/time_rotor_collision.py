"""K19 beside K18: ssrs_rotor_collision_risk and ssrs_rotor_transits of the same build over the point set of
profiles/rotor_transits.md -- --points points (default 1e8, which gives 9.5e7) on a 5000 x 6000 raster, half of them in
tracks of 5000 points that cross the raster northwards, half in whole tracks of --long-length points (default 7.5e6) --
against 300 turbines (20 plants of 15 on the tracks' way, rotor radii of 40 .. 80 m at 10 m a cell, hubs at 80 .. 120 m),
with the heights K14 computes for these points, every rotor facing a wind from 240 degrees, and Band's table of the 300
classes (every turbine has a radius of its own) for Config's placeholder bird and rotor.  HIP events around the library
call alone; after a warm-up of each the two calls ALTERNATE --runs times (default 11) and each gets its median, so that a
drift of the machine falls on both:
  K19   hits, transits, risk and track_risk
  K18   hits and transits: the yardstick, the same 8 B a point and the same walk
in two steps, each a child of its own under `timeout -k 10`:
  spread   the long tracks wander with king's moves
  parked   the long tracks oscillate among four cells on a turbine whose disk is made 1000 cells wide: half of their moves
           are transits, alternating in direction -- every one a hand-over of count AND sum to LDS and a table lookup
Each step also checks that K19's hits and transits are K18's.  Without --step this is the driver: it stops at the first
step that fails and writes the table to --out.  Algorithmic bytes: 8 B per point for both (traj and alt); the elevation
gathers, the turbine tables, the probability table and the atomics are left out."""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=1e8)
ap.add_argument('--long-length', type=float, default=7.5e6)
ap.add_argument('--runs', type=int, default=11)
ap.add_argument('--step', choices=('spread', 'parked'), default=None)
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_SECONDS = 300


def run_step(step):
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', step,
           '--points', repr(args.points), '--long-length', repr(args.long_length), '--runs', str(args.runs)]
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
             f'{head["nlong"]} of {head["long_length"]}, {head["nturb"]} turbines in {head["nclass"]} classes, '
             f'{head["device"]}, {args.runs} alternating runs a call', '',
             '| step | call | B/point | median ms | G points/s | algorithmic GB/s | x K18 | min .. max ms |',
             '|---|---|---|---|---|---|---|---|']
    for step, res in results.items():
        k18 = res['calls']['K18']['median']
        for call in ('K19', 'K18'):
            t = res['calls'][call]
            lines.append(f'| {step} | {call} | 8 | {t["median"]:.3f} | {res["points"] / t["median"] / 1e6:.2f} | '
                         f'{res["points"] * 8 / t["median"] / 1e6:.0f} | {t["median"] / k18:.3f} | '
                         f'{min(t["runs"]):.3f} .. {max(t["runs"]):.3f} |')
    lines.append('')
    for step, res in results.items():
        lines.append(f'{step}: {res["transits"][0]} transits with the wind and {res["transits"][1]} against it (K18 and K19 '
                     f'alike), {res["transit_tracks"]} tracks with one, {res["transit_turbines"]} turbines transited; expected '
                     f'collisions {res["risk"][0]:.3f} with the wind and {res["risk"][1]:.3f} against it, '
                     f'{res["risk_tracks"]} tracks at risk')
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
    from ssrs_amd import Config, flight
    from ssrs_amd import _native as nat
    from ssrs_amd import turbines as tb
    from ssrs_amd._device import stream_ptr

    # the point set and the turbines of time_rotor_transits.py, draw by draw
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
    fleet = tb.Turbines(dict(x=xy[:, 0] * res, y=xy[:, 1] * res, t_hh=hub_m, t_rd=2. * rad))
    bounds = (0., 0., (cols - 1) * res, (rows - 1) * res)
    _, disk_reach, hub, _ = tb.rotor_disks(fleet, dem, bounds, res)
    # Band's table for Config's placeholders; the classes keep the turbines' real radii (in the parked step too: there the
    # crossings of the widened disks fall into its inner rings)
    cfg = Config()
    cls, table, classes = tb.band_collision_table(
        rad, 0., tb.band_parameters(fleet, cfg.rotor_blades, cfg.rotor_rpm, cfg.rotor_max_chord, cfg.rotor_pitch),
        cfg.flight_airspeed, cfg.bird_length, cfg.bird_wingspan, cfg.bird_flight == 'flapping', cfg.collision_model_3d,
        cfg.rotor_chord_profile)
    if which == 'parked':
        # the parked tracks' turbines get a disk of 10 km: every move across their plane is a transit
        held = [(k * 7) % nturb for k in range(nlong)]
        disk_reach[held] = 1000.
    axis = tb.rotor_axes(240., 'row_north', nturb)
    xy_dev, disk_dev, hub_dev, axis_dev, cls_dev, table_dev = (
        torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xy, disk_reach, hub, axis, cls, table.view(np.int32)))
    # (the parked turbines' huge reach is for the test alone: their cull lists are those of their real reach, or every bin
    # of the raster would be occupied)
    bins = tuple(torch.from_numpy(b).to(dev) for b in tb.build_bins(xy, rad / res + tb.TRANSIT_CULL_MARGIN, (rows, cols)))
    ntracks, words = len(lengths), (nturb + 31) // 32
    state = {}

    def fresh():
        state['hits'] = torch.zeros((ntracks, words), dtype=torch.int32, device=dev)
        state['transits'] = torch.zeros((nturb, 2), dtype=torch.int64, device=dev)
        state['risk'] = torch.zeros((nturb, 2), dtype=torch.int64, device=dev)
        state['track_risk'] = torch.zeros((ntracks,), dtype=torch.int64, device=dev)

    def common():
        return (nat.ptr(traj), nat.ptr(off), ntracks, nat.ptr(alt), nat.ptr(cellinfo), rows, cols, nat.ptr(xy_dev),
                nat.ptr(disk_dev), nat.ptr(hub_dev), nat.ptr(axis_dev), 1000. * res, nturb, nat.ptr(bins[0]), nat.ptr(bins[1]),
                nat.ptr(state['hits']), nat.ptr(state['transits']))

    def k18():
        nat.check(nat.lib().ssrs_rotor_transits(*common(), stream_ptr()))

    def k19():
        nat.check(nat.lib().ssrs_rotor_collision_risk(*common(), nat.ptr(cls_dev), nat.ptr(table_dev), int(table.shape[0]),
                                                      nat.ptr(state['risk']), nat.ptr(state['track_risk']), stream_ptr()))

    def timed(fn):
        fresh()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    timed(k18)                                                       # the warm-ups
    timed(k19)
    ms = {'K18': [], 'K19': []}
    kept = {}
    for rep in range(args.runs):
        for name, fn in (('K19', k19), ('K18', k18)) if rep & 1 else (('K18', k18), ('K19', k19)):
            ms[name].append(timed(fn))
            kept[name] = (state['hits'], state['transits'])
            if name == 'K19':
                kept['risk'], kept['track_risk'] = state['risk'], state['track_risk']
    if not (torch.equal(kept['K18'][0], kept['K19'][0]) and torch.equal(kept['K18'][1], kept['K19'][1])):
        sys.exit('K19 and K18 disagree on hits or transits')
    calls = {name: dict(median=float(np.median(runs)), runs=runs) for name, runs in ms.items()}
    per_turbine, per_track = tb.encounter_counts(kept['K19'][0], nturb)
    print(json.dumps(dict(rows=rows, cols=cols, points=total, nshort=nshort, nlong=nlong, long_length=length, nturb=nturb,
                          nclass=int(len(classes)), device=torch.cuda.get_device_name(0), calls=calls,
                          transits=[int(v) for v in kept['K19'][1].sum(0)], transit_tracks=int((per_track > 0).sum()),
                          transit_turbines=int((per_turbine > 0).sum()),
                          risk=[float(v) * 2. ** -32 for v in kept['risk'].sum(0)],
                          risk_tracks=int((kept['track_risk'] != 0).sum()))), flush=True)


if args.step:
    step(args.step)
else:
    driver()
