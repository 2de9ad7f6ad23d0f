"""K20 beside K19: ssrs_site_collision_risk over K19's two point sets (tools/dev/time_rotor_collision.py, draw by draw) --
--points points (default 1e8, which gives 9.5e7) on a 5000 x 6000 raster, half of them in tracks of 5000 points that cross
the raster northwards, half in whole tracks of --long-length points (default 7.5e6), with the heights K14 computes for
them -- for two candidate classes, reach 0.65 and 6.5 cells (hub 90 m), each with ONE axis (a wind from 240 degrees) and
with an axis PER CELL (a raster of wind directions around 240 degrees, 16 B a cell), and Band's table of Config's
placeholder bird and rotor.  ssrs_rotor_collision_risk of the same build on the same points against K19's 300 turbines is
timed beside them for scale.  HIP events around the library call alone; after a warm-up of each the calls ALTERNATE --runs
times (default 11, the order reversed every other round) and each gets its median, so that a drift of the machine falls
on all:
  spread   the long tracks wander with king's moves
  parked   the long tracks oscillate among four cells: the same moves on the same sites millions of times, every one a
           hand-over -- what the LDS table of sites is for
Each step is a child of its own under `timeout -k 10`, and checks that the uniform axis and a per-cell raster FILLED with
that axis give the same integers.  Without --step this is the driver: it stops at the first step that fails and writes the
table to --out.  SSRS_HIP_LIB selects another build of the library (an A/B of the kernel: same tool, same points).
Algorithmic bytes: 8 B per point (traj and alt); the elevation and axis gathers, the table and the atomics are left out --
the pass is bound by f64 issue, (2W + 1)^2 plane tests a testable move, not by its bytes."""
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
STEP_SECONDS = 400
REACHES = (0.65, 6.5)


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
             f'{head["nlong"]} of {head["long_length"]}, {head["device"]}, {args.runs} alternating runs a call, library '
             f'{os.path.basename(head["lib"])}', '',
             '| step | call | median ms | G points/s | x K19 | min .. max ms | transits |',
             '|---|---|---|---|---|---|---|']
    for step, res in results.items():
        k19 = res['calls']['K19']['median']
        for call, t in res['calls'].items():
            lines.append(f'| {step} | {call} | {t["median"]:.3f} | {res["points"] / t["median"] / 1e6:.2f} | '
                         f'{t["median"] / k19:.1f} | {min(t["runs"]):.3f} .. {max(t["runs"]):.3f} | {t["transits"]} |')
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

    # the point set and the turbines of time_rotor_collision.py, draw by draw
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
    ntracks = len(lengths)

    updraft = torch.randn((rows, cols), generator=gen, device=dev, dtype=torch.float32) + 0.75
    dem = torch.rand((rows, cols), generator=gen, device=dev, dtype=torch.float32) * 3. + \
        torch.arange(rows, device=dev, dtype=torch.float32)[:, None] * 0.2
    cellinfo = flight.altitude_cellinfo(updraft, dem, res, 15., 0.75)
    alt = flight.compute_track_altitudes(traj, cellinfo, (rows, cols), offsets=off, want_alt=True, start=100., floor=10.,
                                         ceil=1000., band=(30., 150.))['alt']

    # ---- K19, for scale: the 300 turbines of profiles/collision_risk.md with their real disks (in the parked step too)
    cfg = Config()
    fleet = tb.Turbines(dict(x=xy[:, 0] * res, y=xy[:, 1] * res, t_hh=hub_m, t_rd=2. * rad))
    bounds = (0., 0., (cols - 1) * res, (rows - 1) * res)
    _, disk_reach, hub, _ = tb.rotor_disks(fleet, dem, bounds, res)
    band = (cfg.flight_airspeed, cfg.bird_length, cfg.bird_wingspan, cfg.bird_flight == 'flapping', cfg.collision_model_3d,
            cfg.rotor_chord_profile)
    cls, table, _ = tb.band_collision_table(
        rad, 0., tb.band_parameters(fleet, cfg.rotor_blades, cfg.rotor_rpm, cfg.rotor_max_chord, cfg.rotor_pitch), *band)
    axis = tb.rotor_axes(240., 'row_north', nturb)
    xy_dev, disk_dev, hub_dev, axis_dev, cls_dev, table_dev = (
        torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xy, disk_reach, hub, axis, cls, table.view(np.int32)))
    bins = tuple(torch.from_numpy(b).to(dev) for b in tb.build_bins(xy, rad / res + tb.TRANSIT_CULL_MARGIN, (rows, cols)))
    words = (nturb + 31) // 32

    def k19():
        hits = torch.zeros((ntracks, words), dtype=torch.int32, device=dev)
        transits, risk = (torch.zeros((nturb, 2), dtype=torch.int64, device=dev) for _ in range(2))
        track_risk = torch.zeros((ntracks,), dtype=torch.int64, device=dev)
        return (lambda: nat.check(nat.lib().ssrs_rotor_collision_risk(
            nat.ptr(traj), nat.ptr(off), ntracks, nat.ptr(alt), nat.ptr(cellinfo), rows, cols, nat.ptr(xy_dev), nat.ptr(disk_dev),
            nat.ptr(hub_dev), nat.ptr(axis_dev), 1000. * res, nturb, nat.ptr(bins[0]), nat.ptr(bins[1]), nat.ptr(hits),
            nat.ptr(transits), nat.ptr(cls_dev), nat.ptr(table_dev), int(table.shape[0]), nat.ptr(risk), nat.ptr(track_risk),
            stream_ptr()))), (transits, risk)

    # ---- K20: one class per reach (the rotor's radius is the reach, no clearance), one axis and an axis per cell
    one_axis = torch.from_numpy(tb.rotor_axes(240., 'row_north')[0]).to(dev)
    wdirn = 240. + 30. * torch.randn((rows, cols), generator=gen, device=dev, dtype=torch.float64)
    rad_ = wdirn * (np.pi / 180.)
    cell_axes = torch.stack([torch.sin(rad_), torch.cos(rad_)], -1).contiguous()          # (uc, ur) of 'row_north'
    filled = one_axis.expand(rows, cols, 2).contiguous()
    del wdirn, rad_

    def k20(reach, axes):
        site_table = tb.band_collision_table(np.array([reach * res]), 0., np.array([[cfg.rotor_rpm, cfg.rotor_max_chord,
                                             cfg.rotor_pitch, cfg.rotor_blades]]), *band)[1][0]
        table20 = torch.from_numpy(np.ascontiguousarray(site_table).view(np.int32)).to(dev)
        transits, risk = (torch.zeros((rows, cols, 2), dtype=torch.int64, device=dev) for _ in range(2))
        return (lambda: nat.check(nat.lib().ssrs_site_collision_risk(
            nat.ptr(traj), nat.ptr(off), ntracks, nat.ptr(alt), nat.ptr(cellinfo), rows, cols, reach, 90_000, nat.ptr(axes),
            int(axes.dim() == 3), 1000. * res, nat.ptr(table20), nat.ptr(transits), nat.ptr(risk), stream_ptr()))), (transits, risk)

    calls = {'K19': k19}
    for reach in REACHES:
        calls[f'K20 reach {reach:g} one axis'] = lambda reach=reach: k20(reach, one_axis)
        calls[f'K20 reach {reach:g} axis per cell'] = lambda reach=reach: k20(reach, cell_axes)

    def timed(make):
        fn, outs = make()                                            # (fresh, zeroed outputs outside the events)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), outs

    # the uniform axis against a raster filled with it: the same integers
    for reach in REACHES:
        _, (t1, r1) = timed(lambda: k20(reach, one_axis))
        _, (t2, r2) = timed(lambda: k20(reach, filled))
        if not (torch.equal(t1, t2) and torch.equal(r1, r2)):
            sys.exit(f'reach {reach}: the uniform axis and the filled raster disagree')
    del filled
    ms = {name: [] for name in calls}
    seen = {}
    for name, make in calls.items():                                 # the warm-ups
        timed(make)
    for rep in range(args.runs):
        for name in (list(calls)[::-1] if rep & 1 else list(calls)):
            t, outs = timed(calls[name])
            ms[name].append(t)
            seen[name] = int(outs[0].sum())
    out = {name: dict(median=float(np.median(runs)), runs=runs, transits=seen[name]) for name, runs in ms.items()}
    print(json.dumps(dict(rows=rows, cols=cols, points=total, nshort=nshort, nlong=nlong, long_length=length,
                          device=torch.cuda.get_device_name(0), lib=nat.LIB_PATH, calls=out)), flush=True)


if args.step:
    step(args.step)
else:
    driver()
