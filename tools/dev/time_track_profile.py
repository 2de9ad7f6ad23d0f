"""K22's speed: one ssrs_tracks_score_profile over nmem x nnu combinations against the SAME combinations as nmem * nnu
separate ssrs_tracks_score calls without p, status and maps (K21, the code a user had before K22), on the two workloads of
tools/dev/time_track_score.py: a 5000 x 6000 raster with a rough f64 updraft and an f32 potential that falls northwards,
--points points (default 5e7) as
  steps      tracks of 5000 points that go on step by step across the raster: every move reads a fresh 3 x 3 window
  loiterer   whole tracks of --long-length points (default 2.5e6) that oscillate among four cells
on two grids: (4, 17) -- memories 1..4 x np.linspace(0, 4, 17), fit_tracks' default round -- and (1, 1) -- memory 1, nu 1,
where the profile does K21's work and nothing is shared.  HIP events around the Python calls (the allocation of the rows,
the read-back of the two end offsets, the memset and the launch; for the separate calls all of that once per combination);
after a warm-up of each, in which the profile's rows must equal the separate calls' integer for integer, the two ALTERNATE
--runs times (default 5, the order reversed every other round) and each gets its median.  Each step is a child of its own
under `timeout -k 10`.  Without --step this is the driver: it stops at the first step that fails and writes the table to
--out."""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=5e7)
ap.add_argument('--long-length', type=float, default=2.5e6)
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--step', choices=('steps', 'loiterer'), default=None)
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_SECONDS = 400


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
    results = {step: run_step(step) for step in ('steps', 'loiterer')}
    head = results['steps']
    lines = [f'{head["rows"]} x {head["cols"]}, {head["device"]}, {args.runs} alternating runs a call, library '
             f'{os.path.basename(head["lib"])}', '',
             '| step | points | tracks | grid | profile ms | separate calls ms | separate / profile | profile ms a combination | '
             'profile min .. max | separate min .. max |', '|---|---|---|---|---|---|---|---|---|---|']
    for step, res in results.items():
        for grid, t in res['grids'].items():
            p, s = t['profile'], t['separate']
            lines.append(f'| {step} | {res["points"]:.2e} | {res["ntracks"]} | {grid} | {p["median"]:.3f} | {s["median"]:.3f} | '
                         f'{s["median"] / p["median"]:.2f} | {p["median"] / t["combinations"]:.3f} | '
                         f'{min(p["runs"]):.3f} .. {max(p["runs"]):.3f} | {min(s["runs"]):.3f} .. {max(s["runs"]):.3f} |')
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
    from ssrs_amd import _native as nat
    from ssrs_amd import movmodel

    rows, cols = 5000, 6000
    dev = torch.device('cuda', 0)
    gen = torch.Generator(device=dev).manual_seed(21)
    updraft = torch.rand((rows, cols), generator=gen, device=dev, dtype=torch.float64) * 2.8 + 0.2
    potential = ((rows - torch.arange(rows, device=dev, dtype=torch.float32))[:, None] +
                 torch.rand((rows, cols), generator=gen, device=dev, dtype=torch.float32) * 0.8).contiguous()

    # the two workloads of time_track_score.py
    if which == 'steps':
        length = 5000
        n = max(int(args.points) // length, 1)
        ring = torch.tensor([(1, 1), (1, 0), (1, -1)], device=dev, dtype=torch.int32)
        steps = ring[torch.randint(0, 3, (n, length), generator=gen, device=dev)]
        steps[:, 0, 0] = 2
        steps[:, 0, 1] = torch.randint(200, cols - 200, (n,), generator=gen, device=dev, dtype=torch.int32)
        pts = torch.cumsum(steps, 1)
        traj = torch.stack([pts[..., 0].clamp(1, rows - 2), pts[..., 1].clamp(1, cols - 2)], -1).to(torch.int16).view(-1, 2)
        del steps, pts
    else:
        length = int(args.long_length)
        n = max(int(args.points) // length, 1)
        j = torch.arange(length, device=dev)
        traj = torch.cat([torch.stack([500 + 37 * k + (j & 1), 700 + 91 * k + ((j >> 1) & 1)], 1).to(torch.int16)
                          for k in range(n)])
        del j
    traj = traj.contiguous()
    off = torch.from_numpy(np.arange(n + 1, dtype=np.int64) * length).to(dev)
    total = int(traj.shape[0])

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), res

    grids = {}
    for memories, nus in (((1, 2, 3, 4), np.linspace(0., 4., 17)), ((1,), np.array([1.]))):
        def profile():
            return movmodel.score_tracks_profile(traj, (rows, cols), 0., memories, nus, updraft, potential, offsets=off).rows

        def separate():
            return torch.stack([torch.stack([
                movmodel.score_tracks(traj, (rows, cols), 0., m, float(nu), updraft, potential, offsets=off, want_p=False,
                                      want_status=False).rows for nu in nus], 1) for m in memories], 1)

        calls = dict(profile=profile, separate=separate)
        warm = {name: timed(fn)[1] for name, fn in calls.items()}                    # the warm-ups
        if not torch.equal(warm['profile'], warm['separate']):
            sys.exit(f'{which} {len(memories)} x {len(nus)}: the profile differs from the separate calls')
        if int(warm['profile'][:, 0, 0, 1:].sum()) != total - n:
            sys.exit(f'{which}: the statuses of {int(warm["profile"][:, 0, 0, 1:].sum())} moves were counted')
        del warm
        ms = {name: [] for name in calls}
        for rep in range(args.runs):
            for name in (list(calls)[::-1] if rep & 1 else list(calls)):
                ms[name].append(timed(calls[name])[0])
        grids[f'({len(memories)}, {len(nus)})'] = dict(
            combinations=len(memories) * len(nus),
            **{name: dict(median=float(np.median(runs)), runs=runs) for name, runs in ms.items()})
    print(json.dumps(dict(rows=rows, cols=cols, points=total, ntracks=n, device=torch.cuda.get_device_name(0),
                          lib=nat.LIB_PATH, grids=grids)), flush=True)


if args.step:
    step(args.step)
else:
    driver()
