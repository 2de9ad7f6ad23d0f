"""K21's speed: ssrs_tracks_score on a 5000 x 6000 raster with a rough f64 updraft and an f32 potential that falls
northwards, over --points points (default 5e7) in two shapes,
  steps      tracks of 5000 points that go on step by step across the raster (a heading that wobbles by 45 degrees): every
             move reads a fresh 3 x 3 window, long runs of SCORED moves
  loiterer   whole tracks of --long-length points (default 2.5e6) that oscillate among four cells, the shape of the tracks
             that sit in a basin of the potential: the same windows millions of times, every gather an L1 / L2 hit, and all
             the surprisal of a block lands on a few cells of the maps
each with memory_parameter 1 and 8, with and without the two maps.  HIP events around the library call alone; after a
warm-up of each the calls ALTERNATE --runs times (default 7, the order reversed every other round) and each gets its
median.  Each step is a child of its own under `timeout -k 10`.  Without --step this is the driver: it stops at the first
step that fails and writes the table to --out.
Bytes: a point STREAMS 13 B (4 B read of traj, 8 B of p and 1 B of status written); its move GATHERS 108 B (nine f64 of the
updraft, nine f32 of the potential), which the caches serve for the most part.  Both rates are reported; the streamed one
is what tools/microbench/stream.hip's figures compare with."""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=float, default=5e7)
ap.add_argument('--long-length', type=float, default=2.5e6)
ap.add_argument('--runs', type=int, default=7)
ap.add_argument('--step', choices=('steps', 'loiterer'), default=None)
ap.add_argument('--out', default=None, help='write the markdown table here as well')
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_SECONDS = 240
STREAMED, GATHERED = 13, 108


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
             '| step | points | tracks | call | median ms | G points/s | streamed GB/s | gathered GB/s | min .. max ms | scored |',
             '|---|---|---|---|---|---|---|---|---|---|']
    for step, res in results.items():
        for call, t in res['calls'].items():
            rate = res['points'] / t['median'] / 1e6
            lines.append(f'| {step} | {res["points"]:.2e} | {res["ntracks"]} | {call} | {t["median"]:.3f} | {rate:.2f} | '
                         f'{rate * STREAMED:.1f} | {rate * GATHERED:.1f} | {min(t["runs"]):.3f} .. {max(t["runs"]):.3f} | '
                         f'{t["scored"]} |')
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

    if which == 'steps':
        length = 5000
        n = max(int(args.points) // length, 1)
        # a heading on the ring of eight moves that wobbles by one place a step around north-east .. north-west
        ring = torch.tensor([(1, 1), (1, 0), (1, -1)], device=dev, dtype=torch.int32)
        pick = torch.randint(0, 3, (n, length), generator=gen, device=dev)
        steps = ring[pick]
        steps[:, 0, 0] = 2
        steps[:, 0, 1] = torch.randint(200, cols - 200, (n,), generator=gen, device=dev, dtype=torch.int32)
        pts = torch.cumsum(steps, 1)
        traj = torch.stack([pts[..., 0].clamp(1, rows - 2), pts[..., 1].clamp(1, cols - 2)], -1).to(torch.int16).view(-1, 2)
        lengths = [length] * n
        del pick, steps, pts
    else:
        length = int(args.long_length)
        n = max(int(args.points) // length, 1)
        j = torch.arange(length, device=dev)
        parts = []
        for k in range(n):
            r0, c0 = 500 + 37 * k, 700 + 91 * k
            parts.append(torch.stack([r0 + (j & 1), c0 + ((j >> 1) & 1)], 1).to(torch.int16))
        traj = torch.cat(parts)
        lengths = [length] * n
        del parts, j
    traj = traj.contiguous()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(dev)
    total, ntracks = int(traj.shape[0]), len(lengths)

    # the maps are the caller's and are accumulated into, as in a sweep over chunks: their zeroing is not in the call
    smap = torch.zeros((rows, cols), dtype=torch.int64, device=dev)
    cmap = torch.zeros((rows, cols), dtype=torch.int32, device=dev)

    def call(memory, maps):
        return lambda: movmodel.score_tracks(traj, (rows, cols), 0., memory, 1., updraft, potential, offsets=off,
                                             surprisal_map=smap if maps else None, scored_map=cmap if maps else None)

    calls = {f'memory {m}{", maps" if maps else ""}': call(m, maps) for m in (1, 8) for maps in (False, True)}

    def timed(fn):
        smap.zero_(), cmap.zero_()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), res

    ms = {name: [] for name in calls}
    seen = {}
    for name, fn in calls.items():                                   # the warm-ups
        _, res = timed(fn)
        rows_ = res.host_rows()
        seen[name] = int(rows_[:, 1].sum())
        if int(rows_[:, 1:].sum()) != total - ntracks:
            sys.exit(f'{name}: the statuses of {int(rows_[:, 1:].sum())} moves were counted, {total - ntracks} expected')
        if res.scored_map is not None and int(res.scored_map.sum()) != seen[name]:
            sys.exit(f'{name}: the scored map holds {int(res.scored_map.sum())}, the rows {seen[name]}')
        del res
    for rep in range(args.runs):
        for name in (list(calls)[::-1] if rep & 1 else list(calls)):
            t, res = timed(calls[name])
            ms[name].append(t)
            del res
    out = {name: dict(median=float(np.median(runs)), runs=runs, scored=seen[name]) for name, runs in ms.items()}
    print(json.dumps(dict(rows=rows, cols=cols, points=total, ntracks=ntracks, device=torch.cuda.get_device_name(0),
                          lib=nat.LIB_PATH, calls=out)), flush=True)


if args.step:
    step(args.step)
else:
    driver()
